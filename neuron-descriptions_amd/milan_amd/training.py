"""Training utilities (reference `src/utils/training.py:12-107`): early
stopping on a tracked value and the train / validation splits that
`LanguageModel.fit` uses.  Same semantics and error messages as the
reference; `random_split` draws from torch's global generator like it does."""
from typing import Sequence, Sized, Tuple, cast

from torch.utils import data


class EarlyStopping:
    """Observes a numerical value and determines when it has not improved."""

    def __init__(self, patience: int = 4, decreasing: bool = True):
        self.patience = patience
        self.decreasing = decreasing
        self.best = float('inf') if decreasing else float('-inf')
        self.num_bad = 0

    def __call__(self, value: float) -> bool:
        """Consider `value`; True once patience has been exceeded."""
        improved = self.decreasing and value < self.best
        improved |= not self.decreasing and value > self.best
        if improved:
            self.best = value
            self.num_bad = 0
        else:
            self.num_bad += 1
        return self.num_bad > self.patience

    @property
    def improved(self) -> bool:
        """Whether the last value was an improvement."""
        return self.num_bad == 0


def random_split(dataset: data.Dataset,
                 hold_out: float = .1) -> Tuple[data.Subset, data.Subset]:
    """Random (train, val) split with `int(hold_out * len)` samples in val."""
    if hold_out <= 0 or hold_out >= 1:
        raise ValueError(f'hold_out must be in (0, 1), got {hold_out}')

    size = len(cast(Sized, dataset))
    val_size = int(hold_out * size)
    train_size = size - val_size
    for name, size in (('train', train_size), ('val', val_size)):
        if size == 0:
            raise ValueError(f'hold_out={hold_out} causes {name} set size '
                             'to be zero')

    train, val = data.random_split(dataset, (train_size, val_size))
    return train, val


def fixed_split(dataset: data.Dataset,
                indices: Sequence[int]) -> Tuple[data.Subset, data.Subset]:
    """(samples not in `indices`, samples in `indices`)."""
    size = len(cast(Sized, dataset))
    for index in indices:
        if index < 0 or index >= size:
            raise IndexError(f'dataset index out of bounds: {index}')

    others = sorted(set(range(size)) - set(indices))
    if not others:
        raise ValueError('indices cover entire dataset; nothing to split!')

    return data.Subset(dataset, others), data.Subset(dataset, indices)
