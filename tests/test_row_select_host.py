"""Host side of milan_row_select: the entry point is declared where the C-ABI test looks
for it, an older build of the library stays loadable, and there is no CPU fallback (no GPU)."""
import pathlib
import re

import pytest
import torch

from milan_amd import hip

REPO = pathlib.Path(__file__).resolve().parent.parent


def test_row_select_is_declared_exported_and_probed():
    header = (REPO / 'include' / 'milan_hip.h').read_text()
    lib = hip.load_library()
    assert 'milan_row_select' in hip.SIGNATURES
    assert re.search(r'\bmilan_row_select\s*\(', header)
    assert hasattr(lib, 'milan_row_select')
    # added without a new ABI version: a library built before it still loads
    assert 'milan_row_select' in hip.PROBED
    assert len(hip.SIGNATURES['milan_row_select'][1]) == 12
    assert hip.ABI_VERSION == 11 == lib.milan_abi_version()
    assert sorted(hip.ROW_SELECT_PATHS.values()) == [0, 1, 2, 3]


def test_row_select_checks_its_arguments_before_any_launch():
    lib = hip.load_library()
    assert lib.milan_row_select(None, None, 0., 1, 8, 2, None, 0, None, None, 0, None) != 0
    assert b'null argument' in lib.milan_last_error()


def test_row_select_has_no_cpu_fallback():
    with pytest.raises(hip.HipUnavailableError):
        hip.row_select(torch.zeros(1, 8), 2)
