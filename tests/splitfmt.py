"""The split-f16 storage format (include/milan_hip.h) in plain torch, for the tests.

A row of C channels (C % 8 == 0) is C fp32 words: per 8 channels one 32-byte group
[hi x8 | lo x8] of f16 values, hi = f16(v) (round to nearest even), lo = f16(v - hi), where
v = clamp(x * 2^k, +-65504) -- the clamp is what MILAN_STATUS_SATURATED reports.  The value a
group holds is hi + lo (exact in fp32 and float64), in units of 2^-k.
"""
import torch

F16_MAX = 65504.0


def to_split(x, scale_log2=0):
    """(P, C) float32 -> the split-f16 groups of x * 2^scale_log2 as a float32 tensor of the same
    shape: per 8 channels [hi x8 | lo x8]; and the value they hold (float64, divided by the scale
    again: what a reader of the buffer multiplies with)."""
    p, c = x.shape
    assert c % 8 == 0, c
    v = (x.float() * 2.0 ** scale_log2).clamp(-F16_MAX, F16_MAX)
    hi = v.half()
    lo = (v - hi.float()).half()
    packed = torch.stack([hi.view(p, c // 8, 8), lo.view(p, c // 8, 8)], dim=2)
    held = (hi.double() + lo.double()) / 2.0 ** scale_log2
    return packed.contiguous().view(torch.float32).view(p, c), held


def from_split(y, scale_log2=0):
    """the float64 values a (P, C) split-format buffer holds (divided by 2^scale_log2)"""
    p, c = y.shape
    halves = y.contiguous().view(torch.float16).view(p, c // 8, 2, 8)
    return (halves[:, :, 0].double() + halves[:, :, 1].double()).reshape(p, c) / 2.0 ** scale_log2
