"""What the float64 referees of the network-glue kernels share: the units of their limits, bfloat16 as numpy sees it, and
the comparison of a result with namespace(value, limit).

TEST INFRASTRUCTURE ONLY.  Plain numpy, no GPU.  tests/_readout_ref.py, _gru_ref.py, _norm_ref.py and _motion_ref.py
import these names and their tests reach them through the referee (R.compare, N.compare_bf16, ...).
"""
from types import SimpleNamespace

import numpy as np

from _handoff_bf16_ref import rne64

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
SECOND_ORDER = 1 + 2.0 ** -10
TINY = 2.0 ** -126


def _und(x):
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(x) < TINY, TINY, 0.0)


def _ns(value, limit, **kw):
    return SimpleNamespace(value=value, limit=limit, **kw)


# ---------------------------------------------------------------------------------------------------
# bfloat16 (the upper 16 bits of a float32), round to nearest even
# ---------------------------------------------------------------------------------------------------
def bf16_bits(a):
    """float32 array -> uint16 bits of the nearest bfloat16 (ties to even; NaN quieted)."""
    u = np.ascontiguousarray(a, F32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)


def bf16_widen(bits):
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(F32)


def to_bf16(a):
    """float32 array -> the nearest bfloat16 values, as float32."""
    return bf16_widen(bf16_bits(a)).reshape(np.shape(a))


# ---------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------
def classes(a):
    """0 finite, 1 NaN, 2 +inf, 3 -inf."""
    a = np.asarray(a)
    return np.where(np.isnan(a), 1, np.where(np.isposinf(a), 2, np.where(np.isneginf(a), 3, 0)))


def compare(got, ref):
    """-> (worst |got - value| / limit over the finite cells, cells beyond the limit, cells of another class)."""
    got = np.asarray(got).astype(F64)
    assert got.shape == ref.value.shape, (got.shape, ref.value.shape)
    cg, cr = classes(got), classes(ref.value)
    fin = cr == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        dist = np.abs(got - ref.value)
        beyond = fin & (cg == 0) & ~(dist <= ref.limit)
        ratio = np.where(fin & (cg == 0) & (ref.limit > 0), dist / np.where(ref.limit > 0, ref.limit, 1.0), 0.0)
        ratio = np.where(fin & (cg == 0) & (ref.limit == 0) & (dist > 0), np.inf, ratio)
    return float(ratio.max(initial=0.0)), int(beyond.sum()), int((cg != cr).sum())


# bfloat16 results: the inputs are bfloat16 values held as float32, the float32 result is rounded once, and rounding is
# monotone, so a cell lies in [rne(value - limit), rne(value + limit)]
def band(ref):
    with np.errstate(invalid="ignore", over="ignore"):
        return rne64(ref.value - ref.limit), rne64(ref.value + ref.limit)


def compare_bf16(got32, ref):
    """got32: the bfloat16 cells as float32 -> (cells outside the band, cells of another class)."""
    got = np.asarray(got32, F32)
    lo, hi = band(ref)
    cg, cr = classes(got), classes(ref.value)
    fin = cr == 0
    with np.errstate(invalid="ignore"):
        # a finite value next to the largest bfloat16 may round to infinity: the band says so
        miss = fin & ~((got >= lo) & (got <= hi))
    return int(miss.sum()), int((~fin & (cg != cr)).sum())


def misses(got, ref, dtype="float32"):
    """Cells beyond the limit (outside the band) plus cells of another class."""
    if dtype == "bfloat16":
        return sum(compare_bf16(got, ref))
    _, beyond, other = compare(got, ref)
    return beyond + other
