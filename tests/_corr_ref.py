"""Numpy referee and input builders for the correlation pyramid and lookup (corr_kernels.hip; include/vppx.h has
the arithmetic).

TEST INFRASTRUCTURE ONLY.  Plain numpy, no GPU: tests/test_corr_ref_cpu.py holds the referee to the arrays the
reference's own CorrBlock1D produced (tests/golden/corr_cases.npz) and to torch's CPU avg_pool2d / grid_sample, and
asserts every coverage claim the GPU file (tests/test_gpu_corr.py) relies on, on the very arrays the GPU file uploads.

Every step is one float32 operation on float32 arrays, which numpy rounds correctly, in the order the header gives.
The one fused step, fma(b, wr, s), is the float64 product of the float32 operands (exact: 48 bits) plus s, rounded
to float32 once (`fma32`: the float64 sum is rounded to odd first, so that the second rounding cannot go wrong).

A bfloat16 level is held as its 16 bits (uint16); `_handoff_bf16_ref` has the rounding.
"""
from types import SimpleNamespace

import numpy as np

import _handoff_bf16_ref as BR
import _handoff_ref as R

F32, F64 = np.float32, np.float64
MAX_LEVELS, MAX_RADIUS = 4, 8


# ---------------------------------------------------------------------------------------------------
# the operations
# ---------------------------------------------------------------------------------------------------
def pool(level):
    """[N, W] float32 -> [N, W // 2]: ((+0 + a) + b) / 2, an odd last column dropped."""
    level = np.asarray(level)
    assert level.dtype == F32 and level.ndim == 2
    w = level.shape[1] // 2
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        out = ((F32(0) + level[:, 0:2 * w:2]) + level[:, 1:2 * w:2]) / F32(2)
    assert out.dtype == F32
    return np.ascontiguousarray(out)


def pool_bits(bits):
    """[N, W] bf16 bits -> [N, W // 2] bits: the stored cells widened, pooled in float32, rounded once."""
    return BR.bits(BR.bf16_rne_f32(pool(BR.widen(bits))))


def pyramid(level0, levels):
    """level0 [N, W3] float32 cells or uint16 bf16 bits -> list of `levels` arrays, entry 0 is level0."""
    out = [np.ascontiguousarray(level0)]
    step = pool_bits if out[0].dtype == np.uint16 else pool
    for _ in range(1, levels):
        out.append(step(out[-1]))
    return out


def widened(pyr):
    return [BR.widen(lv) if lv.dtype == np.uint16 else lv for lv in pyr]


def fma32(a, b, c):
    """fma(a, b, c) of float32 arrays, rounded ONCE.  The product of two float32 is exact in float64.  Its sum with c is
    not: rounding it to float64 and then to float32 is two roundings, and the second one goes wrong whenever the product
    sits on a float32 tie that c decides, which weights like 0.75 make common.  So the float64 sum is rounded to odd
    (TwoSum gives the error term; an inexact even sum moves one place towards it), after which the rounding to float32
    is that of the exact value (53 >= 24 + 2 bits)."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        p = a.astype(F64) * b.astype(F64)
        c = c.astype(F64)
        hi = p + c
        t = hi - p
        lo = (p - (hi - t)) + (c - t)
        bits = np.ascontiguousarray(hi).view(np.int64)
        fix = np.isfinite(hi) & np.isfinite(lo) & (lo != 0) & ((bits & 1) == 0)
        away = np.signbit(lo) == np.signbit(hi)                    # the exact value is larger in magnitude than hi
        bits = np.where(fix, np.where(away, bits + 1, bits - 1), bits)
        return bits.view(F64).astype(F32)


def lookup(pyr, coords, radius):
    """pyr: list of [N, Wi] float32 levels (bf16 levels widened first); coords [N] float32 -> [N, L * (2r+1)]
    float32, level-major.  `channels_first` lays it out as the library does."""
    c = np.ascontiguousarray(coords, F32).reshape(-1)
    t = np.arange(-radius, radius + 1).astype(F32)[None, :]
    outs = []
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for i, lev in enumerate(pyr):
            assert lev.dtype == F32 and lev.shape[0] == c.size
            W = lev.shape[1]
            wm1 = F32(W - 1)
            x = t + (c / F32(2 ** i))[:, None]
            xg = (F32(2) * x) / wm1 - F32(1)
            ix = ((xg + F32(1)) / F32(2)) * wm1
            fl = np.floor(ix)
            fl1 = fl + F32(1)
            wr, wl = ix - fl, fl1 - ix
            assert ix.dtype == F32 and wr.dtype == F32 and wl.dtype == F32
            in_a, in_b = (fl >= 0) & (fl <= wm1), (fl1 >= 0) & (fl1 <= wm1)
            a = np.where(in_a, np.take_along_axis(lev, np.where(in_a, fl, 0).astype(np.int64), 1), F32(0))
            b = np.where(in_b, np.take_along_axis(lev, np.where(in_b, fl1, 0).astype(np.int64), 1), F32(0))
            s = F32(0) + a * wl
            assert s.dtype == F32
            o = fma32(b, wr, s)
            outs.append(np.where((in_a | in_b) & np.isfinite(ix), o, F32(0)))
    return np.ascontiguousarray(np.concatenate(outs, axis=1))


def channels_first(out, B, H4, W2):
    """[N, C] -> [B, C, H4, W2], the .permute(0, 3, 1, 2) layout."""
    return np.ascontiguousarray(out.reshape(B, H4, W2, -1).transpose(0, 3, 1, 2))


def same_bits(got, want):
    """Cells whose 32 bits differ; two NaNs count as the same cell (the payload of a NaN is not part of the contract)."""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, (got.shape, want.shape)
    return int(((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))).sum())


# ---------------------------------------------------------------------------------------------------
# input builders: the GPU file and the CPU file see the same arrays
# ---------------------------------------------------------------------------------------------------
ROWS_PER_WORKGROUP = 4
# (B, H4, W2, W3)
PYRAMID_SHAPES = [
    (1, 1, 1, 16),       # the smallest legal call: widths 16, 8, 4, 2
    (1, 2, 3, 17),       # an odd column is dropped
    (1, 1, 5, 30),       # 15, then 7, then 3 cells: odd at two levels
    (1, 3, 7, 127), (1, 1, 2, 128), (1, 2, 3, 129), (1, 1, 3, 130),     # around one 64-lane trip of pairs
    (2, 2, 9, 37),       # two frames that differ
    (1, 2, 240, 240),    # RAFT-Stereo at 960 columns
    (1, 1, 3, 257),
]
LOOKUP_SHAPES = [
    (1, 1, 1, 16),
    (1, 2, 63, 17),
    (1, 1, 65, 30),      # W2 crosses 64 pixels
    (2, 3, 70, 37),      # W2 != W3
    (1, 2, 240, 240),
]
LOOKUP_PARAMS = [(4, 4), (1, 0), (3, 2)]      # (levels, radius)
V_ORDER = np.array([1.0, 0.0, -0.0, 0.5, 2.0, -1.0], F32)       # R.VALUES_OF_V, a modulated row first
NAN_AT = dict(row=0, cell=5)                  # lookup volumes: one NaN cell, read under a weight of zero from coordinate 4
NAN_SHAPE = (1, 2, 63, 17)                    # W3 - 1 = 16: there the round trip of an integer position is exact


def tag(shape):
    return "x".join(str(s) for s in shape)


def volume_case(shape, hints=True, nan_cell=False):
    """-> namespace(corr [B,H4,W2,1,W3] float32, hints, valid [B,1,H,W] or None, v4, B, H4, W2, W3, H, W, N).
    Rows cycle through V_ORDER, then v = 1 mostly; every row's target column lies inside the row, so that the
    modulation leaves normal cells near it and +-0 cells (an underflowed factor) far from it.  A pair of -0 cells (in rows of 32 cells and more a quad
    and an octet too) is planted in the first rows whatever their v."""
    B, H4, W2, W3 = shape
    N = B * H4 * W2
    rng = np.random.default_rng([59, B, H4, W2, W3])
    corr = rng.standard_normal((N, W3)).astype(F32)
    for r in range(min(N, 3)):                                   # row 0: v = 1, row 1: v = 0, row 2: v = -0
        corr[r, 0:2] = -0.0
        if W3 >= 32:                                             # narrower rows keep their cells: the lookup must read something
            corr[r, 4:8] = -0.0
            corr[r, 8:16] = -0.0
            corr[r, 21:23] = -0.0                                # a pair that straddles two pooled cells: -0 with a neighbour
    if nan_cell:
        assert shape == NAN_SHAPE
        corr[NAN_AT["row"], NAN_AT["cell"]] = np.nan
    c = SimpleNamespace(shape=shape, B=B, H4=H4, W2=W2, W3=W3, N=N, corr=corr.reshape(B, H4, W2, 1, W3), hints=None, valid=None,
                        v4=None, H=0, W=0)
    if hints:
        v = R._cycle_v(N, rng, p_zero=0.75)                      # about a third of the rows carry a hint
        k = min(N, len(V_ORDER))
        v[:k] = V_ORDER[:k]
        x = np.tile(np.arange(W2, dtype=F64), B * H4)
        tgt = rng.uniform(0, W3, N)
        h4 = (x * v - tgt).astype(F32).reshape(B, H4, W2)
        c.v4 = v.reshape(B, H4, W2)
        c.H, c.W = 4 * H4 + int(rng.integers(0, 4)), 4 * W2 + int(rng.integers(0, 4))
        c.hints, c.valid = R.scatter_to_full(h4, c.v4, c.H, c.W, rng)
    return c


def modulated_level0(c):
    """Level 0 on the CPU: the float32 referee of the modulation under the library's v == 0 rule.  The device's differs
    from it by its exp; the GPU file pools what the device's modulation call left instead."""
    if c.hints is None:
        return c.corr.reshape(c.N, c.W3)
    return R.raft_modulate(c.corr, c.hints, c.valid, rule="library").out.reshape(c.N, c.W3)


def directed_coords(W3):
    """One of every class the lookup tells apart (the names are what the CPU file asserts)."""
    d = {
        "integer": [1.0, 3.0, 4.0], "half": [2.5, 6.5],
        "zero": [0.0], "minus_zero": [-0.0],
        "last_cell": [float(((W3 >> i) - 1) * 2 ** i) for i in range(MAX_LEVELS)],
        "left_fringe": [-0.25, -1.0, -0.75], "right_fringe": [W3 - 0.5, W3 - 1 + 0.25, W3 - 0.001],
        "half_outside": [1.5, W3 - 2.5, -2.0, W3 + 1.0],
        "far_outside": [-64.0, W3 + 64.0, -1000.0, 8.0 * W3],
        "huge": [1e30, -1e30], "inf": [np.inf, -np.inf], "nan": [np.nan],
    }
    return {k: np.array(v, F32) for k, v in d.items()}


def coords_case(shape):
    """-> [S, B, H4, W2] float32: S sheets of coordinates for one volume, S = 1 unless the volume has fewer pixels than
    there are directed coordinates.  The directed ones come first (pixel NAN_AT's is 4: the NaN cell under a weight of
    zero), the rest are drawn from [-3, W3 + 3) and make up at least seven eighths."""
    B, H4, W2, W3 = shape
    N = B * H4 * W2
    rng = np.random.default_rng([61, B, H4, W2, W3])
    d = np.concatenate([[F32(NAN_AT["cell"] - 1)]] + list(directed_coords(W3).values())).astype(F32)
    total = max(N, 8 * len(d))
    total = (total + N - 1) // N * N
    c = rng.uniform(-3.0, W3 + 3.0, total).astype(F32)
    whole = rng.random(total) < 0.2
    c[whole] = np.floor(c[whole])
    half = rng.random(total) < 0.15
    c[half] = np.floor(c[half]) + F32(0.5)
    # the directed ones at stride N from pixel 0 on: sheet s, pixel 0 first, so that pixel NAN_AT["row"] = 0 of sheet 0 reads 4
    S = total // N
    c = c.reshape(S, N)
    k = 0
    for p in range(N):
        for s in range(S):
            if k < len(d):
                c[s, p] = d[k]
                k += 1
    assert k == len(d)
    return np.ascontiguousarray(c.reshape(S, B, H4, W2))
