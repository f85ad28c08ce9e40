"""Numpy referee and input builders for the fused correlation call (corr_gemm_kernels.hip; include/vppx.h has the
arithmetic): the all-pairs GEMM, / sqrt(D), the hint modulation and the pyramid in one launch.

TEST INFRASTRUCTURE ONLY.  Plain numpy, no GPU: tests/test_corr_fused_ref_cpu.py holds the referee to the arrays the
reference's own CorrBlock1D produced (tests/golden/corr_cases.npz) and asserts, on the very arrays the GPU file
(tests/test_gpu_corr_fused.py) uploads, every premise that file relies on.

Exact features.  make_corr_golden.py's recipe puts every feature on a grid of 1/16 in [-4, 4]: a product is a multiple
of 2^-8 of at most 16, so as long as  sum_k |f2 * f3| < 2^16  every partial sum, in ANY order and grouping, is a
multiple of 2^-8 below 2^16 and therefore a float32 (24 bits).  The float32 accumulator of the matrix cores then holds the
exact dot product whatever its order, level 0 is one correctly rounded division of it, and the test can ask for bits.
`exact_level0` asserts that premise on its inputs.  Such features are bfloat16 values as well (7 bits).

Features that are not exact are held to `_handoff_ref.corr_whole`, the bound of a float32 dot product in any order, plus
the one rounding of a bfloat16 store: half a unit in the last of bfloat16's 8 significant bits at the largest float32
the first bound allows, 2^(e-8) for a magnitude in [2^e, 2^(e+1)) (`bf16_half_ulp`).  That is 2^-9 * 2^(e+1): between
2^-9 and 2^-8 of the value.  The plain product 2^-9 * |value| is NOT a bound of a correct rounding (1 + 2^-8 is a tie
and goes to 1, 2^-8 away; tests/test_corr_fused_ref_cpu.py shows it on the reference's own cells), so the format's own
half unit is what is asserted and the cells beyond 2^-9 * |value| are only counted and printed.
"""
import os
from types import SimpleNamespace

import numpy as np

import _corr_ref as CR
import _handoff_bf16_ref as BR
import _handoff_ref as R

F32, F64 = np.float32, np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
DEVICE_EXP_ULPS = 1.0           # tests/test_gpu_handoff_ref.py's figure, justified there
GOLDEN_TAGS = ["a", "b", "c", "d"]

# (B, D, H4, W2, W3)
DIRECTED_SHAPES = [
    (2, 256, 3, 20, 37),        # full K loop, both W tails, W2 != W3, odd W3, batch and row strides
    (1, 40, 2, 33, 64),         # K tail after whole K steps
    (1, 256, 1, 240, 240),      # the workload's row: every tile whole
    (1, 5, 2, 16, 16),          # uploaded as views one element into their buffers: misaligned inputs
]
MISALIGNED_SHAPE = (1, 5, 2, 16, 16)
LEVELS_SHAPE = (1, 4, 2, 9, 129)
RANDOM_SHAPE = (2, 256, 3, 20, 37)
ONE_HOT_SHAPE = (1, 7, 2, 19, 37)


def tag(shape):
    return "x".join(str(s) for s in shape)


def golden():
    return np.load(os.path.join(HERE, "golden", "corr_cases.npz"))


# ---------------------------------------------------------------------------------------------------
# the operations
# ---------------------------------------------------------------------------------------------------
def exact_level0(f2, f3):
    """fmap2 [B,D,H4,W2], fmap3 [B,D,H4,W3] float32 -> level 0 [N, W3] float32, N = B*H4*W2 rows (b, y, x2):
    the float64 dot product -> float32 (asserted exact, as is every partial sum in any order) -> +0 + -> / sqrt(float32(D))
    in float32."""
    f2, f3 = np.asarray(f2), np.asarray(f3)
    assert f2.dtype == F32 and f3.dtype == F32 and f2.shape[:3] == f3.shape[:3]
    B, D, H4, W2 = f2.shape
    a, b = f2.astype(F64), f3.astype(F64)
    dot = np.einsum("aijk,aijh->ajkh", a, b)
    mag = np.einsum("aijk,aijh->ajkh", np.abs(a), np.abs(b))
    assert (a * 16 == np.round(a * 16)).all() and (b * 16 == np.round(b * 16)).all(), "features are not on the 1/16 grid"
    assert mag.max() < 2.0 ** 16, "a partial sum may need more than 24 bits"
    d32 = dot.astype(F32)
    assert (d32.astype(F64) == dot).all(), "the dot product is not a float32"
    c = (F32(0) + d32) / np.sqrt(F32(D))
    assert c.dtype == F32
    return np.ascontiguousarray(c.reshape(B * H4 * W2, f3.shape[3]))


def einsum_level0(f2, f3):
    """The reference's own arithmetic restated (corr.py:153-155): a float32 einsum, then / sqrt(D) with the float32
    square root, on the CPU.  -> [N, W3] float32."""
    import torch
    a, b = torch.from_numpy(np.ascontiguousarray(f2, F32)), torch.from_numpy(np.ascontiguousarray(f3, F32))
    B, D, H4, W2 = a.shape
    corr = torch.einsum("aijk,aijh->ajkh", a, b).reshape(B, H4, W2, 1, -1).contiguous()
    corr = corr / torch.sqrt(torch.tensor(D).float())
    return corr.numpy().reshape(B * H4 * W2, -1)


def bound(f2, f3, hints, valid, bf16):
    """-> (the float64 value of every cell [N, W3], how far a stored cell may be from it)."""
    c64, lim = R.corr_whole(f2, f3, hints, valid, DEVICE_EXP_ULPS)
    N = c64.shape[0] * c64.shape[1] * c64.shape[2]
    c64, lim = c64.reshape(N, -1), np.broadcast_to(lim, c64.shape).reshape(N, -1)
    if bf16:
        lim = lim + bf16_half_ulp(np.abs(c64) + lim)
    return c64, lim


def bf16_half_ulp(mag):
    """Half a unit in the last place of bfloat16 at magnitude `mag` (float64, >= 0): 2^(e-8) for mag in [2^e, 2^(e+1)),
    and half the subnormal spacing, 2^-134, below 2^-126."""
    _, e = np.frexp(np.maximum(np.asarray(mag, F64), 2.0 ** -126))           # mag = f * 2^e, f in [0.5, 1)
    return np.ldexp(1.0, e - 9)


def bf16_round(level):
    """float32 cells -> their bfloat16 bits, rounded to nearest even once."""
    return BR.bits(BR.bf16_rne_f32(np.ascontiguousarray(level, F32)))


# ---------------------------------------------------------------------------------------------------
# input builders: the GPU file and the CPU file see the same arrays
# ---------------------------------------------------------------------------------------------------
def grid_features(rng, shape):
    """make_corr_golden.py's recipe: a grid of 1/16 in [-4, 4]."""
    return (np.clip(np.round(rng.standard_normal(shape) * 16), -64, 64) / 16).astype(F32)


def _hints(c, rng):
    """Hints as _corr_ref.volume_case makes them: the first rows run through V_ORDER, about a third of the rest carry a
    hint, and every row's target column lies inside the row."""
    N = c.N
    v = R._cycle_v(N, rng, p_zero=0.75)
    k = min(N, len(CR.V_ORDER))
    v[:k] = CR.V_ORDER[:k]
    x = np.tile(np.arange(c.W2, dtype=F64), c.B * c.H4)
    tgt = rng.uniform(0, c.W3, N)
    h4 = (x * v - tgt).astype(F32).reshape(c.B, c.H4, c.W2)
    c.v4 = v.reshape(c.B, c.H4, c.W2)
    c.H, c.W = 4 * c.H4 + int(rng.integers(0, 4)), 4 * c.W2 + int(rng.integers(0, 4))
    c.hints, c.valid = R.scatter_to_full(h4, c.v4, c.H, c.W, rng)


_CASES = {}


def case(shape, kind="grid"):
    """-> namespace(f2 [B,D,H4,W2], f3 [B,D,H4,W3], hints, valid [B,1,H,W], v4 [B,H4,W2], B, D, H4, W2, W3, N, H, W).
    kind "grid": exact features; "random": normal deviates rounded to bfloat16 (so that both dtypes get the same values),
    whose float32 sums are not exact; "one_hot": fmap2 has a single 1 along k at every (b, y, x2), at k = khot[b, y, x2]."""
    key = (shape, kind)
    if key in _CASES:
        return _CASES[key]
    B, D, H4, W2, W3 = shape
    rng = np.random.default_rng([71, B, D, H4, W2, W3, {"grid": 0, "random": 1, "one_hot": 2}[kind]])
    c = SimpleNamespace(shape=shape, B=B, D=D, H4=H4, W2=W2, W3=W3, N=B * H4 * W2)
    if kind == "random":
        c.f2 = BR.bf16_rne_f32(rng.standard_normal((B, D, H4, W2)).astype(F32))
        c.f3 = BR.bf16_rne_f32(rng.standard_normal((B, D, H4, W3)).astype(F32))
    else:
        c.f2, c.f3 = grid_features(rng, (B, D, H4, W2)), grid_features(rng, (B, D, H4, W3))
    if kind == "one_hot":
        c.khot = rng.integers(0, D, (B, H4, W2))
        c.f2 = np.zeros((B, D, H4, W2), F32)
        np.put_along_axis(c.f2, c.khot[:, None], F32(1), axis=1)
    _hints(c, rng)
    _CASES[key] = c
    return c


def golden_case(t):
    """Case t of the recording as a namespace like case()'s, with the recorded arrays under .g(name)."""
    key = ("golden", t)
    if key in _CASES:
        return _CASES[key]
    g = golden()
    f2, f3 = g[f"{t}_f2"], g[f"{t}_f3"]
    B, D, H4, W2 = f2.shape
    c = SimpleNamespace(shape=(B, D, H4, W2, f3.shape[3]), B=B, D=D, H4=H4, W2=W2, W3=f3.shape[3], N=B * H4 * W2, f2=f2, f3=f3,
                        hints=g[f"{t}_hints"], valid=g[f"{t}_valid"], coords=g[f"{t}_coords"])
    c.H, c.W = c.hints.shape[2:]
    c.v4 = R.subsample(c.hints, c.valid, raft=True)[1]
    c.g = lambda name: g[f"{t}_{name}"]
    _CASES[key] = c
    return c


def nonfinite_case():
    """RANDOM_SHAPE's grid features with a NaN and an infinity planted on each side, and where they must show:
    -> (f2, f3, bad [N, W3] bool).  fmap2[b,k,y,x] spoils row (b, y, x); fmap3[b,k,y,x3] spoils column x3 of the rows of
    (b, y).  A product with an infinity is infinite or, against a zero feature, NaN: not finite either way."""
    c = case(RANDOM_SHAPE)
    f2, f3 = c.f2.copy(), c.f3.copy()
    bad = np.zeros((c.B, c.H4, c.W2, c.W3), bool)
    for (b, k, y, x), val in (((0, 3, 1, 7), np.nan), ((1, 200, 2, 19), np.inf)):
        f2[b, k, y, x] = val
        bad[b, y, x, :] = True
    for (b, k, y, x), val in (((1, 255, 0, 36), np.nan), ((0, 31, 2, 8), -np.inf)):
        f3[b, k, y, x] = val
        bad[b, y, :, x] = True
    return f2, f3, bad.reshape(c.N, c.W3)


def pooled_any(mask, levels):
    """[N, W] bool -> list per level: a pooled cell is marked where one of the two cells it pools is."""
    out = [mask]
    for _ in range(1, levels):
        w = out[-1].shape[1] // 2
        out.append(out[-1][:, 0:2 * w:2] | out[-1][:, 1:2 * w:2])
    return out
