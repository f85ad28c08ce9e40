"""bfloat16 side of the hand-off referee: rounding helpers, the acceptance band and the inputs of the bf16 PSMNet
volume and RAFT modulation kernels (handoff_kernels.hip, VPPX_DT_BF16).

TEST INFRASTRUCTURE ONLY.  Plain numpy, built on tests/_handoff_ref.py (imported, not edited).

The rule under test (include/vppx.h): a bf16 cell is widened to float32 (exact), multiplied by the float32 factor in
float32 and rounded to bf16 once, to nearest even.  The device cell is therefore rne(y) of some float32 y that the
float32 referee already bounds: |y - ref.out64| <= R.limit(ref, exp_ulps).  Rounding is monotone, so the cell lies in
[rne64(out64 - lim), rne64(out64 + lim)]: `band()`.  Nothing is added to that.

A bf16 value is held here either as the float32 of the same value (`bf16_rne_f32`, `widen`) or as its 16 bits
(uint16, `bits`): what is uploaded and compared bit for bit goes as bits, so that no NaN pattern passes a float unit.
"""
from types import SimpleNamespace

import numpy as np

import _handoff_ref as R

F32, F64 = np.float32, np.float64
BF16_MAX = F32(np.array([0x7F7F0000], np.uint32).view(F32)[0])      # (2 - 2^-7) * 2^127
SENTINEL16 = 0x7FA5                                                 # a signalling NaN pattern no kernel here produces


# ---------------------------------------------------------------------------------------------------
# rounding
# ---------------------------------------------------------------------------------------------------
def bf16_rne_f32(x32):
    """float32 -> the nearest bf16, ties to even, as float32; bit formula (NaN stays NaN, overflow gives infinity)."""
    x32 = np.ascontiguousarray(x32, F32)
    u = x32.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = np.where(nan, (u & 0xFFFF0000) | 0x00400000, r)
    return r.astype(np.uint32).view(F32).reshape(x32.shape)


def rne64(x):
    """float64 -> the nearest bf16 in ONE rounding, ties to even, as float32: 8 significant bits down to 2^-126, the
    subnormal grid of spacing 2^-133 below, infinity from (2 - 2^-8) * 2^127 on.  (Not through float32: that would
    be two roundings.)"""
    x = np.asarray(x, F64)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        _, e = np.frexp(x)                                       # |x| = m * 2^e, m in [0.5, 1)
        ulp = np.ldexp(1.0, np.maximum(e - 8, -133))
        r = np.rint(x / ulp) * ulp                               # both scalings are by a power of two: exact
        r = np.where(np.abs(r) > F64(BF16_MAX), np.copysign(np.inf, x), r)
        r = np.where(np.isfinite(x), r, x)
    out = r.astype(F32)
    assert np.array_equal(out.astype(F64), r, equal_nan=True)
    return out


def bits(x32):
    """The 16 bits of float32 values that are bf16 values."""
    u = np.ascontiguousarray(x32, F32).view(np.uint32)
    assert not (u & 0xFFFF).any(), "not on the bf16 grid"
    return (u >> 16).astype(np.uint16).reshape(np.shape(x32))


def widen(b16):
    """uint16 bf16 bits -> float32."""
    b16 = np.ascontiguousarray(b16, np.uint16)
    return (b16.astype(np.uint32) << 16).view(F32).reshape(b16.shape)


def band(ref, exp_ulps):
    """-> (lo, hi) float32 bf16 values per cell: where the single rounding of any float32 within R.limit() of
    ref.out64 can land."""
    lim = R.limit(ref, exp_ulps)
    with np.errstate(invalid="ignore", over="ignore"):
        return rne64(ref.out64 - lim), rne64(ref.out64 + lim)


def modulated_normal(ref):
    """Modulated cells (v != 0) right of the plane's cut whose exp is a normal float32 and whose value is finite and
    at least 2^-120: the cells a mutant is counted on."""
    normal, _, _ = R.cell_classes(ref)
    with np.errstate(invalid="ignore"):
        return normal & np.isfinite(ref.out64) & (np.abs(ref.out64) >= 2.0 ** -120)


def outside(got32, ref, exp_ulps):
    """Boolean mask of the modulated cells (v != 0) that miss: finite referee cells outside the band, NaN / infinite
    ones of another class.  got32: the bf16 cells as float32."""
    lo, hi = band(ref, exp_ulps)
    got = np.asarray(got32, F32)
    fin = np.isfinite(ref.out64)
    with np.errstate(invalid="ignore"):
        miss = fin & ~((got >= lo) & (got <= hi))
        miss |= ~fin & ~((np.isnan(got) & np.isnan(ref.out64)) | (got.astype(F64) == ref.out64))
    return miss & (ref.v != 0)


def two_valued(ref, exp_ulps):
    lo, hi = band(ref, exp_ulps)
    return lo != hi


# ---------------------------------------------------------------------------------------------------
# PSMNet inputs
# ---------------------------------------------------------------------------------------------------
# name: (B, C, H4, W4, rH, rW, maxdisp, kind), the format of R.PSM_CASES
NEW_PSM_CASES = {
    "w16_d24": (1, 1, 3, 16, 1, 2, 96, "directed"),    # D4 = 24 > W4 = 16: plane i cuts an 8-wide vector at every position
    "w72":     (1, 2, 30, 72, 3, 1, 16, "directed"),   # 9 * 30 = 270 vectors of 8: the wide route's second block
    "w12":     (1, 2, 4, 12, 0, 3, 24, "directed"),    # a multiple of 4 and not of 8: the narrow route
}
SPECIAL_PSM = ("overflow", "nan_feature")
PSM_NAMES = list(R.PSM_CASES) + list(NEW_PSM_CASES) + list(SPECIAL_PSM)
OVERFLOW_AT = dict(ch=0, i=2, y=1, x=5)                # left channel 0 of plane 2
NAN_AT = dict(ch=1, y=0, x=3)
# quiet NaN, signalling NaN, negative NaN with a payload, +inf, -inf, -0, the smallest and a negative subnormal
COPY_PATTERNS = np.array([0x7FC0, 0x7F81, 0xFFC1, 0x7F80, 0xFF80, 0x8000, 0x0001, 0x807F], np.uint16)


def _build(name):
    """R.psm_case for a shape R.PSM_CASES does not list.  The builder looks its shape up by name, so the entry is
    lent to the table for the length of the call and taken back: the table other files iterate over is unchanged."""
    assert name not in R.PSM_CASES
    R.PSM_CASES[name] = NEW_PSM_CASES[name]
    try:
        return R.psm_case(name)
    finally:
        del R.PSM_CASES[name]


def psm_case(name):
    """The float32 case of that name with both feature maps rounded to bf16 (held as float32)."""
    if name in SPECIAL_PSM:
        c = R.psm_case("w8_every")                               # v = 1 at every pixel
    else:
        c = _build(name) if name in NEW_PSM_CASES else R.psm_case(name)
    c.name = name
    c.fl, c.fr = bf16_rne_f32(c.fl), bf16_rne_f32(c.fr)
    if name == "overflow":                                       # hint exactly on plane i: the factor is 0 + 10 * exp(0) = 10
        o = OVERFLOW_AT
        c.fl[0, o["ch"], o["y"], o["x"]] = BF16_MAX
        c.hints[0, 0, R.nearest_indices(c.H, c.H4)[o["y"]], R.nearest_indices(c.W, c.W4)[o["x"]]] = 4.0 * o["i"]
    if name == "nan_feature":
        c.fl[0, NAN_AT["ch"], NAN_AT["y"], NAN_AT["x"]] = np.nan
    return c


def psm_ref(c):
    return R.psm_volume(c.fl, c.fr, c.maxdisp, c.hints, c.valid, rule="library")


def psm_plain_bits(flb, frb, maxdisp):
    """The un-modulated volume on the 16-bit patterns themselves: copies and 0x0000."""
    B, C, H4, W4 = flb.shape
    D4 = maxdisp // 4
    cost = np.zeros((B, 2 * C, D4, H4, W4), np.uint16)
    for i in range(min(D4, W4)):
        cost[:, :C, i, :, i:] = flb[:, :, :, i:]
        cost[:, C:, i, :, i:] = frb[:, :, :, :W4 - i]
    return cost


def left_of_cut(shape):
    """Boolean [.., D4, H4, W4] mask of the cells with x < i."""
    D4, W4 = shape[2], shape[4]
    return np.broadcast_to((np.arange(W4)[None, :] < np.arange(D4)[:, None])[None, None, :, None, :], shape)


def copy_case():
    """Hint-free features [1,2,3,16] as bits, every COPY_PATTERNS member in both maps, at columns that reach both
    halves of a vector.  maxdisp 24: planes 0..5."""
    rng = np.random.default_rng([53, 16])
    flb = bits(bf16_rne_f32(rng.standard_normal((1, 2, 3, 16)).astype(F32)))
    frb = bits(bf16_rne_f32(rng.standard_normal((1, 2, 3, 16)).astype(F32)))
    n = len(COPY_PATTERNS)
    flb[0, 0, 0, 4:4 + n], flb[0, 1, 2, 8:8 + n] = COPY_PATTERNS, COPY_PATTERNS[::-1]
    frb[0, 0, 1, 0:n], frb[0, 1, 1, 7:7 + n] = COPY_PATTERNS, COPY_PATTERNS
    return SimpleNamespace(flb=flb, frb=frb, maxdisp=24, B=1, C=2, H4=3, W4=16)


# ---------------------------------------------------------------------------------------------------
# RAFT inputs
# ---------------------------------------------------------------------------------------------------
def raft_case(name):
    c = R.raft_case(name)
    c.corr = bf16_rne_f32(c.corr)
    return c


def raft_ref(c):
    return R.raft_modulate(c.corr, c.hints, c.valid, rule="library")


def raft_sentinel_bits(c):
    """The volume's bits with every row of v == 0 replaced by NaN patterns: a kernel that rewrites such a row through
    a float unit, or through a 32-bit word that laps into it, changes them."""
    b = bits(c.corr).copy()
    rows = np.broadcast_to((c.v4 == 0)[..., None, None], b.shape)
    pat = np.where(np.arange(b.shape[-1]) % 2 == 0, SENTINEL16, 0xFF81).astype(np.uint16)
    return np.where(rows, np.broadcast_to(pat, b.shape), b)


# ---------------------------------------------------------------------------------------------------
# numpy emulations of wrong kernels (the CPU file shows that the band rejects them)
# ---------------------------------------------------------------------------------------------------
def mutant_truncate(ref):
    """The float32 product cut to its upper 16 bits instead of rounded."""
    return (np.ascontiguousarray(ref.out).view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)


def mutant_bf16_factor(ref):
    """The factor rounded to bf16 before the product."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        f = bf16_rne_f32(np.ascontiguousarray(ref.mod64.astype(F32)))
        out = bf16_rne_f32(np.ascontiguousarray(np.broadcast_to(ref.c, f.shape) * f))
    return np.where(ref.v == 0, np.broadcast_to(ref.c, out.shape), out)


def mutant_strict_cut(ref):
    """x > i in place of x >= i: the first live column of every plane is 0."""
    out = bf16_rne_f32(ref.out).copy()
    D4, W4 = out.shape[2], out.shape[4]
    for i in range(min(D4, W4)):
        out[:, :, i, :, i] = 0
    return out
