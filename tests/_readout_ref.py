"""Float64 referee, input builders and planted wrong implementations for the read-out kernels (readout_kernels.hip).

TEST INFRASTRUCTURE ONLY.  Plain numpy, no GPU: tests/test_readout_ref_cpu.py holds the referee to the arrays the
reference's own lines produced (tests/golden/readout_cases.npz) and to torch on the CPU, and asserts every coverage
claim the GPU file (tests/test_gpu_readout.py) relies on, on the very arrays the GPU file uploads.

What is float32 and what is float64.  The source indices and lerp weights of the trilinear upsampling are computed in
float32, operation by operation, as ATen computes them for align_corners = False and a given output size:
    scale = float(n_in) / float(n_out);  src = max(fma(scale, dst + 0.5f, -0.5f), 0)
    i0 = (int)src;  i1 = i0 + (i0 < n_in - 1);  l1 = src - i0;  l0 = 1 - l1
They are part of the function's definition, and tests/test_readout_ref_cpu.py pins them against torch: that is where
the fused multiply-add comes from.  ATen writes scale * (dst + 0.5) - 0.5, and both its vectorised CPU kernels and its
device kernels are compiled with contraction on, so the product is not rounded before the subtraction.  Everything
behind them is float64: the three lerps, the subtraction of the maximum, exp, both sums and the division.  bfloat16
inputs are widened exactly before any of this, so the bound holds on the widened values.

limit(): how far a float32 implementation may be from the value, in any association of the lerps and any order of the
sums.  U = 2^-24.  Write z_d for the exact logits (exact in the float32 weights), p_d for the exact softmax and
E = sum_d p_d * d for the value.  A float32 implementation has
  * logits z'_d with |z'_d - z_d| <= 8 U M, M the largest |tap| of the pixel: a logit is a sum of 8 products of three
    weights and a tap, the weights of an axis sum to 1 within U, and in any association a tap passes through at most
    three products and three sums (6 roundings; 8 leaves room for the weights' own sum);
  * weights e'_d = exp(fl(z'_d - m'))(1 + eps), m' its maximum.  Softmax does not change under a common shift, so
    against e_d = exp(z_d - zmax) the relative error of e'_d, beyond a factor common to all d, is at most
        rho_d = 2 (8 U M + U |z_d - zmax| + U |zmax|) + (2 exp_ulps + 3) U
    -- the error of z'_d and of m', each counted twice over (8 U M + U |zmax| bounds either), the rounding of the
    difference, exp within exp_ulps ulp (2 U each), and three roundings for a product with a reciprocal or a division
    of the weight before it is summed;
  * E' = sum p_d (1 + r_d) d / sum p_d (1 + r_d) with |r_d| <= rho_d:  E' - E = sum p_d r_d (d - E) to first order;
  * two float32 sums of D terms, each within D U of its terms' absolute sum in any order: 2 D U |E| for the two
    sums' common part and 2 D U sum p_d |d - E| for the spread, and U |E| for the division.
So
    limit = (2 sum_d p_d rho_d |d - E| + 2 D U |E| + 2 D U sum_d p_d |d - E| + U |E|) (1 + 2^-10)
the last factor being the project's usual allowance for second-order terms (tests/_handoff_ref.py).  No atol.
For RAFT's convex upsampling the logits are the mask cells themselves, 9 takes the place of D, v_k = f * flow_k (exact:
f is a power of two) the place of d, and sum_k p_k |v_k| the place of |E| in the summation term, since the v_k
have both signs.  The sign is exact.

Non-finite input follows the arithmetic: the referee computes with numpy's IEEE semantics (0 * inf = NaN,
inf - inf = NaN, exp(-inf) = 0) and a test compares the class of such a cell, not its distance.
"""
from types import SimpleNamespace

import numpy as np

from _referee import SECOND_ORDER, U, bf16_bits, bf16_widen, classes, compare  # noqa: F401

F32, F64 = np.float32, np.float64


# ---------------------------------------------------------------------------------------------------
# the source indices and weights
# ---------------------------------------------------------------------------------------------------
def lin_src(n_in, n_out, scale_dtype=F32, clamp=True, align_corners=False, fused=True):
    """-> (i0, i1 int64, l0, l1 float32) per output index.  The defaults are ATen's and the kernel's; the switches are
    the planted mistakes: a float64 scale, no clamp of src at 0, align_corners = True.  fused=False rounds the product
    before the subtraction, which is what an ATen built without fused multiply-add does."""
    dst = np.arange(n_out)
    if align_corners:
        sc = F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0)
        src = (sc * dst.astype(F32)).astype(F32)
    elif scale_dtype is F32 and fused:
        # one rounding: the product of two float32 numbers is exact in float64, and so is the difference wherever it is
        # not far below zero (where the clamp takes it)
        scale = F32(n_in) / F32(n_out)
        src = (F64(scale) * (dst.astype(F32) + F32(0.5)).astype(F64) - 0.5).astype(F32)
    elif scale_dtype is F32:
        scale = F32(n_in) / F32(n_out)
        src = (scale * (dst.astype(F32) + F32(0.5))).astype(F32) - F32(0.5)
        assert src.dtype == F32
    else:
        src = (F64(n_in) / F64(n_out)) * (dst.astype(F64) + 0.5) - 0.5
    if clamp:
        src = np.maximum(src, src.dtype.type(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)           # (int): towards zero
    i1 = i0 + (i0 < n_in - 1)
    l1 = (src - i0.astype(src.dtype)).astype(F32)
    l0 = F32(1) - l1
    return i0, i1, l0, l1


def f32_f64_tap_splits(limit=64, ratio=4):
    """Every (n_in, n_out, dst) with n_in < limit and n_out in (ratio * n_in - 3 .. ratio * n_in + 3) at which the
    float32 and the float64 scale pick a different first tap."""
    found = []
    for n_in in range(2, limit):
        for n_out in range(max(1, ratio * n_in - 3), ratio * n_in + 4):
            a, b = lin_src(n_in, n_out)[0], lin_src(n_in, n_out, F64)[0]
            found += [(n_in, n_out, int(d)) for d in np.flatnonzero(a != b)]
    return found


def f64_split_cost(n_in, n_out):
    """[1,n_in,1,1]: +80 on the plane at which the float32 and the float64 scale split (the last such), -80 on every other
    plane, and plane 0, which d = 0 and d = 1 read with weight 1, at 80 - ln 2: two peaks of equal mass, so that the value
    moves with the logit at the split, whose two readings differ by the rounding of src times the 160 between planes."""
    a, b = lin_src(n_in, n_out)[0], lin_src(n_in, n_out, F64)[0]
    d = np.flatnonzero(a != b)
    assert d.size, (n_in, n_out)
    m = int(max(a[d[-1]], b[d[-1]]))
    assert 1 < m < n_in - 1
    cost = np.full((1, n_in, 1, 1), -80.0, F32)
    cost[0, m] = 80.0
    cost[0, 0] = F32(80.0 - np.log(2.0))
    return cost


def window(H, W, crop):
    """test.py's _pad list [left, right, top, bottom] -> (top, left, Hout, Wout)."""
    if crop is None:
        return 0, 0, H, W
    left, right, top, bottom = crop
    return top, left, H - top - bottom, W - left - right


# ---------------------------------------------------------------------------------------------------
# PSMNet: upsample + softmax + regression
# ---------------------------------------------------------------------------------------------------
def _softmax_regress(z, values, spread_terms, M, exp_ulps):
    """z [..., n] float64 logits, values [..., n] (or [n]) float64 -> (E, limit) over the last axis."""
    n = z.shape[-1]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        zmax = np.max(z, axis=-1, keepdims=True)                     # NaN if any logit is NaN, as the sums will be
        a = z - zmax
        e = np.exp(a)
        p = e / np.sum(e, axis=-1, keepdims=True)
        E = np.sum(p * values, axis=-1)
        dev = np.abs(values - E[..., None])
        rho = 2 * (8 * U * M[..., None] + U * np.abs(a) + U * np.abs(zmax)) + (2 * exp_ulps + 3) * U
        rho = np.where(p > 0, rho, 0.0)                              # a logit of -inf has weight exactly 0 in any implementation
        mag = np.abs(E) if spread_terms is None else np.sum(p * np.abs(values), axis=-1)
        lim = 2 * np.sum(p * rho * dev, axis=-1) + 2 * n * U * mag + 2 * n * U * np.sum(p * dev, axis=-1) + U * np.abs(E)
    return E, lim * SECOND_ORDER, p


def psm_logits(cost, D, H, W, crop=None, **how):
    """cost [B,D4,H4,W4] float32 -> (z [B,Hout,Wout,D] float64, M [B,Hout,Wout]): the exact trilinear logits of the
    window's pixels in the float32 weights, and the largest |tap| of each pixel.  `how` goes to lin_src."""
    cost = np.asarray(cost, F32)
    B, D4, H4, W4 = cost.shape
    top, left, Ho, Wo = window(H, W, crop)
    c = cost.astype(F64)
    y0, y1, ly0, ly1 = (a[top:top + Ho] for a in lin_src(H4, H, **how))
    x0, x1, lx0, lx1 = (a[left:left + Wo] for a in lin_src(W4, W, **how))
    d0, d1, ld0, ld1 = lin_src(D4, D, **how)
    with np.errstate(invalid="ignore", over="ignore"):
        absc = np.abs(c)
        M = None
        rows = []
        for yi, ly in ((y0, ly0), (y1, ly1)):
            r = c[:, :, yi, :]                                                               # [B,D4,Ho,W4]
            ra = absc[:, :, yi, :]
            m = np.maximum(ra[..., x0], ra[..., x1])
            m = np.where(np.isfinite(m), m, 0.0).max(axis=1)             # a tap of -inf bounds no rounding: its logits have weight 0
            M = m if M is None else np.maximum(M, m)
            rows.append((r[..., x0] * lx0.astype(F64) + r[..., x1] * lx1.astype(F64)) * ly.astype(F64)[None, None, :, None])
        p = np.moveaxis(rows[0] + rows[1], 1, -1)                                             # [B,Ho,Wo,D4]
        z = p[..., d0] * ld0.astype(F64) + p[..., d1] * ld1.astype(F64)
    return z, M


def psm_readout(cost, D, H, W, crop=None, exp_ulps=1.0, **how):
    """-> namespace(value float64 [B,Hout,Wout], limit, z, p, M)."""
    z, M = psm_logits(cost, D, H, W, crop, **how)
    E, lim, p = _softmax_regress(z, np.arange(D, dtype=F64), None, M, exp_ulps)
    return SimpleNamespace(value=E, limit=lim, z=z, p=p, M=M)


def psm_softmax_first(cost, D, H, W):
    """Planted: softmax over the D4 planes, the probabilities upsampled, renormalised and regressed."""
    cost = np.asarray(cost, F64)
    e = np.exp(cost - cost.max(axis=1, keepdims=True))
    prob = (e / e.sum(axis=1, keepdims=True)).astype(F32)
    z, _ = psm_logits(prob, D, H, W)
    z = z / z.sum(axis=-1, keepdims=True)
    return (z * np.arange(D, dtype=F64)).sum(axis=-1)


# ---------------------------------------------------------------------------------------------------
# RAFT-Stereo: convex upsampling
# ---------------------------------------------------------------------------------------------------
def raft_taps(flow, f, pad="zero", order="ky_kx"):
    """flow [B,C,H4,W4] -> v [B,C,H4,W4,9] float64: f * flow at the 3x3 neighbours, k = 3*ky + kx."""
    flow = np.asarray(flow, F32).astype(F64)
    B, C, H4, W4 = flow.shape
    padded = np.pad(flow, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="constant" if pad == "zero" else "edge")
    v = np.empty((B, C, H4, W4, 9), F64)
    for ky in range(3):
        for kx in range(3):
            k = 3 * ky + kx if order == "ky_kx" else 3 * kx + ky
            v[..., k] = f * padded[:, :, ky:ky + H4, kx:kx + W4]
    return v


def raft_upsample(flow, mask, f, negate=False, channels=None, crop=None, exp_ulps=1.0, pad="zero", order="ky_kx", layout="k_major"):
    """-> namespace(value float64 [B,C,Hout,Wout], limit, z [B,f*H4,f*W4,9], p).  pad / order / layout are the planted
    mistakes: replicate padding, k = 3*kx + ky, the mask channel read as (i*f + j)*9 + k."""
    flow, mask = np.asarray(flow, F32), np.asarray(mask, F32)
    B, C, H4, W4 = flow.shape
    C = C if channels is None else channels
    assert mask.shape == (B, 9 * f * f, H4, W4)
    m = mask.astype(F64)
    m = m.reshape(B, 9, f, f, H4, W4) if layout == "k_major" else np.moveaxis(m.reshape(B, f, f, 9, H4, W4), 3, 1)
    z = m.transpose(0, 4, 2, 5, 3, 1).reshape(B, f * H4, f * W4, 9)                       # [b, f*y+i, f*x+j, k]
    v = raft_taps(flow[:, :C], f, pad, order)                                                # [B,C,H4,W4,9]
    v = np.repeat(np.repeat(v, f, axis=2), f, axis=3)                                        # [B,C,fH4,fW4,9]
    top, left, Ho, Wo = window(f * H4, f * W4, crop)
    z = z[:, top:top + Ho, left:left + Wo]
    v = v[:, :, top:top + Ho, left:left + Wo]
    with np.errstate(invalid="ignore"):
        M = np.where(np.isfinite(z), np.abs(z), 0.0).max(axis=-1)
    E, lim, p = _softmax_regress(z[:, None], v, "abs", M[:, None], exp_ulps)
    if negate:
        E = -E
    return SimpleNamespace(value=E, limit=lim, z=z, p=p)


# ---------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_readout.py (the CPU file asserts what each is said to reach)
# ---------------------------------------------------------------------------------------------------
#            name        B  D4 H4 W4   D    H    W   crop          dtype
PSM_CASES = {
    "one_plane": (1, 1, 1, 1, 4, 4, 4, None, "float32"),               # i1 clamps on every axis
    "pm80":      (1, 2, 1, 1, 8, 4, 4, None, "float32"),               # logits of +80 and -80
    "x4":        (2, 12, 5, 7, 48, 20, 28, None, "float32"),           # exact x4, two frames that differ
    "general":   (1, 12, 5, 7, 50, 23, 30, None, "float32"),           # a general scale on all three axes
    "d192_wide": (1, 48, 3, 66, 192, 12, 264, None, "float32"),        # D = 192, a row wider than one wave
    "crop":      (1, 12, 9, 17, 48, 36, 68, [2, 2, 1, 3], "float32"),
    "nonfinite": (1, 12, 5, 7, 48, 20, 28, None, "float32"),           # NaN, +inf and -inf planted under three pixels
    "x4_bf16":   (2, 12, 5, 7, 48, 20, 28, None, "bfloat16"),
    "f64_split": (1, 106, 1, 1, 422, 1, 1, None, "float32"),           # a float64 scale picks another tap at d = 316; 128 lanes per workgroup
    "many_planes": (1, 200, 2, 3, 50, 5, 70, None, "float32"),         # D < D4; 64 lanes per workgroup
}
PSM_NONFINITE_AT = {"nan": (3, 1, 1), "pinf": (6, 3, 5), "ninf": (9, 1, 5)}      # (plane, row, column) of the planted cells


def psm_case(name):
    B, D4, H4, W4, D, H, W, crop, dtype = PSM_CASES[name]
    rng = np.random.default_rng([2201, B, D4, H4, W4, D])
    cost = (rng.standard_normal((B, D4, H4, W4)) * 3).astype(F32)
    if name == "pm80":
        cost[0, :, 0, 0] = (80.0, -80.0)
    if name in ("x4", "x4_bf16", "general", "crop", "d192_wide"):
        cost[0, :, 0, 0] = 1.25                                         # a pixel where all logits are equal
        cost[0, :, -1, -1] = -6.0
        cost[0, D4 // 2, -1, -1], cost[0, D4 // 2 + 1, -1, -1] = 80.0, 40.0     # a pixel with one dominant logit
        cost[0, :, 0, -1] = np.where(np.arange(D4) % 2 == 0, 80.0, -80.0)     # logits of +-80 at pixel (0, W-1), steep between planes
    if name == "f64_split":
        cost = f64_split_cost(D4, D)
    if name == "nonfinite":
        for key, val in (("nan", np.nan), ("pinf", np.inf), ("ninf", -np.inf)):
            cost[(0,) + PSM_NONFINITE_AT[key]] = val
    if dtype == "bfloat16":
        cost = bf16_widen(bf16_bits(cost))
    return SimpleNamespace(name=name, cost=cost, B=B, D4=D4, H4=H4, W4=W4, D=D, H=H, W=W, crop=crop, dtype=dtype)


#             name        B  C  H4 W4  f  negate channels crop           dtype
RAFT_CASES = {
    "all_padding": (1, 1, 1, 1, 4, False, None, None, "float32"),      # every neighbour is padding
    "two_by_two":  (2, 2, 3, 5, 4, False, None, None, "float32"),      # two frames, two channels
    "wide":        (1, 1, 2, 65, 4, False, None, None, "float32"),     # a row wider than one wave
    "f8":          (1, 1, 3, 5, 8, False, None, None, "float32"),
    "f2":          (1, 2, 3, 5, 2, False, None, None, "float32"),
    "f1":          (1, 1, 3, 5, 1, False, None, None, "float32"),
    "test_py":     (1, 2, 6, 9, 4, True, 1, [3, 2, 1, 2], "float32"),  # test.py:237-245 in one call
    "cropped_f8":  (1, 1, 3, 5, 8, False, None, [4, 4, 3, 2], "float32"),   # half a group of 8 lies outside the window
    "two_bf16":    (2, 2, 3, 5, 4, False, None, None, "bfloat16"),
}


def raft_case(name):
    B, C, H4, W4, f, negate, channels, crop, dtype = RAFT_CASES[name]
    rng = np.random.default_rng([2202, B, C, H4, W4, f])
    flow = (rng.standard_normal((B, C, H4, W4)) * 12).astype(F32)
    mask = (rng.standard_normal((B, 9 * f * f, H4, W4)) * 2.5).astype(F32)
    if H4 * W4 > 1:
        mask[0, :, 0, 0] = 0.5                                          # all logits equal
        mask[0, :, -1, -1] = -4.0
        mask[0, 4 * f * f:5 * f * f, -1, -1] = 40.0                     # one dominant logit: the centre tap
        mask[0, :, 0, 1] = np.where((np.arange(9 * f * f) // (f * f)) % 2 == 0, 80.0, -80.0)
    if dtype == "bfloat16":
        flow, mask = bf16_widen(bf16_bits(flow)), bf16_widen(bf16_bits(mask))
    return SimpleNamespace(name=name, flow=flow, mask=mask, B=B, C=C, H4=H4, W4=W4, f=f, negate=negate, channels=channels, crop=crop,
                           dtype=dtype)
