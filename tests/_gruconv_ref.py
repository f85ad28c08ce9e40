"""Float64 referee, input builders and planted wrong implementations for the 3x3 convolution on the matrix cores and the
ConvGRU made of it (conv_kernels.hip): include/vppx.h has the arithmetic.

TEST INFRASTRUCTURE ONLY.  Plain numpy, no GPU: tests/test_gruconv_ref_cpu.py holds the referee to the arrays the
reference's own ConvGRU.forward produced (tests/golden/gruconv_cases.npz) and shows on the very arrays the GPU file
(tests/test_gpu_gruconv.py) uploads that every planted mistake leaves the limit.

The convolution.  value = bias + the sum of K = 9 Cin products w_k x_k in float64 on the float32 (or widened bfloat16)
cells and the float32 weights -- for bfloat16 storage the weights rounded to bfloat16 once, which is what the packing does, so
that every product is exact in float32.  limit, as tests/_motion_ref._sum derives it: a float32 evaluation in any order
rounds every product once (exactly, for bfloat16 operands) and every one of the K additions once, so a term passes through at
most K + 1 roundings of relative error U = 2^-24 on partial results of at most |bias| + sum |w_k x_k|:
        limit = (K + 1) U (|bias| + sum_k |w_k x_k|) (1 + 2^-10)      (+ T per product that is not zero and below T = 2^-126,
                                                                         + T for a result below T)
There is no atol.  A padding cell and a padding row of K contribute exact zeros.  An input that carries a bound of its own
(r*h on its way into convq, the hidden state of the call before) adds sum_k |w_k| bound_k.

The gates are tests/_gru_ref.py's: sigmoid() and tanh() with the pre-activation's bound dv = the convolution's limit plus
the rounding of `+ c`, and the products and sums of reset() / update() with the same terms those carry, here with the bounds
of z and h passed in, because z reaches the q call through memory and h may be the result of the call before.

bfloat16 storage: a result is the float32 result rounded once: band() of tests/_referee.py for the cell under test, and
stored(), half a unit of the 8-bit significand, for a cell that is read back (z, r*h, hx, the hidden state).
"""
import os
from types import SimpleNamespace

import numpy as np

import _gru_ref as G
from _referee import SECOND_ORDER, TINY, U, _ns, _und, band, bf16_bits, bf16_widen, classes, compare, compare_bf16, misses, to_bf16  # noqa: F401

F32, F64 = np.float32, np.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gruconv_cases.npz")
EXP_ULPS = 1.0
PLANTED = ("flipped", "replicate", "transposed", "swapped", "no_bias", "zr_swapped", "h_into_q", "z_complement")
CONV_KW = {"flipped": dict(flipped=True), "replicate": dict(pad="replicate"), "transposed": dict(transposed=True),
           "swapped": dict(swapped=True), "no_bias": dict(use_bias=False)}


def _relu(v):
    with np.errstate(invalid="ignore"):
        return np.where(v < 0, 0.0, v)                  # a NaN stays NaN


def stored(ns, dtype):
    """A result written to memory and read back: exact in float32, rounded to bfloat16 once otherwise (8 bits of significand:
    half a unit in the last place is at most 2^-8 of the float32 result, which is at most |value| + limit)."""
    if dtype != "bfloat16":
        return ns
    with np.errstate(invalid="ignore"):
        a = np.abs(ns.value) + ns.limit
        return _ns(ns.value, ns.limit + np.where(np.isfinite(a), 2.0 ** -8 * a + _und(ns.value), 0.0))


def weights_of(w, dtype):
    return to_bf16(np.asarray(w, F32)) if dtype == "bfloat16" else np.asarray(w, F32)


def conv3x3(x0, x1, w, bias, dtype="float32", x0_limit=None, x1_limit=None, relu=False, flipped=False, pad="zero", transposed=False,
            swapped=False, use_bias=True):
    """x0 [B,C0,H,W], x1 [B,C1,H,W] or None, w [Cout,C0+C1,3,3] float32, bias [Cout] or None -> namespace(value, limit)
    [B,Cout,H,W].  Planted: flipped (the kernel turned by 180 degrees), pad="replicate", transposed (w[c][m] where w[m][c]
    belongs; Cin == Cout), swapped (cat([x1, x0])), use_bias=False."""
    parts = [np.asarray(x0, F64)] + ([] if x1 is None else [np.asarray(x1, F64)])
    lims = [np.zeros_like(parts[0]) if x0_limit is None else x0_limit]
    if x1 is not None:
        lims.append(np.zeros_like(parts[1]) if x1_limit is None else x1_limit)
    if swapped:
        parts, lims = parts[::-1], lims[::-1]
    x, xl = np.concatenate(parts, axis=1), np.concatenate(lims, axis=1)
    B, Cin, H, W = x.shape
    w = weights_of(w, dtype).astype(F64)
    if transposed:
        w = w.transpose(1, 0, 2, 3)
    if flipped:
        w = w[:, :, ::-1, ::-1]
    M = w.shape[0]
    assert w.shape == (M, Cin, 3, 3), (w.shape, x.shape)
    p4 = ((0, 0), (0, 0), (1, 1), (1, 1))
    xp = np.pad(x, p4, mode="edge" if pad == "replicate" else "constant")
    lp = np.pad(xl, p4)
    b = np.zeros(M) if bias is None or not use_bias else np.asarray(bias, F64)
    val = np.zeros((B, M, H, W)) + b[None, :, None, None]
    mag, und, prop = np.abs(val), np.zeros((B, M, H, W)), np.zeros((B, M, H, W))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for dy in range(3):
            for dx in range(3):
                win, wk = xp[:, :, dy:dy + H, dx:dx + W], w[:, :, dy, dx]
                for f in range(B):                      # [M, Cin, H, W] products of one frame and tap
                    p = wk[:, :, None, None] * win[f][None]
                    val[f] += p.sum(axis=1)
                    mag[f] += np.abs(p).sum(axis=1)
                    und[f] += ((p != 0) & (np.abs(p) < TINY)).sum(axis=1) * TINY
                prop += np.einsum("mc,bchw->bmhw", np.abs(wk), lp[:, :, dy:dy + H, dx:dx + W])
        lim = ((9 * Cin + 1) * U * mag + und + _und(val)) * SECOND_ORDER + prop
    return _ns(_relu(val) if relu else val, lim)


def _pre(a, c):
    """(a + c, its bound): a is a convolution's namespace, c exact."""
    with np.errstate(invalid="ignore"):
        v = a.value + np.asarray(c, F64)
        return v, a.limit + U * np.abs(v)


def zr(x0, x1, wz, bz, wr, br, cz, cr, h, dtype="float32", h_limit=None, x0_limit=None, x1_limit=None, zr_swapped=False, **conv_kw):
    """-> (z, rh), each namespace(value, limit) [B,C,H,W].  Planted: zr_swapped (convr's rows where convz's belong in the pack
    and the reverse), and conv3x3's."""
    if zr_swapped:
        wz, bz, wr, br = wr, br, wz, bz
    kw = dict(dtype=dtype, x0_limit=x0_limit, x1_limit=x1_limit, **conv_kw)
    az, ar = conv3x3(x0, x1, wz, bz, **kw), conv3x3(x0, x1, wr, br, **kw)
    h = np.asarray(h, F64)
    hl = np.zeros_like(h) if h_limit is None else h_limit
    z, lz = G.sigmoid(*_pre(az, cz), EXP_ULPS)
    r, lr = G.sigmoid(*_pre(ar, cr), EXP_ULPS)
    with np.errstate(invalid="ignore"):
        v = r * h
        return _ns(z, lz * SECOND_ORDER), _ns(v, (np.abs(h) * lr + r * hl + U * np.abs(v) + _und(v)) * SECOND_ORDER)


def q(x0, x1, wq, bq, cq, z, h, dtype="float32", z_limit=None, h_limit=None, x0_limit=None, x1_limit=None, z_complement=False, **conv_kw):
    """-> namespace(value = (1 - z) h + z tanh(convq + cq), limit).  z is an input (the buffer the zr call wrote).  Planted:
    z_complement gives z h + (1 - z) q."""
    aq = conv3x3(x0, x1, wq, bq, dtype=dtype, x0_limit=x0_limit, x1_limit=x1_limit, **conv_kw)
    qv, lq = G.tanh(*_pre(aq, cq), EXP_ULPS)
    z, h = np.asarray(z, F64), np.asarray(h, F64)
    lz = np.zeros_like(z) if z_limit is None else z_limit
    hl = np.zeros_like(h) if h_limit is None else h_limit
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        zc = 1.0 - z                                    # z is a float32 (bfloat16) cell in [0, 1]: exact in float64
        if z_complement:
            z, zc = zc, z
        p1, p2 = zc * h, z * qv
        v = p1 + p2
        lim = (np.abs(h) + np.abs(qv)) * lz + z * lq + zc * hl + U * (2 * np.abs(p1) + np.abs(p2) + np.abs(v)) + _und(p1) + _und(p2) + _und(v)
    return _ns(v, lim * SECOND_ORDER)


def gru(h, ctx, xs, W, dtype="float32", h_limit=None, xs_limit=None, h_into_q=False, zr_swapped=False, z_complement=False, **conv_kw):
    """One ConvGRU.forward as assemble + zr + q run it: h [B,C,H,W], ctx [B,3C,H,W] = [cz|cr|cq], xs the list of x sources
    [B,Ci,H,W] (already at h's size), W = dict(convz_weight, convz_bias, ...) -> namespace(value, limit, z, rh).  With bfloat16
    storage z and r*h pass through memory.  Planted: h_into_q (convq reads cat([h, x])), and those of zr, q and conv3x3."""
    C = h.shape[1]
    cz, cr, cq = ctx[:, :C], ctx[:, C:2 * C], ctx[:, 2 * C:]
    x = np.concatenate([np.asarray(a, F64) for a in xs], axis=1)
    xl = np.zeros_like(x) if xs_limit is None else np.concatenate(xs_limit, axis=1)
    hl = np.zeros(h.shape) if h_limit is None else h_limit
    z, rh = zr(h, x, W["convz_weight"], W["convz_bias"], W["convr_weight"], W["convr_bias"], cz, cr, h, dtype, h_limit=hl, x0_limit=hl,
               x1_limit=xl, zr_swapped=zr_swapped, **conv_kw)
    z_call, rh_call = z, rh                              # what the zr call itself is held to
    z, rh = stored(z, dtype), stored(rh, dtype)
    first = _ns(np.asarray(h, F64), hl) if h_into_q else rh
    out = q(first.value, x, W["convq_weight"], W["convq_bias"], cq, z.value, h, dtype, z_limit=z.limit, h_limit=hl, x0_limit=first.limit,
            x1_limit=xl, z_complement=z_complement, **conv_kw)
    return _ns(out.value, out.limit, z=z_call, rh=rh_call)


# ---------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_gruconv.py
# ---------------------------------------------------------------------------------------------------
# name: (B, C0, C1, Cout, H, W)
CASES = {
    "1x1":   (2, 16, 0, 16, 1, 1),          # every tap but the centre is outside the map
    "1x9":   (1, 16, 0, 16, 1, 9),          # ... on a row
    "9x1":   (1, 16, 0, 16, 9, 1),          # ... on a column
    "odd":   (3, 16, 16, 32, 19, 37),       # odd sizes, a plane that is not a whole number of 16 bytes, two sources
    "tiles": (2, 32, 0, 16, 40, 72),        # five tiles of 8 rows, three of 32 columns (the last one 8 wide), two frames
    "deep_zr": (1, 128, 256, 256, 6, 10),   # gru08's zr: 12 (bfloat16) / 24 (float32) chunks of K, four blocks of 64 channels
    "deep_q":  (1, 128, 128, 128, 6, 10),   # gru32's q
}
GRU_CASES = {"odd": (3, 16, 16, 19, 37), "deep": (1, 128, 128, 6, 10)}        # name: (B, C = C0, C1, H, W); zr and q on the same hx
# (tensor, b, c, y, x, value) planted into the context of a GRU case: gate inputs that reach +-inf
GATE_PLANTS = (("cz", 0, 0, 0, 1, np.inf), ("cz", 0, 1, 1, 2, -np.inf), ("cr", 0, 0, 2, 3, np.inf), ("cr", 0, 2, 3, 4, -np.inf),
               ("cq", 0, 0, 4, 1, np.inf), ("cq", 0, 1, 4, 2, -np.inf), ("cz", 0, 3, 5, 9, 90.0), ("cq", 0, 3, 5, 8, -90.0))


def _cells(rng, shape, dtype, scale=1.0):
    a = (rng.standard_normal(shape) * scale).astype(F32)
    return to_bf16(a) if dtype == "bfloat16" else a


def case(name, dtype="float32"):
    """-> namespace(x0, x1 or None, w [Cout,Cin,3,3], bias): weights of about 1.5 / sqrt(K), so that sums are of order 1."""
    B, C0, C1, Cout, H, W = CASES[name]
    rng = np.random.default_rng([5801, B, C0, C1, Cout, H, W])
    K = 9 * (C0 + C1)
    return SimpleNamespace(name=name, B=B, C0=C0, C1=C1, Cout=Cout, H=H, W=W, dtype=dtype, x0=_cells(rng, (B, C0, H, W), dtype),
                           x1=_cells(rng, (B, C1, H, W), dtype) if C1 else None,
                           w=(rng.standard_normal((Cout, C0 + C1, 3, 3)) * (1.5 / np.sqrt(K))).astype(F32),
                           bias=(rng.standard_normal(Cout) * 0.5).astype(F32))


def case_ref(c, **kw):
    return conv3x3(c.x0, c.x1, c.w, c.bias, dtype=c.dtype, **kw)


def gru_case(name, dtype="float32"):
    """-> namespace(h, x [B,C1,H,W], ctx [B,3C,H,W], weights): a hidden state in (-1, 1), weights that move the gates, and a context
    with the cells of GATE_PLANTS."""
    B, C, C1, H, W = GRU_CASES[name]
    rng = np.random.default_rng([5802, B, C, C1, H, W])
    K = 9 * (C + C1)
    Wt = {}
    for cv in ("convz", "convr", "convq"):
        Wt[f"{cv}_weight"] = (rng.standard_normal((C, C + C1, 3, 3)) * (1.5 / np.sqrt(K))).astype(F32)
        Wt[f"{cv}_bias"] = (rng.standard_normal(C) * 0.5).astype(F32)
    h = np.tanh(rng.standard_normal((B, C, H, W)) * 1.2).astype(F32)
    h = to_bf16(h) if dtype == "bfloat16" else h
    ctx = _cells(rng, (B, 3 * C, H, W), dtype)
    for key, b, ch, y, x, val in GATE_PLANTS:
        ctx[b, {"cz": 0, "cr": C, "cq": 2 * C}[key] + ch, y % H, x % W] = val
    return SimpleNamespace(name=name, B=B, C=C, C1=C1, H=H, W=W, dtype=dtype, h=h, x=_cells(rng, (B, C1, H, W), dtype), ctx=ctx, weights=Wt)


def gru_case_ref(c, **kw):
    return gru(c.h, c.ctx, [c.x], c.weights, c.dtype, **kw)


# ---------------------------------------------------------------------------------------------------
# the recording (tests/golden/gruconv_cases.npz)
# ---------------------------------------------------------------------------------------------------
RECORDED = {"a": 2, "b": 1}                      # name: x sources


def load_recording():
    return np.load(GOLDEN)


def recorded_case(g, name):
    """-> (h0, ctx, [x sources], W)"""
    W = {f"{cv}_{p}": g[f"{name}_{cv}_{p}"] for cv in ("convz", "convr", "convq") for p in ("weight", "bias")}
    return g[f"{name}_h0"], g[f"{name}_ctx"], [g[f"{name}_x{k}"] for k in range(RECORDED[name])], W


def recorded_ref(g, name, dtype="float32", **kw):
    """The referee on the recording's inputs, two consecutive calls -> [call 1, call 2] as gru() returns them.  For bfloat16
    the inputs are rounded first (the caller uploads those) and the hidden state passes through memory between the calls."""
    h0, ctx, xs, W = recorded_case(g, name)
    if dtype == "bfloat16":
        h0, ctx, xs = to_bf16(h0), to_bf16(ctx), [to_bf16(a) for a in xs]
    one = gru(h0, ctx, xs, W, dtype, **kw)
    mid = stored(one, dtype)
    two = gru(mid.value, ctx, xs, W, dtype, h_limit=mid.limit, **kw)
    return [one, two]
