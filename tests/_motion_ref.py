"""Float64 referee, input builders and planted wrong implementations for the motion encoder's front
(motion_kernels.hip): cor1 = relu(convc1(lookup)) and flo1 = relu(convf1(flow)); include/vppx.h has the arithmetic.

TEST INFRASTRUCTURE ONLY.  Plain numpy, no GPU: tests/test_motion_ref_cpu.py holds the referee to the arrays the
reference's own lines produced (tests/golden/motion_cases.npz) and shows on the very arrays the GPU file
(tests/test_gpu_motion.py) uploads that every planted mistake leaves the limit.

What is float32 and what is float64.  The taps are `_corr_ref.lookup`'s: float32, operation by operation, bit for bit
what the lookup call stores.  The two sums are float64 on those float32 taps, the float32 flow and the float32 weights.

limit(): how far a float32 evaluation of a sum of K + 1 terms (K products and the bias), in any order, may lie from the
value.  Every product w_k t_k is rounded once and every one of the K additions once (a fused multiply-add rounds less),
so a term passes through at most K + 1 roundings of relative error U = 2^-24 each, on partial results that are at most
|bias| + sum |w_k t_k| in magnitude:
        limit = (K + 1) U (|bias| + sum_k |w_k t_k|) (1 + 2^-10)
The factor 1 + 2^-10 is the project's allowance for second-order terms (tests/_handoff_ref.py); (K + 1) U is at most
6e-6 here.  There is no atol.  Below the smallest normal float32, T = 2^-126, the format keeps no relative precision: a
product that is not zero and below T, and a result below T, carry T each instead.  ReLU is monotone and 1-Lipschitz, so
relu(got) lies within the same limit of relu(value).  A padding cell of the flow and a padding row of K contribute exact
zeros.

bfloat16 outputs: the float32 result is rounded once and rounding is monotone, so a cell lies in
[rne(value - limit), rne(value + limit)]: band() of tests/_referee.py.

Non-finite input follows the arithmetic (numpy's IEEE semantics) and a test compares the class of such a cell.
"""
import os
from types import SimpleNamespace

import numpy as np

import _corr_ref as C
import _handoff_bf16_ref as BR
from _referee import SECOND_ORDER, TINY, U, _ns, band, classes, compare, compare_bf16, misses, to_bf16  # noqa: F401

F32, F64 = np.float32, np.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "motion_cases.npz")
PLANTED = ("tap_order", "flipped", "replicate", "flow_swapped", "no_bias", "no_relu", "taps_bf16")


def _relu(v):
    with np.errstate(invalid="ignore"):
        return np.where(v < 0, 0.0, v)                  # a NaN stays NaN


def _sum(terms_of, n_terms, bias, shape):
    """value and limit of bias + the sum of n_terms products; terms_of(k) -> (w [M], t [cells]) of term k."""
    val = np.zeros(shape) + (0.0 if bias is None else bias.astype(F64)[:, None])
    mag = np.abs(val)
    und = np.zeros(shape)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for k in range(n_terms):
            w, t = terms_of(k)
            p = w.astype(F64)[:, None] * t.astype(F64)[None, :]
            val, mag = val + p, mag + np.abs(p)
            und += np.where((p != 0) & (np.abs(p) < TINY), TINY, 0.0)
        lim = ((n_terms + 1) * U * mag + und + np.where(np.abs(val) < TINY, TINY, 0.0)) * SECOND_ORDER
    return val, lim


def taps_of(pyr, coords, radius, tap_order="level_major", taps_bf16=False):
    """-> [N, K] float32, k = i * (2r+1) + t.  Planted: tap_order="t_major" lays them k = t * levels + i; taps_bf16
    rounds them to bfloat16."""
    taps = C.lookup(C.widened(pyr), coords, radius)
    L, T = len(pyr), 2 * radius + 1
    if tap_order == "t_major":
        taps = np.ascontiguousarray(taps.reshape(-1, L, T).transpose(0, 2, 1).reshape(-1, L * T))
    if taps_bf16:
        taps = BR.bf16_rne_f32(taps)
    return taps


def front(pyr, coords, flow, wc, bias_c, wf, bias_f, radius, tap_order="level_major", flipped=False, pad="zero", flow_swapped=False,
          use_bias=True, relu=True, taps_bf16=False):
    """pyr: list of [N, Wi] levels (float32 cells or bfloat16 bits), coords [B,H4,W2] float32, flow [B,2,H4,W2] float32,
    wc [Cc,K(,1,1)], wf [Cf,2,ks,ks], biases [C] or None -> (cor1, flo1), each namespace(value, limit) [B,C,H4,W2].
    Planted: tap_order, taps_bf16 (taps_of); flipped: the ks x ks kernel turned by 180 degrees (a convolution in the
    mathematical sense); pad="replicate"; flow_swapped: the flow's channels exchanged; use_bias=False; relu=False."""
    B, H4, W2 = coords.shape
    N = B * H4 * W2
    taps = taps_of(pyr, coords, radius, tap_order, taps_bf16)
    K = taps.shape[1]
    wc = np.asarray(wc, F32).reshape(-1, K)
    Cc, Cf, ks = wc.shape[0], wf.shape[0], wf.shape[2]
    if not use_bias:
        bias_c = bias_f = None
    vc, lc = _sum(lambda k: (wc[:, k], taps[:, k]), K, bias_c, (Cc, N))
    p = ks // 2
    wf = np.asarray(wf, F32)
    if flipped:
        wf = wf[:, :, ::-1, ::-1]
    fl = np.asarray(flow, F32)
    if flow_swapped:
        fl = fl[:, ::-1]
    fp = np.pad(fl, ((0, 0), (0, 0), (p, p), (p, p)), mode="edge" if pad == "replicate" else "constant")

    def term(k):
        c, dy, dx = k // (ks * ks), (k % (ks * ks)) // ks, k % ks
        return wf[:, c, dy, dx], fp[:, c, dy:dy + H4, dx:dx + W2].reshape(N)

    vf, lf = _sum(term, 2 * ks * ks, bias_f, (Cf, N))
    out = []
    for v, l, Cn in ((vc, lc, Cc), (vf, lf, Cf)):
        v = v.reshape(Cn, B, H4, W2).transpose(1, 0, 2, 3)
        l = l.reshape(Cn, B, H4, W2).transpose(1, 0, 2, 3)
        out.append(_ns(np.ascontiguousarray(_relu(v) if relu else v), np.ascontiguousarray(l)))
    return out[0], out[1]


PLANTED_KW = {"tap_order": dict(tap_order="t_major"), "flipped": dict(flipped=True), "replicate": dict(pad="replicate"),
              "flow_swapped": dict(flow_swapped=True), "no_bias": dict(use_bias=False), "no_relu": dict(relu=False),
              "taps_bf16": dict(taps_bf16=True)}


def planted(c, name, dtype="float32"):
    """The value a planted wrong implementation gives on case c -> (cor1, flo1) float64 arrays."""
    a, b = front(pyramid_of(c, dtype), c.coords, c.flow, c.wc, c.bias_c, c.wf, c.bias_f, c.radius, **PLANTED_KW[name])
    return a.value, b.value


# ---------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_motion.py
# ---------------------------------------------------------------------------------------------------
# name: (B, H4, W2, W3, levels, radius, ks, Cc, Cf)
CASES = {
    "low_map":   (2, 5, 19, 19, 4, 4, 7, 64, 64),     # a map lower than the 7x7 window, a row tail of 3, widths 19 / 9 / 4 / 2
    "w2_ne_w3":  (1, 9, 37, 40, 4, 4, 7, 64, 64),     # W2 != W3; more than one chunk of 128 pixels, the last one not whole
    "tiles":     (3, 2, 16, 16, 4, 4, 7, 64, 64),     # one exact 16-pixel tile per row, a workgroup spans frames, level 3 is 2 wide
    "k15_ks3":   (2, 5, 19, 19, 3, 2, 3, 16, 48),     # K = 15: not a multiple of 4
    "k1_ks1":    (2, 5, 19, 19, 1, 0, 1, 48, 16),     # K = 1, a 1x1 window
}
NONFINITE_FLOW = {"nan": (0, 0, 2, 5), "inf": (1, 1, 3, 12)}          # (b, c, y, x) planted into the flow of "low_map"


def case(name, nonfinite=False):
    """-> namespace(level0 [N,W3] float32, coords [B,H4,W2], flow [B,2,H4,W2], wc [Cc,K,1,1], bias_c, wf [Cf,2,ks,ks], bias_f,
    ...).  The coordinates are `_corr_ref.directed_coords` first (one pixel each), then drawn from [-3, W3 + 3)."""
    B, H4, W2, W3, levels, radius, ks, Cc, Cf = CASES[name]
    N, K = B * H4 * W2, levels * (2 * radius + 1)
    rng = np.random.default_rng([5603, B, H4, W2, W3, levels, radius, ks, Cc, Cf])
    level0 = rng.standard_normal((N, W3)).astype(F32)
    d = np.concatenate(list(C.directed_coords(W3).values())).astype(F32)
    assert len(d) <= N
    cx = rng.uniform(-3.0, W3 + 3.0, N).astype(F32)
    whole = rng.random(N) < 0.2
    cx[whole] = np.floor(cx[whole])
    cx[:len(d)] = d
    flow = (rng.standard_normal((B, 2, H4, W2)) * 3.0).astype(F32)
    if nonfinite:
        for key, at in NONFINITE_FLOW.items():
            flow[at] = np.nan if key == "nan" else np.inf
    wc = (rng.standard_normal((Cc, K, 1, 1)) * (1.5 / np.sqrt(K))).astype(F32)
    wf = (rng.standard_normal((Cf, 2, ks, ks)) * (1.5 / np.sqrt(2 * ks * ks))).astype(F32)
    bias_c, bias_f = (rng.standard_normal(Cc) * 0.5).astype(F32), (rng.standard_normal(Cf) * 0.5).astype(F32)
    return SimpleNamespace(name=name, B=B, H4=H4, W2=W2, W3=W3, N=N, K=K, levels=levels, radius=radius, ks=ks, Cc=Cc, Cf=Cf, level0=level0,
                           coords=cx.reshape(B, H4, W2), n_directed=len(d), flow=flow, wc=wc, wf=wf, bias_c=bias_c, bias_f=bias_f)


def pyramid_of(c, dtype="float32"):
    """The case's levels: float32 cells, or bfloat16 bits of level 0 rounded once and pooled as stored."""
    if dtype == "bfloat16":
        return C.pyramid(BR.bits(BR.bf16_rne_f32(c.level0)), c.levels)
    return C.pyramid(c.level0, c.levels)


def case_ref(c, dtype="float32"):
    return front(pyramid_of(c, dtype), c.coords, c.flow, c.wc, c.bias_c, c.wf, c.bias_f, c.radius)


def zero_tap_pixels(c, dtype="float32"):
    """[B,H4,W2] bool: pixels whose taps are all +0 (the result is relu(bias_c) exactly)."""
    taps = taps_of(pyramid_of(c, dtype), c.coords, c.radius)
    return (taps.view(np.uint32) == 0).all(axis=1).reshape(c.B, c.H4, c.W2)


def load_recording():
    return np.load(GOLDEN)


def golden_case():
    """The recording as a case -> (namespace as case() returns, with pyr = the recorded levels; cor1, flo1 recorded)."""
    g = load_recording()
    B, _, H4, W2 = g["coords"].shape
    pyr = [g[f"level{i}"] for i in range(4)]
    c = SimpleNamespace(name="golden", B=B, H4=H4, W2=W2, W3=pyr[0].shape[1], N=B * H4 * W2, K=36, levels=4, radius=4, ks=7, Cc=64, Cf=64,
                        level0=pyr[0], pyr=pyr, coords=np.ascontiguousarray(g["coords"][:, 0]), coords2=g["coords"], flow=g["flow"],
                        wc=g["convc1_weight"], wf=g["convf1_weight"], bias_c=g["convc1_bias"], bias_f=g["convf1_bias"], lookup=g["lookup"])
    return c, g["cor1"], g["flo1"]
