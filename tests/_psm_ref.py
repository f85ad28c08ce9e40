"""Float64 referee, cases and planted wrong implementations for PSMNet's feature_extraction on the library's kernels
(models/psmnet/submodule.py:131-253): the convolution with dilation 2 and a residual (conv_kernels.hip through Engine.conv2d),
the pyramid pooling's average pools (spp_kernels.hip through Engine.psm_spp_pool), the fold of a frozen BatchNorm into a
convolution (vppstereo_amd/_convs.fold_bn) and the assembled 320-channel tensor.  include/vppx.h has the arithmetic.

TEST INFRASTRUCTURE ONLY.  Plain numpy, no GPU: tests/test_psm_ref_cpu.py holds the referee to torch in float64 and shows on the
very arrays the GPU file (tests/test_gpu_psm_features.py) uploads that every planted mistake leaves the limit.

The convolution.  At dilation 1 value and limit are tests/_strided_ref.conv's (tests/_conv_ref.conv's at stride 1).  At dilation
2 the sum has the same K = 9 Cin products at other cells, in[y + 2 (dy - 1)][x + 2 (dx - 1)] with +0 outside the map, and
tests/_gruconv_ref.conv3x3's derivation carries over word for word: every product rounded once (exactly, for bfloat16
operands), every one of the K additions once,
        limit = (K + 1) U (|bias| + sum_k |w_k x_k|) (1 + 2^-10)      (+ T per product that is not zero and below T = 2^-126,
                                                                         + T for a result below T)
The residual is one more correctly rounded float32 addition of a value within `limit` of v and an exact cell:
        v' = v + res,      limit' = (limit + U |v + res| (+ T for a sum below T)) (1 + 2^-10)      (+ the residual's own bound)
then the ReLU (monotone, 1-Lipschitz: the same limit) and the scale, as tests/_conv_ref.conv has them.  There is no atol.

A pool.  value = (sum of the k*k window cells) / (k*k).  A float32 evaluation in any order passes a cell through at most k*k - 1
additions and the one division, each within U of a partial result of at most sum |x| in magnitude:
        limit = k*k U (sum |x|) / (k*k) (1 + 2^-10) = U sum |x| (1 + 2^-10)            (+ T for a result below T)
(the second-order terms of 4096 roundings are 2^-13 of the first-order ones).

The fold.  s = gamma / sqrt(var + eps), w' = w s, b' = beta + (conv_bias - mean) s in float64, each rounded to float32 once:
value = the float64 result, limit = U |value| (+ T below T).  A convolution run with folded weights against the unfolded formula
bn(conv(x)) carries that one rounding per weight and bias through the sum: + sum_k U |w'_k x_k| + U |b'|, which convbn() adds.

bfloat16 storage: the float32 result rounded once, band() of tests/_referee.py; a cell that is read back carries
tests/_gruconv_ref.stored()'s half unit.
"""
import os
from types import SimpleNamespace

import numpy as np

import _conv_ref as CR
import _gru_ref as G
import _gruconv_ref as R
import _strided_ref as SR
from _referee import SECOND_ORDER, TINY, U, _ns, _und, band, classes, compare, compare_bf16, misses, to_bf16  # noqa: F401

F32, F64 = np.float32, np.float64
PLANTED_CONV = ("dilation_ignored", "padding_one", "res_behind_relu", "res_behind_scale")
PLANTED_POOL = ("sizes_up", "in_map_count")
PLANTED_FOLD = ("no_eps", "no_mean")
PLANTED_TAIL = ("order_1234",)


# ---------------------------------------------------------------------------------------------------
# the convolution
# ---------------------------------------------------------------------------------------------------
def _mm(wk, a):
    """sum over c of wk[m][c] * a[b][c][y][x] as one matrix product per frame."""
    B, Cc, H, W = a.shape
    return np.matmul(wk, np.ascontiguousarray(a).reshape(B, Cc, H * W)).reshape(B, wk.shape[0], H, W)


def conv3x3_dilated(x0, x1, w, bias, dtype="float32", dilation=2, pad=None, x0_limit=None, x1_limit=None, w_limit=None, fast=False):
    """x0 [B,C0,H,W], x1 [B,C1,H,W] or None, w [Cout,C0+C1,3,3], bias [Cout] or None -> namespace(value, limit) [B,Cout,H,W] of
    the sum with taps `dilation` apart around a window that starts `pad` cells up and left (pad = dilation is nn.Conv2d's
    padding=dilation; the planted padding_one shifts the window and reads +0 where it leaves the map).  w_limit: a bound on every
    weight, carried through the sum.  fast: the sums as matrix products for the large maps of the wrapper's launches (a NaN
    input then reaches every channel through 0 * NaN as well, which is what the kernel's matrix instructions do)."""
    pad = dilation if pad is None else pad
    parts = [np.asarray(x0, F64)] + ([] if x1 is None else [np.asarray(x1, F64)])
    lims = [np.zeros_like(parts[0]) if x0_limit is None else x0_limit]
    if x1 is not None:
        lims.append(np.zeros_like(parts[1]) if x1_limit is None else x1_limit)
    x, xl = np.concatenate(parts, axis=1), np.concatenate(lims, axis=1)
    B, Cin, H, W = x.shape
    w = R.weights_of(w, dtype).astype(F64)
    M = w.shape[0]
    assert w.shape == (M, Cin, 3, 3), (w.shape, x.shape)
    far = 2 * dilation
    p4 = ((0, 0), (0, 0), (pad, far), (pad, far))
    xp, lp = np.pad(x, p4), np.pad(xl, p4)
    b = np.zeros(M) if bias is None else np.asarray(bias, F64)
    val = np.zeros((B, M, H, W)) + b[None, :, None, None]
    mag, und, prop = np.abs(val), np.zeros((B, M, H, W)), np.zeros((B, M, H, W))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for dy in range(3):
            for dx in range(3):
                ys, xs = slice(dilation * dy, dilation * dy + H), slice(dilation * dx, dilation * dx + W)
                win, wk = xp[:, :, ys, xs], w[:, :, dy, dx]
                if fast:                                # T for every product, whether it is below T or not: the count's ceiling
                    val += _mm(wk, win)
                    mag += _mm(np.abs(wk), np.abs(win))
                    und += Cin * TINY
                else:
                    for f in range(B):
                        p = wk[:, :, None, None] * win[f][None]
                        val[f] += p.sum(axis=1)
                        mag[f] += np.abs(p).sum(axis=1)
                        und[f] += ((p != 0) & (np.abs(p) < TINY)).sum(axis=1) * TINY
                if x0_limit is not None or x1_limit is not None:
                    prop += _mm(np.abs(wk), lp[:, :, ys, xs])
                if w_limit is not None:
                    prop += _mm(w_limit[:, :, dy, dx], np.abs(win))
        lim = ((9 * Cin + 1) * U * mag + und + _und(val)) * SECOND_ORDER + prop
    return _ns(val, lim)


def conv2d(x0, x1, w, bias, dtype="float32", stride=1, dilation=1, res=None, relu=False, scale=1.0, x0_limit=None, x1_limit=None,
           res_limit=None, planted=None, pre=None, fast=False):
    """[relu](conv(cat([x0, x1])) + bias [+ res]) * scale for w [Cout,Cin,k,k], k 1 or 3, padding dilation * (k // 2)
    -> namespace(value, limit) [B,Cout,Ho,Wo].  planted: one of PLANTED_CONV.  pre: conv + bias as an earlier call with the same
    inputs, stride and dilation returned it without res, relu and scale, for the epilogues of one sum.  fast: conv3x3_dilated's."""
    assert planted is None or planted in PLANTED_CONV
    assert dilation in (1, 2) and stride in (1, 2) and not (dilation == 2 and stride == 2)
    k = w.shape[2]
    if planted == "dilation_ignored":
        dilation = 1
    if pre is not None:
        a = pre
    elif fast and k == 3:
        a = conv3x3_dilated(x0, x1, w, bias, dtype, dilation, x0_limit=x0_limit, x1_limit=x1_limit, fast=True)
        a = _ns(a.value[:, :, ::stride, ::stride], a.limit[:, :, ::stride, ::stride])
    elif dilation == 2 and k == 3:
        a = conv3x3_dilated(x0, x1, w, bias, dtype, 2, pad=1 if planted == "padding_one" else 2, x0_limit=x0_limit, x1_limit=x1_limit)
    else:
        a = SR.conv(x0, x1, w, bias, dtype, stride=stride, x0_limit=x0_limit, x1_limit=x1_limit)
    v, lim = a.value, a.limit
    scale = float(F32(scale))
    r = None if res is None else np.asarray(res, F64)
    rl = 0.0 if res_limit is None else res_limit

    def add(v, lim):
        out = v + r
        return out, (lim + U * np.abs(out) + _und(out)) * SECOND_ORDER + rl

    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        if r is not None and planted not in ("res_behind_relu", "res_behind_scale"):
            v, lim = add(v, lim)
        if relu:
            v = R._relu(v)
        if r is not None and planted == "res_behind_relu":
            v, lim = add(v, lim)
        if scale != 1.0:
            out = v * scale
            lim = (lim * abs(scale) + U * np.abs(out) + _und(out)) * SECOND_ORDER
            v = out
        if r is not None and planted == "res_behind_scale":
            v, lim = add(v, lim)
    return _ns(v, lim)


def nan_reach(H, W, y, x, dilation=2):
    """The [H, W] mask of output pixels whose 3x3 window at `dilation`, stride 1, holds input cell (y, x)."""
    reach = np.zeros((H, W), bool)
    for i in (-1, 0, 1):
        for j in (-1, 0, 1):
            oy, ox = y + dilation * i, x + dilation * j
            if 0 <= oy < H and 0 <= ox < W:
                reach[oy, ox] = True
    return reach


# the grid of tests/test_gpu_psm_features.py at dilation 2: every map with every Cin and Cout, each under every epilogue
CONV_MAPS = ((1, 1), (2, 2), (8, 32), (9, 33), (17, 70))      # every tap but the centre outside (twice); one exact tile; one pixel
#                                                               into the next tile on both axes; three tile rows and columns
CONV_CINS = ((16, 0), (48, 0), (16, 32))                      # one chunk; one and a half bfloat16 chunks; two sources
CONV_COUTS = (16, 20, 80)                                     # one N tile; a masked store; two channel blocks
EPILOGUES = tuple((res, relu, scale) for res in (False, True) for relu in (False, True) for scale in (1.0, 0.25))

# the named cases of tests/test_psm_ref_cpu.py, points of that grid and two beside it
# name: (ksize, dilation, B, C0, C1, Cout, H, W, res, relu, scale)
CONV_CASES = {
    "px1":     (3, 2, 1, 16, 0, 16, 1, 1, True, False, 1.0),      # every tap but the centre is outside
    "px2":     (3, 2, 2, 16, 0, 16, 2, 2, False, True, 1.0),      # likewise: a 2x2 map has no cell two away
    "tile":    (3, 2, 2, 16, 0, 16, 8, 32, True, True, 1.0),      # exactly one tile, the 16-byte route
    "over":    (3, 2, 2, 48, 0, 20, 9, 33, True, True, 0.25),     # one pixel into the next tile on both axes; one and a half bfloat16
    #                                                               chunks; a part-filled second N tile
    "two":     (3, 2, 2, 16, 32, 80, 17, 70, True, False, 0.25),  # two sources; two channel blocks; three tile rows and columns
    "plain":   (3, 2, 1, 48, 0, 80, 17, 70, False, False, 1.0),   # no residual, no ReLU, scale 1
    "d1_res":  (3, 1, 2, 16, 32, 20, 9, 33, True, True, 1.0),     # dilation 1 with a residual
    "k1_d2":   (1, 2, 2, 48, 0, 20, 9, 33, True, True, 0.25),     # a 1x1 at dilation 2 is the 1x1 itself
}
# planted mistake -> the cases that claim to catch it
CONV_CATCHES = {"dilation_ignored": ("tile", "over", "two", "plain"),          # (px1, px2: only the centre tap is inside either way)
                "padding_one": ("px1", "px2", "tile", "over", "two", "plain"),
                "res_behind_relu": ("tile", "over", "d1_res", "k1_d2"),
                "res_behind_scale": ("over", "two", "k1_d2")}


def make_conv(ks, dil, B, C0, C1, Cout, H, W, dtype="float32", res=True, relu=False, scale=1.0, name=None):
    """-> namespace(x0, x1 or None, w, bias, res or None, ...): weights of about 1.5 / sqrt(K), so that sums are of order 1.  The
    arrays depend on the shape alone: a case with and without its residual has the same inputs."""
    rng = np.random.default_rng([7301, ks, dil, B, C0, C1, Cout, H, W])
    K = ks * ks * (C0 + C1)
    c = SimpleNamespace(name=name, ksize=ks, dilation=dil, B=B, C0=C0, C1=C1, Cout=Cout, H=H, W=W, relu=relu, scale=scale, dtype=dtype,
                        x0=R._cells(rng, (B, C0, H, W), dtype), x1=R._cells(rng, (B, C1, H, W), dtype) if C1 else None,
                        w=(rng.standard_normal((Cout, C0 + C1, ks, ks)) * (1.5 / np.sqrt(K))).astype(F32),
                        bias=(rng.standard_normal(Cout) * 0.5).astype(F32), res=R._cells(rng, (B, Cout, H, W), dtype))
    if not res:
        c.res = None
    return c


def conv_case(name, dtype="float32"):
    ks, dil, B, C0, C1, Cout, H, W, res, relu, scale = CONV_CASES[name]
    return make_conv(ks, dil, B, C0, C1, Cout, H, W, dtype, res, relu, scale, name)


def conv_case_ref(c, **kw):
    kw = dict(dict(dilation=c.dilation, res=c.res, relu=c.relu, scale=c.scale), **kw)
    return conv2d(c.x0, c.x1, c.w, c.bias, dtype=c.dtype, **kw)


def caught(got, ref, dtype="float32"):
    """Whether `got` (an array) leaves the referee: by its shape, or by a cell beyond the limit."""
    if got.shape != ref.value.shape:
        return True
    return misses(got, ref, dtype) > 0


# ---------------------------------------------------------------------------------------------------
# the pools
# ---------------------------------------------------------------------------------------------------
def pool(x, k, lim=None, planted=None):
    """x [B,C,H,W] -> namespace(value, limit) [B,C,H // k,W // k] of nn.AvgPool2d((k, k), stride=(k, k)).  Planted: sizes_up
    (ceil(H / k) by ceil(W / k) windows, +0 behind the map, / (k*k)), in_map_count (the same windows divided by their cells
    inside the map: ceil_mode=True)."""
    assert planted is None or planted in PLANTED_POOL
    x = np.asarray(x, F64)
    B, C, H, W = x.shape
    lim = np.zeros_like(x) if lim is None else lim
    Ho, Wo = (-(-H // k), -(-W // k)) if planted else (H // k, W // k)
    pad = ((0, 0), (0, 0), (0, Ho * k - H if planted else 0), (0, Wo * k - W if planted else 0))
    cut = (slice(None), slice(None), slice(0, Ho * k), slice(0, Wo * k))
    win = lambda a: np.pad(a, pad)[cut].reshape(a.shape[0], a.shape[1], Ho, k, Wo, k)     # noqa: E731
    with np.errstate(invalid="ignore", over="ignore"):
        s, sa, sl = win(x).sum(axis=(3, 5)), win(np.abs(x)).sum(axis=(3, 5)), win(lim).sum(axis=(3, 5))
        n = float(k * k)
        if planted == "in_map_count":
            n = win(np.ones((1, 1, H, W))).sum(axis=(3, 5))
        v = s / n
        return _ns(v, (U * sa + _und(v)) * SECOND_ORDER + sl / float(k * k))


# name: (B, C, H, W, ks)
POOL_CASES = {
    "odd":  (2, 3, 37, 53, (2, 4, 8, 16)),       # neither size a multiple of any window: rows and columns behind every floor boundary
    "odd16": (2, 16, 37, 53, (2, 4, 8, 16)),
    "spp":  (2, 3, 64, 72, (8, 16, 32, 64)),     # PSMNet's windows on the smallest map AvgPool2d(64) takes; 72 = 4.5 * 16
    "spp16": (2, 16, 64, 72, (8, 16, 32, 64)),
    "loose": (1, 3, 37, 53, (3, 5)),             # windows that do not nest: a grid of single cells
    "direct": (1, 2, 96, 100, (1, 7)),           # 9600 grid cells do not fit: the direct route
}
POOL_CATCHES = {"sizes_up": ("odd", "odd16", "spp", "spp16", "loose", "direct"), "in_map_count": ("odd", "odd16", "spp", "spp16", "loose", "direct")}


def pool_case(name, dtype="float32"):
    B, C, H, W, ks = POOL_CASES[name]
    rng = np.random.default_rng([7302, B, C, H, W])
    return SimpleNamespace(name=name, B=B, C=C, H=H, W=W, ks=ks, dtype=dtype, x=R._cells(rng, (B, C, H, W), dtype))


# ---------------------------------------------------------------------------------------------------
# the fold
# ---------------------------------------------------------------------------------------------------
def fold(w, conv_bias, gamma, beta, mean, var, eps, planted=None):
    """-> (namespace(value, limit) of w' [Cout,Cin,k,k], the same of b' [Cout]): float64 values, limit = one rounding to float32.
    gamma / beta None: a norm without affine parameters.  Planted: no_eps, no_mean."""
    assert planted is None or planted in PLANTED_FOLD
    w, mean, var = np.asarray(w, F64), np.asarray(mean, F64), np.asarray(var, F64)
    s = 1.0 / np.sqrt(var + (0.0 if planted == "no_eps" else float(eps)))
    if gamma is not None:
        s = np.asarray(gamma, F64) * s
    cb = np.zeros_like(mean) if conv_bias is None else np.asarray(conv_bias, F64)
    b = (cb - (0.0 if planted == "no_mean" else mean)) * s
    if beta is not None:
        b = np.asarray(beta, F64) + b
    wf = w * s[:, None, None, None]
    one = lambda v: _ns(v, (U * np.abs(v) + _und(v)) * SECOND_ORDER)                      # noqa: E731
    return one(wf), one(b)


def convbn(x0, x1, w, conv_bias, bn, dtype="float32", planted=None, **kw):
    """bn(conv(x)) by the UNFOLDED formula's exact value, with the bound of a float32 run on folded weights: conv2d() on the
    float32-rounded fold, plus the one rounding each folded weight and bias carries.  bn: dict(gamma, beta, mean, var, eps).
    For bfloat16 the packing rounds the folded float32 weight once more: conv2d()'s weights_of() does the same."""
    wf, bf = fold(w, conv_bias, bn.get("gamma"), bn.get("beta"), bn["mean"], bn["var"], bn["eps"], planted=planted)
    a = conv2d(x0, x1, wf.value.astype(F32), bf.value.astype(F32), dtype, **kw)
    x = np.concatenate([np.abs(np.asarray(x0, F64))] + ([] if x1 is None else [np.abs(np.asarray(x1, F64))]), axis=1)
    stride = kw.get("stride", 1)
    k, dil = w.shape[2], kw.get("dilation", 1)
    p = dil * (k // 2)
    xp = np.pad(x, ((0, 0), (0, 0), (p, p), (p, p)))
    H, W = x.shape[2:]
    extra = np.zeros_like(a.value) + bf.limit[None, :, None, None]
    for dy in range(k):
        for dx in range(k):
            win = xp[:, :, dil * dy:dil * dy + H, dil * dx:dil * dx + W][:, :, ::stride, ::stride]
            extra += _mm(wf.limit[:, :, dy, dx], win)
    return _ns(a.value, a.limit + extra * abs(float(F32(kw.get("scale", 1.0)))))


def bn_case(rng, C):
    """Seeded running statistics and affine parameters of a BatchNorm2d(C)."""
    return dict(gamma=(1.0 + 0.3 * rng.standard_normal(C)).astype(F32), beta=(0.3 * rng.standard_normal(C)).astype(F32),
                mean=(0.5 * rng.standard_normal(C)).astype(F32), var=(0.5 + rng.random(C)).astype(F32), eps=1e-5)


# ---------------------------------------------------------------------------------------------------
# the assembled tensor: cat((output_raw, output_skip, branch4, branch3, branch2, branch1), 1)  (submodule.py:208-250)
# ---------------------------------------------------------------------------------------------------
def tail(raw, skip, branches, dtype="float32", ks=(64, 32, 16, 8), planted=None):
    """raw [B,Cr,H,W], skip [B,Cs,H,W]; branches: four (w [Cb,Cs,1,1], bn dict) for branch1 .. branch4 with windows `ks`
    -> namespace(value, limit) [B,Cr+Cs+4Cb,H,W].  Each branch is pool -> folded 1x1 -> ReLU -> (stored) -> interp; the pooled
    tensor and the branch's output pass through memory (R.stored).  Planted: order_1234."""
    assert planted is None or planted in PLANTED_TAIL
    raw, skip = np.asarray(raw, F64), np.asarray(skip, F64)
    H, W = skip.shape[2:]
    outs = []
    for (w, bn), k in zip(branches, ks):
        p = R.stored(pool(skip, k), dtype)
        wf, bf = fold(w, None, bn.get("gamma"), bn.get("beta"), bn["mean"], bn["var"], bn["eps"])
        c = R.stored(conv2d(p.value, None, wf.value.astype(F32), bf.value.astype(F32), dtype, relu=True, x0_limit=p.limit), dtype)
        outs.append(G.interp(c.value, H, W, c.limit))
    order = outs if planted == "order_1234" else outs[::-1]
    vals = [raw, skip] + [v for v, _ in order]
    lims = [np.zeros_like(raw), np.zeros_like(skip)] + [l for _, l in order]
    return _ns(np.concatenate(vals, axis=1), np.concatenate(lims, axis=1))


# ---------------------------------------------------------------------------------------------------
# the recording (tests/golden/psm_cases.npz): the reference's own BasicBlocks and the tail of its feature_extraction.forward
# ---------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "psm_cases.npz")
RECORDED_BLOCKS = {"a": dict(stride=1, dilation=2), "b": dict(stride=2, dilation=1)}


def load_recording():
    return np.load(GOLDEN)


def bn_of(g, prefix, eps=1e-5):
    return dict(gamma=g[prefix + ".weight"], beta=g[prefix + ".bias"], mean=g[prefix + ".running_mean"], var=g[prefix + ".running_var"], eps=eps)


def block(x, g, name, dtype="float32", stride=1, dilation=1, x_limit=None, planted=None, fast=False):
    """BasicBlock.forward (submodule.py:75-84) on the state dict g[name + "."...]: conv2bn(relu(conv1bn(x))) + (downsample(x) or x),
    no ReLU behind the sum.  The hidden tensor and the downsample's output pass through memory (R.stored).
    -> namespace(value, limit, hidden, down), the last two as the launches that make them are held: before the storage's bound."""
    kw = dict(planted=planted if planted in PLANTED_FOLD else None, fast=fast)
    h0 = convbn(x, None, g[f"{name}.conv1.0.0.weight"], None, bn_of(g, f"{name}.conv1.0.1"), dtype, stride=stride, dilation=dilation, relu=True,
                x0_limit=x_limit, **kw)
    h = R.stored(h0, dtype)
    if f"{name}.downsample.0.weight" in g:
        d0 = convbn(x, None, g[f"{name}.downsample.0.weight"], None, bn_of(g, f"{name}.downsample.1"), dtype, stride=stride, x0_limit=x_limit, **kw)
        d = R.stored(d0, dtype)
        res, rl = d.value, d.limit
    else:
        d0, res, rl = None, np.asarray(x, F64), x_limit
    out = convbn(h.value, None, g[f"{name}.conv2.0.weight"], None, bn_of(g, f"{name}.conv2.1"), dtype, dilation=dilation, res=res, res_limit=rl,
                 x0_limit=h.limit, **kw)
    return _ns(out.value, out.limit, hidden=h0, down=d0)


TAIL_SHAPE = (1, 4, 64, 72)


def tail_input():
    """The recorder's integer formula: [1,4,64,72], multiples of 1/8."""
    c, y, x = np.meshgrid(np.arange(4), np.arange(64), np.arange(72), indexing="ij")
    return (((7 * y + 13 * x + 29 * c) % 31 - 15) / 8.0).astype(F32)[None]


def tail_raw_skip():
    """output_raw [1,64,64,72] and output_skip [1,128,64,72] of the recorder's stand-ins, 1x1 convolutions with the integer
    weights below: every product and partial sum is exact in float32."""
    m, c = np.meshgrid(np.arange(64), np.arange(4), indexing="ij")
    w2 = ((5 * m + 3 * c) % 17 - 8) / 16.0
    m, c = np.meshgrid(np.arange(128), np.arange(64), indexing="ij")
    w4 = ((7 * m + 11 * c) % 19 - 9) / 64.0
    raw = np.einsum("mc,bchw->bmhw", w2, tail_input().astype(F64))
    skip = np.einsum("mc,bchw->bmhw", w4, raw)
    assert np.array_equal(raw, raw.astype(F32)) and np.array_equal(skip, skip.astype(F32))
    return raw.astype(F32), skip.astype(F32)


def recorded_branches(g):
    """[(w, bn dict)] for branch1 .. branch4 of the recording."""
    return [(g[f"tail.branch{k}.1.0.weight"], bn_of(g, f"tail.branch{k}.1.1")) for k in (1, 2, 3, 4)]


# ---------------------------------------------------------------------------------------------------
# a stand-in feature_extraction of the reference's structure, and a spied launch against its referee
# ---------------------------------------------------------------------------------------------------
def standin(widths=(16, 16, 32, 32), blocks=(1, 2, 1, 1), branch=16, mid=32, out=16, seed=0):
    """A torch module with `firstconv`, `layer1` .. `layer4`, `branch1` .. `branch4` and `lastconv` laid out as
    models/psmnet/submodule.py:131-177 lays them out (strides 2 in firstconv[0] and layer2[0], dilation 2 in layer4, windows of 64,
    32, 16 and 8), at the given widths, seeded and in eval mode.  Its forward is the plain torch one."""
    import torch
    nn = torch.nn

    def convbn(cin, cout, k, stride, dilation):
        return nn.Sequential(nn.Conv2d(cin, cout, k, stride=stride, padding=dilation * (k // 2), dilation=dilation, bias=False), nn.BatchNorm2d(cout))

    class Block(nn.Module):
        def __init__(self, cin, cout, stride, dilation):
            super().__init__()
            self.conv1 = nn.Sequential(convbn(cin, cout, 3, stride, dilation), nn.ReLU(inplace=True))
            self.conv2 = convbn(cout, cout, 3, 1, dilation)
            self.downsample = convbn(cin, cout, 1, stride, 1) if stride != 1 or cin != cout else None

        def forward(self, x):
            y = self.conv2(self.conv1(x))
            return y + (x if self.downsample is None else self.downsample(x))

    class Features(nn.Module):
        def __init__(self):
            super().__init__()
            w0 = widths[0]
            self.firstconv = nn.Sequential(convbn(3, w0, 3, 2, 1), nn.ReLU(inplace=True), convbn(w0, w0, 3, 1, 1), nn.ReLU(inplace=True),
                                           convbn(w0, w0, 3, 1, 1), nn.ReLU(inplace=True))
            cin = w0
            for k, (w, n, stride, dil) in enumerate(zip(widths, blocks, (1, 2, 1, 1), (1, 1, 1, 2))):
                setattr(self, f"layer{k + 1}", nn.Sequential(*[Block(cin if j == 0 else w, w, stride if j == 0 else 1, dil) for j in range(n)]))
                cin = w
            for k, win in zip((1, 2, 3, 4), (64, 32, 16, 8)):
                setattr(self, f"branch{k}", nn.Sequential(nn.AvgPool2d((win, win), stride=(win, win)), convbn(widths[3], branch, 1, 1, 1),
                                                          nn.ReLU(inplace=True)))
            self.lastconv = nn.Sequential(convbn(widths[1] + widths[3] + 4 * branch, mid, 3, 1, 1), nn.ReLU(inplace=True),
                                          nn.Conv2d(mid, out, 1, bias=False))

        def forward(self, x):
            F = nn.functional
            raw = self.layer2(self.layer1(self.firstconv(x)))
            skip = self.layer4(self.layer3(raw))
            up = [F.interpolate(getattr(self, f"branch{k}")(skip), skip.shape[2:], mode="bilinear", align_corners=True) for k in (4, 3, 2, 1)]
            return self.lastconv(torch.cat([raw, skip] + up, 1))

    fe = Features()
    gen = torch.Generator().manual_seed(7501 + seed)
    with torch.no_grad():
        for m in fe.modules():
            if isinstance(m, nn.Conv2d):
                K = m.in_channels * m.kernel_size[0] * m.kernel_size[1]
                m.weight.copy_(torch.randn(m.weight.shape, generator=gen) * (1.5 / K ** 0.5))
            elif isinstance(m, nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=gen) * 0.5)
                m.running_var.copy_(torch.rand(m.num_features, generator=gen) + 0.5)
                m.weight.copy_(1.0 + 0.3 * torch.randn(m.num_features, generator=gen))
                m.bias.copy_(0.3 * torch.randn(m.num_features, generator=gen))
    return fe.eval()


def launch_plan(fe):
    """The (Conv2d, BatchNorm2d or None, relu) of every Engine.conv2d launch of FusedFeatureExtraction.forward, in its order."""
    plan = [(fe.firstconv[2][0], fe.firstconv[2][1], True), (fe.firstconv[4][0], fe.firstconv[4][1], True)]

    def layer(seq):
        for blk in seq:
            if blk.downsample is not None:
                plan.append((blk.downsample[0], blk.downsample[1], False))
            plan.append((blk.conv1[0][0], blk.conv1[0][1], True))
            plan.append((blk.conv2[0], blk.conv2[1], False))
    for name in ("layer1", "layer2", "layer3", "layer4"):
        layer(getattr(fe, name))
    for k in (4, 3, 2, 1):
        br = getattr(fe, f"branch{k}")
        plan.append((br[1][0], br[1][1], True))
    plan.append((fe.lastconv[0][0], fe.lastconv[0][1], True))
    plan.append((fe.lastconv[2], None, False))
    return plan


def check_conv_launch(rec, conv, bn, relu, what):
    """rec: a LaunchSpy record of Engine.conv2d; conv, bn: the modules whose folded weights the launch ran with."""
    import _raft_loop as L
    from _cells import hold
    x0, cout, ksize = rec.args[0], rec.args[2], rec.args[3]
    kw = rec.kwargs
    dtype = L._dt(x0)
    n = lambda t: None if t is None else t.detach().float().cpu().numpy()                 # noqa: E731
    assert conv.out_channels == cout and conv.kernel_size[0] == ksize and conv.stride[0] == kw.get("stride", 1), what
    assert conv.dilation[0] == kw.get("dilation", 1) and bool(kw.get("relu", False)) == relu and kw.get("x1") is None, what
    args = dict(stride=kw.get("stride", 1), dilation=kw.get("dilation", 1), res=L._np(kw.get("residual")), relu=relu, fast=True)
    if bn is None:
        ref = conv2d(L._np(x0), None, n(conv.weight), n(conv.bias), dtype, **args)
    else:
        bnd = dict(gamma=n(bn.weight), beta=n(bn.bias), mean=n(bn.running_mean), var=n(bn.running_var), eps=bn.eps)
        ref = convbn(L._np(x0), None, n(conv.weight), n(conv.bias), bnd, dtype, **args)
    got = rec.result
    assert tuple(got.shape) == ref.value.shape, (what, tuple(got.shape), ref.value.shape)
    hold(CR, L._np(got), ref, what, dtype)
