"""Float64 referee, input builders and planted wrong implementations for the update block's other convolutions on the
matrix-core kernel (conv_kernels.hip through Engine.raft_conv): any Cout, a 3x3 or a 1x1 kernel, ReLU and a scale.
include/vppx.h has the arithmetic.

TEST INFRASTRUCTURE ONLY.  Plain numpy, no GPU: tests/test_conv_ref_cpu.py holds the referee to the arrays the reference's own
FlowHead.forward produced (tests/golden/heads_cases.npz) and shows on the very arrays the GPU file (tests/test_gpu_conv.py)
uploads that every planted mistake leaves the limit.

The 3x3 sum and its limit are tests/_gruconv_ref.conv3x3's, K = 9 Cin products.  The 1x1 sum has K = Cin products and the same
derivation: every product rounded once (exactly, for bfloat16 operands), every one of the K additions once,
        limit = (K + 1) U (|bias| + sum_k |w_k x_k|) (1 + 2^-10)      (+ T per product that is not zero and below T = 2^-126,
                                                                         + T for a result below T)
The ReLU is monotone and 1-Lipschitz: the same limit around relu(value).  The scale is one more correctly rounded float32
multiplication of a value that lies within `limit` of v:
        out = v * scale,     limit_out = (limit |scale| + U |v scale| (+ T for a product below T)) (1 + 2^-10)
and for scale == 1 nothing is added, as the product is exact.  There is no atol.  bfloat16 storage: the float32 result rounded
once, band() of tests/_referee.py.
"""
import os
from types import SimpleNamespace

import numpy as np

import _gruconv_ref as R
from _referee import SECOND_ORDER, TINY, U, _ns, _und, band, classes, compare, compare_bf16, misses, to_bf16  # noqa: F401

F32, F64 = np.float32, np.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "heads_cases.npz")
PLANTED = ("no_scale", "scale_acc_only", "no_relu", "corner_tap", "padded_rows", "swapped", "flipped")


def conv1x1(x0, x1, w, bias, dtype="float32", x0_limit=None, x1_limit=None, swapped=False, corner_tap=False):
    """x0 [B,C0,H,W], x1 [B,C1,H,W] or None, w [Cout,C0+C1,1,1] float32, bias [Cout] or None -> namespace(value, limit) before the
    ReLU and the scale.  Planted: swapped (cat([x1, x0])), corner_tap (the cell one up and one to the left, +0 outside the map:
    tap (0, 0) of the staged 3x3 window where the centre belongs)."""
    parts = [np.asarray(x0, F64)] + ([] if x1 is None else [np.asarray(x1, F64)])
    lims = [np.zeros_like(parts[0]) if x0_limit is None else x0_limit]
    if x1 is not None:
        lims.append(np.zeros_like(parts[1]) if x1_limit is None else x1_limit)
    if swapped:
        parts, lims = parts[::-1], lims[::-1]
    x, xl = np.concatenate(parts, axis=1), np.concatenate(lims, axis=1)
    if corner_tap:
        x = np.pad(x, ((0, 0), (0, 0), (1, 0), (1, 0)))[:, :, :-1, :-1]
        xl = np.pad(xl, ((0, 0), (0, 0), (1, 0), (1, 0)))[:, :, :-1, :-1]
    B, Cin, H, W = x.shape
    w = R.weights_of(w, dtype).astype(F64)
    M = w.shape[0]
    assert w.shape == (M, Cin, 1, 1), (w.shape, x.shape)
    wk = w[:, :, 0, 0]
    b = np.zeros(M) if bias is None else np.asarray(bias, F64)
    val = np.zeros((B, M, H, W)) + b[None, :, None, None]
    mag, und = np.abs(val), np.zeros((B, M, H, W))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for f in range(B):
            p = wk[:, :, None, None] * x[f][None]               # [M, Cin, H, W]
            val[f] += p.sum(axis=1)
            mag[f] += np.abs(p).sum(axis=1)
            und[f] += ((p != 0) & (np.abs(p) < TINY)).sum(axis=1) * TINY
        prop = np.einsum("mc,bchw->bmhw", np.abs(wk), xl)
        lim = ((Cin + 1) * U * mag + und + _und(val)) * SECOND_ORDER + prop
    return _ns(val, lim)


def conv(x0, x1, w, bias, dtype="float32", relu=False, scale=1.0, x0_limit=None, x1_limit=None, planted=None):
    """[relu](conv(cat([x0, x1])) + bias) * scale for w [Cout,Cin,k,k], k 1 or 3 -> namespace(value, limit) [B,Cout,H,W].
    planted: one of PLANTED."""
    assert planted is None or planted in PLANTED
    k = w.shape[2]
    assert w.shape[2:] == (k, k) and k in (1, 3)
    kw = dict(dtype=dtype, x0_limit=x0_limit, x1_limit=x1_limit, swapped=planted == "swapped")
    if k == 3:
        a = R.conv3x3(x0, x1, w, bias, flipped=planted == "flipped", **kw)
    else:
        a = conv1x1(x0, x1, w, bias, corner_tap=planted == "corner_tap", **kw)
    v, lim = a.value, a.limit
    scale = float(F32(scale))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        if planted == "scale_acc_only":                 # (acc * scale) + bias, and the ReLU behind it
            b = np.zeros(w.shape[0]) if bias is None else np.asarray(bias, F64)
            v = (v - b[None, :, None, None]) * scale + b[None, :, None, None]
        if relu and planted != "no_relu":
            v = R._relu(v)
        if scale != 1.0 and planted not in ("no_scale", "scale_acc_only"):
            out = v * scale
            lim = (lim * abs(scale) + U * np.abs(out) + _und(out)) * SECOND_ORDER
            v = out
    if planted == "padded_rows":
        # channel m of frame b read at row m of a [B, 16 * ceil(Cout / 16), H, W] result: right for frame 0, shifted behind it
        B, M, H, W = v.shape
        pad = np.zeros((B, 16 * ((M + 15) // 16), H, W))
        pad[:, :M] = v
        v = pad.reshape(-1)[:B * M * H * W].reshape(B, M, H, W)
    return _ns(v, lim)


# ---------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_conv.py
# ---------------------------------------------------------------------------------------------------
# name: (ksize, B, C0, C1, Cout, H, W, relu, scale)
CASES = {
    "flow2":  (3, 2, 256, 0, 2, 3, 5, False, 1.0),      # flow_head.conv2: one N tile of two channels, inside one tile of pixels
    "enc14":  (3, 2, 32, 16, 14, 9, 33, True, 1.0),     # two sources of unlike size, one row and one column over a tile
    "enc18":  (3, 2, 16, 0, 18, 8, 32, False, 3.0),     # exactly one tile; a second N tile of two channels; the 16-byte route
    "enc126": (3, 2, 64, 64, 126, 9, 33, True, 1.0),    # encoder.conv: two blocks of 64 channels, the second part-filled
    "head256": (3, 2, 128, 0, 256, 3, 5, True, 1.0),    # flow_head.conv1 / mask[0]: Cout % 16 == 0, the bits of raft_conv3x3
    "mask144": (1, 2, 256, 0, 144, 9, 33, False, .25),  # mask[2] with its .25: three blocks, the last of one N tile
    "mask9":   (1, 2, 16, 0, 9, 8, 32, True, .25),      # a 1x1 of one part-filled N tile, the 16-byte route
    "one1x1":  (1, 2, 32, 16, 25, 3, 5, False, 3.0),    # a 1x1 over two sources
}
# planted mistake -> the cases that claim to catch it
CATCHES = {"no_scale": ("enc18", "mask144", "mask9", "one1x1"), "scale_acc_only": ("enc18", "mask144", "mask9", "one1x1"),
           "no_relu": ("enc14", "enc126", "head256", "mask9"), "corner_tap": ("mask144", "mask9", "one1x1"),
           "padded_rows": ("flow2", "enc14", "enc18", "enc126", "mask9", "one1x1"), "swapped": ("enc14", "enc126", "one1x1"),
           "flipped": ("flow2", "enc14", "enc18", "enc126", "head256")}


def case(name, dtype="float32"):
    """-> namespace(x0, x1 or None, w [Cout,Cin,k,k], bias, relu, scale): weights of about 1.5 / sqrt(K), so that sums are of order 1."""
    ks, B, C0, C1, Cout, H, W, relu, scale = CASES[name]
    rng = np.random.default_rng([6201, ks, B, C0, C1, Cout, H, W])
    K = ks * ks * (C0 + C1)
    return SimpleNamespace(name=name, ksize=ks, B=B, C0=C0, C1=C1, Cout=Cout, H=H, W=W, relu=relu, scale=scale, dtype=dtype,
                           x0=R._cells(rng, (B, C0, H, W), dtype), x1=R._cells(rng, (B, C1, H, W), dtype) if C1 else None,
                           w=(rng.standard_normal((Cout, C0 + C1, ks, ks)) * (1.5 / np.sqrt(K))).astype(F32),
                           bias=(rng.standard_normal(Cout) * 0.5).astype(F32))


def case_ref(c, **kw):
    kw = dict(dict(relu=c.relu, scale=c.scale), **kw)
    return conv(c.x0, c.x1, c.w, c.bias, dtype=c.dtype, **kw)


# ---------------------------------------------------------------------------------------------------
# the recording (tests/golden/heads_cases.npz): the reference's FlowHead(16, 32, 2).forward
# ---------------------------------------------------------------------------------------------------
RECORDED = ("a", "b")


def load_recording():
    return np.load(GOLDEN)


def recorded_ref(g, name, dtype="float32", planted=None):
    """The referee on the recording's input -> (conv1 with its ReLU, conv2 on it).  The hidden tensor passes through memory:
    R.stored() for bfloat16, and its bound goes into conv2's."""
    x = g[f"{name}_x"]
    if dtype == "bfloat16":
        x = to_bf16(x)
    hid = conv(x, None, g["conv1_weight"], g["conv1_bias"], dtype, relu=True, planted=planted if planted != "no_scale" else None)
    mid = R.stored(hid, dtype)
    out = conv(mid.value, None, g["conv2_weight"], g["conv2_bias"], dtype, x0_limit=mid.limit,
               planted=planted if planted in ("flipped", "padded_rows") else None)
    return hid, out
