"""Float64 referee, cases and planted wrong implementations for the convolution kernel at stride 2 (conv_kernels.hip through
Engine.raft_conv(..., stride=2)): nn.Conv2d(Cin, Cout, k, stride=2, padding=k // 2) for k 3 and 1.  include/vppx.h has the arithmetic.

TEST INFRASTRUCTURE ONLY.  Plain numpy, no GPU: tests/test_strided_ref_cpu.py holds the referee to the arrays the reference's own
ResidualBlock(16, 32, 'instance', stride=2) produced (tests/golden/strided_cases.npz) and shows on the very arrays the GPU file
(tests/test_gpu_conv_strided.py) uploads that every planted mistake leaves the limit.

The referee.  Output pixel (y, x) of the strided convolution is, term for term, output pixel (2y, 2x) of the stride-1 convolution
with the same padding: the same K products, the same bias.  So value and limit are tests/_conv_ref.conv's at [:, :, ::2, ::2], for
both kernel sizes, and the limit derived there carries over with no new tolerance and no atol.  The output size is
(H - 1) // 2 + 1 by (W - 1) // 2 + 1, which is what [::2] gives.
"""
import os
from types import SimpleNamespace

import numpy as np

import _conv_ref as CR
import _gruconv_ref as R
from _referee import SECOND_ORDER, TINY, U, _ns, _und, band, classes, compare, compare_bf16, misses, to_bf16  # noqa: F401

F32, F64 = np.float32, np.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "strided_cases.npz")
PLANTED = ("odd_phase", "stride_x_only", "stride_y_only", "floor_size", "dense_1x1", "flipped", "swapped")


def out_size(n, stride=2):
    return (n - 1) // stride + 1


def _padded(a, lim):
    """One row and one column of +0 behind the map (with a bound of 0)."""
    pad = ((0, 0), (0, 0), (0, 1), (0, 1))
    return None if a is None else np.pad(np.asarray(a, F64), pad), None if lim is None else np.pad(lim, pad)


def conv(x0, x1, w, bias, dtype="float32", stride=2, relu=False, scale=1.0, x0_limit=None, x1_limit=None, planted=None):
    """[relu](conv(cat([x0, x1]), stride) + bias) * scale for w [Cout,Cin,k,k], k 1 or 3, padding k // 2
    -> namespace(value, limit) [B,Cout,Ho,Wo].  planted: one of PLANTED (floor_size returns the smaller map)."""
    assert planted is None or planted in PLANTED
    assert stride in (1, 2)
    kw = dict(dtype=dtype, relu=relu, scale=scale, planted=planted if planted in ("flipped", "swapped") else None)
    if stride == 1:
        return CR.conv(x0, x1, w, bias, x0_limit=x0_limit, x1_limit=x1_limit, **kw)
    H, W = x0.shape[2:]
    Ho, Wo = out_size(H), out_size(W)
    if planted == "odd_phase":
        # windows centred at (2y + 1, 2x + 1): the window started at 2y instead of 2y - 1.  The stride-1 result of the map with a
        # row and a column of +0 behind it, at the odd positions.
        (p0, l0), (p1, l1) = _padded(x0, x0_limit), _padded(x1, x1_limit)
        full = CR.conv(p0, p1, w, bias, x0_limit=l0, x1_limit=l1, **kw)
        return _ns(full.value[:, :, 1::2, 1::2], full.limit[:, :, 1::2, 1::2])
    full = CR.conv(x0, x1, w, bias, x0_limit=x0_limit, x1_limit=x1_limit, **kw)
    cut = (slice(None, None, 2), slice(None, None, 2))
    if planted == "stride_x_only":
        cut = (slice(0, Ho), slice(None, None, 2))
    elif planted == "stride_y_only":
        cut = (slice(None, None, 2), slice(0, Wo))
    elif planted == "dense_1x1":                 # the cell at (y, x) of the top-left quarter where (2y, 2x) belongs
        assert w.shape[2] == 1
        cut = (slice(0, Ho), slice(0, Wo))
    v, lim = full.value[(slice(None), slice(None)) + cut], full.limit[(slice(None), slice(None)) + cut]
    if planted == "floor_size":                  # Ho = H / 2: the last row and column of an odd map are missing
        v, lim = v[:, :, :H // 2, :W // 2], lim[:, :, :H // 2, :W // 2]
    else:
        assert v.shape[2:] == (Ho, Wo)
    return _ns(v, lim)


def caught(got, ref, dtype="float32"):
    """Whether `got` (an array) leaves the referee: by its shape, or by a cell beyond the limit on the part they share."""
    if got.shape != ref.value.shape:
        return True
    return misses(got, ref, dtype) > 0


# ---------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_conv_strided.py
# ---------------------------------------------------------------------------------------------------
# name: (ksize, stride, B, C0, C1, Cout, H, W)
CASES = {
    "s2_even":  (3, 2, 2, 16, 0, 16, 16, 64),    # exactly one output tile, the 16-byte route, no cell beyond the map read
    "s2_odd":   (3, 2, 2, 32, 16, 14, 17, 67),   # 9 x 34 out; two sources; a row and two columns over a tile; bottom and right padding
    "s2_c96":   (3, 2, 2, 96, 0, 96, 5, 9),      # a bfloat16 chunk padded from 96 to 128; two channel blocks, the second of two N tiles
    "s2_tiles": (3, 2, 1, 16, 0, 16, 34, 130),   # 17 x 65 out: three tile rows and columns, halos shared between tiles
    "d2_even":  (1, 2, 2, 64, 0, 96, 18, 66),    # the downsample path
    "d2_odd":   (1, 2, 2, 32, 16, 25, 9, 13),    # the downsample path at odd sizes, two sources
    "px1":      (3, 2, 1, 16, 0, 16, 1, 1),      # one pixel in, one pixel out
    "px2":      (3, 2, 1, 16, 0, 16, 2, 2),      # two pixels in, one pixel out
}
# planted mistake -> the cases that claim to catch it
CATCHES = {"odd_phase": ("s2_even", "s2_odd", "s2_c96", "s2_tiles", "d2_even", "d2_odd", "px1", "px2"),
           "stride_x_only": ("s2_even", "s2_odd", "s2_c96", "s2_tiles", "d2_even", "d2_odd"),
           "stride_y_only": ("s2_even", "s2_odd", "s2_c96", "s2_tiles", "d2_even", "d2_odd"),
           "floor_size": ("s2_odd", "s2_c96", "d2_odd", "px1"),
           "dense_1x1": ("d2_even", "d2_odd"),
           "flipped": ("s2_even", "s2_odd", "s2_c96", "s2_tiles", "px2"),
           "swapped": ("s2_odd", "d2_odd")}


def case(name, dtype="float32"):
    """-> namespace(x0, x1 or None, w [Cout,Cin,k,k], bias, ...): weights of about 1.5 / sqrt(K), so that sums are of order 1."""
    ks, stride, B, C0, C1, Cout, H, W = CASES[name]
    rng = np.random.default_rng([6501, ks, stride, B, C0, C1, Cout, H, W])
    K = ks * ks * (C0 + C1)
    return SimpleNamespace(name=name, ksize=ks, stride=stride, B=B, C0=C0, C1=C1, Cout=Cout, H=H, W=W, Ho=out_size(H, stride),
                           Wo=out_size(W, stride), dtype=dtype, x0=R._cells(rng, (B, C0, H, W), dtype),
                           x1=R._cells(rng, (B, C1, H, W), dtype) if C1 else None,
                           w=(rng.standard_normal((Cout, C0 + C1, ks, ks)) * (1.5 / np.sqrt(K))).astype(F32),
                           bias=(rng.standard_normal(Cout) * 0.5).astype(F32))


def case_ref(c, **kw):
    kw = dict(dict(stride=c.stride), **kw)
    return conv(c.x0, c.x1, c.w, c.bias, dtype=c.dtype, **kw)


def nan_reach(ksize, H, W, y, x):
    """The [Ho, Wo] mask of output pixels whose window holds input cell (y, x) at stride 2."""
    reach = np.zeros((out_size(H), out_size(W)), bool)
    r = ksize // 2
    for oy in range(reach.shape[0]):
        for ox in range(reach.shape[1]):
            reach[oy, ox] = abs(2 * oy - y) <= r and abs(2 * ox - x) <= r
    return reach


# ---------------------------------------------------------------------------------------------------
# the recording (tests/golden/strided_cases.npz): the reference's ResidualBlock(16, 32, 'instance', stride=2)
# ---------------------------------------------------------------------------------------------------
def load_recording():
    return np.load(GOLDEN)


def recorded_convs(g, dtype="float32", planted=None):
    """The referee on the recording's input -> (conv1(x), downsample[0](x)), both at stride 2."""
    x = g["x"]
    if dtype == "bfloat16":
        x = to_bf16(x)
    c1 = conv(x, None, g["conv1.weight"], g["conv1.bias"], dtype, planted=planted if planted != "dense_1x1" else None)
    dn = conv(x, None, g["downsample.0.weight"], g["downsample.0.bias"], dtype, planted=planted)
    return c1, dn


# ---------------------------------------------------------------------------------------------------
# a spied Engine.raft_conv launch (tests/_raft_loop.LaunchSpy) against the referee, on the tensors it actually got
# ---------------------------------------------------------------------------------------------------
def check_launch(rec, module, what):
    """rec: a LaunchSpy record of raft_conv; module: the nn.Conv2d whose weights the launch ran with."""
    import _raft_loop as L
    from _cells import hold
    x0, cout, ksize = rec.args[0], rec.args[2], rec.args[3]
    kw = rec.kwargs
    dtype = L._dt(x0)
    w = module.weight.detach().float().cpu().numpy()
    b = None if module.bias is None else module.bias.detach().float().cpu().numpy()
    assert w.shape[0] == cout and w.shape[2] == ksize and module.stride[0] == kw.get("stride", 1), what
    ref = conv(L._np(x0), L._np(kw.get("x1")), w, b, dtype, stride=kw.get("stride", 1), relu=bool(kw.get("relu", False)),
               scale=kw.get("scale", 1.0))
    got = rec.result
    assert tuple(got.shape) == ref.value.shape, (what, tuple(got.shape), ref.value.shape)
    hold(CR, L._np(got), ref, what, dtype)
