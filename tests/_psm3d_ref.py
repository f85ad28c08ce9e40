"""Float64 referee, cases and planted wrong implementations for PSMNet's stride-1 3-D convolutions on the convolution kernel
(models/psmnet/psmnet.py:15-128, 199-213): the 3x3x3 convolution with a residual, a ReLU and a scale (conv_kernels.hip through
Engine.conv3d), the fold of a frozen BatchNorm3d (vppstereo_amd/_convs.fold_bn3d), and the blocks FusedRegularization composes
them into.  include/vppx.h has the arithmetic.

TEST INFRASTRUCTURE ONLY.  Plain numpy, no GPU: tests/test_psm3d_ref_cpu.py holds the referee to torch in float64 and shows on the
very arrays the GPU file (tests/test_gpu_psm3d.py) uploads that every planted mistake leaves the limit.

The convolution is the direct 3-D sum: 27 shifted windows of the zero-padded volume, each one matrix product over the input
channels.  It is NOT the reduction to 3 Cin pseudo-channels of a 3x3 kernel that the implementation uses: a referee built the
implementation's way would share a mistake in the reduction (tests/test_psm3d_ref_cpu.py checks that reduction against
tests/_psm_ref.conv2d separately, which pins the map the packing implements).

The limit is tests/_gruconv_ref.conv3x3's derivation with K = 27 Cin: every product rounded once (exactly, for bfloat16
operands), every one of the K additions once, in any order,
        limit = (K + 1) U (|bias| + sum_k |w_k x_k|) (1 + 2^-10)      + T per product (the ceiling of the count of products below
                                                                        T = 2^-126) + T for a result below T
The residual, the ReLU and the scale are tests/_psm_ref.conv2d's epilogue on this sum (its `pre` argument); bfloat16 storage is
band() of tests/_referee.py, and a cell that is read back carries tests/_gruconv_ref.stored()'s half unit.  There is no atol.

The fold is tests/_psm_ref.fold on the weight seen as [Cout,Cin,3,9]: value = the float64 result, limit = one rounding.  A
convolution run with folded weights against bn(conv(x)) carries that rounding through the sum, as tests/_psm_ref.convbn does.

What FusedRegularization leaves in torch (the stride-2 Conv3d, the ConvTranspose3d, their BatchNorm3d as an operation of its own)
has a referee here as well, so that a whole hourglass can be held: the stride-2 convolution is the stride-1 sum at the even
cells; the transposed one (k 3, stride 2, padding 1, output_padding 1) is the stride-1 sum over the input with a +0 behind every
cell and the kernel turned and transposed, K = 27 Cin being the ceiling of its products; a BatchNorm that is not folded is
        v = (y - mean) s + beta,  s = gamma / sqrt(var + eps):   limit = (limit_y |s| + 8 U (|y| + |mean|) |s| + 2 U (|beta| + |v|))
                                                                         (1 + 2^-10)   (+ T below T)
(three roundings in 1 / sqrt(var + eps), one each in the product with gamma, the difference, the product and the sum).
"""
import os
from types import SimpleNamespace

import numpy as np

import _gruconv_ref as R
import _psm_ref as PR
from _referee import SECOND_ORDER, TINY, U, _ns, _und, band, classes, compare, compare_bf16, misses, to_bf16  # noqa: F401

F32, F64 = np.float32, np.float64
PLANTED_SUM = ("dz_flipped", "depth_wraps", "depth_clamped", "channel_stride_hw")
PLANTED = PLANTED_SUM + ("res_behind_relu", "bn_no_eps")


# ---------------------------------------------------------------------------------------------------
# the convolution
# ---------------------------------------------------------------------------------------------------
def _mm(wk, a):
    """sum over c of wk[m][c] * a[b][c][z][y][x] as one matrix product per frame."""
    B, Cc = a.shape[:2]
    return np.matmul(wk, np.ascontiguousarray(a).reshape(B, Cc, -1)).reshape((B, wk.shape[0]) + a.shape[2:])


def _padded(x, planted=None):
    """x [B,C,D,H,W] -> [B,C,D+2,H+2,W+2]: +0 all round.  Planted: depth_wraps (plane -1 of frame b is plane D-1 of frame b-1, plane
    D of frame b plane 0 of frame b+1; +0 only in front of the first frame and behind the last), depth_clamped (the edge plane
    repeated), channel_stride_hw (channel c starts H*W cells behind channel c-1, not D*H*W)."""
    B, Cc, D, H, W = x.shape
    if planted == "channel_stride_hw":
        flat = x.reshape(B, Cc * D, H, W)
        x = np.stack([flat[:, c:c + D] for c in range(Cc)], axis=1)
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1), (1, 1)))
    if planted == "depth_clamped":
        xp[:, :, 0], xp[:, :, D + 1] = xp[:, :, 1], xp[:, :, D]
    elif planted == "depth_wraps":
        xp[1:, :, 0] = xp[:-1, :, D]
        xp[:-1, :, D + 1] = xp[1:, :, 1]
    return xp


def conv3d_sum(x, w, bias, dtype="float32", x_limit=None, w_limit=None, planted=None):
    """x [B,Cin,D,H,W], w [Cout,Cin,3,3,3] float32, bias [Cout] or None -> namespace(value, limit) [B,Cout,D,H,W] of
    nn.Conv3d(Cin, Cout, 3, stride=1, padding=1).  x_limit: a bound on every input cell, w_limit one on every weight, both carried
    through the sum.  planted: one of PLANTED_SUM.  A NaN input reaches every output channel through 0 * NaN as well, which is what
    the kernel's matrix instructions do."""
    assert planted is None or planted in PLANTED_SUM
    x = np.asarray(x, F64)
    B, Cin, D, H, W = x.shape
    w = R.weights_of(w, dtype).astype(F64)
    M = w.shape[0]
    assert w.shape == (M, Cin, 3, 3, 3), (w.shape, x.shape)
    if planted == "dz_flipped":
        w = w[:, :, ::-1]
    xp = _padded(x, planted)
    lp = None if x_limit is None else _padded(np.broadcast_to(np.asarray(x_limit, F64), x.shape))
    b = np.zeros(M) if bias is None else np.asarray(bias, F64)
    val = np.zeros((B, M, D, H, W)) + b[None, :, None, None, None]
    mag, prop = np.abs(val), np.zeros((B, M, D, H, W))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for dz in range(3):
            for dy in range(3):
                for dx in range(3):
                    cut = (slice(None), slice(None), slice(dz, dz + D), slice(dy, dy + H), slice(dx, dx + W))
                    win, wk = xp[cut], w[:, :, dz, dy, dx]
                    val += _mm(wk, win)
                    mag += _mm(np.abs(wk), np.abs(win))
                    if lp is not None:
                        prop += _mm(np.abs(wk), lp[cut])
                    if w_limit is not None:
                        prop += _mm(w_limit[:, :, dz, dy, dx], np.abs(win))
        K = 27 * Cin
        lim = ((K + 1) * U * mag + K * TINY + _und(val)) * SECOND_ORDER + prop
    return _ns(val, lim)


def conv3d(x, w, bias, dtype="float32", res=None, relu=False, scale=1.0, x_limit=None, res_limit=None, planted=None, pre=None):
    """[relu](conv(x) + bias [+ res]) * scale -> namespace(value, limit) [B,Cout,D,H,W].  planted: one of PLANTED but bn_no_eps (the
    fold's).  pre: conv3d_sum() of the same inputs, for the epilogues of one sum."""
    assert planted is None or planted in PLANTED
    a = pre if pre is not None else conv3d_sum(x, w, bias, dtype, x_limit=x_limit, planted=planted if planted in PLANTED_SUM else None)
    return PR.conv2d(None, None, w, None, dtype, res=res, relu=relu, scale=scale, res_limit=res_limit,
                     planted="res_behind_relu" if planted == "res_behind_relu" else None, pre=a)


def permuted(w):
    """w [Cout,Cin,3,3,3] -> the [Cout,3 Cin,3,3] weight of the pseudo-channels, w2[m][dz * Cin + c][dy][dx] = w[m][c][dz][dy][dx]:
    what Engine.conv3d_pack packs (include/vppx.h)."""
    w = np.asarray(w)
    M, Cin = w.shape[:2]
    return np.ascontiguousarray(w.transpose(0, 2, 1, 3, 4)).reshape(M, 3 * Cin, 3, 3)


def stacked(x):
    """x [B,Cin,D,H,W] -> [B*D,3 Cin,H,W]: frame (b, d) holds planes d-1, d, d+1 of every channel as pseudo-channels dz * Cin + c,
    +0 where the plane is outside the volume."""
    x = np.asarray(x)
    B, Cin, D, H, W = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (0, 0), (0, 0)))
    frames = [np.concatenate([xp[b, :, d + dz] for dz in range(3)], axis=0) for b in range(B) for d in range(D)]
    return np.stack(frames, axis=0)


def nan_reach(D, H, W, z, y, x):
    """The [D, H, W] mask of output cells whose 3x3x3 window holds input cell (z, y, x)."""
    reach = np.zeros((D, H, W), bool)
    reach[max(z - 1, 0):z + 2, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
    return reach


# ---------------------------------------------------------------------------------------------------
# the fold
# ---------------------------------------------------------------------------------------------------
def fold(w, conv_bias, gamma, beta, mean, var, eps, planted=None):
    """tests/_psm_ref.fold for w [Cout,Cin,3,3,3].  planted: bn_no_eps."""
    assert planted in (None, "bn_no_eps")
    w = np.asarray(w)
    wf, bf = PR.fold(w.reshape(w.shape[0], w.shape[1], 3, 9), conv_bias, gamma, beta, mean, var, eps, planted="no_eps" if planted else None)
    return _ns(wf.value.reshape(w.shape), wf.limit.reshape(w.shape)), bf


def convbn(x, w, conv_bias, bn, dtype="float32", planted=None, x_limit=None, **kw):
    """bn(conv(x)) with the bound of a float32 run on folded weights against the UNFOLDED formula: conv3d() on the float32-rounded
    fold, plus the one rounding each folded weight and bias carries through the sum.  bn: dict(gamma, beta, mean, var, eps); kw:
    conv3d's res, relu, scale, res_limit."""
    wf, bf = fold(w, conv_bias, bn.get("gamma"), bn.get("beta"), bn["mean"], bn["var"], bn["eps"], planted="bn_no_eps" if planted == "bn_no_eps" else None)
    a = conv3d_sum(x, wf.value.astype(F32), bf.value.astype(F32), dtype, x_limit=x_limit, w_limit=wf.limit,
                   planted=planted if planted in PLANTED_SUM else None)
    a = _ns(a.value, a.limit + bf.limit[None, :, None, None, None])
    return conv3d(None, w, None, dtype, planted=planted if planted == "res_behind_relu" else None, pre=a, **kw)


def bn_case(rng, C):
    return PR.bn_case(rng, C)


def bn_of(g, prefix, eps=1e-5):
    return PR.bn_of(g, prefix, eps)


# ---------------------------------------------------------------------------------------------------
# what stays in torch: stride 2, the transposed convolution, a BatchNorm3d that is not folded
# ---------------------------------------------------------------------------------------------------
def conv3d_stride2(x, w, bias, dtype="float32", x_limit=None):
    """nn.Conv3d(Cin, Cout, 3, stride=2, padding=1): the stride-1 sum at the even cells."""
    a = conv3d_sum(x, w, bias, dtype, x_limit=x_limit)
    return _ns(a.value[:, :, ::2, ::2, ::2], a.limit[:, :, ::2, ::2, ::2])


def conv_transpose3d(x, w, dtype="float32", x_limit=None):
    """nn.ConvTranspose3d(Cin, Cout, 3, stride=2, padding=1, output_padding=1, bias=False), w [Cin,Cout,3,3,3]: [B,Cin,D,H,W] ->
    [B,Cout,2D,2H,2W]."""
    x = np.asarray(x, F64)
    B, Cin, D, H, W = x.shape
    up, ul = np.zeros((B, Cin, 2 * D, 2 * H, 2 * W)), np.zeros((B, Cin, 2 * D, 2 * H, 2 * W))
    up[:, :, ::2, ::2, ::2] = x
    if x_limit is not None:
        ul[:, :, ::2, ::2, ::2] = x_limit
    wt = np.ascontiguousarray(np.asarray(w, F32).transpose(1, 0, 2, 3, 4)[:, :, ::-1, ::-1, ::-1])
    return conv3d_sum(up, wt, None, dtype, x_limit=ul)


def batchnorm(y, bn):
    """A BatchNorm3d in eval mode as an operation of its own on namespace y (the head of the file has the bound)."""
    e = lambda a: np.asarray(a, F64)[None, :, None, None, None]                         # noqa: E731
    C = y.value.shape[1]
    gamma = np.ones(C) if bn.get("gamma") is None else bn["gamma"]
    beta = np.zeros(C) if bn.get("beta") is None else bn["beta"]
    s = e(gamma) / np.sqrt(e(bn["var"]) + float(bn["eps"]))
    with np.errstate(invalid="ignore", over="ignore"):
        v = (y.value - e(bn["mean"])) * s + e(beta)
        lim = (y.limit * np.abs(s) + 8 * U * (np.abs(y.value) + np.abs(e(bn["mean"]))) * np.abs(s) + 2 * U * (np.abs(e(beta)) + np.abs(v))
               + _und(v)) * SECOND_ORDER
    return _ns(v, lim)


def torch_convbn(x, w, bn, dtype="float32", stride2=False, transposed=False, relu=False, x_limit=None):
    """What the wrapper leaves in torch: conv -> (stored) -> BatchNorm3d -> (stored) [-> ReLU], each result passing through memory
    in the volume's dtype."""
    y = conv_transpose3d(x, w, dtype, x_limit) if transposed else conv3d_stride2(x, w, None, dtype, x_limit) if stride2 else \
        conv3d_sum(x, w, None, dtype, x_limit=x_limit)
    v = R.stored(batchnorm(R.stored(y, dtype), bn), dtype)
    return _ns(R._relu(v.value), v.limit) if relu else v


def add(a, b, dtype="float32", relu=False):
    """[relu](a + b) of two namespaces as one float32 addition, stored in the volume's dtype."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = a.value + b.value
        out = R.stored(_ns(v, (a.limit + b.limit + U * np.abs(v) + _und(v)) * SECOND_ORDER), dtype)
    return _ns(R._relu(out.value), out.limit) if relu else out


def exact(a):
    return _ns(np.asarray(a, F64), np.zeros(np.shape(a)))


# ---------------------------------------------------------------------------------------------------
# the blocks of psmnet.py:199-213 on a state dict g[prefix + ...]
# ---------------------------------------------------------------------------------------------------
def dres1_block(x, g, prefix, dtype="float32", planted=None):
    """Sequential(convbn_3d, ReLU, convbn_3d)(x) + x -> namespace(value, limit, hidden): the hidden tensor passes through memory."""
    h0 = convbn(x, g[f"{prefix}0.0.weight"], None, bn_of(g, f"{prefix}0.1"), dtype, planted=planted, relu=True)
    h = R.stored(h0, dtype)
    out = convbn(h.value, g[f"{prefix}2.0.weight"], None, bn_of(g, f"{prefix}2.1"), dtype, planted=planted, x_limit=h.limit, res=np.asarray(x, F64))
    return _ns(out.value, out.limit, hidden=h0)


def hourglass(x, g, prefix, dtype="float32", presqu=None, postsqu=None):
    """hourglass.forward (psmnet.py:64-83) as FusedRegularization runs it: conv2 and conv4 folded, on the kernel; conv1, conv3,
    conv5, conv6 and the two sums behind the transposed convolutions in torch.  x, presqu, postsqu: arrays (exact cells).
    -> namespace(out, pre, post, conv2, conv4), each a namespace(value, limit); conv2 and conv4 as their launches are held."""
    w, bn = lambda n: g[f"{prefix}{n}.weight"], lambda n: bn_of(g, f"{prefix}{n}")       # noqa: E731
    o1 = torch_convbn(x, w("conv1.0.0"), bn("conv1.0.1"), dtype, stride2=True, relu=True)
    c2 = convbn(o1.value, w("conv2.0"), None, bn("conv2.1"), dtype, x_limit=o1.limit, res=postsqu, relu=True)
    pre = R.stored(c2, dtype)
    o3 = torch_convbn(pre.value, w("conv3.0.0"), bn("conv3.0.1"), dtype, stride2=True, relu=True, x_limit=pre.limit)
    c4 = convbn(o3.value, w("conv4.0.0"), None, bn("conv4.0.1"), dtype, x_limit=o3.limit, relu=True)
    o4 = R.stored(c4, dtype)
    t5 = torch_convbn(o4.value, w("conv5.0"), bn("conv5.1"), dtype, transposed=True, x_limit=o4.limit)
    post = add(t5, pre if presqu is None else exact(presqu), dtype, relu=True)
    out = torch_convbn(post.value, w("conv6.0"), bn("conv6.1"), dtype, transposed=True, x_limit=post.limit)
    return SimpleNamespace(out=out, pre=pre, post=post, conv2=c2, conv4=c4)


# ---------------------------------------------------------------------------------------------------
# cases: the grid of tests/test_gpu_psm3d.py and the named points of tests/test_psm3d_ref_cpu.py
# ---------------------------------------------------------------------------------------------------
SWEEP_B = 2                                   # a wrap between batch frames shows
SWEEP_DEPTHS = (1, 2, 3, 5)                   # at D = 1 both neighbour planes are outside
SWEEP_CINS = (16, 32, 64)                     # at 16 a bfloat16 chunk straddles planes and K = 48 is padded to 64
SWEEP_COUTS = (1, 32, 80)                     # 1 and 80: a masked store; 80: a second channel block
SWEEP_MAPS = ((9, 33), (8, 32), (3, 5))       # part tiles in both directions; the 16-byte route; a map smaller than a tile
EPILOGUES = PR.EPILOGUES                      # (res, relu, scale) for res, relu in (False, True) and scale in (1.0, 0.25)

# name: (B, Cin, Cout, D, H, W, res, relu, scale)
CASES = {
    "straddle": (2, 16, 32, 3, 9, 33, True, True, 0.25),       # one and a half bfloat16 chunks of K; part tiles
    "deep":     (2, 32, 80, 5, 8, 32, True, True, 1.0),        # two channel blocks; the 16-byte route
    "head":     (2, 64, 1, 2, 3, 5, True, False, 1.0),         # a classifier's Cout = 1 with its sum; a map smaller than a tile
    "flat":     (2, 16, 1, 1, 9, 33, False, True, 1.0),        # D = 1: both neighbour planes are outside
}
# planted mistake -> the cases that claim to catch it  (flat: with one plane, dz_flipped and channel_stride_hw read the same cells)
CATCHES = {"dz_flipped": ("straddle", "deep", "head"), "depth_wraps": ("straddle", "deep", "head", "flat"),
           "depth_clamped": ("straddle", "deep", "head", "flat"), "channel_stride_hw": ("straddle", "deep", "head"),
           "res_behind_relu": ("straddle", "deep")}


def make(B, Cin, Cout, D, H, W, dtype="float32", res=True, relu=False, scale=1.0, name=None):
    """-> namespace(x, w, bias, res or None, ...): weights of about 1.5 / sqrt(K), so that sums are of order 1.  The arrays depend on
    the shape alone: a case with and without its residual has the same inputs."""
    rng = np.random.default_rng([7601, B, Cin, Cout, D, H, W])
    c = SimpleNamespace(name=name, B=B, Cin=Cin, Cout=Cout, D=D, H=H, W=W, relu=relu, scale=scale, dtype=dtype,
                        x=R._cells(rng, (B, Cin, D, H, W), dtype),
                        w=(rng.standard_normal((Cout, Cin, 3, 3, 3)) * (1.5 / np.sqrt(27 * Cin))).astype(F32),
                        bias=(rng.standard_normal(Cout) * 0.5).astype(F32), res=R._cells(rng, (B, Cout, D, H, W), dtype))
    if not res:
        c.res = None
    return c


def case(name, dtype="float32"):
    B, Cin, Cout, D, H, W, res, relu, scale = CASES[name]
    return make(B, Cin, Cout, D, H, W, dtype, res, relu, scale, name)


def case_ref(c, planted=None):
    return conv3d(c.x, c.w, c.bias, c.dtype, res=c.res, relu=c.relu, scale=c.scale, planted=planted)


def caught(got, ref, dtype="float32"):
    return PR.caught(got, ref, dtype)


# ---------------------------------------------------------------------------------------------------
# the recording (tests/golden/psm3d_cases.npz): the reference's own dres1-shaped block and its hourglass(16)
# ---------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "psm3d_cases.npz")
DRES1_SHAPE = (2, 16, 3, 9, 13)
HG_SHAPE, HG_SQU = (1, 16, 4, 8, 12), (1, 32, 2, 4, 6)


def load_recording():
    return np.load(GOLDEN)


def _formula(shape, k, mul, mod, den, off=0.0):
    """Tensor k of a module: off + ((mul * i + 3 * k) % mod - mod // 2) / den over the flat index i; exact in float32."""
    i = np.arange(int(np.prod(shape)), dtype=np.int64)
    return (off + ((mul * i + 3 * k) % mod - mod // 2) / float(den)).astype(F32).reshape(shape)


def hourglass_input():
    """[1,16,4,8,12]: multiples of 1/8 between -15/8 and 15/8."""
    return _formula(HG_SHAPE, 0, 7, 31, 8)


def hourglass_state(inplanes=16):
    """The state dict of hourglass(inplanes) by integer formulas, key for key (num_batches_tracked aside): convolution weights
    multiples of 1/128 within +-6/128, gamma 1 +- 4/16, beta +- 3/8, running_mean +- 5/16, running_var 0.5 .. 1.375."""
    c, c2 = inplanes, 2 * inplanes
    convs = {"conv1.0.0": (c2, c), "conv2.0": (c2, c2), "conv3.0.0": (c2, c2), "conv4.0.0": (c2, c2), "conv5.0": (c2, c2), "conv6.0": (c2, c)}
    norms = {"conv1.0.1": c2, "conv2.1": c2, "conv3.0.1": c2, "conv4.0.1": c2, "conv5.1": c2, "conv6.1": c}
    g = {}
    for k, (name, (a, b)) in enumerate(convs.items()):
        g[f"{name}.weight"] = _formula((a, b, 3, 3, 3), k, 7, 13, 128)
    for k, (name, n) in enumerate(norms.items()):
        g[f"{name}.weight"] = _formula((n,), k, 3, 9, 16, 1.0)
        g[f"{name}.bias"] = _formula((n,), k, 5, 7, 8)
        g[f"{name}.running_mean"] = _formula((n,), k, 7, 11, 16)
        g[f"{name}.running_var"] = _formula((n,), k, 3, 8, 8, 1.0)
    return g


# ---------------------------------------------------------------------------------------------------
# a stand-in of the reference's structure, and a spied launch against its referee
# ---------------------------------------------------------------------------------------------------
def standin(cin=32, c=16, seed=0):
    """A torch module with `dres0` .. `dres4` and `classif1` .. `classif3` laid out as models/psmnet/psmnet.py:15-128 lays them
    out, at `c` channels (2 c inside an hourglass) on a `cin`-channel volume, seeded and in eval mode.  Its forward is
    psmnet.py:199-213 in plain torch -> cost3."""
    import torch
    nn = torch.nn

    def convbn_3d(a, b, stride=1):
        return nn.Sequential(nn.Conv3d(a, b, kernel_size=3, padding=1, stride=stride, bias=False), nn.BatchNorm3d(b))

    def up(a, b):
        return nn.Sequential(nn.ConvTranspose3d(a, b, kernel_size=3, padding=1, output_padding=1, stride=2, bias=False), nn.BatchNorm3d(b))

    class Hourglass(nn.Module):
        def __init__(self, n):
            super().__init__()
            self.conv1 = nn.Sequential(convbn_3d(n, 2 * n, 2), nn.ReLU(inplace=True))
            self.conv2 = convbn_3d(2 * n, 2 * n)
            self.conv3 = nn.Sequential(convbn_3d(2 * n, 2 * n, 2), nn.ReLU(inplace=True))
            self.conv4 = nn.Sequential(convbn_3d(2 * n, 2 * n), nn.ReLU(inplace=True))
            self.conv5, self.conv6 = up(2 * n, 2 * n), up(2 * n, n)

        def forward(self, x, presqu, postsqu):
            out = self.conv1(x)
            pre = self.conv2(out)
            pre = torch.relu(pre + postsqu) if postsqu is not None else torch.relu(pre)
            out = self.conv4(self.conv3(pre))
            post = torch.relu(self.conv5(out) + (presqu if presqu is not None else pre))
            return self.conv6(post), pre, post

    class Regularization(nn.Module):
        def __init__(self):
            super().__init__()
            self.dres0 = nn.Sequential(convbn_3d(cin, c), nn.ReLU(inplace=True), convbn_3d(c, c), nn.ReLU(inplace=True))
            self.dres1 = nn.Sequential(convbn_3d(c, c), nn.ReLU(inplace=True), convbn_3d(c, c))
            self.dres2, self.dres3, self.dres4 = Hourglass(c), Hourglass(c), Hourglass(c)
            for k in (1, 2, 3):
                setattr(self, f"classif{k}", nn.Sequential(convbn_3d(c, c), nn.ReLU(inplace=True),
                                                           nn.Conv3d(c, 1, kernel_size=3, padding=1, stride=1, bias=False)))

        def forward(self, cost):
            cost0 = self.dres0(cost)
            cost0 = self.dres1(cost0) + cost0
            out1, pre1, post1 = self.dres2(cost0, None, None)
            out1 = out1 + cost0
            out2, pre2, post2 = self.dres3(out1, pre1, post1)
            out2 = out2 + cost0
            out3, pre3, post3 = self.dres4(out2, pre1, post2)
            out3 = out3 + cost0
            cost1 = self.classif1(out1)
            cost2 = self.classif2(out2) + cost1
            return self.classif3(out3) + cost2

    m = Regularization()
    seed_module(m, torch.Generator().manual_seed(7701 + seed))
    return m.eval()


def seed_module(mod, gen):
    """Seeded BatchNorm3d statistics and affine parameters; convolution weights of about 1.5 / sqrt(K)."""
    import torch
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, (torch.nn.Conv3d, torch.nn.ConvTranspose3d)):
                K = 27 * m.in_channels // (8 if isinstance(m, torch.nn.ConvTranspose3d) else 1)
                m.weight.copy_(torch.randn(m.weight.shape, generator=gen) * (1.5 / K ** 0.5))
            elif isinstance(m, torch.nn.BatchNorm3d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=gen) * 0.5)
                m.running_var.copy_(torch.rand(m.num_features, generator=gen) + 0.5)
                m.weight.copy_(1.0 + 0.3 * torch.randn(m.num_features, generator=gen))
                m.bias.copy_(0.3 * torch.randn(m.num_features, generator=gen))
    return mod.eval()


def launch_plan(m):
    """The (Conv3d, BatchNorm3d or None, relu, has a residual) of every Engine.conv3d launch of FusedRegularization.forward, in its
    order."""
    plan = [(m.dres0[0][0], m.dres0[0][1], True, False), (m.dres0[2][0], m.dres0[2][1], True, False),
            (m.dres1[0][0], m.dres1[0][1], True, False), (m.dres1[2][0], m.dres1[2][1], False, True)]
    for hg, post in ((m.dres2, False), (m.dres3, True), (m.dres4, True)):
        plan += [(hg.conv2[0], hg.conv2[1], True, post), (hg.conv4[0][0], hg.conv4[0][1], True, False)]
    for cl, res in ((m.classif1, False), (m.classif2, True), (m.classif3, True)):
        plan += [(cl[0][0], cl[0][1], True, False), (cl[2], None, False, res)]
    return plan


def check_conv3d_launch(rec, conv, bn, relu, has_res, what):
    """rec: a LaunchSpy record of Engine.conv3d; conv, bn: the modules whose folded weights the launch ran with."""
    import _raft_loop as L
    from _cells import hold
    x, cout = rec.args[0], rec.args[2]
    kw = rec.kwargs
    dtype = L._dt(x)
    n = lambda t: None if t is None else t.detach().float().cpu().numpy()                 # noqa: E731
    assert conv.out_channels == cout and bool(kw.get("relu", False)) == relu and (kw.get("residual") is not None) == has_res, what
    args = dict(res=L._np(kw.get("residual")), relu=relu, scale=kw.get("scale", 1.0))
    if bn is None:
        ref = conv3d(L._np(x), n(conv.weight), n(conv.bias), dtype, **args)
    else:
        bnd = dict(gamma=n(bn.weight), beta=n(bn.bias), mean=n(bn.running_mean), var=n(bn.running_var), eps=bn.eps)
        ref = convbn(L._np(x), n(conv.weight), n(conv.bias), bnd, dtype, **args)
    got = rec.result
    assert tuple(got.shape) == ref.value.shape, (what, tuple(got.shape), ref.value.shape)
    hold(PR, L._np(got), ref, what, dtype)
