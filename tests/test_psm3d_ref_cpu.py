"""The referee of tests/test_gpu_psm3d.py (tests/_psm3d_ref.py) held to torch in float64, the pseudo-channel map the packing
implements held to the 2-D referee, every planted mistake shown to leave the limit on the very arrays the GPU file uploads, and what
vppstereo_amd/_convs.py decides about a Conv3d and folds of a BatchNorm3d.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import _psm3d_ref as P3
import _psm_ref as PR

F32, F64 = np.float32, np.float64
nn = torch.nn
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("vppx_conv3d_packed_bytes", "vppx_conv3d_pack_dev", "vppx_conv3d_dt_dev")


def _t64(a):
    return torch.from_numpy(np.asarray(a, F64))


# ---- the referee against torch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P3.CASES))
def test_the_referee_equals_torch_in_float64(name):
    c = P3.case(name)
    a = P3.conv3d_sum(c.x, c.w, c.bias)
    want = nn.functional.conv3d(_t64(c.x), _t64(c.w), _t64(c.bias), padding=1).numpy()
    mag = nn.functional.conv3d(_t64(np.abs(c.x)), _t64(np.abs(c.w)), _t64(np.abs(c.bias)), padding=1).numpy()
    assert a.value.shape == want.shape == (c.B, c.Cout, c.D, c.H, c.W)
    assert (np.abs(a.value - want) <= 1e-12 * mag).all()
    # the limit is the derivation's: (K + 1) U (|bias| + sum |w x|) (1 + 2^-10) plus the subnormal terms
    K = 27 * c.Cin
    low = (K + 1) * P3.U * mag * P3.SECOND_ORDER
    assert (a.limit >= low * (1 - 1e-9)).all() and (a.limit <= low * (1 + 1e-9) + (K + 1) * P3.TINY * P3.SECOND_ORDER).all()
    # the epilogue: residual in front of the ReLU, then the scale
    full = P3.case_ref(c)
    v = _t64(want) + (0 if c.res is None else _t64(c.res))
    v = (torch.relu(v) if c.relu else v) * c.scale
    assert (np.abs(full.value - v.numpy()) <= 1e-12 * (mag + 1)).all() and (full.limit >= a.limit * abs(c.scale)).all()


def test_stride_two_and_the_transposed_convolution_equal_torch_in_float64():
    rng = np.random.default_rng(7611)
    x, w = rng.standard_normal((2, 16, 4, 6, 5)), rng.standard_normal((32, 16, 3, 3, 3)).astype(F32)
    got = P3.conv3d_stride2(x, w, None).value
    want = nn.functional.conv3d(_t64(x), _t64(w), stride=2, padding=1).numpy()
    assert got.shape == want.shape == (2, 32, 2, 3, 3) and np.abs(got - want).max() <= 1e-11
    wt = rng.standard_normal((16, 32, 3, 3, 3)).astype(F32)
    got = P3.conv_transpose3d(x, wt).value
    want = nn.functional.conv_transpose3d(_t64(x), _t64(wt), stride=2, padding=1, output_padding=1).numpy()
    assert got.shape == want.shape == (2, 32, 8, 12, 10) and np.abs(got - want).max() <= 1e-11
    bn = PR.bn_case(rng, 32)
    y = P3.batchnorm(P3.exact(want), bn)
    ref = nn.functional.batch_norm(_t64(want), _t64(bn["mean"]), _t64(bn["var"]), _t64(bn["gamma"]), _t64(bn["beta"]), False, 0.0, bn["eps"]).numpy()
    assert np.abs(y.value - ref).max() <= 1e-11 and (y.limit > 0).all()


# ---- the map the packing implements --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P3.CASES))
def test_the_permuted_weight_on_stacked_planes_is_the_3d_sum(name):
    """w -> [Cout][3 Cin][3][3] with w2[m][dz * Cin + c] = w[m][c][dz], frame (b, d) = planes d-1 .. d+1 stacked as pseudo-channels:
    tests/_psm_ref.conv2d of that is the referee's 3-D sum, value and limit (K = 9 * 3 Cin = 27 Cin)."""
    c = P3.case(name)
    a = P3.conv3d_sum(c.x, c.w, c.bias)
    w2 = P3.permuted(c.w)
    assert w2.shape == (c.Cout, 3 * c.Cin, 3, 3)
    for m, q, dz in ((0, 0, 0), (c.Cout - 1, c.Cin, 1), (0, 3 * c.Cin - 1, 2), (c.Cout // 2, c.Cin + 3, 1)):
        assert np.array_equal(w2[m, q], c.w[m, q - dz * c.Cin, dz])
    assert np.array_equal(w2, torch.from_numpy(c.w).permute(0, 2, 1, 3, 4).reshape(c.Cout, 3 * c.Cin, 3, 3).numpy())
    flat = PR.conv2d(P3.stacked(c.x), None, w2, c.bias)
    val = flat.value.reshape(c.B, c.D, c.Cout, c.H, c.W).transpose(0, 2, 1, 3, 4)
    lim = flat.limit.reshape(c.B, c.D, c.Cout, c.H, c.W).transpose(0, 2, 1, 3, 4)
    scale = np.abs(a.value) + a.limit / P3.U
    assert (np.abs(val - a.value) <= 1e-12 * scale).all()
    assert (lim <= a.limit * (1 + 1e-9)).all() and (lim >= a.limit * 0.99 - 28 * c.Cin * P3.TINY).all()


# ---- the planted mistakes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("name", list(P3.CASES))
def test_the_unplanted_referee_stays_inside_its_own_limit(name, dtype):
    c = P3.case(name, dtype)
    ref = P3.case_ref(c)
    got = ref.value.astype(F32)
    got = P3.to_bf16(got) if dtype == "bfloat16" else got
    assert not P3.caught(got, ref, dtype)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("planted, name", [(p, n) for p, names in P3.CATCHES.items() for n in names])
def test_every_planted_mistake_leaves_the_limit(planted, name, dtype):
    c = P3.case(name, dtype)
    ref = P3.case_ref(c)
    wrong = P3.case_ref(c, planted=planted).value.astype(F32)
    wrong = P3.to_bf16(wrong) if dtype == "bfloat16" else wrong
    assert P3.caught(wrong, ref, dtype), (planted, name)


def test_every_planted_mistake_is_claimed():
    assert set(P3.CATCHES) | {"bn_no_eps"} == set(P3.PLANTED)
    for name in ("straddle", "deep", "head"):                          # at D >= 2 every mistake of the sum moves a value
        c = P3.case(name)
        base = P3.conv3d_sum(c.x, c.w, c.bias).value
        for planted in P3.PLANTED_SUM:
            assert not np.array_equal(P3.conv3d_sum(c.x, c.w, c.bias, planted=planted).value, base), (name, planted)
    c = P3.case("flat")                                                # one plane: the two that read the same cells there
    base = P3.conv3d_sum(c.x, c.w, c.bias).value
    assert np.array_equal(P3.conv3d_sum(c.x, c.w, c.bias, planted="channel_stride_hw").value, base)
    # depth_wraps: frame 0 reads frame 1 behind its last plane and frame 1 reads frame 0 in front of its first, nothing else moves
    c = P3.case("straddle")
    base, wrap = P3.conv3d_sum(c.x, c.w, c.bias).value, P3.conv3d_sum(c.x, c.w, c.bias, planted="depth_wraps").value
    assert np.array_equal(base[0, :, :-1], wrap[0, :, :-1]) and np.array_equal(base[1, :, 1:], wrap[1, :, 1:])
    assert not np.array_equal(base[0, :, -1], wrap[0, :, -1]) and not np.array_equal(base[1, :, 0], wrap[1, :, 0])


# ---- the fold -----------------------------------------------------------------------------------------------------------------------
def _convbn3d(cin, cout, seed, bias=False, affine=True):
    gen = torch.Generator().manual_seed(seed)
    conv, bn = nn.Conv3d(cin, cout, 3, padding=1, bias=bias), nn.BatchNorm3d(cout, affine=affine)
    with torch.no_grad():
        if bias:
            conv.bias.copy_(torch.randn(cout, generator=gen) * 0.5)
        if affine:
            P3.seed_module(nn.Sequential(conv, bn), gen)
        else:                                         # a norm without gamma and beta: the statistics alone
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) * 0.07)
            bn.running_mean.copy_(torch.randn(cout, generator=gen) * 0.5)
            bn.running_var.copy_(torch.rand(cout, generator=gen) + 0.5)
    return conv.eval(), bn.eval()


@pytest.mark.parametrize("bias, affine", [(False, True), (True, True), (False, False)])
def test_fold_bn3d_is_the_float64_formula(bias, affine):
    from vppstereo_amd._convs import fold_bn3d
    conv, bn = _convbn3d(16, 32, 7621, bias, affine)
    w, b = fold_bn3d(conv, bn)
    assert w.dtype == b.dtype == torch.float32 and tuple(w.shape) == (32, 16, 3, 3, 3) and tuple(b.shape) == (32,) and w.is_contiguous()
    n = lambda t: None if t is None else t.detach().numpy()                               # noqa: E731
    wf, bf = P3.fold(n(conv.weight), n(conv.bias), n(bn.weight), n(bn.bias), n(bn.running_mean), n(bn.running_var), bn.eps)
    assert np.array_equal(w.numpy(), wf.value.astype(F32)) and np.array_equal(b.numpy(), bf.value.astype(F32))
    s = (n(bn.weight).astype(F64) if affine else 1.0) / np.sqrt(n(bn.running_var).astype(F64) + bn.eps)
    want = n(conv.weight).astype(F64) * s[:, None, None, None, None]
    assert (np.abs(wf.value - want) <= 4 * 2.0 ** -53 * np.abs(want)).all()
    # folded against bn(conv(x)) in float64, within the one-rounding bound of tests/_psm_ref.py
    x = np.random.default_rng(7622).standard_normal((2, 16, 3, 5, 7))
    with torch.no_grad():
        want = bn.double()(conv.double()(_t64(x))).numpy()
    got = nn.functional.conv3d(_t64(x), w.double(), b.double(), padding=1).numpy()
    bnd = dict(gamma=n(bn.weight), beta=n(bn.bias), mean=n(bn.running_mean), var=n(bn.running_var), eps=bn.eps)
    ref = P3.convbn(x, n(conv.weight).astype(F32), None if conv.bias is None else n(conv.bias).astype(F32), bnd)
    assert (np.abs(ref.value - got) <= 1e-12 * (np.abs(want) + 1)).all() and (np.abs(got - want) <= ref.limit).all()
    # bn_no_eps: 1e-5 of a variance of order 1 shows on the fold alone, against its one rounding
    ww, bw = P3.fold(n(conv.weight), n(conv.bias), n(bn.weight), n(bn.bias), n(bn.running_mean), n(bn.running_var), bn.eps, planted="bn_no_eps")
    assert P3.caught(ww.value.astype(F32), wf) or P3.caught(bw.value.astype(F32), bf)
    assert not P3.caught(w.numpy(), wf) and not P3.caught(b.numpy(), bf)


def test_fold_bn3d_refuses_what_cannot_be_folded():
    from vppstereo_amd._convs import fold_bn3d, frozen_bn3d
    conv, bn = _convbn3d(16, 16, 7623)
    with pytest.raises(TypeError, match="is BatchNorm2d, not a BatchNorm3d"):
        frozen_bn3d(nn.BatchNorm2d(16).eval(), "the norm")
    with pytest.raises(TypeError, match="training mode"):
        fold_bn3d(conv, bn.train())
    with pytest.raises(TypeError, match="no running statistics"):
        fold_bn3d(conv, nn.BatchNorm3d(16, track_running_stats=False).eval())


# ---- what the kernel takes ----------------------------------------------------------------------------------------------------------
def test_conv3d_plain_takes_the_references_stride_one_layers_and_nothing_else():
    from vppstereo_amd._convs import conv3d_plain
    c3 = lambda a, b, **kw: nn.Conv3d(a, b, **dict(dict(kernel_size=3, padding=1, stride=1, bias=False), **kw))   # noqa: E731
    for cin, cout in ((64, 32), (32, 32), (64, 64), (32, 1), (16, 16), (160, 256)):
        assert conv3d_plain(c3(cin, cout), cin), (cin, cout)
    assert conv3d_plain(c3(32, 32, bias=True), 32)
    assert not conv3d_plain(c3(32, 64, stride=2), 32)                              # the hourglass's conv1 and conv3
    assert not conv3d_plain(c3(32, 32, stride=(1, 1, 2)), 32)
    assert not conv3d_plain(nn.ConvTranspose3d(64, 64, kernel_size=3, padding=1, output_padding=1, stride=2, bias=False), 64)
    assert not conv3d_plain(c3(8, 32), 8) and not conv3d_plain(c3(176, 32), 176) and not conv3d_plain(c3(24, 32), 24)
    assert not conv3d_plain(c3(32, 257), 32)
    assert not conv3d_plain(c3(32, 32), 64)                                        # not the channels it is run on
    assert not conv3d_plain(c3(32, 32, kernel_size=1, padding=0), 32) and not conv3d_plain(c3(32, 32, kernel_size=(1, 3, 3), padding=(0, 1, 1)), 32)
    assert not conv3d_plain(c3(32, 32, padding=0), 32) and not conv3d_plain(c3(32, 32, dilation=2, padding=2), 32)
    assert not conv3d_plain(c3(32, 32, groups=2), 32) and not conv3d_plain(c3(32, 32, padding_mode="replicate"), 32)
    assert not conv3d_plain(nn.Conv2d(32, 32, 3, padding=1), 32)

    class Own(nn.Conv3d):
        def forward(self, x):
            return super().forward(x) * 2

    assert not conv3d_plain(Own(32, 32, 3, padding=1), 32)


def test_the_wrapper_checks_the_structure():
    from vppstereo_amd.psmnet import FusedRegularization
    m = P3.standin()
    w = FusedRegularization(m)
    assert w.launches() == 16 and w.model is m and [k for k in w.state_dict()][0].startswith("model.")
    assert len(P3.launch_plan(m)) == 16
    with pytest.raises(TypeError, match="dtype is"):
        FusedRegularization(m, dtype=torch.float16)
    with pytest.raises(TypeError, match="has no 'dres3'"):
        FusedRegularization(nn.ModuleDict({k: v for k, v in m.named_children() if k != "dres3"}))
    with pytest.raises(TypeError, match=r"dres0\[1\] is Identity, not a ReLU"):
        bad = P3.standin()
        bad.dres0[1] = nn.Identity()
        FusedRegularization(bad)
    with pytest.raises(TypeError, match=r"dres2.conv5\[0\] is Conv3d, not a ConvTranspose3d"):
        bad = P3.standin()
        bad.dres2.conv5[0] = nn.Conv3d(32, 32, 3, padding=1)
        FusedRegularization(bad)
    with pytest.raises(TypeError, match=r"classif2\[2\] is ReLU, not a Conv3d"):
        bad = P3.standin()
        bad.classif2[2] = nn.ReLU()
        FusedRegularization(bad)
    with pytest.raises(TypeError, match=r"dres1\[2\]\[1\] is in training mode"):
        bad = P3.standin()
        bad.dres1[2][1].train()
        FusedRegularization(bad)
    with pytest.raises(TypeError, match=r"dres4 has no 'conv6'"):
        bad = P3.standin()
        del bad.dres4.conv6
        FusedRegularization(bad)
    # a convolution the kernel does not take is counted out, not refused: 8 channels in the classifiers
    odd = P3.standin()
    odd.classif1[0] = nn.Sequential(nn.Conv3d(16, 8, 3, padding=1, bias=False), nn.BatchNorm3d(8)).eval()
    odd.classif1[2] = nn.Conv3d(8, 1, 3, padding=1, bias=False)
    assert FusedRegularization(odd).launches() == 15


def test_the_recording_holds_what_the_formulas_and_the_referee_say():
    g = P3.load_recording()
    assert all(g[k].dtype.kind in "fiu" for k in g.files)
    assert tuple(g["dres1.x"].shape) == P3.DRES1_SHAPE and tuple(g["hg.out"].shape) == P3.HG_SHAPE
    ref = P3.dres1_block(g["dres1.x"], g, "dres1.")
    assert (np.abs(g["dres1.out"].astype(F64) - ref.value) <= 2 * ref.limit).all()
    for planted in P3.PLANTED_SUM:                # (no ReLU behind the block's sum; bn_no_eps shows on the fold alone, above)
        wrong = P3.dres1_block(g["dres1.x"], g, "dres1.", planted=planted).value.astype(F32)
        assert (np.abs(wrong - ref.value) > 2 * ref.limit).any(), planted
    state = P3.hourglass_state(16)
    for k, v in state.items():
        assert v.dtype == F32 and np.array_equal(v.astype(F64) * 128, np.round(v.astype(F64) * 128)), k
    hg = P3.hourglass(P3.hourglass_input(), state, "", presqu=g["hg.presqu"], postsqu=g["hg.postsqu"])
    for name in ("out", "pre", "post"):
        r = getattr(hg, name)
        assert r.value.shape == g[f"hg.{name}"].shape
        assert (np.abs(g[f"hg.{name}"].astype(F64) - r.value) <= 2 * r.limit).all(), name


# ---- the entry points in the header, the library and the binding -----------------------------------------------------------------
def test_the_three_entry_points_are_declared_exported_and_bound():
    import ctypes as C
    from vppstereo_amd import _lib
    with open(os.path.join(ROOT, "include", "vppx.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b(int|size_t) " + name + r"\(", header), name
        assert name in _lib.EXPORTS
    assert header.index("int vppx_conv2d_dt_dev(") < header.index("int vppx_conv3d_dt_dev(") < header.index("int vppx_psm_spp_pool_dt_dev(")
    assert "vppx_conv3d_dt_dev" in header[:header.index("Conventions")]                  # the table of reference lines
    protos = _lib.ABI.protos
    i, i64, vp = C.c_int, C.c_int64, C.c_void_p
    assert protos["vppx_conv3d_packed_bytes"] == (C.c_size_t, [i, i, i])
    assert protos["vppx_conv3d_pack_dev"] == (i, [vp, vp, i, i, i, vp, vp])
    assert protos["vppx_conv3d_dt_dev"] == (i, [vp, i64, i, vp, i, i, i, i, i, vp, i64, i, C.c_float, vp, i64, i, vp])
    lib = C.CDLL(_lib.LIB_PATH)                    # the library's own symbol table, without the binding
    for name in ENTRY_POINTS:
        assert getattr(lib, name) is not None, name
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert getattr(lib, name).argtypes == protos[name][1]
    # the size is host arithmetic: what the 2-D call says of the permuted weight, 0 for what is not built
    assert lib.vppx_conv3d_packed_bytes(32, 64, 1) == lib.vppx_raft_conv_packed_bytes(32, 192, 3, 1) > 0
    assert lib.vppx_conv3d_packed_bytes(1, 160, 0) == lib.vppx_raft_conv_packed_bytes(1, 480, 3, 0) > 0
    for cout, cin, dt in ((32, 8, 0), (32, 176, 0), (32, 0, 0), (0, 32, 0), (257, 32, 1), (32, 32, 2)):
        assert lib.vppx_conv3d_packed_bytes(cout, cin, dt) == 0
    # a NULL context is refused by each before anything else
    assert lib.vppx_conv3d_dt_dev(None, 0, 0, None, 0, 0, 0, 0, 0, None, 0, 0, 0.0, None, 0, 0, None) == -7
    assert lib.vppx_conv3d_pack_dev(None, None, 0, 0, 0, None, None) == -7
