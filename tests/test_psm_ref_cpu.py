"""The referee of tests/_psm_ref.py held to torch on the CPU in float64, its planted mistakes shown to leave the limit on the very
arrays tests/test_gpu_psm_features.py uploads, and what PSMNet's feature path adds outside the kernels: the three entry points in
the header, the library and the binding, conv_plain's rule, the fold of a frozen BatchNorm and its cache.  No GPU."""
import copy
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _gruconv_ref as R
import _psm_ref as PR

F32, F64 = np.float32, np.float64


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("vppx_conv2d_dt_dev", "vppx_psm_spp_pool_dt_dev", "vppx_raft_gru_assemble_strided_dt_dev")


def _t64(a):
    return None if a is None else torch.from_numpy(np.asarray(a, F64))


def _torch_conv(c, dtype):
    x = _t64(c.x0 if c.x1 is None else np.concatenate([c.x0, c.x1], axis=1))
    v = torch.nn.functional.conv2d(x, _t64(R.weights_of(c.w, dtype)), _t64(c.bias), padding=c.dilation * (c.ksize // 2), dilation=c.dilation)
    if c.res is not None:
        v = v + _t64(c.res)
    if c.relu:
        v = torch.relu(v)
    return (v * float(F32(c.scale))).numpy()


# ---- the referee against torch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ("float32", "bfloat16"))
@pytest.mark.parametrize("name", list(PR.CONV_CASES))
def test_the_convolution_referee_equals_torch_in_float64(name, dtype):
    c = PR.conv_case(name, dtype)
    ref = PR.conv_case_ref(c)
    want = _torch_conv(c, dtype)
    assert ref.value.shape == want.shape == (c.B, c.Cout, c.H, c.W)
    # two float64 evaluations of one sum: apart by float64 roundings, a 2^-29 of the float32 limit
    assert (np.abs(ref.value - want) <= ref.limit * 2.0 ** -20).all() and (ref.limit > 0).all()
    # a float32 evaluation (torch's own) keeps the limit
    x = torch.from_numpy(c.x0 if c.x1 is None else np.concatenate([c.x0, c.x1], axis=1))
    v = torch.nn.functional.conv2d(x, torch.from_numpy(R.weights_of(c.w, dtype)), torch.from_numpy(c.bias), padding=c.dilation * (c.ksize // 2),
                                   dilation=c.dilation)
    if c.res is not None:
        v = v + torch.from_numpy(c.res)
    if c.relu:
        v = torch.relu(v)
    got = (v * float(F32(c.scale))).numpy()
    worst, beyond, other = PR.compare(got, ref)
    assert beyond == 0 and other == 0 and 0 < worst < 1, (worst, beyond, other)


@pytest.mark.parametrize("name", list(PR.POOL_CASES))
def test_the_pool_referee_equals_torch_in_float64(name):
    c = PR.pool_case(name)
    for k in c.ks:
        ref = PR.pool(c.x, k)
        want = torch.nn.functional.avg_pool2d(_t64(c.x), (k, k), stride=(k, k)).numpy()
        assert ref.value.shape == want.shape == (c.B, c.C, c.H // k, c.W // k)
        assert (np.abs(ref.value - want) <= ref.limit * 2.0 ** -20).all()
        got = torch.nn.functional.avg_pool2d(torch.from_numpy(c.x), (k, k), stride=(k, k)).numpy()
        assert PR.misses(got, ref) == 0


def test_the_grid_of_the_gpu_file_holds_what_the_issue_names():
    assert PR.CONV_MAPS == ((1, 1), (2, 2), (8, 32), (9, 33), (17, 70)) and PR.CONV_CINS == ((16, 0), (48, 0), (16, 32))
    assert PR.CONV_COUTS == (16, 20, 80) and len(set(PR.EPILOGUES)) == 8
    assert {s for _, _, s in PR.EPILOGUES} == {1.0, 0.25}
    assert [PR.POOL_CASES[n][2:] for n in ("odd", "spp")] == [(37, 53, (2, 4, 8, 16)), (64, 72, (8, 16, 32, 64))]
    assert {PR.POOL_CASES[n][1] for n in ("odd", "odd16", "spp", "spp16")} == {3, 16}
    # both routes of spp_kernels.hip: a grid of (H / g) x (W / g) cells up to 8192, and the direct one
    grid = lambda n: (lambda B, Cc, H, W, ks: (H // np.gcd.reduce(ks)) * (W // np.gcd.reduce(ks)))(*PR.POOL_CASES[n])            # noqa: E731
    assert grid("spp") == 8 * 9 and grid("loose") == 37 * 53 and grid("direct") > 8192


# ---- the planted mistakes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ("float32", "bfloat16"))
@pytest.mark.parametrize("planted", PR.PLANTED_CONV)
def test_every_planted_convolution_mistake_leaves_the_limit(planted, dtype):
    assert set(PR.CONV_CATCHES) == set(PR.PLANTED_CONV)
    assert set().union(*PR.CONV_CATCHES.values()) == set(PR.CONV_CASES), "every case is claimed"
    for name in PR.CONV_CASES:
        c = PR.conv_case(name, dtype)
        ref = PR.conv_case_ref(c)
        wrong = PR.conv_case_ref(c, planted=planted).value.astype(F32)
        if dtype == "bfloat16":
            wrong = PR.to_bf16(wrong)
        if name in PR.CONV_CATCHES[planted]:
            assert PR.caught(wrong, ref, dtype), (planted, name)


@pytest.mark.parametrize("planted", PR.PLANTED_POOL)
def test_every_planted_pool_mistake_leaves_the_limit(planted):
    assert set(PR.POOL_CATCHES) == set(PR.PLANTED_POOL)
    assert set().union(*PR.POOL_CATCHES.values()) == set(PR.POOL_CASES), "every case is claimed"
    for name in PR.POOL_CATCHES[planted]:
        c = PR.pool_case(name)
        assert any(PR.caught(PR.pool(c.x, k, planted=planted).value.astype(F32), PR.pool(c.x, k)) for k in c.ks), (planted, name)


def _bn_arrays(seed, C):
    return PR.bn_case(np.random.default_rng([7304, seed, C]), C)


@pytest.mark.parametrize("planted", PR.PLANTED_FOLD)
def test_every_planted_fold_mistake_leaves_the_limit(planted):
    rng = np.random.default_rng(7305)
    w = (rng.standard_normal((20, 16, 3, 3)) * 0.1).astype(F32)
    bn = _bn_arrays(1, 20)
    wf, bf = PR.fold(w, None, bn["gamma"], bn["beta"], bn["mean"], bn["var"], bn["eps"])
    ww, bw = PR.fold(w, None, bn["gamma"], bn["beta"], bn["mean"], bn["var"], bn["eps"], planted=planted)
    caught = PR.caught(ww.value.astype(F32), wf) or PR.caught(bw.value.astype(F32), bf)
    assert caught, planted
    assert not PR.caught(wf.value.astype(F32), wf) and not PR.caught(bf.value.astype(F32), bf)


def _tail_case(dtype="float32"):
    rng = np.random.default_rng(7306)
    raw, skip = R._cells(rng, (1, 4, 64, 72), dtype), R._cells(rng, (1, 16, 64, 72), dtype)
    branches = [((rng.standard_normal((4, 16, 1, 1)) * 2.0).astype(F32), PR.bn_case(rng, 4)) for _ in range(4)]
    return raw, skip, branches


def test_the_branches_in_the_order_1_to_4_leave_the_limit():
    raw, skip, branches = _tail_case()
    ref = PR.tail(raw, skip, branches)
    assert ref.value.shape == (1, 4 + 16 + 16, 64, 72)
    wrong = PR.tail(raw, skip, branches, planted="order_1234").value.astype(F32)
    assert PR.caught(wrong, ref) and not PR.caught(ref.value.astype(F32), ref)
    # branch4, the window of 8, comes first behind output_skip; branch1, the window of 64, last: one value per channel
    assert (np.ptp(ref.value[0, -4:].reshape(4, -1), axis=1) <= 2 * ref.limit[0, -4:].reshape(4, -1).max(axis=1)).all()
    assert (np.ptp(ref.value[0, 20:24].reshape(4, -1), axis=1) > 0).all()


# ---- the fold against torch, and its cache ---------------------------------------------------------------------------------------
def _convbn(cin, cout, k=3, stride=1, dilation=1, seed=0, bias=False, affine=True):
    g = torch.Generator().manual_seed(7307 + seed)
    conv = torch.nn.Conv2d(cin, cout, k, stride=stride, padding=dilation * (k // 2), dilation=dilation, bias=bias)
    bn = torch.nn.BatchNorm2d(cout, affine=affine)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / (k * k * cin) ** 0.5)
        if bias:
            conv.bias.copy_(torch.randn(cout, generator=g))
        bn.running_mean.copy_(torch.randn(cout, generator=g) * 0.5)
        bn.running_var.copy_(torch.rand(cout, generator=g) + 0.5)
        if affine:
            bn.weight.copy_(1 + 0.3 * torch.randn(cout, generator=g))
            bn.bias.copy_(0.3 * torch.randn(cout, generator=g))
    return conv.eval(), bn.eval()


@pytest.mark.parametrize("bias, affine", [(False, True), (True, True), (False, False)])
def test_fold_bn_is_the_referees_fold_rounded_once(bias, affine):
    from vppstereo_amd._convs import fold_bn
    conv, bn = _convbn(16, 20, bias=bias, affine=affine)
    w, b = fold_bn(conv, bn)
    assert w.dtype == b.dtype == torch.float32 and tuple(w.shape) == (20, 16, 3, 3) and tuple(b.shape) == (20,)
    n = lambda t: None if t is None else t.detach().numpy()                              # noqa: E731
    wf, bf = PR.fold(n(conv.weight), n(conv.bias), n(bn.weight), n(bn.bias), n(bn.running_mean), n(bn.running_var), bn.eps)
    assert np.array_equal(w.numpy(), wf.value.astype(F32)) and np.array_equal(b.numpy(), bf.value.astype(F32))
    # the folded convolution is bn(conv(x)), within the referee's bound for the unfolded formula
    x = torch.randn(2, 16, 9, 13, generator=torch.Generator().manual_seed(1))
    want = bn(conv(x)).detach().double().numpy()
    bnd = dict(gamma=n(bn.weight), beta=n(bn.bias), mean=n(bn.running_mean), var=n(bn.running_var), eps=bn.eps)
    ref = PR.convbn(x.numpy(), None, n(conv.weight), n(conv.bias), bnd)
    got = torch.nn.functional.conv2d(x, w, b, padding=1).numpy()
    assert PR.misses(got, ref) == 0
    assert (np.abs(want - ref.value) <= 2 * ref.limit).all()       # torch's own float32 bn(conv(x)): two evaluations of one value


def test_a_norm_that_cannot_be_folded_is_a_type_error():
    from vppstereo_amd._convs import fold_bn, frozen_bn
    conv, bn = _convbn(16, 16)
    with pytest.raises(TypeError, match="training mode"):
        fold_bn(conv, bn.train())
    with pytest.raises(TypeError, match="no running statistics"):
        frozen_bn(torch.nn.BatchNorm2d(16, track_running_stats=False).eval(), "layer1[0].conv2[1]")
    with pytest.raises(TypeError, match=r"layer1\[0\].conv2\[1\] is InstanceNorm2d"):
        frozen_bn(torch.nn.InstanceNorm2d(16), "layer1[0].conv2[1]")


class _PackSpy:
    """Engine.raft_conv_pack's place in PackedWeights: counts the packings and keeps what was packed."""

    def __init__(self):
        self.calls = []

    def raft_conv_pack(self, w, b, dtype=None):
        self.calls.append((w.clone(), b.clone(), dtype))
        return len(self.calls)


def test_the_fold_cache_follows_running_var_and_forget_weights():
    from vppstereo_amd._convs import PackedWeights, fold_bn
    conv, bn = _convbn(16, 16)
    eng, pw = _PackSpy(), PackedWeights()
    get = lambda dtype=torch.float32: pw._packed_conv_bn(eng, conv, bn, dtype, "cpu")           # noqa: E731
    assert get() == 1 and get() == 1 and len(eng.calls) == 1
    assert torch.equal(eng.calls[0][0], fold_bn(conv, bn)[0])
    with torch.no_grad():
        bn.running_var.mul_(4.0)                   # an in-place write moves the version counter
    assert get() == 2 and get() == 2
    assert torch.equal(eng.calls[1][0], fold_bn(conv, bn)[0]) and not torch.equal(eng.calls[1][0], eng.calls[0][0])
    with torch.no_grad():
        bn.running_mean.add_(1.0), bn.bias.add_(1.0)
    assert get() == 3
    with torch.no_grad():
        bn.weight.mul_(2.0)
    assert get() == 4
    with torch.no_grad():
        conv.weight.mul_(2.0)
    assert get() == 5 and get() == 5
    bn.eps = 1e-3
    assert get() == 6 and get(torch.bfloat16) == 7 and get(torch.bfloat16) == 7
    bn.running_var.data.mul_(2.0)                  # a write through .data is the one change the stamp cannot see
    assert get(torch.bfloat16) == 7
    pw.forget_weights()
    assert get(torch.bfloat16) == 8 and torch.equal(eng.calls[7][0], fold_bn(conv, bn)[0])
    bn.train()
    with pytest.raises(RuntimeError, match="training mode"):
        get()


# ---- conv_plain ------------------------------------------------------------------------------------------------------------------
def test_conv_plain_takes_a_dilated_convolution_only_where_the_caller_names_the_dilation():
    from vppstereo_amd._convs import conv_plain
    d2 = torch.nn.Conv2d(32, 32, 3, padding=2, dilation=2, bias=False)
    d1 = torch.nn.Conv2d(32, 32, 3, padding=1, bias=False)
    both = ((1, 1), (2, 2))
    assert conv_plain(d1, 32) and not conv_plain(d2, 32) and not conv_plain(d2, 32, strides=((1, 1), (2, 2)))
    assert conv_plain(d2, 32, dilations=both) and conv_plain(d1, 32, dilations=both)
    assert not conv_plain(torch.nn.Conv2d(32, 32, 3, padding=1, dilation=2), 32, dilations=both)           # padding 1 at dilation 2
    assert not conv_plain(torch.nn.Conv2d(32, 32, 3, padding=2), 32, dilations=both)                       # padding 2 at dilation 1
    assert not conv_plain(torch.nn.Conv2d(32, 32, 3, padding=3, dilation=3), 32, dilations=((3, 3),))      # not built
    assert not conv_plain(torch.nn.Conv2d(32, 32, 3, stride=2, padding=2, dilation=2), 32, strides=((1, 1), (2, 2)), dilations=both)
    assert conv_plain(torch.nn.Conv2d(32, 32, 1, dilation=2), 32, dilations=both)                           # a 1x1: padding 0
    assert not conv_plain(torch.nn.Conv2d(3, 32, 3, padding=1), 3, dilations=both)                          # the 3-channel stem


# ---- the entry points in the header, the library and the binding -----------------------------------------------------------------
def test_the_three_entry_points_are_declared_exported_and_bound():
    import ctypes as C
    from vppstereo_amd import _lib
    with open(os.path.join(ROOT, "include", "vppx.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.EXPORTS
    assert header.index("int vppx_raft_conv_strided_dt_dev(") < header.index("int vppx_conv2d_dt_dev(")
    assert (_lib.SPP_MAX_LEVELS, _lib.SPP_MAX_K) == (4, 64)
    protos = _lib.ABI.protos
    rt, args = protos["vppx_conv2d_dt_dev"]
    assert rt is C.c_int and len(args) == 22 and args[10] is C.c_int and args[14] is C.c_void_p and args[15] is C.c_int64 and args[17] is C.c_float
    rt, args = protos["vppx_psm_spp_pool_dt_dev"]
    assert rt is C.c_int and len(args) == 11 and args[7] is C.c_void_p and args[8] is C.c_void_p
    rt, args = protos["vppx_raft_gru_assemble_strided_dt_dev"]
    assert rt is C.c_int and len(args) == 9 and args[6] is C.c_int64 and args[8] is C.c_void_p
    lib = C.CDLL(_lib.LIB_PATH)                    # the library's own symbol table, without the binding
    for name in ENTRY_POINTS:
        assert getattr(lib, name) is not None, name
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert getattr(lib, name).argtypes == protos[name][1]
    # a NULL context is refused by each before anything else
    assert lib.vppx_conv2d_dt_dev(None, 0, 0, None, 0, 0, None, 0, 0, 0, 0, 0, 0, 0, None, 0, 0, 0.0, None, 0, 0, None) == -7
    assert lib.vppx_psm_spp_pool_dt_dev(None, 0, 0, 0, 0, 0, 0, None, None, 0, None) == -7
    assert lib.vppx_raft_gru_assemble_strided_dt_dev(None, 0, 0, 0, 0, None, 0, 0, None) == -7


# ---- the recording ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PR.RECORDED_BLOCKS))
def test_the_referee_reproduces_the_recorded_blocks(name):
    """The reference's own BasicBlock.forward in float32, unfolded: another float32 evaluation of the value the referee bounds."""
    g = PR.load_recording()
    ref = PR.block(g[f"{name}.x"], g, name, **PR.RECORDED_BLOCKS[name])
    rec = g[f"{name}.out"]
    assert rec.shape == ref.value.shape == ((2, 16, 9, 13) if name == "a" else (2, 32, 5, 7))
    assert (np.abs(rec.astype(F64) - ref.value) <= ref.limit).all()
    # a fold without the mean leaves the block's limit; one without eps (1e-5 of a variance of order 1) shows on the fold alone, above
    wrong = PR.block(g[f"{name}.x"], g, name, planted="no_mean", **PR.RECORDED_BLOCKS[name]).value
    assert (np.abs(wrong - ref.value) > 2 * ref.limit).any()
    assert ("b.downsample.0.weight" in g) and ("a.downsample.0.weight" not in g)


def test_the_referee_reproduces_the_recorded_tail():
    g = PR.load_recording()
    raw, skip = PR.tail_raw_skip()
    ref = PR.tail(raw, skip, PR.recorded_branches(g))
    rows, heads = list(g["tail.rows"]), list(g["tail.heads"])
    assert ref.value.shape == (1, 320, 64, 72) and {0, 31, 32, 63} <= set(rows)
    assert np.array_equal(ref.value[:, heads][:, :, rows], g["tail.heads_out"].astype(F64))      # output_raw and output_skip: exact
    got, val, lim = g["tail.branches_out"].astype(F64), ref.value[:, 192:][:, :, rows], ref.limit[:, 192:][:, :, rows]
    assert (np.abs(got - val) <= lim).all()
    wrong = PR.tail(raw, skip, PR.recorded_branches(g), planted="order_1234").value[:, 192:][:, :, rows]
    assert (np.abs(got - wrong) > 2 * lim).any()


# ---- the wrapper's wrap-time refusals --------------------------------------------------------------------------------------------
def test_the_wrapper_names_the_part_it_does_not_take():
    from vppstereo_amd.psmnet import FusedFeatureExtraction
    base = PR.standin()                            # built once; every case below breaks a copy of it
    ok = FusedFeatureExtraction(base)
    assert ok.launches() == 2 + (2 + 3 + 2 + 3 + 2) + 1 + 4 + 1 + 2 and ok._channels == (16, 32, (16, 16, 16, 16))

    def broken(change):
        fe = copy.deepcopy(base)
        change(fe)
        return fe

    def drop(name):
        return lambda fe: delattr(fe, name)

    cases = [
        (drop("branch3"), "has no 'branch3'"), (drop("lastconv"), "has no 'lastconv'"), (drop("layer4"), "has no 'layer4'"),
        (lambda fe: fe.layer2[1].conv2[1].train(), r"layer2\[1\].conv2\[1\] is in training mode"),
        (lambda fe: fe.firstconv[2][1].train(), r"firstconv\[2\]\[1\] is in training mode"),
        (lambda fe: setattr(fe.layer3[0], "downsample", torch.nn.Sequential(fe.layer3[0].downsample[0], torch.nn.BatchNorm2d(32, track_running_stats=False).eval())),
         r"layer3\[0\].downsample\[1\] keeps no running statistics"),
        (lambda fe: setattr(fe.layer1[0], "conv2", torch.nn.Sequential(fe.layer1[0].conv2[0], torch.nn.InstanceNorm2d(16))), r"layer1\[0\].conv2\[1\] is InstanceNorm2d"),
        (lambda fe: setattr(fe.layer1[0], "conv1", fe.layer1[0].conv1[0]), r"layer1\[0\].conv1\[0\] is not a Sequential"),
        (lambda fe: setattr(fe, "branch2", torch.nn.Sequential(torch.nn.MaxPool2d(32), fe.branch2[1], fe.branch2[2])), r"branch2\[0\] is MaxPool2d"),
        (lambda fe: setattr(fe, "branch1", torch.nn.Sequential(torch.nn.AvgPool2d(64, stride=32), fe.branch1[1], fe.branch1[2])), r"branch1\[0\] is not an AvgPool2d"),
        (lambda fe: setattr(fe, "lastconv", torch.nn.Sequential(fe.lastconv[0], fe.lastconv[1])), "lastconv is not a Sequential of 3"),
        (lambda fe: setattr(fe, "branch4", torch.nn.Sequential(fe.branch4[0], torch.nn.Sequential(torch.nn.Conv2d(32, 8, 1), torch.nn.BatchNorm2d(8)).eval(), fe.branch4[2])),
         "lastconv.0..0. takes 112 channels"),
        (lambda fe: fe.train(), "is in training mode"),
    ]
    for change, msg in cases:
        with pytest.raises(TypeError, match=msg):
            FusedFeatureExtraction(broken(change))
    with pytest.raises(TypeError, match="dtype is torch.float16"):
        FusedFeatureExtraction(PR.standin(), dtype=torch.float16)


def test_the_standin_has_the_references_keys():
    """Key for key the state dict of the recorded blocks, so that the wrapper that takes the stand-in takes the reference's module."""
    g = PR.load_recording()
    fe = PR.standin()
    keys = lambda prefix: {k[len(prefix):] for k in g.files if k.startswith(prefix)} - {"x", "out"}       # noqa: E731
    assert keys("b.") == set(fe.layer2[0].state_dict()) and keys("a.") == set(fe.layer4[0].state_dict())
    assert keys("tail.branch1.") == set(fe.branch1.state_dict())
    assert fe.layer4[0].conv1[0][0].dilation == (2, 2) and fe.layer4[0].conv1[0][0].padding == (2, 2) and fe.layer2[0].conv1[0][0].stride == (2, 2)
