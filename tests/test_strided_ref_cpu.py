"""The referee of the convolution kernel at stride 2 (tests/_strided_ref.py), held to torch and to the recording of the
reference's own ResidualBlock(16, 32, 'instance', stride=2) (tests/golden/strided_cases.npz), and its planted mistakes on the
arrays tests/test_gpu_conv_strided.py uploads; the new entry point in the header, the library and the derived binding;
`Engine.raft_conv(..., stride=)`; and what vppstereo_amd.extractor does around it: `FusedEncoder(encoder, convs=True)`, which
convolution counts as plain, and the one cache of packed weights that both wrappers use."""
import ctypes as C
import gc
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _conv_ref as CR
import _enc_models as EM
import _norm_ref as N
import _strided_ref as SR

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "vppx_raft_conv_strided_dt_dev"
CPU = torch.device("cpu")
_REFS = {}


def _ref(name, dtype="float32"):
    if (name, dtype) not in _REFS:
        c = SR.case(name, dtype)
        _REFS[name, dtype] = (c, SR.case_ref(c))
    return _REFS[name, dtype]


# ---- the referee -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["s2_odd", "s2_even", "d2_odd", "d2_even", "px1", "px2"])
def test_the_strided_convolutions_are_torchs(name):
    """The float64 value against F.conv2d(stride=2) on the CPU, the size included; a float32 evaluation lies inside the limit."""
    import torch.nn.functional as F
    c, ref = _ref(name)
    x = torch.from_numpy(np.concatenate([c.x0] + ([] if c.x1 is None else [c.x1]), axis=1)).double()
    want = F.conv2d(x, torch.from_numpy(c.w).double(), torch.from_numpy(c.bias).double(), stride=2, padding=c.ksize // 2).numpy()
    assert ref.value.shape == want.shape == (c.B, c.Cout, (c.H - 1) // 2 + 1, (c.W - 1) // 2 + 1), name
    assert np.abs(ref.value - want).max() <= 1e-12 and (ref.limit > 0).all() and ref.limit.max() < 1e-3
    got32 = F.conv2d(x.float(), torch.from_numpy(c.w), torch.from_numpy(c.bias), stride=2, padding=c.ksize // 2).numpy()
    assert SR.misses(got32, ref) == 0, name
    one = SR.case_ref(c, stride=1)               # stride 1 through the same door is tests/_conv_ref.conv
    full = CR.conv(c.x0, c.x1, c.w, c.bias)
    assert np.array_equal(one.value, full.value) and np.array_equal(one.limit, full.limit)
    assert np.array_equal(ref.value, full.value[:, :, ::2, ::2]) and np.array_equal(ref.limit, full.limit[:, :, ::2, ::2])


def test_the_referee_reproduces_the_recording():
    """Every stage of the recorded block from RECORDED inputs alone: the two strided convolutions by this referee, the norms by
    tests/_norm_ref.py's bound for any float32 evaluation, conv2 by tests/_conv_ref.py."""
    g = SR.load_recording()
    assert all(a.dtype == F32 for a in g.values()) and os.path.getsize(SR.GOLDEN) < 200 * 1024
    assert g["x"].shape == (2, 16, 9, 13) and g["conv1.weight"].shape == (32, 16, 3, 3) and g["downsample.0.weight"].shape == (32, 16, 1, 1)
    assert set(g.files) >= {"conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "downsample.0.weight", "downsample.0.bias"}
    for key in ("conv1_out", "down_out", "out"):
        assert g[key].shape == (2, 32, 5, 7), key
    c1, dn = SR.recorded_convs(g)
    for what, got, ref in (("conv1", g["conv1_out"], c1), ("downsample[0]", g["down_out"], dn)):
        worst, beyond, other = SR.compare(got, ref)
        print(f"the recorded {what}(x) against the referee: worst |out - value| / limit {worst:.3f}")
        assert beyond == 0 and other == 0, (what, worst)
    # norm1 + ReLU on the recorded conv1(x), conv2 on its recorded input, norm2 / norm3 + the sum on the recorded pair
    any32 = lambda a: N.stats(a, unit=N.U)                                              # noqa: E731
    mid = N.apply(g["conv1_out"], any32(g["conv1_out"]), any_f32=True)
    assert N.misses(g["conv2_in"], mid) == 0 and (g["conv2_in"] == 0).mean() > 0.2
    assert CR.misses(g["conv2_out"], CR.conv(g["conv2_in"], None, g["conv2.weight"], g["conv2.bias"])) == 0
    out = N.apply(g["conv2_out"], any32(g["conv2_out"]), res=g["down_out"], res_stats=any32(g["down_out"]), any_f32=True)
    assert N.misses(g["out"], out) == 0
    # every planted mistake that the block's two convolutions can make leaves the limit on the recording
    for planted in ("odd_phase", "stride_x_only", "stride_y_only", "floor_size", "dense_1x1", "flipped"):
        w1, wd = SR.recorded_convs(g, planted=planted)
        if planted != "dense_1x1":
            assert SR.caught(w1.value, c1), planted
        if planted != "flipped":
            assert SR.caught(wd.value, dn), planted


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("planted", list(SR.CATCHES))
def test_a_planted_mistake_leaves_the_limit(planted, dtype):
    for name in SR.CATCHES[planted]:
        c, ref = _ref(name, dtype)
        wrong = SR.case_ref(c, planted=planted).value
        got = SR.to_bf16(wrong.astype(F32)) if dtype == "bfloat16" else wrong
        assert SR.caught(got, ref, dtype), (planted, name)
        own = SR.to_bf16(ref.value.astype(F32)) if dtype == "bfloat16" else ref.value
        assert not SR.caught(own, ref, dtype)


def test_the_planted_mistakes_are_all_claimed_and_the_cases_are_the_table():
    assert set(SR.PLANTED) == set(SR.CATCHES) and all(n in SR.CASES for names in SR.CATCHES.values() for n in names)
    assert SR.CASES == {"s2_even": (3, 2, 2, 16, 0, 16, 16, 64), "s2_odd": (3, 2, 2, 32, 16, 14, 17, 67), "s2_c96": (3, 2, 2, 96, 0, 96, 5, 9),
                        "s2_tiles": (3, 2, 1, 16, 0, 16, 34, 130), "d2_even": (1, 2, 2, 64, 0, 96, 18, 66),
                        "d2_odd": (1, 2, 2, 32, 16, 25, 9, 13), "px1": (3, 2, 1, 16, 0, 16, 1, 1), "px2": (3, 2, 1, 16, 0, 16, 2, 2)}
    assert {n for names in SR.CATCHES.values() for n in names} == set(SR.CASES)        # every case catches something


def test_where_a_nan_reaches():
    """The mask the GPU file predicts with, against the definition: the pixels whose float64 result changes."""
    for ks, H, W in ((3, 9, 13), (1, 9, 13), (3, 6, 8)):
        for y, x in ((0, 0), (2, 4), (3, 5), (H - 1, W - 1), (2, 5)):
            reach = SR.nan_reach(ks, H, W, y, x)
            a = np.zeros((1, 16, H, W), F32)
            a[0, 3, y, x] = 1.0
            w = np.ones((2, 16, ks, ks), F32)
            assert np.array_equal(SR.conv(a, None, w, None).value[0, 0] != 0, reach), (ks, H, W, y, x)
    assert SR.nan_reach(3, 9, 13, 2, 4).sum() == 1 and SR.nan_reach(3, 9, 13, 3, 5).sum() == 4 and SR.nan_reach(3, 9, 13, 2, 5).sum() == 2
    assert SR.nan_reach(1, 9, 13, 3, 5).sum() == 0 and SR.nan_reach(1, 9, 13, 2, 5).sum() == 0 and SR.nan_reach(1, 9, 13, 2, 4).sum() == 1
    assert SR.nan_reach(3, 6, 8, 5, 7).sum() == 1                                       # an even map: the last cell lies in one window


# ---- the entry point -------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_strided_call():
    from vppstereo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vppx.h")).read()
    assert SYMBOL in _lib.EXPORTS and SYMBOL in _lib.ABI.protos
    proto = re.search(r"\bint\s+" + SYMBOL + r"\s*\(([^;]*)\)\s*;", hdr).group(1)
    names = [a.split()[-1].lstrip("*") for a in proto.split(",")]
    old = re.search(r"\bint\s+vppx_raft_conv_dt_dev\s*\(([^;]*)\)\s*;", hdr).group(1)
    old = [a.split()[-1].lstrip("*") for a in old.split(",")]
    k = old.index("ksize")
    assert names == old[:k + 1] + ["stride"] + old[k + 1:] and names[-1] == "ctx"      # the same list with `stride` behind ksize
    head = hdr[:hdr.index("Conventions")]
    assert "ResidualBlock conv1 / conv2 / downsample, encoder conv2, output heads -> extractor.py:10-11,45,149,231,240,247" in head
    for said in ("Ho = (H - 1) / stride + 1", "NaN rule", "odd row or column reaches nothing", "serves either stride"):
        assert said in hdr, said


def test_the_library_exports_and_binds_it():
    from vppstereo_amd import _lib
    lib = _lib.load()
    args = lib.vppx_raft_conv_strided_dt_dev.argtypes
    assert len(args) == 19 and args[-1] is C.c_void_p and args[14] is C.c_float and args[9] is C.c_int
    # a NULL context: the context is checked first, as everywhere
    assert lib.vppx_raft_conv_strided_dt_dev(None, 0, 16, None, 0, 0, None, 16, 3, 2, 1, 1, 1, 0, 1.0, None, 0, 0, None) == -7
    assert b"context is NULL" in lib.vppx_last_error()


def test_engine_raft_conv_takes_a_stride():
    from vppstereo_amd.engine import Engine
    sig = inspect.signature(Engine.raft_conv)
    assert sig.parameters["stride"].default == 1
    assert list(sig.parameters)[:9] == ["self", "x0", "packed", "cout", "ksize", "x1", "relu", "scale", "out"]   # no present call changes


# ---- the wrapper -----------------------------------------------------------------------------------------------------------------
def test_fused_encoder_takes_convs():
    from vppstereo_amd.extractor import FusedEncoder
    for enc in (EM.basic(), EM.multi()):
        assert not FusedEncoder(enc).convs and FusedEncoder(enc, convs=True).convs and not FusedEncoder(enc, convs=False).convs
        fused = FusedEncoder(enc, convs=True)
        assert fused._packed == {} and fused.encoder is enc and list(fused.state_dict()) == ["encoder." + k for k in enc.state_dict()]
        # every convolution but the stem is one the kernel takes
        assert not FusedEncoder._conv_plain(enc.conv1, 3)
        assert all(FusedEncoder._conv_plain(m, m.in_channels) for m in EM.convs_of(enc))
    assert len(EM.convs_of(EM.basic())) == 15 and len(EM.convs_of(EM.multi())) == 38
    assert {m.stride for m in EM.convs_of(EM.multi())} == {(1, 1), (2, 2)}


def test_what_counts_as_a_plain_convolution_of_an_encoder():
    from vppstereo_amd.extractor import FusedEncoder
    from vppstereo_amd.update import FusedUpdate
    nn = torch.nn
    plain = FusedEncoder._conv_plain
    for conv in (nn.Conv2d(64, 64, 3, padding=1), nn.Conv2d(64, 96, 3, padding=1, stride=2), nn.Conv2d(64, 96, 1, stride=2),
                 nn.Conv2d(128, 256, 1), nn.Conv2d(96, 128, 3, stride=2, padding=1, bias=False)):
        assert plain(conv, conv.in_channels), conv
    for conv, cin in ((nn.Conv2d(3, 64, 7, stride=2, padding=3), 3),                     # the stem
                      (nn.Conv2d(16, 16, 3, padding=1, stride=(2, 1)), 16), (nn.Conv2d(16, 16, 3, padding=1, stride=(1, 2)), 16),
                      (nn.Conv2d(16, 16, 3, padding=1, stride=3), 16), (nn.Conv2d(16, 16, 3, padding=2, dilation=2), 16),
                      (nn.Conv2d(16, 16, 3, padding=1, groups=2), 16), (nn.Conv2d(24, 16, 3, padding=1), 24),
                      (nn.Conv2d(16, 16, 3, stride=2), 16), (nn.Conv2d(16, 16, 1, stride=2, padding=1), 16),
                      (nn.Conv2d(16, 16, 3, padding=1, stride=2, padding_mode="reflect"), 16), (nn.Conv2d(16, 384, 3, padding=1), 16),
                      (nn.Conv2d(16, 16, 3, padding=1), 32)):
        assert not plain(conv, cin), conv

    class Mine(nn.Conv2d):                       # a subclass with a forward of its own
        def forward(self, x):
            return super().forward(x) + 1

    assert not plain(Mine(16, 16, 3, padding=1), 16)
    # the update block's rule has not moved: stride 1 only
    assert not FusedUpdate._conv_plain(nn.Conv2d(16, 16, 3, padding=1, stride=2), 16) and FusedUpdate._conv_plain(nn.Conv2d(16, 16, 3, padding=1), 16)


class _Stub:
    """Packing returns what it was given, counted."""

    def __init__(self):
        self.calls = 0

    def raft_conv_pack(self, weight, bias=None, dtype=None):
        self.calls += 1
        return (weight.detach().clone(), None if bias is None else bias.detach().clone())


def _follows(owner, eng, conv):
    w, b = owner._packed_conv(eng, conv, torch.float32, CPU)
    return torch.equal(w, conv.weight.detach()) and (b is None or torch.equal(b, conv.bias.detach()))


def test_one_cache_serves_both_wrappers():
    from vppstereo_amd import _convs
    from vppstereo_amd.extractor import FusedEncoder
    from vppstereo_amd.update import FusedUpdate, GruGlue
    for name in ("_packed_conv", "_packed_for", "forget_weights"):                      # one implementation, not two
        assert getattr(FusedEncoder, name) is getattr(_convs.PackedWeights, name) is getattr(GruGlue, name) is getattr(FusedUpdate, name)
        assert name not in vars(FusedEncoder) and name not in vars(GruGlue) and name not in vars(FusedUpdate)
    enc = EM.basic()
    fused, glue, eng = FusedEncoder(enc, convs=True), GruGlue(), _Stub()
    conv = enc.layer2[0].conv1
    first = fused._packed_conv(eng, conv, torch.float32, CPU)
    assert fused._packed_conv(eng, conv, torch.float32, CPU) is first and eng.calls == 1
    assert set(fused._packed) == {id(conv)} and glue._packed == {}                        # a store per wrapper
    assert fused._packed[id(conv)][0][2] == tuple((id(p), p.data_ptr(), p._version) for p in (conv.weight, conv.bias))
    conv.weight.data = torch.randn_like(conv.weight)                                    # `p.data = new`
    assert _follows(fused, eng, conv) and eng.calls == 2 and _follows(glue, eng, conv) and eng.calls == 3
    with torch.no_grad():
        conv.bias.copy_(torch.ones_like(conv.bias))                                     # in place: the version moves
    assert _follows(fused, eng, conv) and eng.calls == 4 and _follows(fused, eng, conv) and eng.calls == 4
    fused._packed_conv(eng, conv, torch.bfloat16, CPU)                                  # another dtype
    assert eng.calls == 5
    fused.forget_weights()
    assert fused._packed == {} and _follows(fused, eng, conv) and eng.calls == 6
    lone = torch.nn.Conv2d(16, 16, 1, stride=2)
    assert _follows(fused, eng, lone) and set(fused._packed) == {id(conv), id(lone)}
    del lone
    gc.collect()
    assert set(fused._packed) == {id(conv)}                                             # the entry dies with its module
