"""The referee of the update block's other convolutions (tests/_conv_ref.py), held to the recording of the reference's own
FlowHead.forward (tests/golden/heads_cases.npz), and its planted mistakes on the arrays tests/test_gpu_conv.py uploads; the new
entry points in the header, the library and the derived binding; and, with stub engines, what vppstereo_amd.update does around
them: the packed-weight cache per convolution, the seven launches of convs=True and `mask=False`."""
import ctypes as C
import gc
import os
import re

import numpy as np
import pytest
import torch

import _conv_ref as CR
import _raft_loop as L

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vppx_raft_conv_packed_bytes", "vppx_raft_conv_pack_dev", "vppx_raft_conv_dt_dev")
_REFS = {}


def _ref(name, dtype="float32"):
    if (name, dtype) not in _REFS:
        c = CR.case(name, dtype)
        _REFS[name, dtype] = (c, CR.case_ref(c))
    return _REFS[name, dtype]


# ---- the referee -----------------------------------------------------------------------------------------------------------------
def test_the_convolutions_are_torchs():
    """The float64 value against F.conv2d on the CPU: a 1x1 over two sources with a scale, a 3x3 with ReLU and a scale."""
    import torch.nn.functional as F
    for name in ("one1x1", "enc14", "mask9"):
        c, ref = _ref(name)
        x = torch.from_numpy(np.concatenate([c.x0] + ([] if c.x1 is None else [c.x1]), axis=1)).double()
        want = F.conv2d(x, torch.from_numpy(c.w).double(), torch.from_numpy(c.bias).double(), padding=c.ksize // 2)
        want = ((F.relu(want) if c.relu else want) * c.scale).numpy()
        assert ref.value.shape == (c.B, c.Cout, c.H, c.W) and np.abs(ref.value - want).max() <= 1e-12, name
        assert (ref.limit > 0).all() and ref.limit.max() < 1e-3
        got32 = F.conv2d(x.float(), torch.from_numpy(c.w), torch.from_numpy(c.bias), padding=c.ksize // 2)
        got32 = ((F.relu(got32) if c.relu else got32) * F32(c.scale)).numpy()
        assert CR.misses(got32, ref) == 0, name                # a float32 evaluation lies inside the limit
    # a 1x1 sum has Cin terms, not 9 Cin: its limit is that much tighter than the 3x3 referee's on the same cells
    c, _ = _ref("mask9")
    w3 = np.zeros((c.Cout, c.C0, 3, 3), F32)
    w3[:, :, 1, 1] = c.w[:, :, 0, 0]
    a, b = CR.conv1x1(c.x0, None, c.w, c.bias), CR.R.conv3x3(c.x0, None, w3, c.bias)
    assert np.array_equal(a.value, b.value) and np.allclose(a.limit * (9 * c.C0 + 1), b.limit * (c.C0 + 1), rtol=1e-12)


def test_scale_one_adds_nothing_and_a_scale_adds_one_rounding():
    c, _ = _ref("enc18")
    one, three = CR.case_ref(c, scale=1.0), CR.case_ref(c, scale=3.0)
    plain = CR.R.conv3x3(c.x0, c.x1, c.w, c.bias)
    assert np.array_equal(one.value, plain.value) and np.array_equal(one.limit, plain.limit)
    assert np.array_equal(three.value, 3.0 * plain.value)
    want = (3.0 * plain.limit + CR.U * np.abs(three.value)) * CR.SECOND_ORDER
    assert np.allclose(three.limit, want, rtol=1e-12)


def test_the_referee_reproduces_the_recording():
    g = CR.load_recording()
    assert all(a.dtype == F32 for a in g.values()) and os.path.getsize(CR.GOLDEN) < 65536
    assert g["conv1_weight"].shape == (32, 16, 3, 3) and g["conv2_weight"].shape == (2, 32, 3, 3)
    for name, hw in (("a", (5, 6)), ("b", (3, 3))):
        assert g[f"{name}_x"].shape == (2, 16) + hw and g[f"{name}_out"].shape == (2, 2) + hw
        pre = CR.conv(g[f"{name}_x"], None, g["conv1_weight"], g["conv1_bias"])
        assert CR.misses(g[f"{name}_conv1_out"], pre) == 0, name
        cut = (g[f"{name}_conv1_out"] < 0).mean()
        assert 0.2 < cut < 0.8, (name, cut)                          # the ReLU matters
        hid, out = CR.recorded_ref(g, name)
        worst, beyond, other = CR.compare(g[f"{name}_out"], out)
        print(f"{name}: the recorded output against the referee, worst |out - value| / limit {worst:.3f}")
        assert beyond == 0 and other == 0, (name, worst)
        for planted in ("no_relu", "flipped", "padded_rows"):
            wrong = CR.recorded_ref(g, name, planted=planted)[1]
            assert CR.misses(wrong.value, out) > 0, (name, planted)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("planted", list(CR.CATCHES))
def test_a_planted_mistake_leaves_the_limit(planted, dtype):
    for name in CR.CATCHES[planted]:
        c, ref = _ref(name, dtype)
        wrong = CR.case_ref(c, planted=planted).value
        got = CR.to_bf16(wrong.astype(F32)) if dtype == "bfloat16" else wrong
        assert CR.misses(got, ref, dtype) > 0, (planted, name)
        own = CR.to_bf16(ref.value.astype(F32)) if dtype == "bfloat16" else ref.value
        assert CR.misses(own, ref, dtype) == 0


def test_the_planted_mistakes_are_all_claimed_and_the_cases_cover_the_table():
    assert set(CR.PLANTED) == set(CR.CATCHES) and all(n in CR.CASES for names in CR.CATCHES.values() for n in names)
    rows = list(CR.CASES.values())
    assert {r[4] for r in rows if r[0] == 3} >= {2, 14, 18, 126} and {r[4] for r in rows if r[0] == 1} >= {144, 9}
    assert {(r[2], r[3]) for r in rows} >= {(16, 0), (32, 16), (64, 64), (128, 0), (256, 0)}
    assert {(r[5], r[6]) for r in rows} == {(3, 5), (8, 32), (9, 33)} and all(r[1] == 2 for r in rows)
    assert {r[8] for r in rows} == {1.0, .25, 3.0} and {r[7] for r in rows} == {True, False}
    for ks in (1, 3):                                                # each kernel size on each map, with and without ReLU
        assert {(r[5], r[6]) for r in rows if r[0] == ks} == {(3, 5), (8, 32), (9, 33)}
        assert {r[7] for r in rows if r[0] == ks} == {True, False}


# ---- the entry points ------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_new_prototypes_with_the_context_last():
    from vppstereo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vppx.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.EXPORTS and name in _lib.ABI.protos, name
    for name in SYMBOLS[1:]:
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr).group(1)
        assert proto.split(",")[-1].strip() == "vppx_ctx *ctx" and not proto.lstrip().startswith("vppx_ctx"), name
    assert "float scale" in re.search(r"\bint\s+vppx_raft_conv_dt_dev\s*\(([^;]*)\)\s*;", hdr).group(1)
    for module in ("convc2", "convf2", "FlowHead", "mask"):
        assert module in hdr[:hdr.index("Conventions")], module


def test_the_library_exports_and_binds_them():
    from vppstereo_amd import _lib
    lib = _lib.load()
    assert lib.vppx_raft_conv_packed_bytes.restype is C.c_size_t
    assert lib.vppx_raft_conv_packed_bytes.argtypes == [C.c_int, C.c_int, C.c_int, C.c_int]
    assert len(lib.vppx_raft_conv_pack_dev.argtypes) == 8 and lib.vppx_raft_conv_pack_dev.argtypes[-1] is C.c_void_p
    args = lib.vppx_raft_conv_dt_dev.argtypes
    assert len(args) == 18 and args[-1] is C.c_void_p and args[13] is C.c_float
    size, old = lib.vppx_raft_conv_packed_bytes, lib.vppx_raft_conv3x3_packed_bytes
    # 0 exactly for what the header says is not built
    for bad in ((0, 16, 3, 0), (-2, 16, 3, 0), (257, 16, 3, 0), (16, 0, 3, 0), (16, 8, 1, 0), (16, 24, 3, 1), (16, 528, 3, 1), (16, 16, 2, 0),
                (16, 16, 5, 0), (16, 16, 0, 1), (16, 16, 3, 2), (16, 16, 1, -1)):
        assert size(*bad) == 0, bad
    for dt in (_lib.DT_F32, _lib.DT_BF16):
        cell = 4 if dt == _lib.DT_F32 else 2
        for ks in (1, 3):
            for cout, cin in ((2, 256), (14, 32), (126, 128), (144, 256), (1, 16), (256, 512)):
                pad = 16 * ((cout + 15) // 16)
                assert size(cout, cin, ks, dt) >= pad * cin * ks * ks * cell + pad * 4, (cout, cin, ks, dt)
                assert size(cout, cin, ks, dt) == size(pad, cin, ks, dt)          # padded to the next multiple of 16
        for cout, cin in ((16, 16), (256, 384), (128, 48)):                       # the 3x3 call's size where both take the shape
            assert size(cout, cin, 3, dt) == old(cout, cin, dt) > 0
    assert old(126, 128, 0) == 0                                                  # the 3x3 call still refuses it
    # a NULL context: the context is checked first, as everywhere
    assert lib.vppx_raft_conv_pack_dev(None, None, 16, 16, 3, 0, None, None) == -7 and b"context is NULL" in lib.vppx_last_error()
    assert lib.vppx_raft_conv_dt_dev(None, 0, 16, None, 0, 0, None, 16, 3, 1, 1, 1, 0, 1.0, None, 0, 0, None) == -7


# ---- stub engines ----------------------------------------------------------------------------------------------------------------
class _Stub:
    """The Engine calls FusedUpdate makes, in torch on the CPU, counted.  Packing returns what it was given."""

    def __init__(self):
        self.calls = []

    def raft_conv_pack(self, weight, bias=None, dtype=None):
        self.calls.append("raft_conv_pack")
        return (weight.detach().clone(), None if bias is None else bias.detach().clone())

    def raft_conv(self, x0, packed, cout, ksize, x1=None, relu=False, scale=1.0, out=None):
        import torch.nn.functional as F
        self.calls.append("raft_conv")
        w, b = packed
        assert w.shape[0] == cout and w.shape[2] == ksize
        y = F.conv2d(x0 if x1 is None else torch.cat([x0, x1], dim=1), w, b, padding=ksize // 2)
        y = (F.relu(y) if relu else y) * scale
        if out is None:
            return y
        out.copy_(y)
        return out

    def raft_gru_assemble(self, sources, out=None):
        self.calls.append("raft_gru_assemble")
        size = out.shape[2:]
        parts = [t if m == "copy" else L._pool2x(t) if m == "pool2x" else L._interp(t, out) for t, m in sources]
        assert all(p.shape[2:] == size for p in parts)
        out.copy_(torch.cat(parts, dim=1))
        return out

    def raft_gru_reset(self, ar, cr, h, hx):
        hx[:, :h.shape[1]] = torch.sigmoid(ar + cr) * h
        return hx

    def raft_gru_update(self, az, cz, aq, cq, h, out=None):
        z = torch.sigmoid(az + cz)
        return (1 - z) * h + z * torch.tanh(aq + cq)


def _state(model, seed=6401):
    gen = torch.Generator().manual_seed(seed)
    sizes = L.map_sizes(40, 72)
    net = [torch.tanh(torch.randn((2, L.HIDDEN) + s, generator=gen)) for s in sizes]
    inp = [list(torch.randn((2, 3 * L.HIDDEN) + s, generator=gen).split(L.HIDDEN, dim=1)) for s in sizes]
    corr = torch.randn((2, L.LEVELS * (2 * L.RADIUS + 1)) + sizes[0], generator=gen)
    flow = torch.randn((2, 2) + sizes[0], generator=gen)
    return net, inp, corr, flow


@pytest.fixture()
def stub(monkeypatch):
    from vppstereo_amd import update as U
    eng = _Stub()
    monkeypatch.setattr(U, "_engine", lambda device: eng)
    return eng


def _close(a, b):
    return a.shape == b.shape and float((a - b).abs().max()) <= 1e-5 * max(1.0, float(b.abs().max()))


def test_mask_false_on_the_default_path(stub):
    """No library: the glue runs in the stub.  `mask=False` returns None in the mask's place and the bits of net and delta_flow."""
    from vppstereo_amd.update import FusedUpdate
    model = L.build_model()
    blk = model.update_block
    ran = []
    hooks = [m.register_forward_hook(lambda m_, i, o: ran.append(1)) for m in blk.mask]
    order = []
    enc = blk.encoder
    hooks += [getattr(enc, n).register_forward_hook(lambda m_, i, o, n=n: order.append(n)) for n in ("convc1", "convc2", "convf1", "convf2", "conv")]
    net, inp, corr, flow = _state(model)
    fused = FusedUpdate(blk)
    n1, m1, d1 = fused([t.clone() for t in net], inp, corr, flow)
    assert len(ran) == 3 and order == ["convc1", "convc2", "convf1", "convf2", "conv"]          # the reference's order, as it was
    n2, m2, d2 = fused([t.clone() for t in net], inp, corr, flow, mask=False)
    assert len(ran) == 3 and m2 is None and m1.shape == (2, 144, 10, 18)
    assert torch.equal(d1, d2) and all(torch.equal(a, b) for a, b in zip(n1, n2))
    want = L._plain_update(blk, [t.clone() for t in net], inp, corr, flow)
    assert _close(m1, want[1]) and _close(d1, want[2]) and all(_close(a, b) for a, b in zip(n1, want[0]))
    assert "raft_conv" not in stub.calls
    for h in hooks:
        h.remove()


def test_convs_true_is_seven_launches_and_five_without_the_mask(stub):
    from vppstereo_amd.update import FusedUpdate
    model = L.build_model()
    blk = model.update_block
    enc = blk.encoder
    seven = [enc.convc2, enc.convf2, enc.conv, blk.flow_head[0], blk.flow_head[2], blk.mask[0], blk.mask[2]]
    ran = []
    for m in seven:
        m.register_forward_hook(lambda m_, i, o: ran.append(m_))
    net, inp, corr, flow = _state(model)
    want = L._plain_update(blk, [t.clone() for t in net], inp, corr, flow)
    ran.clear()
    fused = FusedUpdate(blk, convs=True)
    assert fused.convs and not fused.gru_conv and not fused.motion_front
    n1, m1, d1 = fused([t.clone() for t in net], inp, corr, flow)
    assert ran == [] and stub.calls.count("raft_conv") == 7 and stub.calls.count("raft_conv_pack") == 7
    assert _close(m1, want[1]) and _close(d1, want[2]) and all(_close(a, b) for a, b in zip(n1, want[0]))
    assert d1.shape == (2, 2, 10, 18) and m1.shape == (2, 144, 10, 18)
    assert sorted(fused._bufs) == ["cor2", "flo2", "flow_head", "mask", "motion"] and tuple(fused._bufs["motion"].shape) == (2, L.MOTION, 10, 18)
    kept = {k: v.data_ptr() for k, v in fused._bufs.items()}
    n2, m2, d2 = fused([t.clone() for t in net], inp, corr, flow, mask=False)
    assert m2 is None and stub.calls.count("raft_conv") == 12 and stub.calls.count("raft_conv_pack") == 7
    assert torch.equal(d1, d2) and all(torch.equal(a, b) for a, b in zip(n1, n2)) and d2.data_ptr() != d1.data_ptr()
    assert {k: v.data_ptr() for k, v in fused._bufs.items()} == kept             # the buffers between the convolutions are kept
    # a head that is not plain falls back by itself: the other six stay on the kernel
    blk.mask[2].padding_mode = "replicate"
    n3, m3, d3 = fused([t.clone() for t in net], inp, corr, flow)
    assert ran == [blk.mask[2]] and stub.calls.count("raft_conv") == 18 and _close(m3, want[1])
    blk.mask[2].padding_mode = "zeros"
    ran.clear()
    # a hidden state of a dtype the kernel does not store: everything in torch
    blk.double()
    fused([t.double() for t in net], [[c.double() for c in lv] for lv in inp], corr.double(), flow.double())
    assert ran == seven[:3] + [seven[3], seven[4], seven[5], seven[6]] and stub.calls.count("raft_conv") == 18


def test_what_counts_as_a_plain_convolution():
    from vppstereo_amd.update import FusedUpdate
    nn = torch.nn
    plain = FusedUpdate._conv_plain
    assert plain(nn.Conv2d(128, 126, 3, padding=1), 128) and plain(nn.Conv2d(256, 144, 1), 256) and plain(nn.Conv2d(256, 2, 3, padding=1), 256)
    assert plain(nn.Conv2d(16, 1, 1, bias=False), 16)
    for conv, cin in ((nn.Conv2d(128, 126, 3, padding=1), 112), (nn.Conv2d(24, 16, 3, padding=1), 24), (nn.Conv2d(16, 16, 3), 16),
                      (nn.Conv2d(16, 16, 3, padding=1, stride=2), 16), (nn.Conv2d(16, 16, 3, padding=2, dilation=2), 16),
                      (nn.Conv2d(16, 16, 3, padding=1, groups=2), 16), (nn.Conv2d(16, 16, 3, padding=1, padding_mode="replicate"), 16),
                      (nn.Conv2d(16, 16, 5, padding=2), 16), (nn.Conv2d(16, 16, 1, padding=1), 16), (nn.Conv2d(16, 272, 3, padding=1), 16),
                      (nn.Conv2d(528, 16, 1), 528), (nn.Conv2d(16, 16, (1, 3), padding=(0, 1)), 16), (nn.Linear(16, 16), 16)):
        assert not plain(conv, cin), conv
    # the heads it knows
    seq = nn.Sequential(nn.Conv2d(16, 32, 3, padding=1), nn.ReLU(), nn.Conv2d(32, 2, 3, padding=1))
    assert FusedUpdate._head_convs(seq) == (seq[0], seq[2])

    class Head(nn.Module):                       # the reference's FlowHead, attribute for attribute
        def __init__(self):
            super().__init__()
            self.conv1, self.conv2, self.relu = nn.Conv2d(16, 32, 3, padding=1), nn.Conv2d(32, 2, 3, padding=1), nn.ReLU(inplace=True)

    head = Head()
    assert FusedUpdate._head_convs(head) == (head.conv1, head.conv2)
    assert FusedUpdate._head_convs(nn.Sequential(seq[0], nn.Tanh(), seq[2])) is None and FusedUpdate._head_convs(seq[0]) is None
    head.extra = nn.Conv2d(2, 2, 1)
    assert FusedUpdate._head_convs(head) is None


# ---- the packed weights of one convolution follow the module -------------------------------------------------------------------
CPU = torch.device("cpu")


def _follows(glue, eng, conv):
    w, b = glue._packed_conv(eng, conv, torch.float32, CPU)
    return torch.equal(w, conv.weight.detach()) and (b is None) == (conv.bias is None) and (b is None or torch.equal(b, conv.bias.detach()))


def test_the_cache_packs_once_and_again_after_each_replacement():
    from vppstereo_amd.update import GruGlue
    glue, eng = GruGlue(), _Stub()
    conv, other = torch.nn.Conv2d(32, 14, 3, padding=1), torch.nn.Conv2d(32, 144, 1, bias=False)
    first = glue._packed_conv(eng, conv, torch.float32, CPU)
    for _ in range(3):
        assert glue._packed_conv(eng, conv, torch.float32, CPU) is first
    assert len(eng.calls) == 1 and _follows(glue, eng, conv) and _follows(glue, eng, other) and len(eng.calls) == 2
    assert glue._packed[id(conv)][2] is None and glue._packed[id(conv)][3]() is conv            # the GRUs' layout: second slot empty
    conv.weight.data = torch.randn_like(conv.weight)                                           # `p.data = new`
    assert _follows(glue, eng, conv) and len(eng.calls) == 3
    conv.load_state_dict({k: torch.randn_like(v) for k, v in conv.state_dict().items()})       # in place: the version moves
    assert _follows(glue, eng, conv) and len(eng.calls) == 4
    conv.load_state_dict({k: torch.randn_like(v) for k, v in conv.state_dict().items()}, assign=True)
    assert _follows(glue, eng, conv) and len(eng.calls) == 5
    with torch.no_grad():
        conv.bias.copy_(torch.ones(14))
    assert _follows(glue, eng, conv) and len(eng.calls) == 6
    assert _follows(glue, eng, conv) and _follows(glue, eng, other) and len(eng.calls) == 6    # not again otherwise
    glue._packed_conv(eng, conv, torch.bfloat16, CPU)                                          # another dtype
    assert len(eng.calls) == 7
    conv.weight.data.mul_(2.0)                                                                 # through p.data: cannot be seen ...
    glue._packed_conv(eng, conv, torch.bfloat16, CPU)
    assert len(eng.calls) == 7
    glue.forget_weights()                                                                      # ... and forget_weights() clears these too
    assert glue._packed == {} and _follows(glue, eng, conv) and len(eng.calls) == 8
    _follows(glue, eng, other)
    assert set(glue._packed) == {id(conv), id(other)}
    del conv
    gc.collect()
    assert list(glue._packed) == [id(other)]                                                   # the entry dies with its module
