"""The motion encoder's front (motion_kernels.hip: the lookup fused into convc1, and convf1) and
vppstereo_amd.update.FusedUpdate(block, motion_front=True) against the float64 referee of tests/_motion_ref.py.

No atol.  Every finite float32 cell is held to the referee's limit(), every bfloat16 cell to the band the single
rounding of a float32 inside that limit can reach; a cell that is not finite must have the referee's class.  Sentinel
cells in front of, behind and between the outputs must be intact.  What the cases reach, and that the planted mistakes
leave the limit on these very arrays, is asserted on the CPU in tests/test_motion_ref_cpu.py."""
from types import SimpleNamespace

import numpy as np
import pytest

import _corr_ref as CR
import _gru_ref as G
import _motion_ref as R
from _cells import DTYPES, INVALID, SENTINEL16, SENTINEL32, UNSUPPORTED
from _cells import bits as _bits, dev as _dev, guarded as _guarded, guards_intact as _guards_intact, hold, host as _host
from _cells import tdtype as _tdtype

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
_REFS = {}


@pytest.fixture(scope="module")
def eng():
    import torch
    from vppstereo_amd.engine import Engine
    assert torch.cuda.is_available()
    return Engine()


def _pyramid(eng, levels, shift=0):
    """Host levels ([N,Wi] float32 cells or uint16 bfloat16 bits) on the device, laid out as raft_corr_pyramid lays them
    (level 0 on its own, levels 1.. back to back); shift: both buffers start that many cells off a 16-byte boundary."""
    import torch
    N, W3 = levels[0].shape
    bf16 = levels[0].dtype == np.uint16
    tdt = torch.bfloat16 if bf16 else torch.float32
    cells, off = eng._corr_offsets(N, W3, len(levels))

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a).view(np.int16) if bf16 else np.ascontiguousarray(a)).to(eng.device)
        return t.view(tdt) if bf16 else t

    l0 = torch.zeros((N * W3 + shift,), dtype=tdt, device=eng.device)[shift:]
    l0.copy_(up(levels[0]).reshape(-1))
    out = [l0.view(N, 1, 1, W3)]
    pyr = torch.zeros((cells + shift,), dtype=tdt, device=eng.device)[shift:]
    for i in range(1, len(levels)):
        Wi = W3 >> i
        pyr[off[i]:off[i] + N * Wi].copy_(up(levels[i]).reshape(-1))
        out.append(pyr[off[i]:off[i] + N * Wi].view(N, 1, 1, Wi))
    return out


def _ref(name, pdtype, nonfinite=False):
    key = (name, pdtype, nonfinite)
    if key not in _REFS:
        c = R.case(name, nonfinite=nonfinite)
        _REFS[key] = (c, R.pyramid_of(c, pdtype), R.case_ref(c, pdtype))
    return _REFS[key]


def _weights(eng, c):
    return _dev(eng, c.wc), _dev(eng, c.bias_c), _dev(eng, c.wf), _dev(eng, c.bias_f)


def _coords(eng, c):
    """[B,H4,W2], or for the case with W2 != W3 channel 0 of a [B,2,H4,W2] tensor whose channel 1 is NaN."""
    if c.name != "w2_ne_w3":
        return _dev(eng, c.coords)
    two = np.full((c.B, 2, c.H4, c.W2), np.nan, F32)
    two[:, 0] = c.coords
    return _dev(eng, two)


# ---- the cases against the referee -----------------------------------------------------------------------------------
@pytest.mark.parametrize("odtype", DTYPES)
@pytest.mark.parametrize("pdtype", DTYPES)
@pytest.mark.parametrize("name", list(R.CASES))
def test_front_equals_the_referee(eng, name, pdtype, odtype):
    import torch
    c, levels, (ref_c, ref_f) = _ref(name, pdtype)
    pyr, coords, flow, w = _pyramid(eng, levels), _coords(eng, c), _dev(eng, c.flow), _weights(eng, c)
    sc, sf = (c.B, c.Cc, c.H4, c.W2), (c.B, c.Cf, c.H4, c.W2)
    buf_c, out_c = _guarded(eng, sc, odtype)
    buf_f, out_f = _guarded(eng, sf, odtype)
    got = eng.raft_motion_front(pyr, coords, flow, *w, radius=c.radius, out=(out_c, out_f))
    torch.cuda.synchronize()
    assert got[0].data_ptr() == out_c.data_ptr() and got[1].data_ptr() == out_f.data_ptr() and got[0].dtype == _tdtype(odtype)
    hold(R, _host(out_c), ref_c, f"{name} cor1 (pyramid {pdtype})", odtype)
    hold(R, _host(out_f), ref_f, f"{name} flo1 (pyramid {pdtype})", odtype)
    assert _guards_intact(buf_c, int(np.prod(sc))) and _guards_intact(buf_f, int(np.prod(sf)))
    bits_c, bits_f = _bits(out_c), _bits(out_f)
    # a pixel whose taps are all +0 (a coordinate far outside, infinite or NaN) gives relu(bias) exactly
    zero = R.zero_tap_pixels(c, pdtype)
    assert zero.sum() >= 9
    want = _dev(eng, np.maximum(c.bias_c, 0)).to(_tdtype(odtype)).float().cpu().numpy()
    at_zero = _host(out_c).transpose(0, 2, 3, 1)[zero]
    assert np.array_equal(at_zero, np.broadcast_to(want, at_zero.shape))
    # fresh outputs of the asked dtype: the same bits
    fresh = eng.raft_motion_front(pyr, coords, flow, *w, radius=c.radius, out_dtype=_tdtype(odtype))
    assert fresh[0].shape == sc and fresh[1].shape == sf and fresh[0].is_contiguous()
    assert np.array_equal(_bits(fresh[0]), bits_c) and np.array_equal(_bits(fresh[1]), bits_f)
    # the two halves of one [B,Cc+Cf,H4,W2] buffer, and the same with a channel between them that stays as it is
    plane = c.H4 * c.W2
    for gap in (0, 1):
        shape = (c.B, c.Cc + gap + c.Cf, c.H4, c.W2)
        buf, both = _guarded(eng, shape, odtype)
        if plane % 8 == 0:
            assert both.data_ptr() % 16 == 0 and both[:, c.Cc + gap:].data_ptr() % 16 == 0          # the 16-byte route
        eng.raft_motion_front(pyr, coords, flow, *w, radius=c.radius, out=(both[:, :c.Cc], both[:, c.Cc + gap:]))
        torch.cuda.synchronize()
        assert np.array_equal(_bits(both[:, :c.Cc]), bits_c) and np.array_equal(_bits(both[:, c.Cc + gap:]), bits_f), gap
        assert _guards_intact(buf, int(np.prod(shape)))
        if gap:
            assert (_bits(both[:, c.Cc]) == (SENTINEL16 if odtype == "bfloat16" else SENTINEL32)).all()
    # every pointer one cell off its buffer's boundary: the cell-by-cell route, the same bits
    buf_c2, out_c2 = _guarded(eng, sc, odtype, shift=1)
    buf_f2, out_f2 = _guarded(eng, sf, odtype, shift=1)
    assert out_c2.data_ptr() % 16 != 0 and out_f2.data_ptr() % 16 != 0
    flat = torch.zeros((flow.numel() + 1,), dtype=torch.float32, device=eng.device)
    flow2 = flat[1:].view(*flow.shape)
    flow2.copy_(flow)
    eng.raft_motion_front(_pyramid(eng, levels, shift=1), coords, flow2, *w, radius=c.radius, out=(out_c2, out_f2))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out_c2), bits_c) and np.array_equal(_bits(out_f2), bits_f)
    assert _guards_intact(buf_c2, int(np.prod(sc)), shift=1) and _guards_intact(buf_f2, int(np.prod(sf)), shift=1)


@pytest.mark.parametrize("pdtype", DTYPES)
def test_taps_are_the_lookups_bit_for_bit(eng, pdtype):
    """A convc1 that passes tap k to channel k (and its negative to channel k of a second call), no bias: a sum of one term and
    zeros is exact, so cor1 is relu(+-lookup) bit for bit, from the lookup call itself and from the referee."""
    import torch
    for name in ("low_map", "w2_ne_w3", "k15_ks3"):
        c, levels, _ = _ref(name, pdtype)
        assert c.K <= 36
        wc = np.zeros((96, c.K, 1, 1), F32)
        wc[np.arange(c.K), np.arange(c.K)] = 1.0
        wc[48 + np.arange(c.K), np.arange(c.K)] = -1.0
        pyr, coords = _pyramid(eng, levels), _coords(eng, c)
        look = eng.raft_corr_lookup(pyr, coords, c.radius)
        assert CR.same_bits(_host(look), CR.channels_first(R.taps_of(levels, c.coords, c.radius), c.B, c.H4, c.W2)) == 0
        for half in (0, 1):                                       # 48 channels at a time: 36 live ones
            w = _dev(eng, wc[48 * half:48 * half + 48])
            cor, _ = eng.raft_motion_front(pyr, coords, _dev(eng, c.flow), w, None, _dev(eng, c.wf), None, radius=c.radius)
            torch.cuda.synchronize()
            want = torch.relu(-look if half else look)
            got = cor[:, :c.K]
            assert bool(((got == want) | (torch.isnan(got) & torch.isnan(want))).all()), (name, half)
            assert bool((got[want != 0].view(torch.int32) == want[want != 0].view(torch.int32)).all())
            assert bool((cor[:, c.K:] == 0).all())


# ---- the recording -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("odtype", DTYPES)
@pytest.mark.parametrize("pdtype", DTYPES)
def test_front_replays_the_recording(eng, pdtype, odtype):
    import torch
    c, cor1, flo1 = R.golden_case()
    levels = c.pyr if pdtype == "float32" else CR.pyramid(R.BR.bits(R.BR.bf16_rne_f32(c.level0)), 4)
    key = ("golden", pdtype)
    if key not in _REFS:
        _REFS[key] = R.front(levels, c.coords, c.flow, c.wc, c.bias_c, c.wf, c.bias_f, c.radius)
    ref_c, ref_f = _REFS[key]
    got_c, got_f = eng.raft_motion_front(_pyramid(eng, levels), _dev(eng, c.coords2), _dev(eng, c.flow), _dev(eng, c.wc), _dev(eng, c.bias_c),
                                         _dev(eng, c.wf), _dev(eng, c.bias_f), radius=4, out_dtype=_tdtype(odtype))
    torch.cuda.synchronize()
    hold(R, _host(got_c), ref_c, "recording cor1", odtype)
    hold(R, _host(got_f), ref_f, "recording flo1", odtype)
    # against the recording itself: both lie within the limit of one value.  flo1 does not depend on the pyramid.
    pairs = [(got_f, flo1, ref_f)] + ([(got_c, cor1, ref_c)] if pdtype == "float32" else [])
    for got, rec, ref in pairs:
        g = _host(got).astype(F64)
        if odtype == "float32":
            assert (np.abs(g - rec) <= 2 * ref.limit).all()
        else:
            assert ((g >= R.BR.rne64(rec - 2 * ref.limit)) & (g <= R.BR.rne64(rec + 2 * ref.limit))).all()


# ---- a flow that is not finite -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("odtype", DTYPES)
def test_a_nan_and_an_inf_in_the_flow_stay_in_their_windows(eng, odtype):
    import torch
    c, levels, (ref_c, ref_f) = _ref("low_map", "float32", nonfinite=True)
    got_c, got_f = eng.raft_motion_front(_pyramid(eng, levels), _coords(eng, c), _dev(eng, c.flow), *_weights(eng, c), radius=c.radius,
                                         out_dtype=_tdtype(odtype))
    torch.cuda.synchronize()
    hold(R, _host(got_c), ref_c, "nonfinite flow: cor1", odtype)
    hold(R, _host(got_f), ref_f, "nonfinite flow: flo1", odtype)      # classes: NaN, +inf; -inf is cut by the ReLU
    b, _, y, x = R.NONFINITE_FLOW["nan"]
    nan = np.isnan(_host(got_f))
    want = np.zeros_like(nan)
    want[b, :, max(y - 3, 0):y + 4, max(x - 3, 0):x + 4] = True
    assert np.array_equal(nan, want)
    assert np.isposinf(_host(got_f)).sum() > 100 and not np.isneginf(_host(got_f)).any() and np.isfinite(_host(got_c)).all()


# ---- refusals: before anything is launched, with no output byte touched ------------------------------------------------------
def test_refusals_leave_every_byte_alone(eng):
    import torch
    lib, ctx = eng.lib, eng.ctx.handle
    inp = torch.full((1 << 16,), 1.0, dtype=torch.float32, device=eng.device)
    out = torch.full((1 << 16,), SENTINEL32, dtype=torch.int32, device=eng.device)
    p, o = inp.data_ptr(), out.data_ptr()
    o2 = o + 4 * (1 << 15)
    eng._bind_stream()

    def call(corr=p, pyr=p, coords=p, cs=35, flow=p, fs=70, wc=p, bc=p, Cc=16, wf=p, bf=p, Cf=16, ks=3, B=2, H4=5, W2=7, W3=16, levels=4,
             radius=4, oc=o, ocs=16 * 35, of=o2, ofs=16 * 35, dtype=0, odtype=0):
        return lib.vppx_raft_motion_front_dt_dev(ctx, corr, pyr, coords, cs, flow, fs, wc, bc, Cc, wf, bf, Cf, ks, B, H4, W2, W3, levels, radius,
                                                 oc, ocs, of, ofs, dtype, odtype)

    def lookup(corr=p, pyr=p, coords=p, cs=35, B=2, H4=5, W2=7, W3=16, levels=4, radius=4, out_=o, dtype=0):
        return lib.vppx_raft_corr_lookup_dt_dev(ctx, corr, pyr, coords, cs, B, H4, W2, W3, levels, radius, out_, dtype)

    bad = "vppx_raft_motion_front: bad arguments"
    # everything the lookup refuses, with the lookup's codes
    for kw in (dict(corr=None), dict(coords=None), dict(pyr=None), dict(B=0), dict(H4=0), dict(W2=-1), dict(W3=0), dict(levels=0),
               dict(radius=-1), dict(dtype=2), dict(levels=5), dict(radius=9), dict(W3=15), dict(cs=34)):
        rc, text = call(**kw), lib.vppx_last_error().decode()
        assert rc == lookup(**kw) and rc in (INVALID, UNSUPPORTED), (kw, rc)
        assert text.startswith("vppx_raft_motion_front"), (kw, text)
    table = (
        (dict(flow=None), INVALID, bad), (dict(wc=None), INVALID, bad), (dict(wf=None), INVALID, bad), (dict(oc=None), INVALID, bad),
        (dict(of=None), INVALID, bad),
        (dict(fs=69), INVALID, "flow_frame_stride 69 is less than 2 planes of 5x7"),
        (dict(ocs=16 * 35 - 1), INVALID, "out_c_frame_stride 559 is less than 16 planes of 5x7"),
        (dict(ofs=0), INVALID, "out_f_frame_stride 0 is less than 16 planes"),
        (dict(Cc=0), INVALID, "the channels must be positive and the window odd"), (dict(Cf=-16), INVALID, "the channels must be positive"),
        (dict(ks=2), INVALID, "a 2x2 window"), (dict(ks=0), INVALID, "a 0x0 window"), (dict(ks=-1), INVALID, "window odd"),
        (dict(odtype=2), INVALID, "out_dtype 2 is neither VPPX_DT_F32 (0) nor VPPX_DT_BF16 (1)"), (dict(odtype=-1), INVALID, "out_dtype -1"),
        (dict(Cc=24, ocs=24 * 35), UNSUPPORTED, "multiples of 16 up to 64"), (dict(Cf=8), UNSUPPORTED, "multiples of 16 up to 64"),
        (dict(Cc=80, ocs=80 * 35), UNSUPPORTED, "up to 64"), (dict(Cf=128, ofs=128 * 35), UNSUPPORTED, "up to 64"),
        (dict(ks=9), UNSUPPORTED, "windows up to 7x7"),
        (dict(B=1 << 11, H4=1 << 10, W2=1 << 10, cs=1 << 20, fs=1 << 21, ocs=1 << 24, ofs=1 << 24), UNSUPPORTED, "more than one launch takes"),
    )
    for n, (kw, code, msg) in enumerate(table):
        rc = call(**kw)
        text = lib.vppx_last_error().decode()
        assert rc == code and msg in text, (n, rc, code, msg, text)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL32).all() and (inp.cpu().numpy() == 1.0).all()
    # what is allowed: NULL biases, the smallest of everything
    assert call(bc=None, bf=None, ks=1, B=1, H4=1, W2=1, W3=2, levels=1, radius=0, cs=1, fs=2, ocs=16, ofs=16) == 0
    torch.cuda.synchronize()
    raw = out.cpu().numpy()
    assert (raw[16:1 << 15] == SENTINEL32).all() and (raw[(1 << 15) + 16:] == SENTINEL32).all() and (raw[:16] != SENTINEL32).all()

    # through Engine
    c, levels, _ = _ref("k15_ks3", "float32")
    pyr, coords, flow, (wc, bc, wf, bf) = _pyramid(eng, levels), _coords(eng, c), _dev(eng, c.flow), _weights(eng, c)
    with pytest.raises(ValueError, match=r"convc1_weight: expected \[Cc,27,1,1\]"):
        eng.raft_motion_front(pyr, coords, flow, wc, bc, wf, bf, radius=4)
    with pytest.raises(ValueError, match="flow: expected shape"):
        eng.raft_motion_front(pyr, coords, flow[:, :1].contiguous(), wc, bc, wf, bf, radius=2)
    with pytest.raises(ValueError, match=r"convf1_weight: expected \[Cf,2,ks,ks\]"):
        eng.raft_motion_front(pyr, coords, flow, wc, bc, wf[:, :1].contiguous(), bf, radius=2)
    with pytest.raises(ValueError, match="convc1_bias: expected shape"):
        eng.raft_motion_front(pyr, coords, flow, wc, bf, wf, bf, radius=2)
    with pytest.raises(ValueError, match="out_dtype must be"):
        eng.raft_motion_front(pyr, coords, flow, wc, bc, wf, bf, radius=2, out_dtype=torch.float16)
    with pytest.raises(ValueError, match="the pyramid has"):
        eng.raft_motion_front(pyr, coords[:1].contiguous(), flow[:1].contiguous(), wc, bc, wf, bf, radius=2)
    with pytest.raises(ValueError, match=r"out\[1\]: expected shape"):
        eng.raft_motion_front(pyr, coords, flow, wc, bc, wf, bf, radius=2, out=(torch.empty((c.B, c.Cc, c.H4, c.W2), device=eng.device),
                                                                                  torch.empty((c.B, c.Cc, c.H4, c.W2), device=eng.device)))


# ---- one context across changing shapes ----------------------------------------------------------------------------------
def test_one_context_through_changing_shapes(eng):
    """The cases in turn through one context, both dtypes alternating, with the lookup and the GRU's gates between them;
    the first call again at the end gives the first call's bits."""
    import torch
    gc = G.gate_case("c3_5x7")
    gref = G.update(gc.az, gc.cz, gc.aq, gc.cq, gc.h, 1.0)
    first = None
    plan = list(R.CASES) + ["low_map"]
    for step, name in enumerate(plan):
        pdtype, odtype = DTYPES[step % 2], DTYPES[(step // 2) % 2]
        if step == len(plan) - 1:
            pdtype, odtype = DTYPES[0], DTYPES[0]
        c, levels, (ref_c, ref_f) = _ref(name, pdtype)
        pyr, coords = _pyramid(eng, levels), _coords(eng, c)
        look = eng.raft_corr_lookup(pyr, coords, c.radius)
        got_c, got_f = eng.raft_motion_front(pyr, coords, _dev(eng, c.flow), *_weights(eng, c), radius=c.radius, out_dtype=_tdtype(odtype))
        h = eng.raft_gru_update(*(_dev(eng, a) for a in (gc.az, gc.cz, gc.aq, gc.cq, gc.h)))
        torch.cuda.synchronize()
        assert CR.same_bits(_host(look), CR.channels_first(R.taps_of(levels, c.coords, c.radius), c.B, c.H4, c.W2)) == 0
        hold(R, _host(got_c), ref_c, f"step {step} {name} cor1", odtype)
        hold(R, _host(got_f), ref_f, f"step {step} {name} flo1", odtype)
        assert G.misses(_host(h), gref) == 0
        if step == 0:
            first = (_bits(got_c), _bits(got_f))
    assert np.array_equal(_bits(got_c), first[0]) and np.array_equal(_bits(got_f), first[1])


# ---- FusedUpdate -------------------------------------------------------------------------------------------------------------
class _Conv:
    """A stand-in convolution that replays the recording: it holds what it is given to `check` and returns `result`.
    `weight` and `bias` are what FusedUpdate hands to the fused launch."""

    def __init__(self, name, log, check, result, weight=None, bias=None):
        self.name, self.log, self.check, self.result, self.weight, self.bias = name, log, check, result, weight, bias

    def __call__(self, x):
        self.log.append(self.name)
        self.check(x)
        return self.result(x)


def test_fused_update_with_the_motion_front_replays_the_recording(eng):
    import torch
    from vppstereo_amd.corr import CorrBlock1D, DeferredCorr
    from vppstereo_amd.update import FusedUpdate
    c, cor1, flo1 = R.golden_case()
    key = ("golden", "float32")
    if key not in _REFS:
        _REFS[key] = R.front(c.pyr, c.coords, c.flow, c.wc, c.bias_c, c.wf, c.bias_f, c.radius)
    ref_c, ref_f = _REFS[key]
    log, seen = [], {}

    def exact(want):
        def check(x):
            assert CR.same_bits(_host(x), want) == 0
        return check

    def keep(name, ref, rec):
        def check(x):
            assert x.dtype == torch.float32 and x.is_contiguous()
            seen[name] = _host(x)
            hold(R, seen[name], ref, f"the input of {name}")
            assert (np.abs(seen[name].astype(F64) - rec) <= 2 * ref.limit).all()
        return check

    def pointwise(cout):
        def f(x):
            k = torch.linspace(-1.5, 1.5, cout, device=x.device).view(1, cout, 1, 1)
            return torch.sin(x.float().sum(dim=1, keepdim=True) * 0.7 + k) * 2.0
        return f

    nothing = lambda x: None                                                             # noqa: E731
    enc = SimpleNamespace(
        convc1=_Conv("convc1", log, exact(c.lookup), lambda x: _dev(eng, cor1), _dev(eng, c.wc), _dev(eng, c.bias_c)),
        convf1=_Conv("convf1", log, exact(c.flow), lambda x: _dev(eng, flo1), _dev(eng, c.wf), _dev(eng, c.bias_f)),
        convc2=_Conv("convc2", log, keep("convc2", ref_c, cor1), pointwise(8)),
        convf2=_Conv("convf2", log, keep("convf2", ref_f, flo1), pointwise(8)),
        conv=_Conv("conv", log, nothing, pointwise(6)))
    hid = 4
    gru = SimpleNamespace(**{cv: _Conv(f"gru08.{cv}", log, nothing, pointwise(hid)) for cv in ("convz", "convr", "convq")})
    blk = SimpleNamespace(encoder=enc, gru08=gru, gru16=None, gru32=None, flow_head=_Conv("flow_head", log, nothing, pointwise(2)),
                          mask=_Conv("mask", log, nothing, pointwise(9)), n_gru_layers=1)
    rng = np.random.default_rng(5604)
    net_h = np.tanh(rng.standard_normal((c.B, hid, c.H4, c.W2))).astype(F32)
    inp_h = rng.standard_normal((c.B, 3 * hid, c.H4, c.W2)).astype(F32)

    block = CorrBlock1D.__new__(CorrBlock1D)                  # the recorded pyramid in the drop-in block, without its constructor
    block.num_levels, block.radius, block._eng, block.corr_pyramid = 4, 4, eng, _pyramid(eng, c.pyr)
    coords = _dev(eng, c.coords2)
    deferred = block.deferred(coords)
    assert isinstance(deferred, DeferredCorr) and deferred.radius == 4 and deferred.coords is coords
    assert CR.same_bits(_host(deferred.materialize()), c.lookup) == 0 and CR.same_bits(_host(block(coords)), c.lookup) == 0

    def run(fused, corr):
        del log[:]
        seen.clear()
        net = [_dev(eng, net_h)]
        res = fused(net, [list(_dev(eng, inp_h).split(hid, dim=1))], corr, _dev(eng, c.flow), iter16=False, iter32=False)
        torch.cuda.synchronize()
        return list(log), dict(seen), [_host(t) for t in (res[0][0], res[1], res[2])]

    tail = ["convc2", "convf2", "conv", "gru08.convz", "gru08.convr", "gru08.convq", "flow_head", "mask"]
    assert FusedUpdate(blk).motion_front is False
    fused_log, fused_seen, fused_out = run(FusedUpdate(blk, motion_front=True), deferred)
    assert fused_log == tail                                   # convc1 and convf1 did not run: the launch made their outputs
    for mode, corr in ((False, deferred), (False, _dev(eng, c.lookup)), (True, _dev(eng, c.lookup))):
        old_log, old_seen, old_out = run(FusedUpdate(blk, motion_front=mode), corr)
        assert old_log[:4] == ["convc1", "convc2", "convf1", "convf2"] and sorted(old_log) == sorted(["convc1", "convf1"] + tail)
        assert np.array_equal(old_seen["convc2"], cor1) and np.array_equal(old_seen["convf2"], flo1)
        # the two paths: each within the limit of the value, so within twice the limit of each other
        for name, ref in (("convc2", ref_c), ("convf2", ref_f)):
            assert (np.abs(fused_seen[name].astype(F64) - old_seen[name]) <= 2 * ref.limit).all()
        for a, b in zip(fused_out, old_out):
            assert a.shape == b.shape and np.isfinite(a).all()
