"""tests/_raft_loop.py without a GPU: the plain composition can fail the end-to-end bound of tests/test_gpu_raft_loop.py, the spy
records what it says, the adapters accept a referee's own value and refuse one cell moved by three limits, and the packed-weight
cache of vppstereo_amd.update.GruGlue follows its GRU's parameters and dies with its GRU."""
import copy
import gc
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _raft_loop as L

F32, F64 = np.float32, np.float64
B, H, W, ITERS, CROP = 2, 40, 72, 3, (3, 5, 2, 6)
FACTOR = 4                                   # the end-to-end bound: fused error <= FACTOR * plain error
_RUNS = {}


def _tensors(a, dtype=torch.float32):
    return [torch.from_numpy(getattr(a, k)).to(dtype) for k in ("image0", "image2", "image3", "hints", "validhints")]


def _named(res):
    return {"flow": res.flow, "net0": res.net[0], "net1": res.net[1], "net2": res.net[2], "disparity": res.disparity}


def _run(dtype, schedule="default", mistake=None):
    """One plain forward on the CPU, made once per (dtype, schedule, mistake) and left unchanged."""
    key = (dtype, schedule, mistake)
    if key not in _RUNS:
        if "model" not in _RUNS:
            _RUNS["model"] = L.build_model()
        model = _RUNS["model"] if dtype == torch.float32 else copy.deepcopy(_RUNS["model"]).double()
        res = L.plain_forward(model, *_tensors(L.inputs(B, H, W), dtype), iters=ITERS, schedule=schedule, crop=CROP, mistake=mistake)
        _RUNS[key] = {k: v.double().numpy() for k, v in _named(res).items()}
    return _RUNS[key]


def _yardstick(schedule="default"):
    ref, f32 = _run(torch.float64, schedule), _run(torch.float32, schedule)
    return {k: float(np.abs(f32[k] - ref[k]).max()) for k in ref}


# ---- the composition ---------------------------------------------------------------------------------------------------------
def test_the_yardstick_is_a_float32_error():
    ref = _run(torch.float64)
    assert ref["flow"].shape == (B, 2, 10, 18) and ref["disparity"].shape == (B, 1, H - 8, W - 8)
    assert [ref[f"net{i}"].shape for i in range(3)] == [(B, 16) + s for s in L.map_sizes(H, W)] == [(B, 16, 10, 18), (B, 16, 5, 9), (B, 16, 3, 5)]
    assert (ref["flow"][:, 1] == 0).all() and np.abs(ref["flow"][:, 0]).max() > 0.5        # the flow moves, along the row only
    assert np.allclose(ref["disparity"].mean(), -4 * ref["flow"][:, 0].mean(), atol=0.5 * np.abs(ref["flow"][:, 0]).max())
    for k, e in _yardstick().items():
        scale = np.abs(ref[k]).max()
        print(f"float32 against float64, {k}: max error {e:.3e} at a scale of {scale:.3f}")
        assert 0 < e < 1e-3 * scale, k


@pytest.mark.parametrize("mistake", L.MISTAKES)
def test_a_planted_mistake_leaves_the_bound(mistake):
    """Each mistake in the composition, evaluated in float64, lies further from the float64 run than FACTOR times what float32
    arithmetic does: the bound of the GPU file can fail."""
    ref, bad, yard = _run(torch.float64), _run(torch.float64, mistake=mistake), _yardstick()
    over = {k: float(np.abs(bad[k] - ref[k]).max()) / yard[k] for k in ref}
    print(f"{mistake}: distance / yardstick " + ", ".join(f"{k} {v:.3g}" for k, v in over.items()))
    assert max(over.values()) > 100 * FACTOR, over
    if mistake == "flow_sign":
        assert over["disparity"] > 100 * FACTOR and over["flow"] == 0
    else:
        assert over["net0"] > FACTOR and over["disparity"] > FACTOR and over["flow"] > FACTOR, over


def test_the_schedules_differ():
    a, b = _run(torch.float64), _run(torch.float64, "slow_fast")
    yard = _yardstick("slow_fast")
    assert all(np.abs(a[k] - b[k]).max() > FACTOR * yard[k] for k in a)


def test_the_lookup_and_the_pyramid_are_the_referees():
    """plain_lookup and plain_pyramid against tests/_corr_ref.py, whose arithmetic is the library's: the same taps within float32
    rounding of a linear interpolation."""
    import _corr_ref as CR
    rng = np.random.default_rng(6003)
    level0 = rng.standard_normal((2 * 3 * 18, 18)).astype(F32)
    cx = rng.uniform(-3, 21, (2, 3, 18)).astype(F32)
    cx.reshape(-1)[:40] = np.floor(cx.reshape(-1)[:40])
    pyr = CR.pyramid(level0, 4)
    mine = L.plain_pyramid(torch.from_numpy(level0).view(2, 3, 18, 18))
    for a, b in zip(mine, pyr):
        assert np.array_equal(a.numpy().reshape(b.shape), b)
    want = CR.channels_first(CR.lookup(pyr, cx, 4), 2, 3, 18)
    got = L.plain_lookup(mine, torch.from_numpy(cx)).numpy()
    assert got.shape == want.shape == (2, 36, 3, 18)
    assert np.abs(got - want).max() <= 32 * 2.0 ** -24 * np.abs(level0).max()


def test_the_volume_is_the_referees():
    import _handoff_ref as HR
    a = L.inputs(B, H, W)
    rng = np.random.default_rng(6004)
    f2, f3 = rng.standard_normal((B, 8, 10, 18)), rng.standard_normal((B, 8, 10, 18))
    c64, _ = HR.corr_whole(f2.astype(F32), f3.astype(F32), a.hints, a.validhints, 1.0)
    got = L.plain_volume(torch.from_numpy(f2.astype(F32)).double(), torch.from_numpy(f3.astype(F32)).double(), torch.from_numpy(a.hints).double(),
                         torch.from_numpy(a.validhints).double()).numpy()
    _, v = HR.subsample(a.hints, a.validhints, raft=True)
    assert 5 <= int((v != 0).sum()) < v.size // 2                               # some rows are modulated, most are not
    assert np.abs(got - c64[:, :, :, 0, :]).max() <= 1e-5 * np.abs(c64).max()    # c64 goes through a float32 cell on its way


# ---- the spy -------------------------------------------------------------------------------------------------------------------
class _FakeEngine:
    def raft_norm_apply(self, x, stats, weight=None, bias=None, relu=True, out=None):
        out.copy_(x * 2 + stats.sum())
        return out

    def raft_gru_zr(self, hx, packed, cz, cr, h, z=None, rh=None):
        z.fill_(1.0), rh.fill_(2.0)
        return z, rh

    def raft_gru_assemble(self, sources, out=None):
        raise RuntimeError("refused")


def _restored(eng):
    return not vars(eng) and all(getattr(eng, n).__func__ is getattr(_FakeEngine, n) for n in ("raft_norm_apply", "raft_gru_zr", "raft_gru_assemble"))


def test_the_spy_copies_before_and_after_and_restores():
    eng = _FakeEngine()
    names = ("raft_norm_apply", "raft_gru_zr", "raft_gru_assemble")
    x, st = torch.arange(6.0).view(1, 1, 2, 3), torch.ones(1, 1, 2)
    with L.LaunchSpy(eng, names) as spy:
        assert "raft_norm_apply" in vars(eng)
        assert eng.raft_norm_apply(x, st, relu=True, out=x) is x               # in place
        z, rh = torch.zeros(2), torch.zeros(2)
        eng.raft_gru_zr([x, (x, "copy")], None, x, x, x, z=z, rh=rh)
    assert _restored(eng)
    a, b = spy.records
    assert a.name == "raft_norm_apply" and torch.equal(a.args[0], torch.arange(6.0).view(1, 1, 2, 3))      # as it was before the call
    assert torch.equal(a.result, x) and torch.equal(a.out["out"], x) and a.result is not x and a.kwargs["relu"] is True
    assert torch.equal(a.kwargs["out"], a.args[0])                               # the buffer as handed in
    assert isinstance(b.args[0], list) and isinstance(b.args[0][1], tuple) and b.args[0][1][1] == "copy" and b.args[1] is None
    assert torch.equal(b.out["z"], torch.ones(2)) and torch.equal(b.out["rh"], 2 * torch.ones(2)) and torch.equal(b.kwargs["z"], torch.zeros(2))
    assert spy.counts() == {"raft_norm_apply": 1, "raft_gru_zr": 1, "raft_gru_assemble": 0} and spy.of("raft_gru_zr") == [b]
    x.zero_()
    assert a.result.abs().sum() > 0                                              # copies of their own


def test_the_spy_restores_after_an_exception():
    eng = _FakeEngine()
    with pytest.raises(RuntimeError, match="refused"):
        with L.LaunchSpy(eng, ("raft_norm_apply", "raft_gru_zr", "raft_gru_assemble")) as spy:
            eng.raft_gru_assemble([])
    assert _restored(eng) and spy.records == []
    eng.raft_norm_apply = "mine"                                                 # an attribute of the instance's own comes back
    with L.LaunchSpy(eng, ("raft_gru_zr",)):
        pass
    with L.LaunchSpy(eng, ("raft_norm_apply",)):
        assert callable(eng.raft_norm_apply)
    assert eng.raft_norm_apply == "mine"


# ---- the adapters ------------------------------------------------------------------------------------------------------------
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, F32))


def _rec(name, args, kwargs=None, result=None, out=None):
    return SimpleNamespace(name=name, args=tuple(args), kwargs=dict(kwargs or {}), result=result, out=dict(out or {}))


def _moved(ref, by=3.0):
    """The referee's value as float32 cells, and the same with the cell of the largest finite limit moved by `by` limits (at
    least by four float32 units in the last place, so that the move survives the rounding to float32)."""
    good = ref.value.astype(F32)
    lim = np.where(np.isfinite(ref.limit) & np.isfinite(ref.value), ref.limit, 0.0)
    at = np.unravel_index(np.argmax(lim), lim.shape)
    assert lim[at] > 0
    bad = good.copy()
    bad[at] = F32(ref.value[at] + max(by * lim[at], 4 * np.spacing(np.abs(good[at]))))
    assert abs(float(bad[at]) - ref.value[at]) > lim[at]
    return good, bad


def _accepts_then_refuses(check, make, ref, *extra):
    good, bad = _moved(ref)
    check(make(good), *extra, "fabricated")
    with pytest.raises(AssertionError):
        check(make(bad), *extra, "one cell moved")


def test_norm_adapters():
    import _norm_ref as N
    rng = np.random.default_rng(6010)
    x = rng.standard_normal((2, 3, 5, 7)).astype(F32) * 2 + 0.5
    _accepts_then_refuses(L.check_norm_stats, lambda v: _rec("raft_norm_stats", [_t(x)], dict(eps=1e-5), _t(v)), N.stats_value(N.stats(x)))
    st = rng.standard_normal((2, 3, 2)).astype(F32)
    st[..., 1] = np.abs(st[..., 1]) + 0.5
    w, b, res = rng.standard_normal(3).astype(F32), rng.standard_normal(3).astype(F32), rng.standard_normal(x.shape).astype(F32)
    rst = np.abs(rng.standard_normal((3, 2))).astype(F32) + 0.5
    ref = N.apply(x, L._given(st), w, b, relu_inner=True, res=res, res_stats=L._given(rst), res_weight=b, res_bias=w)
    kw = dict(relu=True, residual=_t(res), residual_stats=_t(rst), residual_weight=_t(b), residual_bias=_t(w))
    _accepts_then_refuses(L.check_norm_apply, lambda v: _rec("raft_norm_apply", [_t(x), _t(st), _t(w), _t(b)], kw, _t(v)), ref)
    ref = N.apply(x, L._given(rst), relu_inner=False)                            # one set of statistics for every frame, the plain norm
    _accepts_then_refuses(L.check_norm_apply, lambda v: _rec("raft_norm_apply", [_t(x), _t(rst)], dict(relu=False), _t(v)), ref)


def test_corr_adapter():
    import _corr_fused_ref as FR
    import _corr_ref as CR
    a = L.inputs(1, 8, 40)
    rng = np.random.default_rng(6011)
    f2, f3 = rng.standard_normal((1, 8, 2, 10)).astype(F32), rng.standard_normal((1, 8, 2, 10)).astype(F32)
    c64, lim = FR.bound(f2, f3, a.hints, a.validhints, False)
    ref = SimpleNamespace(value=c64, limit=lim)

    def make(level0):
        pyr = CR.pyramid(np.ascontiguousarray(level0, F32), 3)
        return _rec("raft_corr_fused", [_t(f2), _t(f3), _t(a.hints), _t(a.validhints), 3], {}, [_t(p).view(p.shape[0], 1, 1, p.shape[1]) for p in pyr])

    _accepts_then_refuses(L.check_corr_fused, make, ref)
    rec = make(c64.astype(F32))
    rec.result[2][3, 0, 0, 1] += 1e-3                                             # a level above that is not the pooled level below
    with pytest.raises(AssertionError, match="level 2"):
        L.check_corr_fused(rec, "level moved")


def test_motion_adapter():
    import _motion_ref as M
    c = M.case("k15_ks3")
    pyr = M.pyramid_of(c)
    ref_c, ref_f = M.case_ref(c)
    coords2 = np.stack([c.coords, np.zeros_like(c.coords)], axis=1)

    def make(cor, flo):
        return _rec("raft_motion_front", [[_t(p).view(p.shape[0], 1, 1, p.shape[1]) for p in pyr], _t(coords2), _t(c.flow), _t(c.wc), _t(c.bias_c),
                                          _t(c.wf), _t(c.bias_f), c.radius], dict(out_dtype=torch.float32), (_t(cor), _t(flo)))

    _accepts_then_refuses(L.check_motion_front, lambda v: make(v, ref_f.value), ref_c)
    _accepts_then_refuses(L.check_motion_front, lambda v: make(ref_c.value, v), ref_f)


def test_assemble_adapter():
    import _gru_ref as G
    rng = np.random.default_rng(6012)
    h, p, i = (rng.standard_normal(s).astype(F32) for s in ((2, 4, 5, 9), (2, 3, 10, 18), (2, 2, 3, 5)))
    ref = G.assemble([(h, "copy"), (p, "pool2x"), (i, "interp")], 5, 9)
    src = [(_t(h), "copy"), (_t(p), "pool2x"), (_t(i), "interp")]
    _accepts_then_refuses(L.check_assemble, lambda v: _rec("raft_gru_assemble", [src], dict(out=_t(np.zeros_like(v))), _t(v), dict(out=_t(v))), ref)


def test_gru_adapters():
    import _gruconv_ref as R
    rng = np.random.default_rng(6013)
    C, C1, shape = 16, 16, (1, 16, 5, 7)
    Wt = {}
    for cv in ("convz", "convr", "convq"):
        Wt[f"{cv}_weight"] = (rng.standard_normal((C, C + C1, 3, 3)) * 0.1).astype(F32)
        Wt[f"{cv}_bias"] = (rng.standard_normal(C) * 0.5).astype(F32)
    h, x = np.tanh(rng.standard_normal(shape)).astype(F32), rng.standard_normal(shape).astype(F32)
    cz, cr, cq = (rng.standard_normal(shape).astype(F32) for _ in range(3))
    hx = np.concatenate([h, x], axis=1)
    z, rh = R.zr(hx, None, Wt["convz_weight"], Wt["convz_bias"], Wt["convr_weight"], Wt["convr_bias"], cz, cr, h)
    zr_rec = lambda zv, rv: _rec("raft_gru_zr", [_t(hx), None, _t(cz), _t(cr), _t(h)], dict(z=_t(zv), rh=_t(rv)), (_t(zv), _t(rv)))     # noqa: E731
    _accepts_then_refuses(L.check_gru_zr, lambda v: zr_rec(v, rh.value), z, Wt)
    _accepts_then_refuses(L.check_gru_zr, lambda v: zr_rec(z.value, v), rh, Wt)
    z32, rh32 = z.value.astype(F32), rh.value.astype(F32)
    ref = R.q(rh32, x, Wt["convq_weight"], Wt["convq_bias"], cq, z32, h)
    _accepts_then_refuses(L.check_gru_q, lambda v: _rec("raft_gru_q", [_t(rh32), None, _t(cq), _t(z32), _t(h)], dict(x1=_t(x)), _t(v)), ref, Wt)
    gru = SimpleNamespace(**{cv: SimpleNamespace(weight=_t(Wt[f"{cv}_weight"]), bias=_t(Wt[f"{cv}_bias"])) for cv in ("convz", "convr", "convq")})
    assert all(np.array_equal(v, Wt[k]) for k, v in L.gru_weights(gru).items())


def test_upsample_adapter():
    import _readout_ref as RO
    rng = np.random.default_rng(6014)
    flow, mask = rng.standard_normal((1, 2, 3, 4)).astype(F32) * 3, rng.standard_normal((1, 144, 3, 4)).astype(F32)
    ref = RO.raft_upsample(flow, mask, 4, negate=True, channels=1, crop=[1, 2, 3, 0])
    kw = dict(negate=True, channels=1, crop=[1, 2, 3, 0])
    _accepts_then_refuses(L.check_upsample, lambda v: _rec("raft_upsample", [_t(flow), _t(mask)], kw, _t(v)), ref)
    with pytest.raises(AssertionError):                                          # the sign
        L.check_upsample(_rec("raft_upsample", [_t(flow), _t(mask)], kw, _t(-ref.value)), "negated")


def test_check_all_refuses_a_launch_without_a_referee():
    spy = SimpleNamespace(records=[_rec("raft_gru_reset", [])])
    with pytest.raises(AssertionError, match="no referee"):
        L.check_all(spy, L.build_model(), L.map_sizes(H, W))


# ---- the packed weights follow the module ------------------------------------------------------------------------------------
class _Packer:
    """An engine whose packing counts its calls and returns what it was given."""

    def __init__(self):
        self.calls = 0

    def raft_conv3x3_pack(self, weight, bias=None, dtype=None):
        self.calls += 1
        return (weight.detach().clone(), None if bias is None else bias.detach().clone())


CPU = torch.device("cpu")


def _gru(seed, scale=1.0):
    torch.manual_seed(seed)
    g = torch.nn.Module()
    g.convz, g.convr, g.convq = (torch.nn.Conv2d(32, 16, 3, padding=1) for _ in range(3))
    with torch.no_grad():
        g.convq.weight.mul_(scale)
    return g


def _packed(glue, eng, gru):
    """-> (convz + convr weights, convq's weight) the glue holds for this GRU now."""
    zr, q = glue._packed_weights(eng, gru, torch.float32, CPU)
    return zr[0], q[0]


def _current(gru):
    return torch.cat([gru.convz.weight, gru.convr.weight]).detach(), gru.convq.weight.detach()


def _follows(glue, eng, gru):
    got, want = _packed(glue, eng, gru), _current(gru)
    return torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_packing_happens_once_while_nothing_changes():
    from vppstereo_amd.update import GruGlue
    glue, eng, gru = GruGlue(), _Packer(), _gru(1)
    first = glue._packed_weights(eng, gru, torch.float32, CPU)
    assert eng.calls == 2 and _follows(glue, eng, gru)
    for _ in range(3):
        again = glue._packed_weights(eng, gru, torch.float32, CPU)
        assert again[0] is first[0] and again[1] is first[1]
    assert eng.calls == 2
    glue._packed_weights(eng, gru, torch.bfloat16, CPU)                          # another dtype: packed again
    assert eng.calls == 4


def test_packing_follows_p_data_assignment():
    """`p.data = new` changes neither id(p) nor p._version; the storage moves."""
    from vppstereo_amd.update import GruGlue
    glue, eng, gru = GruGlue(), _Packer(), _gru(2)
    assert _follows(glue, eng, gru)
    p = gru.convq.weight
    before = (id(p), p._version, p.data_ptr())
    p.data = torch.randn_like(p)
    assert (id(p), p._version) == before[:2] and p.data_ptr() != before[2]
    assert _follows(glue, eng, gru), "the packed weights are those of before `p.data = new`"
    assert eng.calls == 4
    gru.convz.bias.data = torch.ones(16)                                         # a bias likewise
    zr, _ = glue._packed_weights(eng, gru, torch.float32, CPU)
    assert eng.calls == 6 and torch.equal(zr[1][:16], torch.ones(16))


def test_packing_follows_load_state_dict_copy_and_to():
    from vppstereo_amd.update import GruGlue
    glue, eng, gru = GruGlue(), _Packer(), _gru(3)
    assert _follows(glue, eng, gru)
    calls = eng.calls
    new = {k: torch.randn_like(v) for k, v in gru.state_dict().items()}
    gru.load_state_dict(new)                                                     # in place
    assert _follows(glue, eng, gru) and eng.calls == calls + 2
    new = {k: torch.randn_like(v) for k, v in gru.state_dict().items()}
    gru.load_state_dict(new, assign=True)                                        # other parameter objects
    assert gru.convq.weight.data_ptr() == new["convq.weight"].data_ptr()
    assert _follows(glue, eng, gru) and eng.calls == calls + 4
    with torch.no_grad():
        gru.convr.weight.copy_(torch.randn_like(gru.convr.weight))
    assert _follows(glue, eng, gru) and eng.calls == calls + 6
    gru.to(torch.float64)                                                        # a module moved by .to(): every storage is new
    assert _follows(glue, eng, gru) and eng.calls == calls + 8
    assert _follows(glue, eng, gru) and eng.calls == calls + 8


def test_a_write_through_p_data_needs_forget_weights():
    """`p.data.mul_()` moves neither the pointer nor the version: it cannot be seen, and forget_weights() is the way out.
    FusedUpdate inherits it."""
    from vppstereo_amd.update import FusedUpdate, GruGlue
    glue, eng, gru = GruGlue(), _Packer(), _gru(4)
    assert _follows(glue, eng, gru)
    p = gru.convq.weight
    before = (id(p), p._version, p.data_ptr())
    p.data.mul_(3.0)
    assert (id(p), p._version, p.data_ptr()) == before
    assert not _follows(glue, eng, gru) and eng.calls == 2                      # documented: the old packed weights
    glue.forget_weights()
    assert glue._packed == {} and _follows(glue, eng, gru) and eng.calls == 4
    assert FusedUpdate.forget_weights is GruGlue.forget_weights


def test_an_entry_goes_with_its_gru():
    from vppstereo_amd.update import GruGlue
    glue, eng, gru = GruGlue(), _Packer(), _gru(5)
    other = _gru(6)
    assert _follows(glue, eng, gru) and _follows(glue, eng, other) and len(glue._packed) == 2
    del gru
    gc.collect()
    assert list(glue._packed) == [id(other)]


TRIES = 4096


class _Plain:
    """A convolution as a plain object."""


class _PlainGru:
    """A GRU as a plain object of a size few other objects have, so that little else competes for its freed address."""
    __slots__ = ("convz", "convr", "convq", "__weakref__") + tuple(f"pad{k}" for k in range(27))


def _hunt(make, wanted):
    """Objects of `make` are built and kept until every address of `wanted` has come back -> ({address: object}, tries)."""
    found, others = {}, []
    for tries in range(1, TRIES + 1):
        obj = make()
        if id(obj) in wanted and id(obj) not in found:
            found[id(obj)] = obj
            if len(found) == len(wanted):
                break
        else:
            others.append(obj)
    return found, tries


def test_a_new_gru_at_a_freed_grus_address_is_packed_again():
    """The module-level glue behind fused_gru() outlives the GRUs it has seen.  One GRU is shown to it and freed; objects and
    parameters are then built until the GRU's address and its six parameters' addresses have all come back, and a GRU with other
    weights is put together from them: everything the old stamp looked at (id() and version counter) is the same, and the
    weights are not."""
    from vppstereo_amd import update as U
    eng = _Packer()
    names = [(cv, p) for cv in ("convz", "convr", "convq") for p in ("weight", "bias")]
    shapes = {"weight": (16, 32, 3, 3), "bias": (16,)}

    def build(objs):
        g = objs.pop()
        for cv in ("convz", "convr", "convq"):
            setattr(g, cv, _Plain())
        for (cv, p), t in zip(names, objs):
            setattr(getattr(g, cv), p, t)
        return g

    gru = build([torch.nn.Parameter(torch.full(shapes[p], 1.0), requires_grad=False) for _, p in names] + [_PlainGru()])
    key = id(gru)
    first = [(id(getattr(getattr(gru, cv), p)), getattr(getattr(gru, cv), p)._version) for cv, p in names]
    try:
        assert _follows(U._glue, eng, gru) and eng.calls == 2
        del gru
        gc.collect()
        objs, tries_g = _hunt(_PlainGru, {key})         # first: the longer the address lies free, the likelier something else takes it
        # the addresses may come back in any order: each parameter gets the shape of the role its address had
        params, tries_p = _hunt(lambda: torch.nn.Parameter(torch.zeros(1), requires_grad=False), {a for a, _ in first})
        for (a, _), (_, p) in zip(first, names):
            if a in params:
                params[a].data = torch.full(shapes[p], 2.0)
        if len(params) < 6 or len(objs) < 1:
            pytest.skip(f"the allocator brought {len(params)} of 6 parameter addresses and {len(objs)} of 1 GRU address back "
                        f"within {TRIES} tries each")
        print(f"the first GRU's id() came back after {tries_g} objects, its six parameters' after {tries_p} parameters")
        gru = build([params[a] for a, _ in first] + [objs[key]])
        assert id(gru) == key and [(id(getattr(getattr(gru, cv), p)), getattr(getattr(gru, cv), p)._version) for cv, p in names] == first
        assert _follows(U._glue, eng, gru), "the packed weights are those of a GRU that is gone"
        assert eng.calls == 4
    finally:
        U._glue._packed.pop(key, None)
