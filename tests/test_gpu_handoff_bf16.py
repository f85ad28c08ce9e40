"""The bfloat16 PSMNet volume and RAFT modulation (handoff_kernels.hip, VPPX_DT_BF16) against the band of
tests/_handoff_bf16_ref.py: a modulated cell is the single rounding of a float32 within R.limit() of the float64
referee, so it lies in [rne64(out64 - lim), rne64(out64 + lim)], and nothing is allowed beyond that.  Cells that are
not modulated (no hints, v == 0) and the cells left of a plane's cut are compared bit for bit.  What each input reaches
is asserted on the CPU in tests/test_handoff_bf16_cpu.py, on these very arrays."""
import numpy as np
import pytest

import _handoff_bf16_ref as BR
import _handoff_ref as R
from _cells import SENTINEL16 as S16

pytestmark = pytest.mark.gpu

DEVICE_EXP_ULPS = 1.0           # tests/test_gpu_handoff_ref.py's figure, justified there
_REFS = {}


def _psm(name):
    if name not in _REFS:
        c = BR.psm_case(name)
        _REFS[name] = (c, BR.psm_ref(c))
    return _REFS[name]


def _raft(name):
    if "raft " + name not in _REFS:
        c = BR.raft_case(name)
        _REFS["raft " + name] = (c, BR.raft_ref(c))
    return _REFS["raft " + name]


@pytest.fixture(scope="module")
def eng():
    import torch
    from vppstereo_amd.engine import Engine
    assert torch.cuda.is_available()
    return Engine()


def _dev(eng, a):
    import torch
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(eng.device)


def _bf(eng, b16, lead=0):
    """uint16 bits -> bfloat16 device tensor of the same shape, `lead` elements into its buffer (lead = 1: the tensor is
    2-byte aligned and no more)."""
    import torch
    b16 = np.ascontiguousarray(b16, np.uint16)
    buf = torch.full((b16.size + lead + 8,), S16, dtype=torch.int16, device=eng.device)
    assert buf.data_ptr() % 16 == 0
    buf[lead:lead + b16.size] = torch.from_numpy(b16.view(np.int16).reshape(-1)).to(eng.device)
    t = buf[lead:lead + b16.size].view(torch.bfloat16).view(b16.shape)
    assert t.is_contiguous() and t.data_ptr() == buf.data_ptr() + 2 * lead
    return t, buf


def _bits(t):
    import torch
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _guards_intact(buf, lead, n):
    w = buf.cpu().numpy().view(np.uint16)
    return (w[:lead] == S16).all() and (w[lead + n:] == S16).all()


def _psm_lib(eng, c, fl, fr, cost, with_hints=True, dtype=1, entry="vppx_psmnet_cost_volume_dt_dev"):
    from vppstereo_amd import _lib
    h, v = _dev(eng, c.hints), _dev(eng, c.valid)
    eng._bind_stream()
    args = (eng.ctx.handle, fl.data_ptr(), fr.data_ptr(), h.data_ptr() if with_hints else None, v.data_ptr() if with_hints else None,
            c.B, c.C, c.H4, c.W4, c.H, c.W, c.maxdisp, cost.data_ptr())
    _lib.check(getattr(eng.lib, entry)(*args, dtype) if entry.endswith("_dt_dev") else getattr(eng.lib, entry)(*args))
    eng.torch.cuda.synchronize()


def _hold_psm(got_bits, c, ref, what):
    want_plain = BR.psm_plain_bits(BR.bits(c.fl), BR.bits(c.fr), c.maxdisp)
    left = BR.left_of_cut(got_bits.shape)
    assert (got_bits[left] == 0).all(), f"{what}: a cell with x < i is not 0x0000"
    keep = (ref.v == 0) & ~left
    assert np.array_equal(got_bits[keep], want_plain[keep]), f"{what}: a cell with v == 0 is not the feature's bits"
    miss = BR.outside(BR.widen(got_bits), ref, DEVICE_EXP_ULPS) & ~left
    cells = BR.modulated_normal(ref)
    print(f"{what}: {int(cells.sum())} modulated cells of normal size, {int((miss & cells).sum())} outside the band, "
          f"{int((miss & ~cells).sum())} others outside")
    assert not miss.any(), f"{what}: {int(miss.sum())} modulated cells outside the band (or of another class than NaN / infinity)"


# ---- PSMNet volume ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BR.PSM_NAMES)
def test_psm_bf16_volume_is_inside_the_band(eng, name):
    import torch
    c, ref = _psm(name)
    fl, _ = _bf(eng, BR.bits(c.fl))
    fr, _ = _bf(eng, BR.bits(c.fr))
    cost = eng.psmnet_cost_volume(fl, fr, c.maxdisp, _dev(eng, c.hints), _dev(eng, c.valid))
    assert cost.dtype == torch.bfloat16 and cost.shape == ref.out.shape
    got = _bits(cost)
    _hold_psm(got, c, ref, f"psm bf16 {name}")
    plain = _bits(eng.psmnet_cost_volume(fl, fr, c.maxdisp))
    want_plain = BR.psm_plain_bits(BR.bits(c.fl), BR.bits(c.fr), c.maxdisp)
    assert np.array_equal(plain, want_plain)
    # the same call with each tensor in turn one element into its buffer: 2-byte aligned and no more, which takes the
    # narrow route at every W4.  The same bits, and nothing written outside the volume.
    n = got.size
    for which in ("cost", "fl", "fr"):
        lead = {k: int(k == which) for k in ("cost", "fl", "fr")}
        fl1, _ = _bf(eng, BR.bits(c.fl), lead["fl"])
        fr1, _ = _bf(eng, BR.bits(c.fr), lead["fr"])
        for with_hints, want in ((True, got), (False, plain)):
            out, buf = _bf(eng, np.full(n, S16, np.uint16), lead["cost"])
            _psm_lib(eng, c, fl1, fr1, out, with_hints)
            assert _guards_intact(buf, lead["cost"], n), (which, with_hints)
            assert np.array_equal(_bits(out), want.reshape(-1)), (which, with_hints)


@pytest.mark.parametrize("lead", [0, 1])
def test_psm_bf16_cells_without_a_hint_are_copies_of_the_bits(eng, lead):
    """Quiet and signalling NaN patterns, both infinities, -0 and subnormals: with no hints at all, and with hints whose
    valid map is 0 (or -0) at every pixel."""
    c = BR.copy_case()
    want = BR.psm_plain_bits(c.flb, c.frb, c.maxdisp)
    fl, _ = _bf(eng, c.flb, lead)
    fr, _ = _bf(eng, c.frb)
    assert np.array_equal(_bits(eng.psmnet_cost_volume(fl, fr, c.maxdisp)), want)
    H, W = 4 * c.H4 + 1, 4 * c.W4 + 2
    hints = np.full((1, 1, H, W), 7.0, np.float32)
    valid = np.zeros((1, 1, H, W), np.float32)
    valid[0, 0, ::2] = -0.0
    assert np.array_equal(_bits(eng.psmnet_cost_volume(fl, fr, c.maxdisp, _dev(eng, hints), _dev(eng, valid))), want)
    # one pixel with a hint: every other cell is still a copy, in the hinted pixel's own vector too
    valid[0, 0, R.nearest_indices(H, c.H4)[1], R.nearest_indices(W, c.W4)[9]] = 1.0
    got = _bits(eng.psmnet_cost_volume(fl, fr, c.maxdisp, _dev(eng, hints), _dev(eng, valid)))
    other = np.ones(want.shape, bool)
    other[:, :, :, 1, 9] = False
    assert np.array_equal(got[other], want[other]) and not np.array_equal(got, want)


# ---- RAFT modulation --------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("name", list(R.RAFT_CASES))
def test_raft_bf16_modulation_is_inside_the_band(eng, name, lead):
    import torch
    c, ref = _raft(name)
    before = BR.raft_sentinel_bits(c)
    corr, buf = _bf(eng, before, lead)
    got = eng.raft_corr_modulate_(corr, _dev(eng, c.hints), _dev(eng, c.valid))
    assert got is corr and got.dtype == torch.bfloat16
    got = _bits(got)
    assert _guards_intact(buf, lead, before.size)
    rows = np.broadcast_to((c.v4 == 0)[..., None, None], before.shape)
    assert np.array_equal(got[rows], before[rows]), "a row with v == 0 was rewritten"
    miss = BR.outside(BR.widen(got), ref, DEVICE_EXP_ULPS)
    cells = BR.modulated_normal(ref)
    print(f"raft bf16 {name}: {int(cells.sum())} modulated cells of normal size, {int(miss.sum())} outside the band")
    assert not miss.any()


# ---- the float32 case of the new entries ------------------------------------------------------------------
def test_dt_entries_with_f32_equal_the_float32_entries_bit_for_bit(eng):
    import torch
    from vppstereo_amd import _lib
    c = R.psm_case("w68")
    fl, fr = _dev(eng, c.fl), _dev(eng, c.fr)
    n = 2 * c.B * c.C * c.D4 * c.H4 * c.W4
    outs = []
    for entry in ("vppx_psmnet_cost_volume_dev", "vppx_psmnet_cost_volume_dt_dev"):
        out = torch.zeros(n, dtype=torch.float32, device=eng.device)
        _psm_lib(eng, c, fl, fr, out, True, _lib.DT_F32, entry)
        outs.append(out.cpu().numpy().view(np.uint32))
    assert np.array_equal(outs[0], outs[1]) and outs[0].any()
    r = R.raft_case("w65")
    h, v = _dev(eng, r.hints), _dev(eng, r.valid)
    a, b = _dev(eng, r.corr), _dev(eng, r.corr)
    eng._bind_stream()
    _lib.check(eng.lib.vppx_raft_corr_modulate_dev(eng.ctx.handle, a.data_ptr(), h.data_ptr(), v.data_ptr(), r.B, r.H4, r.W2, r.W3, r.H, r.W))
    _lib.check(eng.lib.vppx_raft_corr_modulate_dt_dev(eng.ctx.handle, b.data_ptr(), h.data_ptr(), v.data_ptr(), r.B, r.H4, r.W2, r.W3, r.H,
                                                      r.W, _lib.DT_F32))
    assert np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))
    assert not np.array_equal(a.cpu().numpy(), r.corr)


# ---- refusals: nothing is launched, outputs keep their bytes, inputs are unchanged -------------------------
def test_refusals_leave_every_byte_alone(eng):
    import torch
    from vppstereo_amd._lib import VppxError
    inp = torch.full((4096,), 1.0, dtype=torch.float32, device=eng.device)
    out = torch.full((4096,), 0x7FA5A5A5, dtype=torch.int32, device=eng.device)
    p, o = inp.data_ptr(), out.data_ptr()
    eng._bind_stream()
    rc = eng.lib.vppx_psmnet_cost_volume_dt_dev(eng.ctx.handle, p, p, p, p, 1, 1, 2, 2, 8, 8, 8, o, 2)
    assert rc == -1 and eng.lib.vppx_last_error().decode() == "vppx_psmnet_cost_volume: dtype 2 is neither VPPX_DT_F32 (0) nor VPPX_DT_BF16 (1)"
    rc = eng.lib.vppx_raft_corr_modulate_dt_dev(eng.ctx.handle, o, p, p, 1, 2, 2, 2, 8, 8, 2)
    assert rc == -1 and eng.lib.vppx_last_error().decode() == "vppx_raft_corr_modulate: dtype 2 is neither VPPX_DT_F32 (0) nor VPPX_DT_BF16 (1)"
    # the float32 entries' own checks, through the bf16 case, with their messages
    rc = eng.lib.vppx_psmnet_cost_volume_dt_dev(eng.ctx.handle, p, p, p, None, 1, 1, 2, 2, 8, 8, 8, o, 1)
    assert rc == -1 and eng.lib.vppx_last_error().decode() == "vppx_psmnet_cost_volume: bad arguments"
    rc = eng.lib.vppx_psmnet_cost_volume_dt_dev(eng.ctx.handle, p, p, p, p, 1, 1, 2, 2, 12, 8, 8, o, 1)
    assert rc == -1 and eng.lib.vppx_last_error().decode() == "hints are 12x8: sub-sampled by 4 that is 3x2, but the features are 2x2"
    rc = eng.lib.vppx_psmnet_cost_volume_dt_dev(eng.ctx.handle, p, p, None, None, 1, 1, 2, 2, 8, 8, 4 * 65536, o, 1)
    assert rc == -10 and eng.lib.vppx_last_error().decode() == "psmnet cost volume: maxdisp/4 and B must be <= 65535"
    rc = eng.lib.vppx_raft_corr_modulate_dt_dev(eng.ctx.handle, o, p, p, 1, 2, 2, 0, 8, 8, 1)
    assert rc == -1 and eng.lib.vppx_last_error().decode() == "vppx_raft_corr_modulate: bad arguments"
    eng.torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x7FA5A5A5).all() and (inp.cpu().numpy() == 1.0).all()

    # through Engine
    bf = lambda *s: torch.full(s, 3.0, dtype=torch.bfloat16, device=eng.device)        # noqa: E731
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=eng.device)            # noqa: E731
    corr = bf(2, 2, 3, 1, 5)
    h = f32(2, 1, 8, 12)
    with pytest.raises(ValueError, match="feature maps must have the same dtype"):
        eng.psmnet_cost_volume(bf(2, 4, 2, 3), f32(2, 4, 2, 3), 8)
    with pytest.raises(ValueError, match="feature maps must have the same dtype"):
        eng.psmnet_cost_volume(f32(2, 4, 2, 3), bf(2, 4, 2, 3), 8)
    with pytest.raises(ValueError, match="feature maps must have the same dtype"):
        eng.raft_corr(bf(2, 4, 2, 3), f32(2, 4, 2, 5))
    with pytest.raises(ValueError, match="fea_l: expected contiguous"):
        eng.psmnet_cost_volume(bf(2, 4, 2, 3).half(), bf(2, 4, 2, 3).half(), 8)
    for args, msg in (((corr, h.bfloat16(), h), "hints: expected contiguous"), ((corr, h, h.bfloat16()), "validhints: expected contiguous"),
                      ((corr, h, f32(2, 1, 8, 11)), "hints / validhints must be \\[B,1,H,W\\]")):
        with pytest.raises(ValueError, match=msg):
            eng.raft_corr_modulate_(*args)
    with pytest.raises(ValueError, match="hints: expected contiguous"):
        eng.psmnet_cost_volume(bf(2, 4, 2, 3), bf(2, 4, 2, 3), 8, h.bfloat16(), h)
    with pytest.raises(VppxError, match="hints are 12x12: sub-sampled by 4 that is 3x3, but the features are 2x3") as e:
        eng.raft_corr_modulate_(corr, f32(2, 1, 12, 12), f32(2, 1, 12, 12))
    assert e.value.code == -1
    assert (corr == 3.0).all().item()


# ---- Engine.raft_corr -------------------------------------------------------------------------------------
def test_raft_corr_with_bf16_maps_returns_bf16_and_modulates_its_own_result(eng):
    import torch
    c, _ = _raft("w65_narrow")
    rng = np.random.default_rng(71)
    f2, _ = _bf(eng, BR.bits(BR.bf16_rne_f32(rng.standard_normal((c.B, 8, c.H4, c.W2)).astype(np.float32))))
    f3, _ = _bf(eng, BR.bits(BR.bf16_rne_f32(rng.standard_normal((c.B, 8, c.H4, c.W3)).astype(np.float32))))
    h, v = _dev(eng, c.hints), _dev(eng, c.valid)
    plain = eng.raft_corr(f2, f3)
    full = eng.raft_corr(f2, f3, h, v)
    assert plain.dtype == full.dtype == torch.bfloat16 and full.shape == (c.B, c.H4, c.W2, 1, c.W3)
    again = eng.raft_corr_modulate_(plain.clone(), h, v)
    assert np.array_equal(_bits(full), _bits(again)) and not np.array_equal(_bits(full), _bits(plain))
    ref = R.raft_modulate(BR.widen(_bits(plain)), c.hints, c.valid, rule="library")
    assert not BR.outside(BR.widen(_bits(full)), ref, DEVICE_EXP_ULPS).any()


# ---- one context, both dtypes -----------------------------------------------------------------------------
def _f32_psm(e, name):
    a = R.psm_case(name)
    return e.psmnet_cost_volume(_dev(e, a.fl), _dev(e, a.fr), a.maxdisp, _dev(e, a.hints), _dev(e, a.valid)).cpu().numpy().view(np.uint32)


def _bf16_psm(e, name):
    b, _ = _psm(name)
    return _bits(e.psmnet_cost_volume(_bf(e, BR.bits(b.fl))[0], _bf(e, BR.bits(b.fr))[0], b.maxdisp, _dev(e, b.hints), _dev(e, b.valid)))


def _f32_raft(e, name):
    r = R.raft_case(name)
    return e.raft_corr_modulate_(_dev(e, r.corr), _dev(e, r.hints), _dev(e, r.valid)).cpu().numpy().view(np.uint32)


def _bf16_raft(e, name):
    r, _ = _raft(name)
    return _bits(e.raft_corr_modulate_(_bf(e, BR.bits(r.corr))[0], _dev(e, r.hints), _dev(e, r.valid)))


def test_one_context_through_float32_bf16_float32_equals_fresh_contexts(eng):
    """WS_HANDOFF_H / _V hold the sub-sampled hints of whichever call came last, in whichever shape and for whichever
    dtype: float32, bf16, float32 on shapes that grow and shrink, on one context, against each call alone on a context of
    its own."""
    from vppstereo_amd.engine import Engine
    calls = ((_f32_psm, "w68"), (_bf16_psm, "w16_d24"), (_bf16_raft, "w130"), (_f32_raft, "w65"), (_bf16_psm, "w72"), (_f32_psm, "w5_tall"))
    shared = [fn(eng, name) for fn, name in calls]
    for (fn, name), got in zip(calls, shared):
        assert np.array_equal(fn(Engine(), name), got), (fn.__name__, name)
