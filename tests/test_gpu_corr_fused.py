"""The fused correlation call (corr_gemm_kernels.hip: GEMM on the matrix cores, / sqrt(D), hint modulation, pyramid) against
the numpy referee of tests/_corr_fused_ref.py: bit for bit where the features make the float32 sums exact, within the
referee's bound where they do not; its refusals; vppstereo_amd.corr.CorrBlock1DFused on the arrays the reference's own
CorrBlock1D produced.  What each input reaches is asserted on the CPU in tests/test_corr_fused_ref_cpu.py, on these very
arrays."""
import ctypes as C

import numpy as np
import pytest

import _corr_fused_ref as FR
import _corr_ref as CR
import _handoff_bf16_ref as BR
import _handoff_ref as R
from _cells import DTYPES, GUARD, SENTINEL16 as S16, SENTINEL32 as S32

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
ALL_SHAPES = FR.GOLDEN_TAGS + FR.DIRECTED_SHAPES


def _id(s):
    return s if isinstance(s, str) else FR.tag(s)


def _case(s):
    return FR.golden_case(s) if isinstance(s, str) else FR.case(s)


@pytest.fixture(scope="module")
def eng():
    import torch
    from vppstereo_amd.engine import Engine
    assert torch.cuda.is_available()
    return Engine()


def _dev(eng, a):
    import torch
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(eng.device)


def _feat(eng, a, dtype, misaligned=False):
    """A feature map [B,D,H4,W] of float32 values that bfloat16 holds -> device tensor of `dtype`; `misaligned`: a view
    that starts one element into its buffer."""
    import torch
    a = np.ascontiguousarray(a, F32)
    if dtype == "float32":
        flat = _dev(eng, a.reshape(-1))
    else:
        u = a.view(np.uint32)
        assert not (u & 0xFFFF).any(), "not a bfloat16 value"
        flat = _dev(eng, (u >> 16).astype(np.uint16).view(np.int16).reshape(-1)).view(torch.bfloat16)
    if misaligned:
        buf = torch.zeros(flat.numel() + 9, dtype=flat.dtype, device=eng.device)
        buf[1:1 + flat.numel()] = flat
        flat = buf[1:1 + flat.numel()]
        assert flat.data_ptr() % 16 != 0
    return flat.view(a.shape)


def _maps(eng, c, dtype):
    mis = c.shape == FR.MISALIGNED_SHAPE
    return _feat(eng, c.f2, dtype, mis), _feat(eng, c.f3, dtype, mis)


def _host(t):
    """A device tensor's cells as the referee holds them: float32 values or bf16 bits, [N, W]."""
    import torch
    if t.dtype == torch.bfloat16:
        a = t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    else:
        a = t.cpu().numpy()
    return a.reshape(a.shape[0], -1) if a.ndim == 4 else a


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == F32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def _fused(eng, c, dtype, hints=False, levels=4):
    f2, f3 = _maps(eng, c, dtype)
    h, v = (_dev(eng, c.hints), _dev(eng, c.valid)) if hints else (None, None)
    return eng.raft_corr_fused(f2, f3, h, v, levels)


_F32_PLAIN = {}


def _f32_plain(eng, s):
    """The float32 fused pyramid without hints of a shape, computed once: (device list, host list)."""
    if _id(s) not in _F32_PLAIN:
        pyr = _fused(eng, _case(s), "float32")
        _F32_PLAIN[_id(s)] = (pyr, [_host(p) for p in pyr])
    return _F32_PLAIN[_id(s)]


# ---- 1. float32, no hints, exact features ----------------------------------------------------------------------
@pytest.mark.parametrize("s", ALL_SHAPES, ids=_id)
def test_float32_levels_equal_the_exact_referee_bit_for_bit(eng, s):
    c = _case(s)
    pyr, host = _f32_plain(eng, s)
    assert len(pyr) == 4 and [tuple(p.shape) for p in pyr] == [(c.N, 1, 1, c.W3 >> i) for i in range(4)]
    assert pyr[2].data_ptr() == pyr[1].data_ptr() + c.N * (c.W3 >> 1) * 4, "levels 1.. are not views into one buffer"
    want = CR.pyramid(FR.exact_level0(c.f2, c.f3), 4)
    for i in range(4):
        assert _same(host[i], want[i]), (_id(s), i, int((host[i].view(np.uint32) != want[i].view(np.uint32)).sum()))
    if isinstance(s, str):      # the recording, D = 2, 3, 8 included, where torch's reciprocal multiply cannot be equal
        for i in range(4):
            assert _same(host[i], c.g(f"plain_level{i}"))
        out = eng.raft_corr_lookup(pyr, _dev(eng, c.coords), 4).cpu().numpy()
        assert _same(out, c.g("plain_lookup"))


# ---- 2. asymmetry -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_hot_fmap2_picks_a_plane_of_fmap3(eng, dtype):
    """f2 != f3 and W2 != W3 in every directed shape of test 1, so a swapped or transposed operand fails there; here row
    x2 of level 0 is plane khot[b, y, x2] of fmap3, divided by sqrt(D)."""
    c = FR.case(FR.ONE_HOT_SHAPE, "one_hot")
    got = _host(_fused(eng, c, dtype)[0])
    plane = np.take_along_axis(c.f3[:, :, :, None, :], c.khot[:, None, :, :, None], axis=1)[:, 0].reshape(c.N, c.W3)
    want = (F32(0) + np.ascontiguousarray(plane)) / np.sqrt(F32(c.D))
    assert _same(got, want if dtype == "float32" else FR.bf16_round(want))


# ---- 3. float32 with hints --------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", ALL_SHAPES, ids=_id)
def test_float32_with_hints_equals_the_pyramid_call_on_the_plain_level0(eng, s):
    c = _case(s)
    plain, plain_host = _f32_plain(eng, s)
    got = [_host(p) for p in _fused(eng, c, "float32", hints=True)]
    level0 = plain[0].clone().view(c.B, c.H4, c.W2, 1, c.W3)
    want = [_host(p) for p in eng.raft_corr_pyramid(level0, _dev(eng, c.hints), _dev(eng, c.valid), 4)]
    for i in range(4):
        assert _same(got[i], want[i]), (_id(s), i)
    rows0 = c.v4.reshape(-1) == 0
    assert rows0.any() and _same(got[0][rows0], plain_host[0][rows0]), "a row with v == 0 lost its plain bits"
    assert not _same(got[0][~rows0], plain_host[0][~rows0])


# ---- 4. bfloat16, exact features --------------------------------------------------------------------------------
@pytest.mark.parametrize("hints", [False, True], ids=["plain", "hints"])
@pytest.mark.parametrize("s", ALL_SHAPES, ids=_id)
def test_bfloat16_level0_is_the_float32_result_rounded_once(eng, s, hints):
    import torch
    c = _case(s)
    f32 = _f32_plain(eng, s)[1][0] if not hints else _host(_fused(eng, c, "float32", hints=True, levels=1)[0])
    pyr = _fused(eng, c, "bfloat16", hints=hints)
    assert all(p.dtype == torch.bfloat16 for p in pyr)
    got = [_host(p) for p in pyr]
    assert _same(got[0], FR.bf16_round(f32)), (_id(s), int((got[0] != FR.bf16_round(f32)).sum()))
    again = eng.raft_corr_pyramid(pyr[0].clone().view(c.B, c.H4, c.W2, 1, c.W3), None, None, 4)
    for i in range(1, 4):
        assert _same(got[i], _host(again[i])), (_id(s), i)
        assert _same(got[i], CR.pyramid(got[0], 4)[i])


# ---- 5. random features -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("hints", [False, True], ids=["plain", "hints"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_random_features_stay_within_the_bound(eng, dtype, hints):
    """Measured on an MI355X, worst distance / bound: float32 0.0049 with and without hints (the bound allows D roundings
    of the dot product at its absolute sum; the kernel's errors mostly cancel), bfloat16 0.974 (the rounding of the store
    is nearly all of the bound and is reached)."""
    c = FR.case(FR.RANDOM_SHAPE, "random")
    got = CR.widened([_host(_fused(eng, c, dtype, hints=hints)[0])])[0]
    c64, lim = FR.bound(c.f2, c.f3, c.hints if hints else None, c.valid if hints else None, dtype == "bfloat16")
    dist = np.abs(got.astype(F64) - c64)
    beyond = ~(dist <= lim) & (got != 0)
    worst = float(np.max(np.where(lim > 0, dist / np.where(lim > 0, lim, 1.0), 0.0)))
    line = f"random features {dtype} hints={hints}: worst distance / bound {worst:.4f}, {int(beyond.sum())} of {got.size} beyond"
    if dtype == "bfloat16":
        plain = FR.bound(c.f2, c.f3, c.hints if hints else None, c.valid if hints else None, False)[1] + 2.0 ** -9 * np.abs(c64)
        line += f"; beyond corr_whole + 2^-9 * |value| (no bound of a correct rounding): {int((~(dist <= plain) & (got != 0)).sum())}"
    print(line)
    assert np.isfinite(got).all() and not beyond.any()


# ---- 6. non-finite features -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_nonfinite_features_spoil_their_row_or_column_and_nothing_else(eng, dtype):
    f2, f3, bad = FR.nonfinite_case()
    c = FR.case(FR.RANDOM_SHAPE)
    # bfloat16 holds NaN and the infinities: the upload checks the low 16 bits only
    f2, f3 = (np.where(np.isnan(f), np.uint32(0x7FC00000).view(F32), f).astype(F32) for f in (f2, f3))
    pyr = eng.raft_corr_fused(_feat(eng, f2, dtype), _feat(eng, f3, dtype), None, None, 4)
    marks = FR.pooled_any(bad, 4)
    for i in range(4):
        got = CR.widened([_host(pyr[i])])[0]
        assert np.array_equal(~np.isfinite(got), marks[i]), (dtype, i)


# ---- 7. levels --------------------------------------------------------------------------------------------------
def _raw(eng, c, dtype, levels, hints=False):
    """The C entry with guard cells around corr (a row on each side) and behind pyr -> (levels as host arrays, guards
    intact)."""
    import torch
    from vppstereo_amd import _lib
    bf = dtype == "bfloat16"
    f2, f3 = _maps(eng, c, dtype)
    off = (C.c_int64 * 4)()
    cells = int(eng.lib.vppx_raft_corr_pyramid_cells(c.N, c.W3, levels, off))
    assert cells >= 0
    pat, it = (S16, torch.int16) if bf else (S32, torch.int32)
    corr = torch.full(((c.N + 2) * c.W3,), pat, dtype=it, device=eng.device)
    buf = torch.full((cells + GUARD,), pat, dtype=it, device=eng.device)
    h, v = (_dev(eng, c.hints), _dev(eng, c.valid)) if hints else (None, None)
    eng._bind_stream()
    _lib.check(eng.lib.vppx_raft_corr_fused_dt_dev(eng.ctx.handle, f2.data_ptr(), f3.data_ptr(), h.data_ptr() if hints else None,
                                                   v.data_ptr() if hints else None, c.B, c.D, c.H4, c.W2, c.W3, c.H if hints else 0,
                                                   c.W if hints else 0, levels, corr.data_ptr() + c.W3 * corr.element_size(),
                                                   buf.data_ptr() if levels > 1 else None, _lib.DT_BF16 if bf else _lib.DT_F32))
    torch.cuda.synchronize()
    view = (lambda a: a.view(np.uint16)) if bf else (lambda a: a.view(F32))
    rc, rb = corr.cpu().numpy(), buf.cpu().numpy()
    word = np.uint16 if bf else np.uint32
    guards = (rc[:c.W3].view(word) == pat).all() and (rc[(c.N + 1) * c.W3:].view(word) == pat).all() and (rb[cells:].view(word) == pat).all()
    out = [view(rc[c.W3:(c.N + 1) * c.W3]).reshape(c.N, c.W3)]
    out += [view(rb[off[i]:off[i] + c.N * (c.W3 >> i)]).reshape(c.N, c.W3 >> i) for i in range(1, levels)]
    return out, bool(guards)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fewer_levels_write_nothing_beyond_them(eng, dtype):
    c = FR.case(FR.LEVELS_SHAPE)
    level0 = FR.exact_level0(c.f2, c.f3)
    want = CR.pyramid(level0 if dtype == "float32" else FR.bf16_round(level0), 4)
    for levels in (1, 2, 3, 4):
        got, guards = _raw(eng, c, dtype, levels)
        assert guards, (dtype, levels)
        assert len(got) == levels
        for i in range(levels):
            assert _same(got[i], want[i]), (dtype, levels, i)
    got, guards = _raw(eng, c, dtype, 3, hints=True)
    assert guards


# ---- 8. refusals: before anything is launched, with no output byte touched ---------------------------------------
def test_refusals_leave_every_byte_alone(eng):
    import torch
    from vppstereo_amd._lib import VppxError
    lib, ctx = eng.lib, eng.ctx.handle
    inp = torch.full((4096,), 1.0, dtype=torch.float32, device=eng.device)
    out = torch.full((4096,), S32, dtype=torch.int32, device=eng.device)
    pyr = torch.full((4096,), S32, dtype=torch.int32, device=eng.device)
    p, o, q = inp.data_ptr(), out.data_ptr(), pyr.data_ptr()
    eng._bind_stream()
    INVALID, UNSUPPORTED = -1, -10

    def fused(f2=p, f3=p, hints=None, valid=None, B=1, D=3, H4=2, W2=2, W3=16, H=8, W=8, levels=4, corr=o, pyr_=q, dtype=0):
        return lib.vppx_raft_corr_fused_dt_dev(ctx, f2, f3, hints, valid, B, D, H4, W2, W3, H, W, levels, corr, pyr_, dtype)

    for rc, code in (
            (fused(f2=None), INVALID), (fused(f3=None), INVALID), (fused(corr=None), INVALID), (fused(pyr_=None), INVALID),
            (fused(hints=p, valid=None), INVALID), (fused(B=0), INVALID), (fused(D=0), INVALID), (fused(D=-4), INVALID),
            (fused(H4=0), INVALID), (fused(W2=-1), INVALID), (fused(W3=0), INVALID), (fused(levels=0), INVALID),
            (fused(W3=15), INVALID), (fused(W3=3, levels=2), INVALID), (fused(W3=1, levels=1), INVALID),
            (fused(dtype=2), INVALID), (fused(dtype=-1), INVALID), (fused(levels=5, W3=64), UNSUPPORTED)):
        assert rc == code, (rc, code, lib.vppx_last_error().decode())
        assert lib.vppx_last_error()
    assert fused(f2=None) == INVALID and lib.vppx_last_error().decode() == "vppx_raft_corr_fused: bad arguments"
    assert fused(B=0) == INVALID and lib.vppx_last_error().decode() == "vppx_raft_corr_fused: bad arguments"
    assert fused(dtype=2) == INVALID
    assert lib.vppx_last_error().decode() == "vppx_raft_corr_fused: dtype 2 is neither VPPX_DT_F32 (0) nor VPPX_DT_BF16 (1)"
    assert fused(levels=5, W3=64) == UNSUPPORTED
    assert lib.vppx_last_error().decode() == "vppx_raft_corr_fused: 5 levels of radius 0, at most 4 levels and radius 8 are built"
    assert fused(W3=15) == INVALID and lib.vppx_last_error().decode().startswith("vppx_raft_corr_fused: level 3 of a 15-wide row has 1 cells")
    # with hints: the modulation call's check of H / 4 and W / 4, and its message
    assert fused(hints=p, valid=p, H=12, W=8) == INVALID
    assert lib.vppx_last_error().decode() == "hints are 12x8: sub-sampled by 4 that is 3x2, but the features are 2x2"
    assert fused(hints=p, valid=p, H=8, W=13, dtype=1) == INVALID
    assert lib.vppx_last_error().decode() == "hints are 8x13: sub-sampled by 4 that is 2x3, but the features are 2x2"
    assert lib.vppx_raft_corr_fused_dt_dev(None, p, p, None, None, 1, 3, 2, 2, 16, 8, 8, 4, o, q, 0) == -7
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == S32).all() and (pyr.cpu().numpy() == S32).all() and (inp.cpu().numpy() == 1.0).all()
    # what is allowed: one level without a buffer
    assert fused(levels=1, pyr_=None, W3=2) == 0
    torch.cuda.synchronize()
    assert (inp.cpu().numpy() == 1.0).all() and (out.cpu().numpy()[8:] == S32).all() and (pyr.cpu().numpy() == S32).all()

    # through Engine
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=eng.device)            # noqa: E731
    with pytest.raises(ValueError, match="same dtype"):
        eng.raft_corr_fused(f32(1, 3, 2, 16), f32(1, 3, 2, 16).bfloat16())
    with pytest.raises(ValueError, match=r"fmap2 / fmap3 must be"):
        eng.raft_corr_fused(f32(1, 3, 2, 16), f32(1, 4, 2, 16))
    with pytest.raises(ValueError, match="fmap2: expected contiguous"):
        eng.raft_corr_fused(f32(1, 3, 2, 16).double(), f32(1, 3, 2, 16))
    with pytest.raises(ValueError, match=r"hints / validhints must be"):
        eng.raft_corr_fused(f32(1, 3, 2, 16), f32(1, 3, 2, 16), f32(1, 1, 8, 64), f32(1, 1, 8, 65))
    with pytest.raises(VppxError) as e:
        eng.raft_corr_fused(f32(1, 3, 2, 16), f32(1, 3, 2, 64), num_levels=5)
    assert e.value.code == UNSUPPORTED
    with pytest.raises(VppxError) as e:
        eng.raft_corr_fused(f32(1, 3, 2, 16), f32(1, 3, 2, 15))
    assert e.value.code == INVALID


# ---- 9. the drop-in on the reference's own arrays -----------------------------------------------------------------
@pytest.mark.parametrize("t", FR.GOLDEN_TAGS)
def test_drop_in_blocks_on_the_golden_arrays(eng, t):
    import torch
    from test_gpu_corr import _carried_bound
    from vppstereo_amd.corr import CorrBlock1D, CorrBlock1DFused
    c = FR.golden_case(t)
    f2, f3, coords, h, v = (_dev(eng, a) for a in (c.f2, c.f3, c.coords, c.hints, c.valid))
    B, H4, W2, W3, N = c.B, c.H4, c.W2, c.W3, c.N
    ref = R.raft_modulate(c.g("plain_level0").reshape(B, H4, W2, 1, W3), c.hints, c.valid, rule="library")
    plain_rows = (ref.v.reshape(N, W3) == 0).all(axis=1)              # every level-0 tap of such a pixel is un-modulated
    mask = np.broadcast_to(plain_rows.reshape(B, 1, H4, W2), (B, 36, H4, W2))
    assert plain_rows.any() and not plain_rows.all()
    truth, bound = _carried_bound(ref, N, W3, c.coords[:, 0], 4, 4)
    truth, bound = CR.channels_first(truth, B, H4, W2), CR.channels_first(bound, B, H4, W2)
    for make in (lambda *a: CorrBlock1DFused(*a, num_levels=4, radius=4), lambda *a: CorrBlock1D(*a, num_levels=4, radius=4, fused=True)):
        blk = make(f2, f3)
        assert len(blk.corr_pyramid) == 4 and (blk.num_levels, blk.radius) == (4, 4)
        got = blk(coords)
        assert got.dtype == torch.float32 and got.is_contiguous() and got.shape == (B, 36, H4, W2)
        assert _same(got.cpu().numpy(), c.g("plain_lookup"))
        blk = make(f2, f3, h, v)
        assert len(blk.corr_pyramid) == 4
        got = blk(coords).cpu().numpy()
        want = c.g("hints_lookup")
        assert np.array_equal(got.view(np.uint32)[mask], want.view(np.uint32)[mask]), "cells that read un-modulated rows alone"
        dist = np.abs(got.astype(F64) - truth)
        beyond = ~(dist <= bound) & ~mask
        worst = float(np.max(np.where(~mask & (bound > 0), dist / np.where(bound > 0, bound, 1.0), 0.0)))
        print(f"fused drop-in {t}: {int((~mask).sum())} cells read modulated rows, worst distance / bound {worst:.3f}")
        assert not beyond.any()
    assert CorrBlock1DFused(f2, f3, fused=False).corr_pyramid[0].data_ptr() != 0
    with pytest.raises(TypeError):
        CorrBlock1D(f2, f3, None, None, 4, 4, True)                  # keyword-only
    # the default block is today's: torch's GEMM and division, then the pyramid and the lookup
    for args in ((), (h, v)):
        blk = CorrBlock1D(f2, f3, *args, num_levels=4, radius=4)
        pyr = eng.raft_corr_pyramid(eng.raft_corr(f2, f3), *(args or (None, None)), 4)
        own = CorrBlock1D.corr(f2, f3)
        assert _same(_host(own.view(N, 1, 1, W3)), _host(eng.raft_corr(f2, f3).view(N, 1, 1, W3)))
        for i in range(4):
            assert _same(_host(blk.corr_pyramid[i]), _host(pyr[i]))
        assert _same(blk(coords).cpu().numpy(), eng.raft_corr_lookup(pyr, coords, 4).cpu().numpy())


# ---- 10. one context --------------------------------------------------------------------------------------------
def test_one_context_serves_the_fused_call_among_others(eng):
    """raft_corr_fused (float32, hints), a small vpp_rsgm call, raft_corr_fused at another shape in bfloat16 (hints again:
    the scratch of the sub-sampled hints is the other hand-off calls'), and a lookup, in that order on one Engine: each
    result is bit for bit that of the same call on a fresh Engine."""
    import torch
    import synth
    from vppstereo_amd.engine import Engine
    ca, cb = FR.case(FR.DIRECTED_SHAPES[0]), FR.case(FR.DIRECTED_SHAPES[1])
    b = synth.make_batch(2, 60, 112, 64, 0.04, seed=7)
    coords = np.random.default_rng(77).uniform(-3, cb.W3 + 3, (cb.B, cb.H4, cb.W2)).astype(F32)

    def second_pyramid(e):
        return e.raft_corr_fused(_feat(e, cb.f2, "bfloat16"), _feat(e, cb.f3, "bfloat16"), _dev(e, cb.hints), _dev(e, cb.valid), 3)

    steps = [
        lambda e: [_host(p) for p in e.raft_corr_fused(_dev(e, ca.f2), _dev(e, ca.f3), _dev(e, ca.hints), _dev(e, ca.valid), 4)],
        lambda e: [e.vpp_rsgm(_dev(e, b["left"]), _dev(e, b["right"]), _dev(e, b["hints"]), seed=3, rsgm_kw=dict(dmax=64)).cpu().numpy()],
        lambda e: [_host(p) for p in second_pyramid(e)],
        lambda e: [e.raft_corr_lookup(second_pyramid(e), _dev(e, coords), 2).cpu().numpy()],
    ]
    one = [step(eng) for step in steps]
    for k, step in enumerate(steps):
        want = step(Engine())
        assert len(want) == len(one[k]) > 0
        for g, w in zip(one[k], want):
            assert _same(g, w), k
    torch.cuda.synchronize()
