"""The correlation pyramid and lookup kernels (corr_kernels.hip) against the numpy referee of tests/_corr_ref.py, bit
for bit, in float32 and bfloat16; the refusals of the two C entries; vppstereo_amd.corr.CorrBlock1D on the arrays the
reference's own CorrBlock1D produced.  What each input reaches is asserted on the CPU in tests/test_corr_ref_cpu.py,
on these very arrays.

Level 0 under hints is held to what vppx_raft_corr_modulate_dt_dev leaves on a copy of the same input, byte for byte:
that kernel is held to the float64 referee in tests/test_gpu_handoff_ref.py, and no tolerance is restated here."""
import ctypes as C
import os

import numpy as np
import pytest

import _corr_ref as CR
import _handoff_bf16_ref as BR
import _handoff_ref as R
from _cells import DTYPES, GUARD, SENTINEL16 as S16, SENTINEL32 as S32

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
_CASES = {}


def _case(shape, hints, nan_cell=False):
    key = (shape, hints, nan_cell)
    if key not in _CASES:
        _CASES[key] = CR.volume_case(shape, hints=hints, nan_cell=nan_cell)
    return _CASES[key]


@pytest.fixture(scope="module")
def eng():
    import torch
    from vppstereo_amd.engine import Engine
    assert torch.cuda.is_available()
    return Engine()


def _dev(eng, a):
    import torch
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(eng.device)


def _cells(eng, level0, dtype):
    """[N, W3] float32 values -> (device tensor of the storage type, its cells as the referee holds them: float32
    values or bf16 bits)."""
    import torch
    if dtype == "float32":
        host = np.ascontiguousarray(level0, F32)
        return _dev(eng, host), host
    host = BR.bits(BR.bf16_rne_f32(level0))
    return _dev(eng, host.view(np.int16)).view(torch.bfloat16), host


def _host(t):
    """A device tensor's cells as the referee holds them."""
    import torch
    if t.dtype == torch.bfloat16:
        return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == F32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    return a.shape == b.shape and np.array_equal(a, b)


def _same_or_nan(a, b):
    """_same, with two NaN cells counted as equal whatever their payload."""
    wa, wb = CR.widened([np.ascontiguousarray(a)])[0], CR.widened([np.ascontiguousarray(b)])[0]
    return wa.shape == wb.shape and CR.same_bits(wa, wb) == 0


def _offsets(eng, N, W3, levels):
    off = (C.c_int64 * 4)()
    cells = eng.lib.vppx_raft_corr_pyramid_cells(N, W3, levels, off)
    assert cells >= 0
    return int(cells), list(off)[:levels]


def _pyramid(eng, corr, c, levels, with_hints):
    """The C entry on `corr` (device, modified in place under hints) -> (pooled levels 1.. as host arrays, the buffer's
    guard cells intact)."""
    import torch
    from vppstereo_amd import _lib
    bf = corr.dtype == torch.bfloat16
    cells, off = _offsets(eng, c.N, c.W3, levels)
    buf = torch.full((cells + GUARD,), S16 if bf else S32, dtype=torch.int16 if bf else torch.int32, device=eng.device)
    h, v = (_dev(eng, c.hints), _dev(eng, c.valid)) if with_hints else (None, None)
    eng._bind_stream()
    _lib.check(eng.lib.vppx_raft_corr_pyramid_dt_dev(eng.ctx.handle, corr.data_ptr(), h.data_ptr() if with_hints else None,
                                                     v.data_ptr() if with_hints else None, c.B, c.H4, c.W2, c.W3, c.H, c.W, levels,
                                                     buf.data_ptr() if levels > 1 else None, _lib.DT_BF16 if bf else _lib.DT_F32))
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    raw = raw.view(np.uint16) if bf else raw.view(F32)
    out = [raw[off[i]:off[i] + c.N * (c.W3 >> i)].reshape(c.N, c.W3 >> i) for i in range(1, levels)]
    guard = raw[cells:].view(np.uint16 if bf else np.uint32)
    return out, bool((guard == (S16 if bf else S32)).all())


# ---- pyramid ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", CR.PYRAMID_SHAPES, ids=CR.tag)
def test_pyramid_without_hints_equals_the_referee_and_leaves_corr_alone(eng, shape, dtype):
    c = _case(shape, False)
    corr, host = _cells(eng, c.corr.reshape(c.N, c.W3), dtype)
    for levels in (4, 1, 2, 3) if shape == (1, 2, 3, 129) else (4,):
        got, guard = _pyramid(eng, corr, c, levels, False)
        assert guard and _same(_host(corr), host)
        want = CR.pyramid(host, levels)
        assert len(got) == levels - 1
        for i in range(1, levels):
            assert _same(got[i - 1], want[i]), (shape, dtype, levels, i)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", CR.PYRAMID_SHAPES, ids=CR.tag)
def test_pyramid_with_hints_modulates_like_the_modulation_call_and_pools_what_it_wrote(eng, shape, dtype):
    c = _case(shape, True)
    corr, host = _cells(eng, c.corr.reshape(c.N, c.W3), dtype)
    alone = corr.clone()
    got, guard = _pyramid(eng, corr, c, 4, True)
    eng.raft_corr_modulate_(alone.view(c.B, c.H4, c.W2, 1, c.W3), _dev(eng, c.hints), _dev(eng, c.valid))
    level0 = _host(corr)
    assert guard and _same(level0, _host(alone)), "level 0 is not what the modulation call leaves"
    rows0 = c.v4.reshape(-1) == 0
    assert _same(level0[rows0], host[rows0])
    if (~rows0).any():
        assert not _same(level0[~rows0], host[~rows0])
    want = CR.pyramid(level0, 4)
    for i in range(1, 4):
        assert _same(got[i - 1], want[i]), (shape, dtype, i)
    if rows0.any():         # rows with v == 0 are not modulated and are pooled all the same
        assert all(np.any(CR.widened([got[i]])[0][rows0] != 0) for i in range(3))
    wide = CR.widened([level0])[0]
    neg0 = (wide == 0) & np.signbit(wide)
    w = c.W3 // 2
    pair = neg0[:, 0:2 * w:2] & neg0[:, 1:2 * w:2]
    assert pair.any() and (got[0][pair] == 0).all() and not np.signbit(CR.widened([got[0]])[0][pair]).any(), "-0 and -0 pool to +0"
    # the same through Engine: entry 0 is corr itself, the others are views into one buffer
    corr2, _ = _cells(eng, c.corr.reshape(c.N, c.W3), dtype)
    corr2 = corr2.view(c.B, c.H4, c.W2, 1, c.W3)
    pyr = eng.raft_corr_pyramid(corr2, _dev(eng, c.hints), _dev(eng, c.valid), 4)
    assert len(pyr) == 4 and pyr[0].data_ptr() == corr2.data_ptr() and pyr[0].shape == (c.N, 1, 1, c.W3)
    assert pyr[2].data_ptr() == pyr[1].data_ptr() + c.N * (c.W3 >> 1) * corr2.element_size()
    for i in range(4):
        assert pyr[i].shape == (c.N, 1, 1, c.W3 >> i) and _same(_host(pyr[i]).reshape(c.N, -1), want[i])


# ---- lookup ----------------------------------------------------------------------------------------------------
def _lookup_case(eng, shape, dtype, levels):
    """The library's own pyramid of the case with hints (the NaN cell planted where the case has one), on the device and
    downloaded."""
    c = _case(shape, True, shape == CR.NAN_SHAPE)
    corr, _ = _cells(eng, c.corr.reshape(c.N, c.W3), dtype)
    pyr = eng.raft_corr_pyramid(corr.view(c.B, c.H4, c.W2, 1, c.W3), _dev(eng, c.hints), _dev(eng, c.valid), levels)
    host = [_host(p).reshape(c.N, -1) for p in pyr]
    return c, pyr, host


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("levels,radius", CR.LOOKUP_PARAMS)
@pytest.mark.parametrize("shape", CR.LOOKUP_SHAPES, ids=CR.tag)
def test_lookup_equals_the_referee_bit_for_bit(eng, shape, levels, radius, dtype):
    import torch
    c, pyr, host = _lookup_case(eng, shape, dtype, levels)
    for want, have in zip(CR.pyramid(host[0], levels), host):
        assert _same_or_nan(want, have)
    sheets = CR.coords_case(shape)
    S, taps = len(sheets), 2 * radius + 1
    bare = _dev(eng, sheets)
    two = torch.full((S, c.B, 2, c.H4, c.W2), float("nan"), dtype=torch.float32, device=eng.device)
    two[:, :, 0] = bare
    out = torch.full((2, S, c.B, levels * taps, c.H4, c.W2), float("nan"), dtype=torch.float32, device=eng.device)
    for s in range(S):
        eng.raft_corr_lookup(pyr, bare[s], radius, out=out[0, s])
        eng.raft_corr_lookup(pyr, two[s], radius, out=out[1, s])
    got = out.cpu().numpy()
    assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32)), "channel 1 of the coordinates was read"
    wide = CR.widened(host)
    bad = 0
    for s in range(S):
        want = CR.channels_first(CR.lookup(wide, sheets[s], radius), c.B, c.H4, c.W2)
        bad += CR.same_bits(got[0, s], want)
    print(f"lookup {CR.tag(shape)} L{levels} r{radius} {dtype}: {S} sheets, {got[0].size} cells, {bad} differ")
    assert bad == 0
    if shape == CR.NAN_SHAPE:     # pixel 0 of sheet 0 reads the NaN cell as its right tap under a weight of exactly zero
        assert sheets[0].reshape(-1)[0] == CR.NAN_AT["cell"] - 1 and np.isnan(wide[0][0, CR.NAN_AT["cell"]])
        assert np.isnan(got[0, 0, 0, radius, 0, 0])
    fresh = eng.raft_corr_lookup(pyr, bare[0], radius)
    assert fresh.shape == (c.B, levels * taps, c.H4, c.W2) and np.array_equal(fresh.cpu().numpy().view(np.uint32), got[0, 0].view(np.uint32))


# ---- refusals: before anything is launched, with no output byte touched ----------------------------------------
def test_refusals_leave_every_byte_alone(eng):
    import torch
    from vppstereo_amd._lib import VppxError
    lib, ctx = eng.lib, eng.ctx.handle
    inp = torch.full((4096,), 1.0, dtype=torch.float32, device=eng.device)
    out = torch.full((4096,), S32, dtype=torch.int32, device=eng.device)
    p, o = inp.data_ptr(), out.data_ptr()
    eng._bind_stream()
    INVALID, UNSUPPORTED = -1, -10

    def pyramid(corr=p, hints=None, valid=None, B=1, H4=2, W2=2, W3=16, H=8, W=8, levels=4, pyr=o, dtype=0):
        return lib.vppx_raft_corr_pyramid_dt_dev(ctx, corr, hints, valid, B, H4, W2, W3, H, W, levels, pyr, dtype)

    def lookup(corr=p, pyr=p, coords=p, stride=4, B=1, H4=2, W2=2, W3=16, levels=4, radius=4, out_=o, dtype=0):
        return lib.vppx_raft_corr_lookup_dt_dev(ctx, corr, pyr, coords, stride, B, H4, W2, W3, levels, radius, out_, dtype)

    for rc, code in (
            (pyramid(corr=None), INVALID), (pyramid(pyr=None), INVALID), (pyramid(hints=p, valid=None), INVALID),
            (pyramid(B=0), INVALID), (pyramid(H4=0), INVALID), (pyramid(W2=-1), INVALID), (pyramid(W3=0), INVALID),
            (pyramid(levels=0), INVALID), (pyramid(dtype=2), INVALID), (pyramid(dtype=-1), INVALID),
            (pyramid(W3=15), INVALID), (pyramid(W3=3, levels=2), INVALID), (pyramid(W3=1, levels=1), INVALID),
            (pyramid(levels=5, W3=64), UNSUPPORTED),
            (lookup(corr=None), INVALID), (lookup(pyr=None), INVALID), (lookup(coords=None), INVALID), (lookup(out_=None), INVALID),
            (lookup(B=0), INVALID), (lookup(H4=0), INVALID), (lookup(W2=0), INVALID), (lookup(W3=-3), INVALID),
            (lookup(levels=0), INVALID), (lookup(radius=-1), INVALID), (lookup(dtype=2), INVALID), (lookup(stride=3), INVALID),
            (lookup(W3=15), INVALID), (lookup(W3=1, levels=1, pyr=None), INVALID),
            (lookup(levels=5, W3=64), UNSUPPORTED), (lookup(radius=9), UNSUPPORTED)):
        assert rc == code, (rc, code, lib.vppx_last_error().decode())
        assert lib.vppx_last_error()
    assert pyramid(dtype=2) == INVALID
    assert lib.vppx_last_error().decode() == "vppx_raft_corr_pyramid: dtype 2 is neither VPPX_DT_F32 (0) nor VPPX_DT_BF16 (1)"
    # with hints: the modulation call's check of H / 4 and W / 4, and its message
    assert pyramid(hints=p, valid=p, H=12, W=8) == INVALID
    assert lib.vppx_last_error().decode() == "hints are 12x8: sub-sampled by 4 that is 3x2, but the features are 2x2"
    assert pyramid(hints=p, valid=p, H=8, W=13, dtype=1) == INVALID
    assert lib.vppx_last_error().decode() == "hints are 8x13: sub-sampled by 4 that is 2x3, but the features are 2x2"
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == S32).all() and (inp.cpu().numpy() == 1.0).all()
    # what is allowed: one level without a buffer
    assert pyramid(levels=1, pyr=None, W3=2) == 0 and lookup(levels=1, pyr=None, W3=2, radius=0) == 0
    torch.cuda.synchronize()
    assert (inp.cpu().numpy() == 1.0).all() and (out.cpu().numpy()[4:] == S32).all()

    # through Engine
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=eng.device)            # noqa: E731
    corr = f32(1, 2, 2, 1, 16)
    with pytest.raises(ValueError, match="corr must be"):
        eng.raft_corr_pyramid(f32(1, 2, 2, 2, 16))
    with pytest.raises(VppxError) as e:
        eng.raft_corr_pyramid(corr, num_levels=5)
    assert e.value.code == UNSUPPORTED
    with pytest.raises(VppxError) as e:
        eng.raft_corr_pyramid(f32(1, 2, 2, 1, 15))
    assert e.value.code == INVALID
    pyr = eng.raft_corr_pyramid(corr)
    with pytest.raises(ValueError, match="coords must be"):
        eng.raft_corr_lookup(pyr, f32(1, 3, 2, 2))
    with pytest.raises(ValueError, match="the pyramid has 4 rows"):
        eng.raft_corr_lookup(pyr, f32(1, 3, 2))
    with pytest.raises(ValueError, match="coords: expected contiguous"):
        eng.raft_corr_lookup(pyr, f32(1, 2, 2).double())
    with pytest.raises(ValueError, match="views raft_corr_pyramid returned"):
        eng.raft_corr_lookup([pyr[0], pyr[1], pyr[2].clone(), pyr[3]], f32(1, 2, 2))
    with pytest.raises(VppxError) as e:
        eng.raft_corr_lookup(pyr, f32(1, 2, 2), radius=9)
    assert e.value.code == UNSUPPORTED


DEVICE_EXP_ULPS = 1.0           # tests/test_gpu_handoff_ref.py's figure, justified there


# ---- the drop-in on the reference's own arrays --------------------------------------------------------------------
def _carried_bound(ref, N, W3, coords, levels, radius, extra0=None):
    """-> (truth, bound) [N, levels * taps] float64.  `truth` is the lookup in float64 of the float64 referee's level 0
    (ref.out64), with the positions and weights the float32 steps give (they depend on the coordinate alone).  `bound`
    is how far a float32 implementation may be from it whose level 0 is within R.limit() of ref.out64:
      pooling   E_i[k] = (E_{i-1}[2k] + E_{i-1}[2k+1]) / 2  +  U * (|Q_i[k]| + that)       one rounding, of the sum
      tap sum   wl * E[a] + wr * E[b]                          the convex combination
                + U * wl * (|Qa| + Ea)                         the rounding of a * wl
                + U * (wl * (|Qa| + Ea) + wr * (|Qb| + Eb))    the rounding of the fma
    times 1 + 2^-10 for the second-order terms, plus 2^-148 per rounding that may land in the subnormal range (the
    halving is exact above it).  `extra0` [N, W3] is a further distance at level 0 that the caller accounts for; nothing
    else is added."""
    U = R.U
    Q = [ref.out64.reshape(N, W3)]
    E = [R.limit(ref, DEVICE_EXP_ULPS).reshape(N, W3) * (ref.v.reshape(N, W3) != 0)]
    if extra0 is not None:
        E[0] = E[0] + extra0
    for i in range(1, levels):
        w = Q[-1].shape[1] // 2
        q = (Q[-1][:, 0:2 * w:2] + Q[-1][:, 1:2 * w:2]) / 2
        e = (E[-1][:, 0:2 * w:2] + E[-1][:, 1:2 * w:2]) / 2
        Q.append(q)
        E.append(e + U * (np.abs(q) + e) * (1 + 2.0 ** -10) + 2.0 ** -148)
    c = np.ascontiguousarray(coords, F32).reshape(-1)
    t = np.arange(-radius, radius + 1).astype(F32)[None, :]
    truth, bound = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(levels):
            W = Q[i].shape[1]
            wm1 = F32(W - 1)
            x = t + (c / F32(2 ** i))[:, None]
            ix = (((F32(2) * x) / wm1 - F32(1) + F32(1)) / F32(2)) * wm1
            fl = np.floor(ix)
            fl1 = fl + F32(1)
            wr, wl = (ix - fl).astype(F64), (fl1 - ix).astype(F64)
            in_a, in_b = (fl >= 0) & (fl <= wm1), (fl1 >= 0) & (fl1 <= wm1)
            ia, ib = np.where(in_a, fl, 0).astype(np.int64), np.where(in_b, fl1, 0).astype(np.int64)
            qa, ea = (np.where(in_a, np.take_along_axis(z, ia, 1), 0.0) for z in (Q[i], E[i]))
            qb, eb = (np.where(in_b, np.take_along_axis(z, ib, 1), 0.0) for z in (Q[i], E[i]))
            live = (in_a | in_b) & np.isfinite(ix)
            ma, mb = wl * (np.abs(qa) + ea), wr * (np.abs(qb) + eb)
            truth.append(np.where(live, wl * qa + wr * qb, 0.0))
            bound.append(np.where(live, wl * ea + wr * eb + (U * ma + U * (ma + mb)) * (1 + 2.0 ** -10) + 2 * 2.0 ** -148, 0.0))
    return np.concatenate(truth, axis=1), np.concatenate(bound, axis=1)


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_drop_in_block_on_the_golden_arrays(eng, tag):
    """The golden arrays were recorded on a CPU.  Level 0 before the modulation is a GEMM, exact on these features in any
    order, divided by sqrt(D), and that division is torch's: on the device torch divides by a host scalar by multiplying
    with its reciprocal, so the block's own level 0 is the recording's bit for bit only where sqrt(D) is a power of two
    (D = 4, case b) and up to three roundings away otherwise; the reference run on the device does the same.  So the
    bit-for-bit half of the check is made where its premise holds: the pyramid and the lookup are run on the recorded
    level 0 for every case (path A), and the block itself (path B) is held bit for bit to path A on its own level 0, to
    the recording bit for bit where the division is exact, and to the carried bound, widened by those three roundings
    and nothing else, where it is not."""
    import torch
    from vppstereo_amd.corr import CorrBlock1D
    g = np.load(os.path.join(HERE, "golden", "corr_cases.npz"))
    f2, f3, coords = (_dev(eng, g[f"{tag}_{k}"]) for k in ("f2", "f3", "coords"))
    hints, valid = g[f"{tag}_hints"], g[f"{tag}_valid"]
    h, v = _dev(eng, hints), _dev(eng, valid)
    B, _, H4, W2 = coords.shape
    N, W3, D = B * H4 * W2, f3.shape[3], f2.shape[1]
    plain0 = g[f"{tag}_plain_level0"]
    ref = R.raft_modulate(plain0.reshape(B, H4, W2, 1, W3), hints, valid, rule="library")
    plain_rows = (ref.v.reshape(N, W3) == 0).all(axis=1)              # every level-0 tap of such a pixel is un-modulated
    mask = np.broadcast_to(plain_rows.reshape(B, 1, H4, W2), (B, 36, H4, W2))
    assert plain_rows.any() and not plain_rows.all()
    truth, bound = _carried_bound(ref, N, W3, g[f"{tag}_coords"][:, 0], 4, 4)
    truth, bound = CR.channels_first(truth, B, H4, W2), CR.channels_first(bound, B, H4, W2)

    def run(level0, with_hints):
        pyr = eng.raft_corr_pyramid(level0.clone().view(B, H4, W2, 1, W3), h if with_hints else None, v if with_hints else None, 4)
        return pyr, eng.raft_corr_lookup(pyr, coords, 4).cpu().numpy()

    def held(got, want, truth, bound, what):
        """Cells that read un-modulated rows alone: the recording's bits.  The rest: within the carried bound."""
        assert np.array_equal(got.view(np.uint32)[mask], want.view(np.uint32)[mask]), what
        dist = np.abs(got.astype(F64) - truth)
        beyond = ~(dist <= bound) & ~mask
        worst = float(np.max(np.where(~mask & (bound > 0), dist / np.where(bound > 0, bound, 1.0), 0.0)))
        print(f"drop-in {tag} {what}: {int((~mask).sum())} cells read modulated rows, worst distance / bound {worst:.3f}, "
              f"{int(beyond.sum())} beyond")
        assert not beyond.any(), what

    # path A: the recorded level 0
    pyr, out = run(_dev(eng, plain0), False)
    for i in range(4):
        assert _same(_host(pyr[i]).reshape(N, -1), g[f"{tag}_plain_level{i}"]), (tag, i)
    assert _same(out, g[f"{tag}_plain_lookup"])
    pyr, out_a = run(_dev(eng, plain0), True)
    held(out_a, g[f"{tag}_hints_lookup"], truth, bound, "recorded level 0")
    # the reference's own lookup obeys the same bound (its exp is the host's)
    assert not (~(np.abs(g[f"{tag}_hints_lookup"].astype(F64) - truth) <= bound) & ~mask).any()

    # path B: the block
    own = CorrBlock1D.corr(f2, f3)
    assert own.shape == (B, H4, W2, 1, W3)
    exact = D in (1, 4, 16)
    assert _same(own.cpu().numpy().reshape(N, W3), plain0) == exact, "torch divides by sqrt(D) differently than assumed"
    for with_hints in (False, True):
        blk = CorrBlock1D(f2, f3, *((h, v) if with_hints else ()), num_levels=4, radius=4)
        assert len(blk.corr_pyramid) == 4 and (blk.num_levels, blk.radius) == (4, 4)
        got = blk(coords)
        assert got.dtype == torch.float32 and got.is_contiguous() and got.shape == (B, 36, H4, W2)
        got = got.cpu().numpy()
        pyr, same = run(own.reshape(N, W3), with_hints)
        assert _same(got, same), "the block is not the pyramid and lookup of its own level 0"
        for i in range(4):
            assert _same(_host(blk.corr_pyramid[i]), _host(pyr[i]))
        want = g[f"{tag}_{'hints' if with_hints else 'plain'}_lookup"]
        if exact:
            assert _same(got, out_a if with_hints else g[f"{tag}_plain_lookup"])
        else:
            # a * fl(1 / s) against fl(a / s): the reciprocal, the product and the recording's own quotient, one rounding each
            r = ref if with_hints else R.raft_modulate(plain0.reshape(B, H4, W2, 1, W3), hints, np.zeros_like(valid), rule="library")
            extra = 3 * R.U * np.abs(r.out64.reshape(N, W3)) * (1 + 2.0 ** -10)
            t, b = _carried_bound(r, N, W3, g[f"{tag}_coords"][:, 0], 4, 4, extra0=extra)
            t, b = CR.channels_first(t, B, H4, W2), CR.channels_first(b, B, H4, W2)
            dist = np.abs(got.astype(F64) - t)
            print(f"drop-in {tag} block, hints={with_hints}: worst distance / bound "
                  f"{float(np.max(np.where(b > 0, dist / np.where(b > 0, b, 1.0), 0.0))):.3f}")
            assert (dist <= b).all()
            assert (np.abs(want.astype(F64) - t) <= b).all()
