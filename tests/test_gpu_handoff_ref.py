"""The hand-off kernels (handoff_kernels.hip: sub-sampling, PSMNet volume, RAFT modulation, both decoders; and
to_nchw_kernel) against the float64 referee of tests/_handoff_ref.py, at the shapes where they change path.

No atol.  A modulated cell is held to `R.limit(ref, DEVICE_EXP_ULPS)`: the distance to the float64 value that one
float32 implementation can reach whose expf is within DEVICE_EXP_ULPS of the true value, through the three float32
roundings behind it (derivation in the referee).  DEVICE_EXP_ULPS = 1 is the figure of HIP's math-API reference for
`expf`, QUOTED FROM MEMORY of the published table: no installed document of the toolkit states an accuracy for it, so
the figure could not be checked against a file; docs/NOTEBOOK.md has what an MI355X's `expf` measured.  Where the exp
is subnormal or underflows the bound is absolute, 2^-126 times the other terms
(a flushed result is legitimate); tests/test_handoff_ref_cpu.py asserts that the normal cells are a fifth of a case
where a row can hold as many, and all of them in the `*_all` cases.  Cells with v == 0 are compared bit for bit with the
un-modulated input, copies and decoders bit for bit throughout.  What each case reaches is asserted on the CPU in
tests/test_handoff_ref_cpu.py on these very arrays."""
import os

import numpy as np
import pytest

import _handoff_ref as R
from _cells import SENTINEL32 as SENTINEL, sentinels

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "frontend_cases.npz"))
DEVICE_EXP_ULPS = 1.0


@pytest.fixture(scope="module")
def eng():
    import torch
    from vppstereo_amd.engine import Engine
    assert torch.cuda.is_available()
    return Engine()


def _dev(eng, a):
    import torch
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(eng.device)


def _hold(got, ref, what):
    worst, beyond, changed = R.compare(got, ref, DEVICE_EXP_ULPS)
    normal, sub, zero = R.cell_classes(ref)
    print(f"{what}: {int(normal.sum())} normal / {int(sub.sum())} subnormal / {int(zero.sum())} zero exp cells, "
          f"worst {worst:g} ulp of the referee's float32 cell")
    assert changed == 0, f"{what}: {changed} cells with v == 0 are not the input's bits"
    assert beyond == 0, f"{what}: {beyond} cells beyond the limit"
    return worst


# ---- RAFT modulation --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.RAFT_CASES))
def test_raft_modulation_equals_the_referee(eng, name):
    c = R.raft_case(name)
    ref = R.raft_modulate(c.corr, c.hints, c.valid, rule="library")
    got = eng.raft_corr_modulate_(_dev(eng, c.corr), _dev(eng, c.hints), _dev(eng, c.valid)).cpu().numpy()
    _hold(got, ref, f"raft {name}")
    if not (c.v4 != 0).any():
        assert np.array_equal(got.view(np.uint32), c.corr.view(np.uint32))


def test_raft_frames_of_a_batch_equal_one_frame_calls(eng):
    c = R.raft_case("w130")
    both = eng.raft_corr_modulate_(_dev(eng, c.corr), _dev(eng, c.hints), _dev(eng, c.valid)).cpu().numpy()
    for f in range(c.B):
        one = eng.raft_corr_modulate_(_dev(eng, c.corr[f:f + 1]), _dev(eng, c.hints[f:f + 1]), _dev(eng, c.valid[f:f + 1])).cpu().numpy()
        assert np.array_equal(one.view(np.uint32), both[f:f + 1].view(np.uint32)), f


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_raft_golden_and_whole_corr(eng, tag):
    f2, f3, hints, valid = (G[f"raft_{tag}_{k}"] for k in ("f2", "f3", "hints", "valid"))
    ref = R.raft_modulate(G[f"raft_{tag}_pre"], hints, valid, rule="library")
    got = eng.raft_corr_modulate_(_dev(eng, G[f"raft_{tag}_pre"]), _dev(eng, hints), _dev(eng, valid)).cpu().numpy()
    _hold(got, ref, f"raft golden {tag}")
    # the whole CorrBlock1D.corr: a library GEMM in front.  A float32 dot product of Dc terms is within
    # Dc * 2^-24 * sum |a_i * b_i| of the exact one in any order of summation; / sqrt(Dc) adds its rounding, the
    # float32 sqrt's and the rounding of the cell handed to the modulation (3 * 2^-24 relative, 4 allowed)
    Dc = f2.shape[1]
    a, b = f2.astype(np.float64), f3.astype(np.float64)
    dot = np.einsum("aijk,aijh->ajkh", a, b)[:, :, :, None, :]
    mag = np.einsum("aijk,aijh->ajkh", np.abs(a), np.abs(b))[:, :, :, None, :]
    c64 = dot / np.sqrt(float(Dc))
    c_err = (Dc * R.U * mag) / np.sqrt(float(Dc)) + 4 * R.U * np.abs(c64)
    whole = R.raft_modulate(c64.astype(np.float32), hints, valid, rule="library")
    keep = whole.v == 0
    factor = np.where(keep, 1.0, np.abs(whole.mod64))
    lim = np.where(keep, 0.0, R.limit(whole, DEVICE_EXP_ULPS)) + factor * c_err * (1 + 2.0 ** -10)
    full = eng.raft_corr(_dev(eng, f2), _dev(eng, f3), _dev(eng, hints), _dev(eng, valid)).cpu().numpy()
    want = np.where(keep, c64, c64 * whole.mod64)
    miss = np.abs(full.astype(np.float64) - want) / lim
    print(f"raft_corr {tag}: worst |got - float64| / bound = {miss.max():g}")
    assert full.shape == ref.out.shape and miss.max() <= 1.0
    plain = eng.raft_corr(_dev(eng, f2), _dev(eng, f3)).cpu().numpy()
    assert (np.abs(plain.astype(np.float64) - c64) <= c_err).all()


def test_non_finite_hint_under_an_invalid_pixel_leaves_the_row_untouched(eng):
    """The documented rule (include/vppx.h): v == 0 is untouched.  The reference's arithmetic gives NaN here."""
    c = R.raft_case("w65")
    y, x = np.argwhere(c.v4[0] == 0)[0]
    c.hints[0, 0, R.nearest_indices(c.H, c.H4)[y], R.nearest_indices(c.W, c.W2)[x]] = np.inf
    got = eng.raft_corr_modulate_(_dev(eng, c.corr), _dev(eng, c.hints), _dev(eng, c.valid)).cpu().numpy()
    assert np.array_equal(got[0, y, x].view(np.uint32), c.corr[0, y, x].view(np.uint32))
    assert np.isnan(R.raft_modulate(c.corr, c.hints, c.valid, rule="reference").out[0, y, x]).all()
    _hold(got, R.raft_modulate(c.corr, c.hints, c.valid, rule="library"), "raft w65 with an inf hint")
    p = R.psm_case("w8")
    y, x = np.argwhere(p.v4[0] == 0)[0]
    p.hints[0, 0, R.nearest_indices(p.H, p.H4)[y], R.nearest_indices(p.W, p.W4)[x]] = np.nan
    got = eng.psmnet_cost_volume(_dev(eng, p.fl), _dev(eng, p.fr), p.maxdisp, _dev(eng, p.hints), _dev(eng, p.valid)).cpu().numpy()
    ref = R.psm_volume(p.fl, p.fr, p.maxdisp, p.hints, p.valid, rule="library")
    assert np.array_equal(got[0, :, :, y, x].view(np.uint32), ref.plain[0, :, :, y, x].view(np.uint32))
    assert np.isnan(R.psm_volume(p.fl, p.fr, p.maxdisp, p.hints, p.valid, rule="reference").out[0, :, :, y, x]).all()
    _hold(got, ref, "psm w8 with a NaN hint")


def test_non_finite_hint_under_a_valid_pixel_follows_the_arithmetic(eng):
    """v != 0: an infinite hint puts exp at 0 (the cells become c * (1 - v)), a NaN hint makes the pixel's cells NaN, on
    the device as in the referee; compare() holds such cells to the referee's class."""
    for bad in (np.inf, -np.inf, np.nan):
        c = R.raft_case("w65")
        y, x = np.argwhere(c.v4[0] == 1)[0]
        c.hints[0, 0, R.nearest_indices(c.H, c.H4)[y], R.nearest_indices(c.W, c.W2)[x]] = bad
        ref = R.raft_modulate(c.corr, c.hints, c.valid, rule="library")
        assert np.isnan(ref.out[0, y, x]).all() if np.isnan(bad) else (ref.out[0, y, x] == 0).all()
        got = eng.raft_corr_modulate_(_dev(eng, c.corr), _dev(eng, c.hints), _dev(eng, c.valid)).cpu().numpy()
        _hold(got, ref, f"raft w65 with a {bad} hint under v = 1")
        p = R.psm_case("w8")
        y, x = np.argwhere(p.v4[0] == 1)[0]
        p.hints[0, 0, R.nearest_indices(p.H, p.H4)[y], R.nearest_indices(p.W, p.W4)[x]] = bad
        ref = R.psm_volume(p.fl, p.fr, p.maxdisp, p.hints, p.valid, rule="library")
        assert np.isnan(ref.out[0, :, :, y, x]).any() if np.isnan(bad) else (ref.out[0, :, :, y, x] == 0).all()
        got = eng.psmnet_cost_volume(_dev(eng, p.fl), _dev(eng, p.fr), p.maxdisp, _dev(eng, p.hints), _dev(eng, p.valid)).cpu().numpy()
        _hold(got, ref, f"psm w8 with a {bad} hint under v = 1")


# ---- PSMNet volume ----------------------------------------------------------------------------------------
def _psm_through_lib(eng, c, cost_ptr, with_hints=True):
    from vppstereo_amd import _lib
    fl, fr, h, v = _dev(eng, c.fl), _dev(eng, c.fr), _dev(eng, c.hints), _dev(eng, c.valid)
    eng._bind_stream()
    _lib.check(eng.lib.vppx_psmnet_cost_volume_dev(eng.ctx.handle, fl.data_ptr(), fr.data_ptr(), h.data_ptr() if with_hints else None,
                                                   v.data_ptr() if with_hints else None, c.B, c.C, c.H4, c.W4, c.H, c.W,
                                                   c.maxdisp, cost_ptr))
    eng.torch.cuda.synchronize()


@pytest.mark.parametrize("name", list(R.PSM_CASES))
def test_psm_volume_equals_the_referee(eng, name):
    c = R.psm_case(name)
    ref = R.psm_volume(c.fl, c.fr, c.maxdisp, c.hints, c.valid, rule="library")
    got = eng.psmnet_cost_volume(_dev(eng, c.fl), _dev(eng, c.fr), c.maxdisp, _dev(eng, c.hints), _dev(eng, c.valid)).cpu().numpy()
    _hold(got, ref, f"psm {name}")
    plain = eng.psmnet_cost_volume(_dev(eng, c.fl), _dev(eng, c.fr), c.maxdisp).cpu().numpy()
    assert np.array_equal(plain.view(np.uint32), ref.plain.view(np.uint32))       # a copy: exact, zeros left of x = i included
    # the other kernel at the same W4: a cost pointer one float into a larger buffer takes the scalar kernel
    n = ref.out.size
    for with_hints, want in ((True, got), (False, plain)):
        buf = sentinels(eng, n + 9, "float32")
        assert buf.data_ptr() % 16 == 0
        _psm_through_lib(eng, c, buf.data_ptr() + 4, with_hints)
        words = buf.cpu().numpy()
        assert words[0] == SENTINEL and (words[n + 1:] == SENTINEL).all()
        assert np.array_equal(words[1:n + 1].view(np.uint32), want.reshape(-1).view(np.uint32))


@pytest.mark.parametrize("tag", ["a", "b", "c", "e"])
def test_psm_golden_equals_the_referee(eng, tag):
    fl, fr, hints, valid = (G[f"psm_{tag}_{k}"] for k in ("fl", "fr", "hints", "valid"))
    maxdisp = int(G[f"psm_{tag}_meta"][0])
    ref = R.psm_volume(fl, fr, maxdisp, hints, valid, rule="library")
    got = eng.psmnet_cost_volume(_dev(eng, fl), _dev(eng, fr), maxdisp, _dev(eng, hints), _dev(eng, valid)).cpu().numpy()
    _hold(got, ref, f"psm golden {tag}")


def test_subsampling_where_float32_and_float64_scales_part(eng):
    """W = 106: destination column 13 reads source column 52 with the float32 scale of F.upsample and 53 with a
    float64 one (searched in tests/test_handoff_ref_cpu.py); every unread pixel is a decoy hint."""
    c = R.psm_case("split", split=(106, 13))
    ref = R.psm_volume(c.fl, c.fr, c.maxdisp, c.hints, c.valid, rule="library")
    got = eng.psmnet_cost_volume(_dev(eng, c.fl), _dev(eng, c.fr), c.maxdisp, _dev(eng, c.hints), _dev(eng, c.valid)).cpu().numpy()
    _hold(got, ref, "psm W = 106")
    corr = np.random.default_rng(9).standard_normal((1, c.H4, c.W4, 1, 5)).astype(np.float32)
    ref = R.raft_modulate(corr, c.hints, c.valid, rule="library")
    got = eng.raft_corr_modulate_(_dev(eng, corr), _dev(eng, c.hints), _dev(eng, c.valid)).cpu().numpy()
    _hold(got, ref, "raft W = 106")


# ---- decoders ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("little", [True, False])
@pytest.mark.parametrize("rows,rowwords", R.PFM_SHAPES)
def test_pfm_payload_is_copied_as_bits(eng, rows, rowwords, little):
    channels = 3 if rowwords == 2880 else 1
    w = R.pfm_payload(rows, rowwords, int(little))
    raw = np.frombuffer(w.astype("<u4" if little else ">u4").tobytes(), np.uint8)
    got = eng.pfm_decode(_dev(eng, raw), rows, rowwords // channels, channels, little).cpu().numpy()
    assert got.shape == ((rows, rowwords // 3, 3) if channels == 3 else (rows, rowwords))
    assert np.array_equal(got.view(np.uint32).reshape(rows, rowwords), R.pfm_decode_bits(raw, rows, rowwords // channels, channels, little))
    assert np.array_equal(got.view(np.uint32).reshape(rows, rowwords), w[::-1])


def test_pfm_payload_one_byte_into_a_tensor_is_refused(eng):
    from vppstereo_amd._lib import VppxError
    raw = _dev(eng, np.zeros(4 * 6 + 1, np.uint8))
    with pytest.raises(VppxError, match="payload 4-byte aligned") as e:
        eng.pfm_decode(raw[1:], 2, 3, 1, True)
    assert e.value.code == -1
    out = sentinels(eng, 6, "float32")
    eng._bind_stream()
    rc = eng.lib.vppx_pfm_decode_dev(eng.ctx.handle, raw.data_ptr() + 1, 2, 3, 1, 1, out.data_ptr())
    eng.torch.cuda.synchronize()
    assert rc == -1 and (out.cpu().numpy() == SENTINEL).all()


@pytest.mark.parametrize("n", R.KITTI_SIZES)
def test_kitti_decode_sizes_values_and_no_valid(eng, n):
    import torch
    u16 = R.kitti_samples(n)
    want_d, want_v = R.kitti_decode(u16)
    d, v = eng.kitti_disp_decode(torch.from_numpy(u16.view(np.int16)).to(eng.device))
    assert np.array_equal(d.cpu().numpy(), want_d) and np.array_equal(v.cpu().numpy(), want_v)
    # valid = NULL (allowed by the header), outputs one word longer than n
    src = torch.from_numpy(np.concatenate([u16, np.array([7], np.uint16)]).view(np.int16)).to(eng.device)
    disp = sentinels(eng, n + 1, "float32")
    eng._bind_stream()
    assert eng.lib.vppx_kitti_disp_decode_dev(eng.ctx.handle, src.data_ptr(), n, disp.data_ptr(), None) == 0
    words = disp.cpu().numpy()
    assert words[n] == SENTINEL and np.array_equal(words[:n].view(np.float32), want_d)


# ---- to_nchw_kernel ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.NCHW_CASES))
def test_to_network_input_shapes(eng, name):
    import torch
    import torch.nn.functional as F
    a, mult = R.nchw_image(name)
    B, H, W, C = a.shape
    x = torch.from_numpy(a / 255.).permute(0, 3, 1, 2).float()                        # test.py:179
    ph, pw = (((H // mult) + 1) * mult - H) % mult, (((W // mult) + 1) * mult - W) % mult
    want = F.pad(x, [pw // 2, pw - pw // 2, ph // 2, ph - ph // 2], mode="replicate") if ph or pw else x
    assert np.array_equal(R.to_nchw(a, mult)[0], want.numpy())
    t = _dev(eng, a)
    got = eng.to_network_input(t, pad_multiple=mult).cpu()
    assert got.shape == want.shape and torch.equal(got, want)
    assert torch.equal(eng.to_network_input(t, dtype=torch.bfloat16, pad_multiple=mult).cpu(), want.to(torch.bfloat16))


# ---- refusals: nothing is launched, the outputs keep their bytes ------------------------------------------
def _refusal_table(p):
    """(entry point, arguments behind the context, code, message).  p: pointers to device buffers that are
    large enough for the shapes named here, so that a check that fails to refuse still reads and writes in bounds."""
    bad = {"nchw": "vppx_u8_to_nchw: bad arguments", "psm": "vppx_psmnet_cost_volume: bad arguments",
           "raft": "vppx_raft_corr_modulate: bad arguments", "kitti": "vppx_kitti_disp_decode: bad arguments",
           "pfm": "vppx_pfm_decode: bad arguments (channels must be 1 or 3, payload 4-byte aligned)"}
    rows = []
    ok = dict(B=1, H=4, W=4, C=1, pad_multiple=4)
    for k, v in (("src", None), ("dst", None), ("B", 0), ("H", 0), ("W", -1), ("C", 0), ("pad_multiple", 0)):
        a = dict(ok, src=p.inp, dst=p.out)
        a[k] = v
        rows.append((f"nchw {k}", "vppx_u8_to_nchw_dev", (a["B"], a["H"], a["W"], a["C"], a["pad_multiple"], a["src"], a["dst"], 0), -1, bad["nchw"]))
    ok = dict(fl=p.inp, fr=p.inp, hints=None, valid=None, B=1, C=1, H4=2, W4=2, H=8, W=8, maxdisp=8, cost=p.out)
    for k, v in (("fl", None), ("fr", None), ("cost", None), ("B", 0), ("C", 0), ("H4", 0), ("W4", -2), ("maxdisp", 3)):
        rows.append((f"psm {k}", None, dict(ok, **{k: v}), -1, bad["psm"]))
    rows.append(("psm hints without validhints", None, dict(ok, hints=p.inp), -1, bad["psm"]))
    rows.append(("psm hints of another size", None, dict(ok, hints=p.inp, valid=p.inp, H=12),
                 -1, "hints are 12x8: sub-sampled by 4 that is 3x2, but the features are 2x2"))
    rows.append(("psm D4 above the grid", None, dict(ok, maxdisp=4 * 65536), -10, "psmnet cost volume: maxdisp/4 and B must be <= 65535"))
    ok = dict(corr=p.out, hints=p.inp, valid=p.inp, B=1, H4=2, W2=2, W3=2, H=8, W=8)
    for k, v in (("corr", None), ("hints", None), ("valid", None), ("B", 0), ("H4", 0), ("W2", 0), ("W3", -1)):
        a = dict(ok, **{k: v})
        rows.append((f"raft {k}", "vppx_raft_corr_modulate_dev", tuple(a[x] for x in ("corr", "hints", "valid", "B", "H4", "W2", "W3", "H", "W")), -1, bad["raft"]))
    a = dict(ok, W=13)
    rows.append(("raft hints of another size", "vppx_raft_corr_modulate_dev", tuple(a[x] for x in ("corr", "hints", "valid", "B", "H4", "W2", "W3", "H", "W")),
                 -1, "hints are 8x13: sub-sampled by 4 that is 2x3, but the features are 2x2"))
    for k, a in (("png", (None, 4, p.out, p.out2)), ("disp", (p.inp, 4, None, p.out2)), ("n", (p.inp, -1, p.out, p.out2))):
        rows.append((f"kitti {k}", "vppx_kitti_disp_decode_dev", a, -1, bad["kitti"]))
    ok = dict(raw=p.inp, H=2, W=2, channels=1, little=1, out=p.out)
    for k, v in (("raw", None), ("out", None), ("H", 0), ("W", 0), ("channels", 2), ("channels", 4), ("raw", p.inp + 2)):
        a = dict(ok, **{k: v})
        rows.append((f"pfm {k}={v if k != 'raw' or v is None else 'misaligned'}", "vppx_pfm_decode_dev", tuple(a[x] for x in ("raw", "H", "W", "channels", "little", "out")), -1, bad["pfm"]))
    for i, r in enumerate(rows):
        if r[1] is None:
            a = r[2]
            rows[i] = (r[0], "vppx_psmnet_cost_volume_dev", tuple(a[x] for x in ("fl", "fr", "hints", "valid", "B", "C", "H4", "W4", "H", "W", "maxdisp", "cost")), r[3], r[4])
    return rows


def test_every_argument_check_of_the_library_refuses_and_writes_nothing(eng):
    from types import SimpleNamespace
    inp = _dev(eng, np.full(4096, 1.0, np.float32))
    out, out2 = sentinels(eng, 4096, "float32"), sentinels(eng, 4096, "float32")
    rows = _refusal_table(SimpleNamespace(inp=inp.data_ptr(), out=out.data_ptr(), out2=out2.data_ptr()))
    assert len(rows) == 7 + 11 + 8 + 3 + 7
    eng._bind_stream()
    for what, fn, args, code, msg in rows:
        rc = getattr(eng.lib, fn)(eng.ctx.handle, *args)
        assert rc == code, (what, rc)
        assert eng.lib.vppx_last_error().decode() == msg, what
    eng.torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all() and (out2.cpu().numpy() == SENTINEL).all()
    assert (inp.cpu().numpy() == 1.0).all()


def test_every_tensor_check_of_the_raft_entries_refuses_before_anything_is_queued(eng):
    """Engine.raft_corr / raft_corr_modulate_ check their tensors against each other like psmnet_cost_volume: the
    library sees H / 4 == H4 and W / 4 == W2 only, and would read past a shorter tensor."""
    import torch
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=eng.device)      # noqa: E731
    corr = torch.full((2, 2, 3, 1, 5), 3.0, dtype=torch.float32, device=eng.device)
    h = z(2, 1, 8, 12)
    shape = "hints / validhints must be \\[B,1,H,W\\]"
    cases = [((corr, h, z(2, 1, 8, 11)), shape),                  # validhints smaller than hints
             ((corr, h, z(1, 1, 8, 12)), shape),
             ((corr, z(1, 1, 8, 12), z(1, 1, 8, 12)), shape),      # a batch of hints shorter than the volume's
             ((corr, z(2, 2, 8, 12), z(2, 2, 8, 12)), shape),
             ((torch.full((2, 2, 3, 2, 5), 3.0, device=eng.device), h, h), "corr must be \\[B,H4,W2,1,W3\\]"),
             ((corr, h.double(), h), "hints: expected contiguous"),
             ((corr, h, h[:, :, :, ::2]), "validhints: expected contiguous")]
    for args, msg in cases:
        with pytest.raises(ValueError, match=msg):
            eng.raft_corr_modulate_(*args)
    assert (corr == 3.0).all().item()
    f2 = z(2, 4, 2, 3)
    for args, msg in [((f2, z(2, 4, 3, 3)), "fmap2 / fmap3 must be"), ((f2, z(1, 4, 2, 3)), "fmap2 / fmap3 must be"),
                      ((f2, z(2, 5, 2, 3)), "fmap2 / fmap3 must be"), ((f2, z(2, 4, 2, 5), h, z(2, 1, 8, 11)), shape),
                      ((f2, z(2, 4, 2, 5), z(1, 1, 8, 12), z(1, 1, 8, 12)), shape)]:
        with pytest.raises(ValueError, match=msg):
            eng.raft_corr(*args)
    # what the library itself can see is still its refusal
    from vppstereo_amd._lib import VppxError
    with pytest.raises(VppxError, match="hints are 12x12") as e:
        eng.raft_corr_modulate_(corr, z(2, 1, 12, 12), z(2, 1, 12, 12))
    assert e.value.code == -1 and (corr == 3.0).all().item()
    assert eng.raft_corr(f2, z(2, 4, 2, 5), h, h).shape == (2, 2, 3, 1, 5)          # W3 != W2 is a legitimate call
