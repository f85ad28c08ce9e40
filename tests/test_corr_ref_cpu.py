"""The numpy referee of the correlation pyramid and lookup (tests/_corr_ref.py) against the arrays the reference's own
CorrBlock1D produced and against torch's CPU avg_pool2d / grid_sample, bit for bit; the coverage the GPU file
(tests/test_gpu_corr.py) claims for its inputs, asserted on those inputs; the new symbols of the C-ABI."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _corr_ref as CR
import _handoff_bf16_ref as BR
import _handoff_ref as R

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "corr_cases.npz"))
GOLD_TAGS = ("a", "b", "c", "d")


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- torch's composition, written out as CorrBlock1D composes it ---------------------------------------------
def torch_lookup(pyr, coords, radius):
    """pyr: [N,1,1,Wi] tensors, coords [B,H4,W2] -> [B, L*(2r+1), H4, W2]."""
    B, H4, W2 = coords.shape
    c = torch.from_numpy(np.ascontiguousarray(coords)).reshape(B * H4 * W2, 1, 1, 1)
    per_level = []
    for i, lv in enumerate(pyr):
        W = lv.shape[-1]
        dx = torch.linspace(-radius, radius, 2 * radius + 1).view(1, 1, 2 * radius + 1, 1)
        x0 = dx + c / 2 ** i
        grid = torch.cat([2 * x0 / (W - 1) - 1, torch.zeros_like(x0)], dim=-1)
        per_level.append(F.grid_sample(lv, grid, align_corners=True).view(B, H4, W2, -1))
    return torch.cat(per_level, dim=-1).permute(0, 3, 1, 2).contiguous().float().numpy()


# ---- the golden arrays -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plain", "hints"])
@pytest.mark.parametrize("tag", GOLD_TAGS)
def test_referee_equals_the_reference_bit_for_bit(tag, kind):
    level0 = GOLD[f"{tag}_{kind}_level0"]
    pyr = CR.pyramid(level0, 5)
    for i in range(1, 5):
        assert _bits_equal(pyr[i], GOLD[f"{tag}_{kind}_level{i}"]), (tag, kind, i)
    coords = GOLD[f"{tag}_coords"]
    B, _, H4, W2 = coords.shape
    got = CR.channels_first(CR.lookup(pyr[:4], coords[:, 0], 4), B, H4, W2)
    want = GOLD[f"{tag}_{kind}_lookup"]
    assert _bits_equal(got, want), (tag, kind, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    assert (want != 0).mean() > 0.25          # not a lookup of zeros (17-wide rows leave few taps inside the upper levels)
    if kind == "hints":     # the modulated volume holds cells of both zeros: the pooling's +0 start is exercised
        assert (level0.view(np.uint32) == 0x80000000).any() and (level0.view(np.uint32) == 0).any()


def test_golden_coordinates_hold_the_directed_values():
    for tag in GOLD_TAGS:
        c = GOLD[f"{tag}_coords"][:, 0].reshape(-1)
        W = GOLD[f"{tag}_coords"].shape[3]
        for v in (W - 1, W - 0.5, -4.0, -5.0, W + 3.0, -0.25, 1e30, -1e30):
            assert (c == F32(v)).any(), (tag, v)
        assert ((c == 0) & ~np.signbit(c)).any() and ((c == 0) & np.signbit(c)).any()
        assert np.isfinite(c).all()


# ---- torch on the GPU file's own cases -----------------------------------------------------------------------
def _pool_equals_torch(got, want, below):
    """Bit for bit, but for one sign: where the two cells below have a negative sum whose half rounds to zero (a tie
    at half the smallest subnormal of the storage type), the result is -0 (IEEE, the referee, the device), and this
    torch's CPU avg_pool2d returns +0.  Such sums arise where the modulation's factor underflows; nothing else
    differs.  got / want / below: float32 values (bfloat16 cells widened)."""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    w = got.shape[1]
    with np.errstate(invalid="ignore"):
        neg = (F32(0) + below[:, 0:2 * w:2]) + below[:, 1:2 * w:2] < 0
    sign = neg & (got.view(np.uint32) == 0x80000000) & (want.view(np.uint32) == 0)
    assert not ((got.view(np.uint32) != want.view(np.uint32)) & ~sign).any()


@pytest.mark.parametrize("shape", CR.PYRAMID_SHAPES, ids=CR.tag)
def test_pyramid_referee_equals_avg_pool2d_on_the_gpu_cases(shape):
    for hints in (False, True):
        c = CR.volume_case(shape, hints=hints)
        level0 = CR.modulated_level0(c)
        pyr = CR.pyramid(level0, 4)
        for i in range(1, 4):       # each level from the referee's level below, so that one sign does not travel upwards
            want = F.avg_pool2d(torch.from_numpy(pyr[i - 1])[:, None, None, :], [1, 2], stride=[1, 2]).numpy().reshape(c.N, -1)
            _pool_equals_torch(pyr[i], want, pyr[i - 1])
        # bfloat16 storage: what torch's bfloat16 avg_pool2d gives
        bpyr = CR.pyramid(BR.bits(BR.bf16_rne_f32(level0)), 4)
        for i in range(1, 4):
            below = torch.from_numpy(BR.widen(bpyr[i - 1])).to(torch.bfloat16)[:, None, None, :]
            want = F.avg_pool2d(below, [1, 2], stride=[1, 2]).float().numpy().reshape(c.N, -1)
            _pool_equals_torch(BR.widen(bpyr[i]), want, BR.widen(bpyr[i - 1]))


@pytest.mark.parametrize("shape", CR.LOOKUP_SHAPES, ids=CR.tag)
def test_lookup_referee_equals_grid_sample_on_the_gpu_cases(shape):
    c = CR.volume_case(shape, hints=True)
    level0 = CR.modulated_level0(c)
    sheets = CR.coords_case(shape)
    for levels, radius in CR.LOOKUP_PARAMS:
        pyr = CR.pyramid(level0, levels)
        tpyr = [torch.from_numpy(lv)[:, None, None, :] for lv in pyr]
        for coords in sheets:
            got = CR.channels_first(CR.lookup(pyr, coords, radius), c.B, c.H4, c.W2)
            want = torch_lookup(tpyr, np.where(np.isfinite(coords), coords, F32(0)), radius)
            fin = np.broadcast_to(np.isfinite(coords)[:, None], got.shape)    # torch's index of a non-finite position is undefined
            assert np.array_equal(got.view(np.uint32)[fin], want.view(np.uint32)[fin]), (shape, levels, radius)
            assert (got[~fin].view(np.uint32) == 0).all()                     # the library's rule: +0


# ---- what the inputs reach -----------------------------------------------------------------------------------
def test_pyramid_cases_cover_what_the_gpu_file_says():
    residues = set()
    for shape in CR.PYRAMID_SHAPES:
        c = CR.volume_case(shape, hints=True)
        residues.add(c.N % CR.ROWS_PER_WORKGROUP)
        assert (c.H // 4, c.W // 4) == (c.H4, c.W2)
        _, v = R.subsample(c.hints, c.valid, raft=True)
        assert np.array_equal(v.view(np.uint32), c.v4.view(np.uint32))
        vb = c.v4.reshape(-1).view(np.uint32)
        if c.N >= len(CR.V_ORDER):
            for want in CR.V_ORDER:
                assert (vb == np.array([want], F32).view(np.uint32)[0]).any(), (shape, want)
        level0 = CR.modulated_level0(c)
        pyr = CR.pyramid(level0, 4)
        neg0 = level0.view(np.uint32) == 0x80000000
        pair = neg0[:, 0:2 * (c.W3 // 2):2] & neg0[:, 1:2 * (c.W3 // 2):2]
        assert pair.any() and (pyr[1].view(np.uint32)[pair] == 0).all(), "a pair of -0 cells pools to +0"
        if c.N >= 2:
            assert (c.v4.reshape(-1)[1] == 0) and pair[1].any() and np.abs(pyr[3][1]).max() > 0
    assert residues == {0, 1, 2, 3}
    widths = {s[3] for s in CR.PYRAMID_SHAPES}
    assert {16, 17, 30, 127, 128, 129, 130, 240, 257} <= widths
    two = CR.volume_case((2, 2, 9, 37))
    assert not np.array_equal(two.corr[0], two.corr[1]) and not np.array_equal(two.v4[0], two.v4[1])


@pytest.mark.parametrize("shape", CR.LOOKUP_SHAPES, ids=CR.tag)
def test_lookup_coordinates_hold_every_class_and_reach_the_volume(shape):
    B, H4, W2, W3 = shape
    sheets = CR.coords_case(shape)
    assert sheets.shape[1:] == (B, H4, W2)
    flat = sheets.reshape(-1)
    for name, vals in CR.directed_coords(W3).items():
        for v in vals:
            hit = np.isnan(flat) if np.isnan(v) else (flat == v) & (np.signbit(flat) == np.signbit(v))
            assert hit.any(), (name, v)
    assert sheets[0].reshape(-1)[CR.NAN_AT["row"]] == CR.NAN_AT["cell"] - 1
    rest = flat[np.isfinite(flat) & (np.abs(flat) < 1e29)]
    assert ((rest >= -3) & (rest < W3 + 3)).mean() >= 0.75 and rest.size >= 0.8 * flat.size
    frac = (flat[np.isfinite(flat)] % 1)
    assert (frac == 0).any() and (frac == 0.5).any() and ((frac != 0) & (frac != 0.5)).any()
    # at least half of the lookup's cells are nonzero, at the full four levels of radius four
    c = CR.volume_case(shape, hints=True, nan_cell=shape == CR.NAN_SHAPE)
    pyr = CR.pyramid(CR.modulated_level0(c), 4)
    cells = np.concatenate([CR.lookup(pyr, s, 4).reshape(-1) for s in sheets])
    print(f"{CR.tag(shape)}: {float((cells != 0).mean()):.3f} of the lookup cells are nonzero")
    assert (cells != 0).mean() >= 0.5
    # the NaN cell is read under a weight of zero, and the result is NaN
    if shape == CR.NAN_SHAPE:
        first = CR.lookup(pyr[:1], sheets[0], 4)
        cell = pyr[0][CR.NAN_AT["row"]]
        assert np.isnan(cell[CR.NAN_AT["cell"]]) and np.isnan(cell).sum() == 1 and np.isnan(first[CR.NAN_AT["row"], 4])
        assert np.isnan(first[CR.NAN_AT["row"]]).sum() == 2          # taps 4 (weight 0) and 5; none elsewhere


def test_far_outside_and_non_finite_coordinates_give_plus_zero():
    c = CR.volume_case((1, 1, 65, 30), hints=False)
    pyr = CR.pyramid(CR.modulated_level0(c), 4)
    d = CR.directed_coords(30)
    bad = np.concatenate([d["far_outside"], d["huge"], d["inf"], d["nan"]])
    coords = np.resize(bad, 65).astype(F32)
    out = CR.lookup(pyr, coords, 4)
    assert (out.view(np.uint32) == 0).all()


# ---- the C-ABI ------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_bound():
    from vppstereo_amd import _lib
    lib = _lib.load()
    i, vp = C.c_int, C.c_void_p
    for name in ("vppx_raft_corr_pyramid_cells", "vppx_raft_corr_pyramid_dt_dev", "vppx_raft_corr_lookup_dt_dev"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.vppx_raft_corr_pyramid_cells.argtypes == [C.c_int64, i, i, vp]     # int64_t *offsets: untyped, as every pointer to a scalar
    assert lib.vppx_raft_corr_pyramid_cells.restype == C.c_int64
    assert lib.vppx_raft_corr_pyramid_dt_dev.argtypes == [vp, vp, vp, vp, i, i, i, i, i, i, i, vp, i]
    assert lib.vppx_raft_corr_lookup_dt_dev.argtypes == [vp, vp, vp, vp, C.c_int64, i, i, i, i, i, i, vp, i]
    assert (_lib.CORR_MAX_LEVELS, _lib.CORR_MAX_RADIUS) == (4, 8)
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "vppx.h")).read()
    assert "#define VPPX_CORR_MAX_LEVELS 4" in hdr and "#define VPPX_CORR_MAX_RADIUS 8" in hdr


def test_pyramid_cells_needs_no_device():
    from vppstereo_amd import _lib
    lib = _lib.load()
    off = (C.c_int64 * 4)(-1, -1, -1, -1)
    assert lib.vppx_raft_corr_pyramid_cells(6, 17, 4, off) == 6 * (8 + 4 + 2)
    assert list(off) == [0, 0, 48, 72]
    assert lib.vppx_raft_corr_pyramid_cells(5, 30, 1, None) == 0
    assert lib.vppx_raft_corr_pyramid_cells(1 << 33, 240, 2, None) == (1 << 33) * 120
    assert lib.vppx_raft_corr_pyramid_cells(0, 17, 4, off) == -1
    assert lib.vppx_raft_corr_pyramid_cells(6, 17, 0, off) == -1
    assert lib.vppx_raft_corr_pyramid_cells(6, 17, 5, off) == -10
    assert list(off) == [0, 0, 48, 72]
