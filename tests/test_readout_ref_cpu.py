"""The float64 referee of tests/_readout_ref.py, held without a GPU to what it stands in for, on the very arrays
tests/test_gpu_readout.py uploads:

  * it reproduces the arrays the reference's own lines produced (tests/golden/readout_cases.npz) and torch's CPU
    composition of those lines within limit() at every cell;
  * its source indices and weights are torch's, exactly;
  * planted wrong implementations each exceed limit() on at least one case, so the bound can tell;
  * the cases reach what the GPU file says they reach."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _readout_ref as R

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "readout_cases.npz"))
F32, F64 = np.float32, np.float64


# ---- the reference's lines, restated in torch ------------------------------------------------------------------
def torch_psm(cost, D, H, W, crop=None):
    """psmnet.py:227-233 + submodule.py:125-128 + test.py:242-245 on cost [B,D4,H4,W4]."""
    c = F.interpolate(torch.from_numpy(np.asarray(cost, F32))[:, None], size=[D, H, W], mode="trilinear", align_corners=False)
    pred = F.softmax(torch.squeeze(c, 1), dim=1)
    disp = torch.arange(D, dtype=torch.float32).view(1, D, 1, 1)
    out = torch.sum(pred * disp, 1)
    top, left, Ho, Wo = R.window(H, W, crop)
    return out[..., top:top + Ho, left:left + Wo].numpy()


def torch_raft(flow, mask, f, negate=False, channels=None, crop=None):
    """raft_stereo.py:69-81, :154 and test.py:238-245."""
    flow, mask = torch.from_numpy(np.asarray(flow, F32)), torch.from_numpy(np.asarray(mask, F32))
    N, D, H, W = flow.shape
    m = torch.softmax(mask.view(N, 1, 9, f, f, H, W), dim=2)
    up = F.unfold(f * flow, [3, 3], padding=1).view(N, D, 9, 1, 1, H, W)
    up = torch.sum(m * up, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(N, D, f * H, f * W)
    if channels is not None:
        up = up[:, :channels]
    if negate:
        up = -up
    top, left, Ho, Wo = R.window(f * H, f * W, crop)
    return up[..., top:top + Ho, left:left + Wo].numpy()


def _psm_ref(c):
    return R.psm_readout(c.cost, c.D, c.H, c.W, c.crop)


def _raft_ref(c):
    return R.raft_upsample(c.flow, c.mask, c.f, c.negate, c.channels, c.crop)


# ---- the indices and weights are torch's ------------------------------------------------------------------------
@pytest.mark.parametrize("n_in,n_out", [(1, 4), (2, 8), (12, 48), (12, 50), (5, 23), (7, 30), (48, 192), (106, 422), (200, 50), (9, 33),
                                        (66, 264), (3, 1), (4, 4)])
def test_source_indices_and_weights_are_atens(n_in, n_out):
    """A one-hot basis through torch's trilinear upsampling along the depth axis gives the weight of every source cell
    at every output cell: l0 at i0 and l1 at i1, summed where the two coincide."""
    eye = torch.eye(n_in, dtype=torch.float32).view(n_in, 1, n_in, 1, 1)
    w = F.interpolate(eye, size=[n_out, 1, 1], mode="trilinear", align_corners=False).view(n_in, n_out).numpy()
    # ATen's kernels for AVX2 and AVX-512 are compiled with fused multiply-add, the baseline ones are not
    fused = torch.backends.cpu.get_cpu_capability() != "DEFAULT"
    i0, i1, l0, l1 = R.lin_src(n_in, n_out, fused=fused)
    want = np.zeros((n_in, n_out), F32)
    cols = np.arange(n_out)
    want[i0, cols] = l0
    np.add.at(want, (i1, cols), np.where(i1 == i0, F32(0), l1))
    same = i1 == i0
    want[i0[same], cols[same]] = l0[same] + l1[same]
    assert np.array_equal(w, want)
    assert (i1 == i0 + (i0 < n_in - 1)).all() and (l0 == F32(1) - l1).all()


# ---- golden arrays and torch's composition within limit() at every cell ------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_psm_referee_reproduces_the_reference(tag):
    D, H, W = (int(v) for v in G[f"psm_{tag}_meta"])
    cost = G[f"psm_{tag}_cost3"][:, 0]
    ref = R.psm_readout(cost, D, H, W)
    worst, beyond, other = R.compare(G[f"psm_{tag}_pred"], ref)
    here = torch_psm(cost, D, H, W)
    worst_t, beyond_t, other_t = R.compare(here, ref)
    with np.errstate(invalid="ignore"):
        rec = float(np.max(np.abs(here.astype(F64) - G[f"psm_{tag}_pred"]) / ref.limit))
    print(f"psm golden {tag}: recording {worst:.3f} of the limit, torch here {worst_t:.3f}, recording against torch here {rec:.3f}; "
          f"largest limit {ref.limit.max():.2e} px")
    assert (beyond, other, beyond_t, other_t) == (0, 0, 0, 0)


@pytest.mark.parametrize("tag", ["a", "b", "c", "d", "e"])
def test_raft_referee_reproduces_the_reference(tag):
    f = 2 ** int(G[f"raft_{tag}_meta"][0])
    flow, mask = G[f"raft_{tag}_flow"], G[f"raft_{tag}_mask"]
    ref = R.raft_upsample(flow, mask, f)
    worst, beyond, other = R.compare(G[f"raft_{tag}_up"], ref)
    here = torch_raft(flow, mask, f)
    worst_t, beyond_t, other_t = R.compare(here, ref)
    rec = float(np.max(np.abs(here.astype(F64) - G[f"raft_{tag}_up"]) / ref.limit))
    print(f"raft golden {tag}: recording {worst:.3f} of the limit, torch here {worst_t:.3f}, recording against torch here {rec:.3f}")
    assert (beyond, other, beyond_t, other_t) == (0, 0, 0, 0)


@pytest.mark.parametrize("name", list(R.PSM_CASES))
def test_psm_cases_hold_torchs_composition(name):
    c = R.psm_case(name)
    ref = _psm_ref(c)
    top, left, Ho, Wo = R.window(c.H, c.W, c.crop)
    assert ref.value.shape == (c.B, Ho, Wo)
    worst, beyond, other = R.compare(torch_psm(c.cost, c.D, c.H, c.W, c.crop), ref)
    print(f"psm {name}: torch's float32 composition is at {worst:.3f} of the limit; largest limit {np.nanmax(ref.limit):.2e} px")
    assert (beyond, other) == (0, 0)


@pytest.mark.parametrize("name", list(R.RAFT_CASES))
def test_raft_cases_hold_torchs_composition(name):
    c = R.raft_case(name)
    ref = _raft_ref(c)
    worst, beyond, other = R.compare(torch_raft(c.flow, c.mask, c.f, c.negate, c.channels, c.crop), ref)
    print(f"raft {name}: torch's float32 composition is at {worst:.3f} of the limit")
    assert (beyond, other) == (0, 0)


# ---- planted wrong implementations --------------------------------------------------------------------------------
def _worst_over_cases(cases, wrong):
    worst = 0.0
    for c, ref in cases:
        w, beyond, other = R.compare(wrong(c), ref)
        worst = max(worst, w if other == 0 else np.inf)
    return worst


PSM_FINITE = [n for n in R.PSM_CASES if n != "nonfinite"]


@pytest.mark.parametrize("what,wrong", [
    ("align_corners=True", lambda c: R.psm_readout(c.cost, c.D, c.H, c.W, c.crop, align_corners=True).value),
    ("src not clamped at 0", lambda c: R.psm_readout(c.cost, c.D, c.H, c.W, c.crop, clamp=False).value),
    ("softmax before upsampling", lambda c: R.psm_softmax_first(c.cost, c.D, c.H, c.W)[(slice(None),) + _win(c)]),
    ("float64 scale", lambda c: R.psm_readout(c.cost, c.D, c.H, c.W, c.crop, scale_dtype=F64).value),
])
def test_planted_psm_mistakes_exceed_the_limit(what, wrong):
    cases = [(c, _psm_ref(c)) for c in map(R.psm_case, PSM_FINITE)]
    worst = _worst_over_cases(cases, wrong)
    print(f"planted '{what}': {worst:.3g} of the limit at its worst cell")
    assert worst > 1.0


def _win(c):
    top, left, Ho, Wo = R.window(c.H, c.W, c.crop)
    return slice(top, top + Ho), slice(left, left + Wo)


def test_float64_scale_is_caught_where_it_picks_another_tap():
    """The float64 scale differs from ATen's float32 one by the rounding of src alone, and the interpolation is continuous in
    src: it shows only where src is large (its rounding grows with it) and the logits are steep.  Sizes at which the two
    pick different taps are searched for, as tests/_handoff_ref.py's f32_f64_index_splits does; the case the GPU file runs
    is one of them."""
    assert len(R.f32_f64_tap_splits(64)) >= 10
    c = R.psm_case("f64_split")
    a, b = R.lin_src(c.D4, c.D)[0], R.lin_src(c.D4, c.D, F64)[0]
    assert (a != b).any()
    ref = _psm_ref(c)
    worst, _, _ = R.compare(R.psm_readout(c.cost, c.D, c.H, c.W, scale_dtype=F64).value, ref)
    print(f"float64 scale at {c.D4} -> {c.D}: {worst:.2f} of the limit")
    assert worst > 1.0
    assert 20 < ref.value[0, 0, 0] < c.D - 20, "the two peaks do not balance"


@pytest.mark.parametrize("what,how", [("replicate padding", dict(pad="edge")), ("k = 3*kx + ky", dict(order="kx_ky")),
                                      ("mask channel (i*f+j)*9 + k", dict(layout="k_minor"))])
def test_planted_raft_mistakes_exceed_the_limit(what, how):
    cases = [(c, _raft_ref(c)) for c in map(R.raft_case, R.RAFT_CASES)]
    worst = _worst_over_cases(cases, lambda c: R.raft_upsample(c.flow, c.mask, c.f, c.negate, c.channels, c.crop, **how).value)
    print(f"planted '{what}': {worst:.3g} of the limit at its worst cell")
    assert worst > 1.0


# ---- what the cases reach -------------------------------------------------------------------------------------------
def test_psm_cases_reach_what_they_claim():
    lanes = {}                                                     # the launcher's LDS budget: 16 bytes per disparity, a float per plane and lane
    for name in R.PSM_CASES:
        c = R.psm_case(name)
        T = 256
        while T >= 64 and 16 * c.D + 4 * c.D4 * T > 65536:
            T >>= 1
        lanes[name] = T
    assert lanes["x4"] == 256 and lanes["d192_wide"] == 256 and lanes["f64_split"] == 128 and lanes["many_planes"] == 64
    # one plane: i1 == i0 on every axis
    c = R.psm_case("one_plane")
    for n_in, n_out in ((c.D4, c.D), (c.H4, c.H), (c.W4, c.W)):
        i0, i1, _, _ = R.lin_src(n_in, n_out)
        assert (i1 == i0).all()
    # +-80
    c = R.psm_case("pm80")
    assert c.cost.max() == 80 and c.cost.min() == -80
    # exact x4: four constant weights per axis, src clamps at the border, frames differ
    c = R.psm_case("x4")
    for n_in, n_out in ((c.D4, c.D), (c.H4, c.H), (c.W4, c.W)):
        i0, i1, l0, l1 = R.lin_src(n_in, n_out)
        assert sorted(set(l1.tolist())) == [0.0, 0.125, 0.375, 0.625, 0.875]
        unclamped = R.lin_src(n_in, n_out, clamp=False)
        assert (unclamped[3][:2] < 0).all() and (l1[:2] == 0).all(), "border pixels whose src clamps"
        assert i0[-1] == n_in - 1 and i1[-1] == n_in - 1
    assert not np.array_equal(c.cost[0], c.cost[1])
    ref = _psm_ref(c)
    assert not np.array_equal(ref.value[0], ref.value[1])
    # a pixel where all logits are equal, one with a dominant logit, one with logits near +-80
    z = ref.z[0]
    flat = np.ptp(z, axis=-1) == 0
    assert flat[0, 0] and abs(ref.value[0, 0, 0] - (c.D - 1) / 2) < 1e-9
    assert ref.p[0, -1, -1].max() > 0.99
    assert z[0, -1].max() == 80 and z[0, -1].min() == -80
    # general scale: more than five distinct weights on every axis
    c = R.psm_case("general")
    for n_in, n_out in ((c.D4, c.D), (c.H4, c.H), (c.W4, c.W)):
        assert len(set(R.lin_src(n_in, n_out)[3].tolist())) > 5
    # D = 192 and a row of more than 64 pixels, whose width is no multiple of 64
    c = R.psm_case("d192_wide")
    assert c.D == 192 and c.W > 64 and c.W % 64 and _psm_ref(c).limit.max() < 2e-2
    # crop: the window is strictly inside on all four sides, and the cropped value is the uncropped one's window
    c = R.psm_case("crop")
    top, left, Ho, Wo = R.window(c.H, c.W, c.crop)
    assert top > 0 and left > 0 and top + Ho < c.H and left + Wo < c.W and top != left and top != c.H - top - Ho
    whole = R.psm_readout(c.cost, c.D, c.H, c.W).value
    assert np.array_equal(_psm_ref(c).value, whole[:, top:top + Ho, left:left + Wo])
    # non-finite: NaN and +inf make NaN pixels, -inf is weight 0; other pixels stay finite
    c = R.psm_case("nonfinite")
    ref = _psm_ref(c)
    cls = R.classes(ref.value)[0]
    assert set(np.unique(cls)) == {0, 1} and 0 < (cls == 1).sum() < cls.size // 2
    clean = c.cost.copy()
    for key in R.PSM_NONFINITE_AT:
        clean[(0,) + R.PSM_NONFINITE_AT[key]] = 0.0
    for key in ("nan", "pinf", "ninf"):
        one = clean.copy()
        one[(0,) + R.PSM_NONFINITE_AT[key]] = c.cost[(0,) + R.PSM_NONFINITE_AT[key]]
        k1 = R.classes(R.psm_readout(one, c.D, c.H, c.W).value)[0]
        _, y, x = R.PSM_NONFINITE_AT[key]
        reads = k1[4 * y:4 * y + 4, 4 * x:4 * x + 4]
        if key == "ninf":       # weight 0 where the lerp weights are positive; NaN only under a weight of exactly zero
            assert (reads == 0).any() and set(np.unique(k1)) <= {0, 1}
        else:
            assert (reads == 1).all() and (k1 == 1).sum() < k1.size // 2
    assert np.array_equal(R.classes(torch_psm(c.cost, c.D, c.H, c.W)), R.classes(ref.value)), "torch gives the same classes"
    # bfloat16: every cell is a bfloat16 value, and not the float32 case's
    c = R.psm_case("x4_bf16")
    assert (c.cost.view(np.uint32) & 0xFFFF == 0).all() and not np.array_equal(c.cost, R.psm_case("x4").cost)


def test_raft_cases_reach_what_they_claim():
    c = R.raft_case("all_padding")
    v = R.raft_taps(c.flow, c.f)
    assert (np.delete(v[0, 0, 0, 0], 4) == 0).all() and v[0, 0, 0, 0, 4] != 0
    c = R.raft_case("two_by_two")
    ref = _raft_ref(c)
    assert ref.value.shape == (2, 2, 12, 20) and not np.array_equal(ref.value[0], ref.value[1]) and not np.array_equal(ref.value[:, 0], ref.value[:, 1])
    z = ref.z[0]
    assert (np.ptp(z[:c.f, :c.f], axis=-1) == 0).all(), "all logits equal"
    assert ref.p[0, 0, -1, -1].max() > 0.99 and ref.p[0, 0, -1, -1].argmax() == 4, "one dominant logit"
    assert z[0, c.f].max() == 80 and z[0, c.f].min() == -80
    c = R.raft_case("wide")
    assert c.W4 > 64
    assert {R.raft_case(n).f for n in R.RAFT_CASES} == {1, 2, 4, 8}
    c = R.raft_case("test_py")
    assert c.negate and c.channels == 1 and c.C == 2
    top, left, Ho, Wo = R.window(c.f * c.H4, c.f * c.W4, c.crop)
    assert top % c.f and left % c.f and (left + Wo) % c.f, "the window cuts groups of f pixels on both sides"
    whole = R.raft_upsample(c.flow, c.mask, c.f).value
    assert np.array_equal(_raft_ref(c).value, -whole[:, :1, top:top + Ho, left:left + Wo])
    c = R.raft_case("cropped_f8")
    top, left, Ho, Wo = R.window(c.f * c.H4, c.f * c.W4, c.crop)
    assert left % 8 == 4 and Wo % 4 == 0, "aligned to 4 floats, half a group of 8 outside"
    c = R.raft_case("two_bf16")
    assert (c.flow.view(np.uint32) & 0xFFFF == 0).all() and (c.mask.view(np.uint32) & 0xFFFF == 0).all()
