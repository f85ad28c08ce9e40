"""tests/_handoff_ref.py without a GPU: the float64 referee against the golden arrays the reference's own code
produced and against oracle/frontends.py, and every coverage claim tests/test_gpu_handoff_ref.py makes about its
inputs, asserted on those inputs (the practice of tests/_stage_inputs.py / test_stage_inputs_cpu.py)."""
import os

import numpy as np
import pytest

import _handoff_ref as R
from oracle import frontends as FO

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "frontend_cases.npz"))
PSM_GOLDEN, RAFT_GOLDEN = ("a", "b", "c", "e"), ("a", "b", "c", "d")
# torch's float32 exp on the CPU is Sleef's 1.0-ulp routine: the golden arrays are held to limit() at one ulp of the
# exp.  numpy's float32 exp is not: it is taken out of the comparison instead (exp=np.exp makes the referee the oracle).
TORCH_EXP_ULPS = 1.0


def _psm_golden(tag, **kw):
    return R.psm_volume(G[f"psm_{tag}_fl"], G[f"psm_{tag}_fr"], int(G[f"psm_{tag}_meta"][0]), G[f"psm_{tag}_hints"],
                        G[f"psm_{tag}_valid"], **kw)


def _raft_golden(tag, **kw):
    return R.raft_modulate(G[f"raft_{tag}_pre"], G[f"raft_{tag}_hints"], G[f"raft_{tag}_valid"], **kw)


# ---- the referee against the reference and the oracle ---------------------------------------------------
@pytest.mark.parametrize("tag", PSM_GOLDEN + ("d",))
def test_psm_referee_equals_the_reference(tag):
    if tag == "d":                                              # no hints: copies
        ref = R.psm_volume(G["psm_d_fl"], G["psm_d_fr"], int(G["psm_d_meta"][0]))
        assert np.array_equal(ref.out, G["psm_d_cost"]) and np.array_equal(ref.out64, G["psm_d_cost"])
        return
    ref = _psm_golden(tag)
    worst, beyond, changed = R.compare(G[f"psm_{tag}_cost"], ref, TORCH_EXP_ULPS)
    print(f"psm_{tag}: torch is at most {worst:g} ulp from the referee on the normal cells")
    assert beyond == 0 and changed == 0
    lib = _psm_golden(tag, rule="library")                      # finite hints: the two rules are one
    assert np.array_equal(lib.out.view(np.uint32), ref.out.view(np.uint32))


@pytest.mark.parametrize("tag", RAFT_GOLDEN)
def test_raft_referee_equals_the_reference(tag):
    ref = _raft_golden(tag)
    worst, beyond, changed = R.compare(G[f"raft_{tag}_post"], ref, TORCH_EXP_ULPS)
    print(f"raft_{tag}: torch is at most {worst:g} ulp from the referee on the normal cells")
    assert beyond == 0 and changed == 0
    lib = _raft_golden(tag, rule="library")
    assert np.array_equal(lib.out.view(np.uint32), ref.out.view(np.uint32))


def test_referee_equals_the_oracle_in_everything_but_the_exp():
    """With numpy's float32 exp put in the referee's place of the float64 one, the two are one function, bit for
    bit: on the golden inputs and on every built case (v = -0, 0.5, 2, hints off the planes and off the row)."""
    for tag in PSM_GOLDEN:
        got = FO.psmnet_cost_volume(G[f"psm_{tag}_fl"], G[f"psm_{tag}_fr"], int(G[f"psm_{tag}_meta"][0]), G[f"psm_{tag}_hints"],
                                    G[f"psm_{tag}_valid"])
        assert np.array_equal(got.view(np.uint32), _psm_golden(tag, exp=np.exp).out.view(np.uint32)), tag
    for tag in RAFT_GOLDEN:
        got = FO.raft_corr_modulate(G[f"raft_{tag}_pre"], G[f"raft_{tag}_hints"], G[f"raft_{tag}_valid"])
        assert np.array_equal(got.view(np.uint32), _raft_golden(tag, exp=np.exp).out.view(np.uint32)), tag
    for name in R.PSM_CASES:
        c = R.psm_case(name)
        got = FO.psmnet_cost_volume(c.fl, c.fr, c.maxdisp, c.hints, c.valid)
        ref = R.psm_volume(c.fl, c.fr, c.maxdisp, c.hints, c.valid, exp=np.exp)
        assert np.array_equal(got.view(np.uint32), ref.out.view(np.uint32)), name
        assert np.array_equal(FO.psmnet_cost_volume(c.fl, c.fr, c.maxdisp), ref.plain), name
    for name in R.RAFT_CASES:
        c = R.raft_case(name)
        got = FO.raft_corr_modulate(c.corr, c.hints, c.valid)
        assert np.array_equal(got.view(np.uint32), R.raft_modulate(c.corr, c.hints, c.valid, exp=np.exp).out.view(np.uint32)), name
    for n_in in (4, 7, 23, 106, 159, 543, 1242):
        assert np.array_equal(R.nearest_indices(n_in, n_in // 4), FO.nearest_indices(n_in, n_in // 4))


def test_measured_distances_of_the_two_cpu_exps():
    """What docs/NOTEBOOK.md quotes: numpy's and torch's float32 exp against the float64 one, on the arguments of
    every committed case, in ulp of the float32 exp (normal results only), and the factor of numpy's."""
    import torch
    worst = dict(numpy=0.0, torch=0.0, numpy_factor=0.0, torch_cell=0.0)
    refs = [_psm_golden(t) for t in PSM_GOLDEN] + [_raft_golden(t) for t in RAFT_GOLDEN]
    cells = [G[f"psm_{t}_cost"] for t in PSM_GOLDEN] + [G[f"raft_{t}_post"] for t in RAFT_GOLDEN]
    for ref, cell in zip(refs, cells):
        normal, _, _ = R.cell_classes(ref)
        arg, e64 = np.unique(ref.arg[normal]), None
        e64 = np.exp(arg.astype(np.float64))
        for name, e32 in (("numpy", np.exp(arg)), ("torch", torch.exp(torch.from_numpy(arg)).numpy())):
            worst[name] = max(worst[name], float((np.abs(e32.astype(np.float64) - e64) / R.ulp32(e64)).max()))
            if name == "numpy":
                f64 = 10.0 * e64
                f32 = np.float32(10) * e32
                worst["numpy_factor"] = max(worst["numpy_factor"], float((np.abs(f32.astype(np.float64) - f64) / R.ulp32(f64)).max()))
        worst["torch_cell"] = max(worst["torch_cell"], R.compare(cell, ref, TORCH_EXP_ULPS)[0])
    print("measured maxima (ulp):", worst)
    assert worst["torch"] <= TORCH_EXP_ULPS                     # Sleef's documented bound holds on these arguments
    assert worst["numpy"] <= 4.0                                # reported, not relied on: glibc-free SIMD exp, a few ulp


def test_v_zero_rule_switch_on_a_non_finite_hint():
    """The one documented difference: an invalid pixel whose hint is inf (a Middlebury map keeps inf for unknown
    pixels).  hints * valid is NaN there, so the reference's arithmetic turns the pixel's cells into NaN; the
    library's rule leaves them untouched.  For finite hints the two rules agree bit for bit (tests above)."""
    c = R.raft_case("w65")
    y, x = np.argwhere(c.v4[0] == 0)[0]
    iy, ix = R.nearest_indices(c.H, c.H4)[y], R.nearest_indices(c.W, c.W2)[x]
    c.hints[0, 0, iy, ix] = np.inf
    ref, lib = (R.raft_modulate(c.corr, c.hints, c.valid, rule=r) for r in ("reference", "library"))
    assert np.isnan(ref.out[0, y, x]).all()
    assert np.array_equal(lib.out[0, y, x], c.corr[0, y, x])
    rest = np.ones(ref.out.shape, bool)
    rest[0, y, x] = False
    assert np.array_equal(ref.out[rest], lib.out[rest])
    p = R.psm_case("w8")
    y, x = np.argwhere(p.v4[0] == 0)[0]
    p.hints[0, 0, R.nearest_indices(p.H, p.H4)[y], R.nearest_indices(p.W, p.W4)[x]] = -np.inf
    ref, lib = (R.psm_volume(p.fl, p.fr, p.maxdisp, p.hints, p.valid, rule=r) for r in ("reference", "library"))
    assert np.isnan(ref.out[0, :, :, y, x]).all()
    assert np.array_equal(lib.out[0, :, :, y, x], lib.plain[0, :, :, y, x])


def test_compare_holds_non_finite_cells_to_their_class():
    """A NaN hint under v = 1 makes the referee's cells NaN; compare() must not let any finite value pass there."""
    c = R.raft_case("w65")
    y, x = np.argwhere(c.v4[0] == 1)[0]
    c.hints[0, 0, R.nearest_indices(c.H, c.H4)[y], R.nearest_indices(c.W, c.W2)[x]] = np.nan
    ref = R.raft_modulate(c.corr, c.hints, c.valid, rule="library")
    assert np.isnan(ref.out[0, y, x]).all()
    assert R.compare(ref.out, ref, 1.0)[1:] == (0, 0)
    wrong = ref.out.copy()
    wrong[0, y, x, 0, 3] = 0.0
    assert R.compare(wrong, ref, 1.0)[1] == 1
    wrong = ref.out.copy()
    wrong[0, (y + 1) % c.H4, x, 0, 0] = np.nan                   # and a NaN where the referee is finite
    assert R.compare(wrong, ref, 1.0)[1] + R.compare(wrong, ref, 1.0)[2] == 1


def test_decoders_are_exact():
    d, v = R.kitti_decode(G["kitti_u16"])
    assert np.array_equal(d, G["kitti_disp"]) and np.array_equal(v, G["kitti_valid"])
    everything = np.arange(65536, dtype=np.uint16)
    d, v = R.kitti_decode(everything)
    od, ov = FO.kitti_disp_decode(everything)
    assert np.array_equal(d, od) and np.array_equal(v, ov) and v.sum() == 65535
    for tag in ("g", "c"):
        H, W, ch, little = (int(x) for x in G[f"pfm_{tag}_meta"])
        bits = R.pfm_decode_bits(G[f"pfm_{tag}_raw"], H, W, ch, bool(little))
        assert np.array_equal(bits, G[f"pfm_{tag}_dec"].view(np.uint32).reshape(H, W * ch))
    for rows, rowwords in [(1, 255), (1, 256), (3, 257)]:
        w = R.pfm_payload(rows, rowwords, 0)
        for little in (True, False):
            raw = w.astype("<u4" if little else ">u4").tobytes()
            bits = R.pfm_decode_bits(raw, rows, rowwords, 1, little)
            assert np.array_equal(bits, w[::-1])
            assert np.array_equal(bits.view(np.float32), FO.pfm_decode(raw, rows, rowwords, 1, little), equal_nan=True)


def test_to_nchw_referee_is_the_reference_glue():
    import torch
    import torch.nn.functional as F
    for name in R.NCHW_CASES:
        a, mult = R.nchw_image(name)
        ref, (ph, pw) = R.to_nchw(a, mult)
        x = torch.from_numpy(a / 255.).permute(0, 3, 1, 2).float()
        want = F.pad(x, [pw // 2, pw - pw // 2, ph // 2, ph - ph // 2], mode="replicate") if ph or pw else x
        assert np.array_equal(ref, want.numpy()), name


# ---- coverage claims of the GPU file, asserted on its inputs ------------------------------------------------
def test_values_of_v_are_exact_in_float32():
    """limit() counts three roundings behind the exp: 1 - v and v * 10 must add none."""
    for v in R.VALUES_OF_V:
        v = np.float32(v)
        assert float(np.float32(1) - v) == 1.0 - float(v) and float(v * np.float32(10)) == 10.0 * float(v)


@pytest.mark.parametrize("name", list(R.RAFT_CASES))
def test_raft_case_claims(name):
    c = R.raft_case(name)
    B, H4, W2, W3, rH, rW, kind = R.RAFT_CASES[name]
    ref = R.raft_modulate(c.corr, c.hints, c.valid, rule="library")
    h, v = R.subsample(c.hints, c.valid)
    assert np.array_equal(v.view(np.uint32), c.v4.view(np.uint32))          # the sign of -0 survives the scatter
    assert (c.H % 4, c.W % 4) == (rH, rW)
    assert (c.valid != 0).mean() > 0.9 or kind in ("none",) and (c.valid != 0).mean() > 0.5     # decoys are hints too
    normal, sub, zero = R.cell_classes(ref)
    modulated = int((ref.v != 0).sum())
    rows = c.v4 != 0
    if kind == "none":
        assert modulated == 0 and np.array_equal(ref.out, c.corr)
        return
    if kind in ("every", "all_normal"):
        assert rows.all()
    if kind == "all_normal":
        assert normal.sum() == modulated == c.corr.size
        return
    # a row holds at most 27 cells with a normal exp (|k - target| < 13.2), so a fifth of the cells is out of reach
    # from W3 = 136 on whatever the hints: a fifth where the row allows it, else three quarters of what it allows
    # (six directed rows aim off the row, and a target near either end loses the cells beyond it).  The 0.75 is chosen,
    # not derived: a floor that says "most of what a row can hold", under what the builder gives (0.78 .. 0.91 of 27 / W3)
    assert normal.sum() / modulated >= min(0.2, 0.75 * 27 / W3), normal.sum() / modulated
    if kind == "directed":
        assert {np.float32(x).tobytes() for x in R.VALUES_OF_V} <= {x.tobytes() for x in c.v4.reshape(-1)}
        tgt = ref.target[rows]
        for t in range((W3 + 63) // 64):
            assert ((tgt >= 64 * t) & (tgt < min(64 * t + 64, W3))).any(), f"no target in trip {t}"
        assert (tgt < -0.25).any() and (tgt > W3 - 1 + 0.25).any()
        assert sub.any() and zero.any()
        assert (rows & (np.arange(W2)[None, None, :] == 0)).any() or W2 > 1


def test_raft_cases_reach_every_row_residue_and_every_width():
    res = {name: (v[0] * v[1] * v[2]) % 4 for name, v in R.RAFT_CASES.items()}
    assert (res["w1"], res["w63"], res["w65"], res["w64"]) == (1, 2, 3, 0)
    assert {v[3] for v in R.RAFT_CASES.values()} >= {1, 63, 64, 65, 128, 130, 240}
    assert R.RAFT_CASES["w65_narrow"][2] < 65 < R.RAFT_CASES["w65_wide"][2]
    assert {(v[4], v[5]) for v in R.RAFT_CASES.values()} >= {(0, 0), (1, 2), (3, 1), (2, 3)}
    two = R.raft_case("w130")
    assert not np.array_equal(two.corr[0], two.corr[1]) and not np.array_equal(two.v4[0], two.v4[1])
    # the golden cases past one trip
    assert G["raft_c_post"].shape[4] == 66 and G["raft_d_post"].shape[4] == 130 and G["psm_e_cost"].shape[2:] == (12, 2, 68)


@pytest.mark.parametrize("kind,tag", [("raft", t) for t in RAFT_GOLDEN] + [("psm", t) for t in PSM_GOLDEN])
def test_golden_cases_have_cells_in_the_normal_range(kind, tag):
    ref = _raft_golden(tag) if kind == "raft" else _psm_golden(tag)
    normal, _, _ = R.cell_classes(ref)
    share = normal.sum() / (ref.v != 0).sum()
    # RAFT: hints uniform over the row, and a row holds at most 27 cells with a normal exp.  The 0.4 is chosen, not
    # derived: the reference's script aims about half of the targets left of the row (docs/NOTEBOOK.md), so these
    # cases hold 0.42 and 0.47 of 27 / W3 (d, c); golden c (W3 = 66) is at 19.0 %, below the fifth its width would allow
    assert share >= (min(0.2, 0.4 * 27 / ref.out.shape[4]) if kind == "raft" else 0.2), share


@pytest.mark.parametrize("name", list(R.PSM_CASES))
def test_psm_case_claims(name):
    c = R.psm_case(name)
    B, C, H4, W4, rH, rW, maxdisp, kind = R.PSM_CASES[name]
    ref = R.psm_volume(c.fl, c.fr, c.maxdisp, c.hints, c.valid, rule="library")
    h, v = R.subsample(c.hints, c.valid)
    assert np.array_equal(v.view(np.uint32), c.v4.view(np.uint32))
    assert (c.H % 4, c.W % 4) == (rH, rW) and ref.out.shape == (B, 2 * C, maxdisp // 4, H4, W4)
    normal, sub, zero = R.cell_classes(ref)
    modulated = int((ref.v != 0).sum())
    if kind == "none":
        assert modulated == 0 and np.array_equal(ref.out, ref.plain)
        return
    if kind == "all_normal":
        assert (c.v4 != 0).all() and normal.sum() == modulated == ref.out.size
        return
    assert normal.sum() / modulated >= 0.2
    if kind == "directed":
        assert {np.float32(x).tobytes() for x in R.VALUES_OF_V} <= {x.tobytes() for x in c.v4.reshape(-1)}
        on = h[c.v4 != 0]
        D4 = maxdisp // 4
        assert (on == np.floor(on)).any() and (on - np.floor(on) == 0.5).any() and (on > D4).any() and (on * 4 > maxdisp).any()
    # the zeros left of x = i and the first copied column x = i (x - i = 0) are there to be compared
    for i in range(min(maxdisp // 4, W4)):
        assert (ref.plain[:, :, i, :, :i] == 0).all() and np.array_equal(ref.plain[:, C:, i, :, i], c.fr[:, :, :, 0])


def test_psm_cases_reach_every_width_kernel_and_block():
    t = R.PSM_CASES
    assert {v[3] for v in t.values()} >= {1, 3, 4, 5, 8, 68}
    vec = {k for k, v in t.items() if v[3] % 4 == 0}
    assert any(t[k][6] // 4 > t[k][3] for k in vec) and any(t[k][6] // 4 > t[k][3] for k in set(t) - vec)
    assert {t["w4_d1"][6] // 4, t["w5_d1"][6] // 4} == {1} and {t["w4_d1"][6], t["w5_d1"][6]} == {4, 7}
    assert t["w5_d1"][1] == 1 and t["w8"][1] == 1
    assert t["w8"][6] // 4 >= 8                                  # planes 0 .. 7 cut both vectors of a row at every position
    assert t["w68"][3] // 4 * t["w68"][2] > 256 and t["w5_tall"][3] * t["w5_tall"][2] > 256     # a second block of each kernel
    assert {v[4] for v in t.values()} == {0, 1, 2, 3} and {v[5] for v in t.values()} == {0, 1, 2, 3}


def test_float32_and_float64_scale_pick_different_source_pixels():
    """The search the sub-sampling case rests on: below 2048 there are widths at which floor(dst * scale) differs
    between a float32 and a float64 product; the smallest is 106 at dst = 13 (float32 reads column 52, float64 53:
    106 / 26 rounds down in float32 and 13 times it stays below 53).
    The built case plants different hints at the two columns."""
    splits = R.f32_f64_index_splits()
    assert splits and splits[0] == (106, 13)
    W, dst = splits[0]
    a, b = R.nearest_indices(W, W // 4), R.nearest_indices(W, W // 4, np.float64)
    assert (int(a[dst]), int(b[dst])) == (52, 53)
    c = R.psm_case("split", split=(W, dst))
    assert c.W == W and c.hints[0, 0, 0, a[dst]] != c.hints[0, 0, 0, b[dst]]
    h, _ = R.subsample(c.hints, c.valid)
    assert h[0, 0, dst] * 4 == c.hints[0, 0, R.nearest_indices(c.H, c.H4)[0], 52]
    # the clamp: W = 4 * W4 + 3 reads at most column W - 1
    assert R.nearest_indices(7, 1)[0] == 0 and R.nearest_indices(23, 5).max() <= 22


def test_decoder_and_nchw_shapes_are_the_ones_claimed():
    assert set(R.PFM_SHAPES) == {(r, w) for r in (1, 540) for w in (255, 256, 257, 960, 2880)}
    w = R.pfm_payload(3, 255, 1)
    f = w.view(np.float32)
    assert np.isnan(f).any() and np.isposinf(f).any() and np.isneginf(f).any() and (w == 0x7F800001).any()
    assert set(R.KITTI_VALUES) <= set(R.kitti_samples(257)) and R.kitti_samples(0).size == 0 and R.kitti_samples(1)[0] == 0
    for name, (B, H, W, C, mult) in R.NCHW_CASES.items():
        _, (ph, pw) = R.to_nchw(R.nchw_image(name)[0], mult)
        if name in ("no_pad", "mult1"):
            assert (ph, pw) == (0, 0)
        if name == "odd_pad":
            assert ph % 2 == 1 and pw % 2 == 1
        if name == "wide":
            assert W + pw > 256
        if name == "c1":
            assert C == 1 and (ph or pw)
