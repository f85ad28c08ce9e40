"""The input builders of tests/test_gpu_stages.py, checked with the oracle alone: every builder asserts on the oracle's own
intermediates that its case reaches what it was written for (tests/_stage_inputs.py), so building a case is the test.  What is
asserted here on top is what the GPU tests rely on without looking: the geometry, the tile rule, the case lists."""
import ctypes as C

import numpy as np
import pytest

import _stage_inputs as si
import oracle


def test_geometry_is_the_reference_s_padding():
    for H, W in si.FRONT_SHAPES + si.GUIDED_SHAPES + ((5, 31), (16, 17), (47, 48)):
        pad = (C.c_int * 4)()
        oracle.lib().rsgmo_pad_amounts(H, W, pad)
        pt, pb, pl, pr, Hp, Wp = si.geom(H, W)
        assert (pl, pr, pt, pb) == tuple(pad) and Hp == H + pt + pb and Wp == W + pl + pr
        assert Hp % 16 == 0 and Wp % 16 == 0 and Hp - H < 16 and Wp - W < 16


def test_interior_tile_rule_at_its_thresholds():
    """H >= 33 and W >= 129 at maximal padding; one row or column less and no tile is interior."""
    assert [si.interior_tiles(H, W) for (H, W) in si.FRONT_SHAPES] == [0, 0, 0, 0, 1, 1, 1, 2, 1, 12]
    assert si.interior_tiles(32, 129) == 0 and si.interior_tiles(33, 128) == 0 and si.interior_tiles(33, 129) == 1
    assert si.interior_tiles(21, 512) == 0 and si.interior_tiles(512, 128) == 0   # every gray frame the suite had before
    # source byte offsets of the rows an interior tile loads, C = 3: every residue mod 4 occurs among the shapes
    res = set()
    for H, W in ((34, 131), (37, 203), (40, 160)):
        pt, _, pl, _, _, _ = si.geom(H, W)
        res |= {(((14 - pt + ly) * W + 62 - pl) * 3) % 4 for ly in range(20)}
    assert res == {0, 1, 2, 3}


@pytest.mark.parametrize("H,W,C,B", si.front_cases())
def test_front_cases_reach_what_they_claim(H, W, C, B):
    for kind in si.front_kinds(C):
        c = si.front_case(H, W, C, B, kind)
        Hp, Wp = si.geom(H, W)[4:]
        assert c["left"].shape == (B, H, W, C) and c["gray_left"].shape == c["census_l"].shape == (B, Hp, Wp)
        assert (c["interior"] > 0) == ((H, W) not in si.FRONT_NO_INTERIOR)
        assert not np.array_equal(c["census_l"], c["census_r"])
        assert not c["left"].flags.writeable
    assert len(si.front_kinds(3)) == 3 and len(si.front_kinds(1)) == 2


@pytest.mark.parametrize("Hp,Wp,B", si.mid_cases())
def test_mid_cases_reach_what_they_claim(Hp, Wp, B):
    c = si.mid_case(Hp, Wp, B)
    floor = 3 if (Hp, Wp) == (16, 16) else 20
    assert c["filled"] >= floor and c["refused"] >= floor
    for k in ("disp_l", "disp_r"):
        a = c[k]
        assert a.shape == (B, Hp, Wp) and np.isfinite(a).all()
        holes = a[a <= 0]
        assert (holes == -10).any() and (holes == 0).any() and ((holes > -0.5) & (holes < 0)).any()
        assert (a[a > 0] % 1 != 0).any()
    if (Hp, Wp, B) == si.MID_DIRECTED:
        assert len(c["seen"]) == 15 * 64


def test_mid_directed_case_is_in_the_list():
    assert si.MID_DIRECTED in si.mid_cases()
    assert float(si.NEAR3) == 3.0 - 2.0 ** -22


@pytest.mark.parametrize("H,W,D,B,density", si.guided_cases())
def test_guided_cases_reach_what_they_claim(H, W, D, B, density):
    c = si.guided_case(H, W, D, B, density)
    pt, pl, Hp, Wp = c["geom"]
    assert c["ref_rows"].shape == (c["n"], D) and c["owner"].shape == (B, Hp, Wp)
    assert not c["owner"][:, :pt].any() and not c["owner"][:, pt + H:].any()       # a padding pixel owns no row
    assert not c["owner"][:, :, :pl].any() and not c["owner"][:, :, pl + W:].any()
    if density == 0:
        assert c["n"] == 0
    elif density == 100:
        assert c["n"] == B * H * W
    else:
        assert 0.03 < c["n"] / (B * H * W) < 0.09


def test_guided_case_list_covers_the_lane_loop_and_the_densities():
    cases = si.guided_cases()
    assert {d for (_, _, d, _, _) in cases} == {8, 40, 64, 192, 256}           # < a wave, partial, 1 / 3 / 4 trips
    assert {(h, w) for (h, w, _, _, _) in cases} == set(si.GUIDED_SHAPES)
    assert {b for (_, _, _, b, _) in cases} == {1, 3} and {p for (*_, p) in cases} == {0, 5, 100}
    assert all((h, w) == (24, 48) for (h, w, _, _, p) in cases if p == 100)
    assert all((h, w) != (34, 300) for (h, w, d, _, _) in cases if d == 256)


def test_tie_case_stage_natives_and_compute_rsgm_are_one_oracle():
    c = si.tie_case()
    B, H, W = si.TIE["B"], si.TIE["H"], si.TIE["W"]
    Hp, Wp = si.geom(H, W)[4:]
    assert c["raw_l"].shape == c["pad_r"].shape == (B, Hp, Wp) and c["final"].shape == (B, H, W)
    assert (c["raw_l"] < 0).any() and (c["raw_l"] % 1 != 0).any()     # invalid pixels and sub-pixel values
    assert (c["final"] > 0).mean() > 0.5
