"""CPU oracle (oracle/rsgm_oracle.c, vpp_oracle.c) vs golden vectors produced by importing the
reference's Python glue (tests/golden/make_glue_golden.py): rsgm.py, filter.py,
vpp_standalone.py, losses.py."""
import os

import numpy as np
import pytest

import oracle

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(GOLDEN, "glue_cases.npz"))


def test_linear_interpolate(G):  # rsgm.py:67-113
    for i in range(3):
        a = G[f"linint{i}_in"].copy()
        oracle._linear_interpolate(a, 15, 3)
        assert np.array_equal(a, G[f"linint{i}_out"]), i
        assert not np.array_equal(a, G[f"linint{i}_in"])


def test_left_right_check(G):  # rsgm.py:230-248
    for i in range(2):
        m = oracle._left_right_check(G[f"lrc{i}_dl"], G[f"lrc{i}_dr"], 1)
        assert np.array_equal(m, G[f"lrc{i}_mask"]), i
        assert set(np.unique(m)) == {0, 128, 255}


def test_interpolate_background(G):  # rsgm.py:185-227
    for i in range(3):
        a = G[f"bg{i}_in"].copy()
        oracle._interpolate_background(a)
        assert np.array_equal(a, G[f"bg{i}_out"]), i


def test_occlusion_heuristic_conf(G):  # filter.py:246-292 (conf map = g_occ of test.py:154)
    for i in range(2):
        _, conf = oracle.occlusion_heuristic(G[f"occ{i}_in"])
        assert np.array_equal(conf, G[f"occ{i}_conf"]), i
        hints = G[f"occ{i}_in"] > 0
        assert 0 < (conf[hints] == 0).sum() < hints.sum()  # some hints kept, some flagged


def test_bilateral_filling(G):  # vpp_standalone.py:372-394
    for i in range(2):
        out = oracle.bilateral_filling(G[f"bil{i}_dmap"], G[f"bil{i}_img"], int(G[f"bil{i}_n"]), 2, 1, .001)
        assert np.array_equal(out, G[f"bil{i}_out"]), i


def test_patch_size_based_on_distance(G):  # vpp_standalone.py:7-11
    got = [oracle.patch_radius(float(d), 1.0, 50.0, 7, 0.3) for d in G["patch_d"]]
    assert got == G["patch_n"].tolist()
    assert set(got) == {0, 1, 2, 3}


def test_vpp_wrapper_structure(G):  # vpp_standalone.py:396-432
    left, right = G["vppw_left"], G["vppw_right"]
    lc, rc = oracle.vpp(left, right, np.zeros(left.shape[:2], np.float64))
    assert np.array_equal(lc, G["vppw_lc0"]) and np.array_equal(rc, G["vppw_rc0"])
    assert lc is not left
    lcg, _ = oracle.vpp(left[..., 0], right[..., 0], np.zeros(left.shape[:2], np.float32))
    assert list(lcg.shape) == G["vppw_lcg_shape"].tolist()


def test_guided_metrics(G):  # losses.py:13-24
    m = oracle.guided_metrics(G["gm_disp"], G["gm_gt"], G["gm_valid"])
    got = np.asarray([m['bad 1.0'], m['bad 2.0'], m['bad 3.0'], m['bad 4.0'], m['avgerr'], m['rms']])
    assert np.allclose(got, G["gm_out"], rtol=1e-6, atol=1e-7)


def test_guided_dsi(G):  # rsgm.py:116-127
    for i in range(2):
        got = oracle._guided_dsi(G[f"gdsi{i}_dsi"], G[f"gdsi{i}_hints"], G[f"gdsi{i}_valid"])
        assert got.dtype == np.uint16 and np.array_equal(got, G[f"gdsi{i}_out"]), i
        assert not np.array_equal(got, G[f"gdsi{i}_dsi"])


def test_hint_range_equals_the_reference_wrappers_numpy_statements():
    """vppstereo_amd.vpp_standalone.hint_range replaces `np.count_nonzero(gt) == 0` and `gt[gt > 0].min() / .max()`
    (vpp_standalone.py:407,410-411) by two reductions and one pass over the bit patterns: same early-out, same (dmin, dmax) bit
    for bit, same ValueError when the non-zero hints are all <= 0 or NaN -- over zeros, signed zeros, denormals, negatives,
    infinities, NaNs and random maps."""
    import pytest
    from vppstereo_amd.vpp_standalone import hint_range

    def ref(gt):
        if np.count_nonzero(gt) == 0:
            return (None, None)
        pos = gt[gt > 0]
        return float(pos.min()), float(pos.max())

    rng = np.random.default_rng(5)
    cases = [np.zeros((5, 7), np.float32), np.array([[0, -0.0], [0, 0]], np.float32), np.array([[0, 3.5], [1e-30, 0]], np.float32),
             np.array([[0, -2.0], [0.5, 7]], np.float32), np.array([[np.inf, 2], [0, 0]], np.float32), np.array([[np.nan, 2], [0, 5]], np.float32),
             np.array([[1e-45, 0], [0, 0]], np.float32), np.array([[-np.inf, 1.25]], np.float32), np.full((3, 3), 191.5, np.float32)]
    for _ in range(60):
        a = rng.normal(0, 10, (13, 17)).astype(np.float32)
        a[rng.random(a.shape) < 0.7] = 0
        cases.append(a)
    for c in cases:
        assert hint_range(c) == ref(c), c
    for bad in (np.array([[0, -1.0]], np.float32), np.array([[np.nan, 0]], np.float32), np.array([[-np.inf, -0.0]], np.float32)):
        with pytest.raises(ValueError):
            ref(bad)
        with pytest.raises(ValueError):
            hint_range(bad)
    assert hint_range(np.zeros((0, 4), np.float32)) == (None, None)


def _build_and_load(_):
    import ctypes
    import oracle
    path = oracle.build(force=True)
    return ctypes.CDLL(path).rsgmo_get_simd()


def test_oracle_build_is_safe_when_many_processes_ask_at_once():
    """bench.py's all-cores CPU leg forks one worker per core and each loads the oracle: with a stale library every one of them
    used to run the compiler onto the same file, and some loaded it half written ("file too short").  Now one compiles into a
    file of its own, renamed when complete, and the others wait."""
    import multiprocessing as mp
    with mp.get_context("fork").Pool(6) as pool:
        assert pool.map(_build_and_load, range(6), chunksize=1) == [0] * 6
    assert not [f for f in os.listdir(os.path.dirname(oracle.__file__)) if f.endswith(".tmp")]
