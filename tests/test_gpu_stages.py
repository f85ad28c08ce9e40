"""The three fused kernels of the hot path that have no pyrSGM-style stage of their own, each through a stage entry that
queues the very launch compute_rsgm makes, each against the oracle's own pieces, bit for bit:

  pad_gray_census_kernel    Engine.rsgm_front        vs pad_reflect -> rgb2gray -> census5x5_SSE
  median_interp_clip_kernel Engine.rsgm_mid          vs median3x3_SSE -> _linear_interpolate(., 15, 3) -> clip
  guided_rows_kernel        Engine.rsgm_guided_rows  vs costMeasureCensus5x5_xyd_SSE -> _guided_dsi

Behind these kernels the whole call runs the left/right check, the speckle filter and the background fill, which erase or
overwrite most of what a wrong census code or a wrong interpolated value would change: the final map is a weak witness.
The inputs come from tests/_stage_inputs.py, whose builders assert on the oracle's intermediates that every case reaches the
code it names (checked without a GPU by tests/test_stage_inputs_cpu.py).  Integers are exact and the floats are the same
IEEE operations on both sides: np.array_equal everywhere."""
import ctypes as C

import numpy as np
import pytest

import _stage_inputs as si

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    from vppstereo_amd.engine import Engine
    assert torch.cuda.is_available()
    return Engine()


def _dev(eng, a):
    import torch
    return torch.from_numpy(np.array(a)).to(eng.device)   # (a copy: the cases are read-only)


def _where(got, ref):
    """Where two maps differ, for the message of a failed comparison: count, first indices, bounding box."""
    bad = np.argwhere(got != ref)
    return dict(n=len(bad), first=bad[:4].tolist(), lo=bad.min(0).tolist(), hi=bad.max(0).tolist()) if len(bad) else None


# ------------------------------------------------------------------------------------------------------------------ front
@pytest.mark.parametrize("H,W,C,B", si.front_cases())
def test_front_stage_equals_pad_gray_census_of_the_oracle(eng, H, W, C, B):
    """blockIdx.z of the launch is image set * B + frame: three distinct images, so that a swapped set or frame shows."""
    for kind in si.front_kinds(C):
        c = si.front_case(H, W, C, B, kind)
        gray, cl, cr = eng.rsgm_front(_dev(eng, c["left"]), _dev(eng, c["left_vpp"]), _dev(eng, c["right_vpp"]))
        gray, cl, cr = gray.cpu().numpy(), cl.cpu().numpy(), cr.cpu().numpy()
        assert gray.dtype == np.uint8 and cl.dtype == np.uint32 and cr.dtype == np.uint32
        assert np.array_equal(gray, c["gray_left"]), (kind, _where(gray, c["gray_left"]))
        assert np.array_equal(cl, c["census_l"]), (kind, _where(cl, c["census_l"]))
        assert np.array_equal(cr, c["census_r"]), (kind, _where(cr, c["census_r"]))


# -------------------------------------------------------------------------------------------------------------------- mid
@pytest.mark.parametrize("Hp,Wp,B", si.mid_cases())
def test_mid_stage_equals_median_interpolate_clip_of_the_oracle(eng, Hp, Wp, B):
    c = si.mid_case(Hp, Wp, B)
    dl, dr = _dev(eng, c["disp_l"]), _dev(eng, c["disp_r"])
    ol, o_r = eng.rsgm_mid(dl, dr)
    ol, o_r = ol.cpu().numpy(), o_r.cpu().numpy()
    assert np.array_equal(ol, c["ref_l"]), _where(ol, c["ref_l"])
    assert np.array_equal(o_r, c["ref_r"]), _where(o_r, c["ref_r"])
    assert np.array_equal(dl.cpu().numpy(), c["disp_l"]) and np.array_equal(dr.cpu().numpy(), c["disp_r"])   # inputs untouched


# ----------------------------------------------------------------------------------------------------------------- guided
@pytest.mark.parametrize("H,W,D,B,density", si.guided_cases())
def test_guided_rows_stage_equals_guided_dsi_of_the_oracle(eng, H, W, D, B, density):
    import torch
    c = si.guided_case(H, W, D, B, density)
    n, owner = c["n"], c["owner"]
    gmap, rows, count = eng.rsgm_guided_rows(_dev(eng, c["census_l"]), _dev(eng, c["census_r"]), _dev(eng, c["hints"]),
                                             _dev(eng, c["validhints"]), D)
    assert rows.shape == (B * H * W, D) and rows.dtype == torch.uint16
    gmap, rows, count = gmap.cpu().numpy(), rows.cpu().numpy(), count.cpu().numpy()
    assert int(count[0]) == n
    assert np.array_equal(gmap >= 0, owner), _where(gmap >= 0, owner)     # the hint pixels, shifted by the pad
    assert (gmap[~owner] == -1).all()                                      # padding pixels among them
    idx = gmap[owner]                                                      # raster order, as ref_rows
    assert np.array_equal(np.sort(idx), np.arange(n))                      # a permutation of 0 .. n-1
    got = rows[idx]
    assert np.array_equal(got, c["ref_rows"]), _where(got, c["ref_rows"])


# ---------------------------------------------------------------------------------------------- stage entry = the pipeline
def test_stage_entries_and_the_whole_call_are_one_pipeline(eng):
    """Once on real WTA output: the oracle's raw WTA + sub-pixel maps through rsgm_mid are compute_rsgm's padded maps; those
    through rsgm_post are its final map; and eng.rsgm on the same frames gives that map too."""
    c = si.tie_case()
    H, W, D = si.TIE["H"], si.TIE["W"], si.TIE["D"]
    ol, o_r = eng.rsgm_mid(_dev(eng, c["raw_l"]), _dev(eng, c["raw_r"]))
    assert np.array_equal(ol.cpu().numpy(), c["pad_l"]), _where(ol.cpu().numpy(), c["pad_l"])
    assert np.array_equal(o_r.cpu().numpy(), c["pad_r"]), _where(o_r.cpu().numpy(), c["pad_r"])
    post = eng.rsgm_post(_dev(eng, c["pad_l"]), _dev(eng, c["pad_r"]), H, W).cpu().numpy()
    whole = eng.rsgm(_dev(eng, c["left"]), _dev(eng, c["left_vpp"]), _dev(eng, c["right_vpp"]), dmax=D).cpu().numpy()
    assert np.array_equal(post, c["final"]), _where(post, c["final"])
    assert np.array_equal(whole, c["final"]), _where(whole, c["final"])
    assert np.array_equal(post, whole)


# ------------------------------------------------------------------------------------------------------ the entries' manners
def test_stage_entries_leave_the_route_lists_alone(eng):
    """Like vppx_rsgm_post_dev: a stage call neither clears nor extends what the last whole call recorded."""
    c = si.tie_case()
    eng.rsgm(_dev(eng, c["left"]), _dev(eng, c["left_vpp"]), _dev(eng, c["right_vpp"]), dmax=si.TIE["D"])
    before = (eng.last_routes(), eng.last_front_routes())
    assert before[0]
    f = si.front_case(16, 16, 1, 1, "random")
    eng.rsgm_front(_dev(eng, f["left"]), _dev(eng, f["left_vpp"]), _dev(eng, f["right_vpp"]))
    m = si.mid_case(16, 16, 1)
    eng.rsgm_mid(_dev(eng, m["disp_l"]), _dev(eng, m["disp_r"]))
    g = si.guided_case(24, 48, 8, 1, 5)
    eng.rsgm_guided_rows(_dev(eng, g["census_l"]), _dev(eng, g["census_r"]), _dev(eng, g["hints"]), _dev(eng, g["validhints"]), 8)
    assert (eng.last_routes(), eng.last_front_routes()) == before


def test_stage_entries_refuse_bad_arguments_before_they_launch(eng):
    """Host-side argument checks: NULL pointers, maps that are no multiple of 16, a bad dmax, a bad channel count."""
    import torch
    from vppstereo_amd import _lib
    lib, h = eng.lib, eng.ctx.handle
    buf = torch.zeros(64 * 64 * 8, dtype=torch.int32, device=eng.device)
    p, null = C.c_void_p(buf.data_ptr()), None

    def code(rc):
        with pytest.raises(_lib.VppxError) as e:
            _lib.check(rc)
        return e.value.code

    for k in range(6):
        a = [p] * 6
        a[k] = null
        assert code(lib.vppx_rsgm_front_dev(h, 1, 16, 16, 1, *a)) == -1
    for k in range(7):
        a = [p] * 7
        a[k] = null
        assert code(lib.vppx_rsgm_guided_rows_dev(h, 1, 16, 16, 8, *a)) == -1
    for k in range(4):
        a = [p] * 4
        a[k] = null
        assert code(lib.vppx_rsgm_mid_dev(h, 1, 16, 16, *a)) == -1
    assert code(lib.vppx_rsgm_front_dev(h, 1, 16, 16, 2, p, p, p, p, p, p)) == -1
    assert code(lib.vppx_rsgm_front_dev(h, 1, 4, 16, 1, p, p, p, p, p, p)) == -1
    assert code(lib.vppx_rsgm_front_dev(h, 0, 16, 16, 1, p, p, p, p, p, p)) == -1
    for Hp, Wp in ((16, 24), (24, 16), (0, 16), (16, 0), (16, 8), (17, 32)):
        assert code(lib.vppx_rsgm_mid_dev(h, 1, Hp, Wp, p, p, p, p)) == -1
    assert code(lib.vppx_rsgm_mid_dev(h, 0, 16, 16, p, p, p, p)) == -1
    assert code(lib.vppx_rsgm_guided_rows_dev(h, 1, 16, 16, 12, p, p, p, p, p, p, p)) == -2    # dmax % 8
    assert code(lib.vppx_rsgm_guided_rows_dev(h, 1, 16, 16, 264, p, p, p, p, p, p, p)) == -3   # dmax > 256
    assert code(lib.vppx_rsgm_guided_rows_dev(h, 1, 16, 16, 0, p, p, p, p, p, p, p)) == -1
    assert code(lib.vppx_rsgm_guided_rows_dev(h, 1, 3, 16, 8, p, p, p, p, p, p, p)) == -1
    torch.cuda.synchronize()
    assert not buf.any()     # nothing was launched
