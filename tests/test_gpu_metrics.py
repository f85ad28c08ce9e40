"""GPU parity of the evaluation metrics (metrics_kernels.hip through vppx_guided_metrics_dev / _host, Engine.guided_metrics and the
evaluating call vppx_occ_vpp_rsgm_eval_dev).  The checker is the CPU oracle (oracle.guided_metrics, pinned to the reference by
tests/test_oracle_glue.py) and, for the error map, the reference's two numpy statements -- never the code under test.

Bound on the two sums.  The oracle adds the same non-negative float32 terms in index order in float64, the kernels add them in a
fixed tree order; each order is within (n - 1) * 2^-53 relative of the exact sum, so the two differ by at most 2 (n - 1) * 2^-53;
the division and the square root add one rounding each on either side: |ours - oracle| <= (2 * n_valid + 4) * 2^-53 * oracle.
Counts (bad 1.0 ... 4.0, n_valid) are integers divided once in float64 on both sides: bit-equal."""
import ctypes as C
import os

import numpy as np
import pytest

import _metrics_ref as MR
import oracle
import synth

pytestmark = pytest.mark.gpu

# the comparison and its bound live in tests/_metrics_ref.py (the sequence tests hold their references to the same ones)
KEYS, _check_record, _numpy_errormap, _same_bits = MR.KEYS, MR.check_record, MR.numpy_errormap, MR.same_bits


def _data(B, H, W, seed):
    rng = np.random.default_rng(seed)
    gt = rng.uniform(0, 190, (B, H, W)).astype(np.float32)
    err = np.where(rng.random((B, H, W)) < 0.7, rng.normal(0, 0.6, (B, H, W)), rng.uniform(-40, 40, (B, H, W)))
    disp = (gt + err).astype(np.float32)
    # the reference's float mask: the test is `> 0`, so 0.5 counts and -1 does not
    valid = rng.choice(np.array([0, 1, 0.5, -1], np.float32), size=(B, H, W), p=[0.3, 0.4, 0.2, 0.1]).astype(np.float32)
    return disp, gt, valid


@pytest.fixture(scope="module")
def eng():
    from vppstereo_amd.engine import Engine
    return Engine()


def _run(eng, disp, gt, valid, gt_scale=1, errormap=False):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    em = torch.full(disp.shape, -7.0, dtype=torch.float32, device=eng.device) if errormap else None
    m = eng.guided_metrics(t(disp), t(gt), t(valid), gt_scale=gt_scale, errormap=em)
    torch.cuda.synchronize()
    assert m.dtype == torch.float64 and tuple(m.shape) == (disp.shape[0], 8)
    return (m.cpu().numpy(), em.cpu().numpy()) if errormap else m.cpu().numpy()


@pytest.mark.parametrize("B", [1, 3, 32])
@pytest.mark.parametrize("H,W", [(1, 1), (7, 13), (375, 1242), (540, 960)])
def test_batches_and_shapes_against_the_oracle(eng, B, H, W):
    disp, gt, valid = _data(B, H, W, seed=1000 * B + H)
    if (H, W) == (1, 1):
        valid[0] = 1
    recs, em = _run(eng, disp, gt, valid, errormap=True)
    for f in range(B):
        _check_record(recs[f], disp[f], gt[f], valid[f], tag=f"B{B} {H}x{W} f{f}")
    assert _same_bits(em, _numpy_errormap(disp, gt, valid))


def test_no_valid_pixel_all_valid_and_the_float_mask(eng):
    disp, gt, valid = _data(4, 37, 53, seed=5)
    valid[0] = 0                    # nothing valid: six NaN, n_valid 0
    valid[1] = 1                    # everything valid
    valid[2] = 0.5                  # > 0: valid
    valid[3] = -1                   # not > 0: invalid (and not == 0: the error map multiplies the error by False)
    recs, em = _run(eng, disp, gt, valid, errormap=True)
    for f in range(4):
        _check_record(recs[f], disp[f], gt[f], valid[f], tag=f"mask f{f}")
    assert np.isnan(recs[0][:6]).all() and recs[0][6] == 0
    assert recs[1][6] == 37 * 53 and recs[2][6] == 37 * 53
    assert np.isnan(recs[3][:6]).all() and recs[3][6] == 0
    assert _same_bits(em, _numpy_errormap(disp, gt, valid))


def test_errors_of_exactly_1_2_3_4_are_not_bad(eng):
    """strict `>`: a pixel whose error is exactly t is not counted by bad t."""
    gt = np.tile(np.arange(16, dtype=np.float32) + 10, (1, 5, 1))          # [1, 5, 16]
    disp = gt.copy()
    for row, t in enumerate((1.0, 2.0, 3.0, 4.0)):
        disp[0, row] += np.float32(t)
    disp[0, 4] += np.float32(4.5)
    valid = np.ones_like(gt)
    recs = _run(eng, disp, gt, valid)
    _check_record(recs[0], disp[0], gt[0], valid[0], tag="exact")
    assert recs[0][:4].tolist() == [4 / 5, 3 / 5, 2 / 5, 1 / 5]


def test_nan_disparities_follow_ieee_like_the_oracle(eng):
    """A voided lock-step call leaves NaN: under a valid pixel the compares are false and the sums NaN; under an invalid one nothing."""
    disp, gt, valid = _data(2, 21, 40, seed=9)
    valid[0, 3, 5], disp[0, 3, 5] = 1, np.nan          # NaN under a valid pixel
    valid[1, 3, 5], disp[1, 3, 5] = 0, np.nan          # NaN under an invalid one
    valid[1, 4, 5], disp[1, 4, 5] = -1, np.nan         # (-1: the error map keeps NaN * False)
    recs, em = _run(eng, disp, gt, valid, errormap=True)
    for f in range(2):
        _check_record(recs[f], disp[f], gt[f], valid[f], tag=f"nan f{f}")
    assert np.isnan(recs[0][4]) and np.isnan(recs[0][5]) and not np.isnan(recs[0][:4]).any()
    assert not np.isnan(recs[1][:6]).any()
    want = _numpy_errormap(disp, gt, valid)
    assert np.isnan(want[0, 3, 5]) and want[1, 3, 5] == 0 and np.isnan(want[1, 4, 5])
    assert _same_bits(em, want)


@pytest.mark.parametrize("s,Hg,Wg", [(2, 375, 1242), (3, 375, 1242), (2, 18, 27), (3, 20, 31)])
def test_gt_scale_decimates_and_divides_the_ground_truth_on_the_device(eng, s, Hg, Wg):
    """test.py:150-152: F.interpolate(nearest, 1 / s) of gt and validgt, gt / s (float32)."""
    Ho, Wo = Hg // s, Wg // s
    _, gt, valid = _data(3, Hg, Wg, seed=s * 100 + Hg)
    rng = np.random.default_rng(4)
    gts = (gt[:, ::s, ::s][:, :Ho, :Wo] / np.float32(s)).astype(np.float32)
    vs = np.ascontiguousarray(valid[:, ::s, ::s][:, :Ho, :Wo])
    disp = (gts + rng.normal(0, 1.5, gts.shape)).astype(np.float32)
    recs, em = _run(eng, disp, gt, valid, gt_scale=s, errormap=True)
    for f in range(3):
        _check_record(recs[f], disp[f], gts[f], vs[f], tag=f"s{s} f{f}")
    assert _same_bits(em, _numpy_errormap(disp, gts, vs))


def test_a_gt_shape_that_gt_scale_does_not_take_to_the_map_is_refused(eng):
    """gt of 375 rows at gt_scale 1 against the 374-row map iscale = 2, oscale = 1 returns: the Python wrapper and the C entry
    points refuse before anything is launched."""
    import torch
    from vppstereo_amd import _lib
    disp = torch.zeros((1, 374, 64), dtype=torch.float32, device=eng.device)
    gt = torch.zeros((1, 375, 64), dtype=torch.float32, device=eng.device)
    with pytest.raises(ValueError, match="374 x 64"):
        eng.guided_metrics(disp, gt, gt)
    with pytest.raises(ValueError, match="go together"):
        eng.guided_metrics(disp, gt, None)
    out = torch.full((1, 8), 5.0, dtype=torch.float64, device=eng.device)
    lib = _lib.load()
    ep = _lib.eval_params()
    rc = lib.vppx_guided_metrics_dev(eng.ctx.handle, C.byref(ep), 1, 374, 64, disp.data_ptr(), 375, 64, gt.data_ptr(), gt.data_ptr(),
                                     out.data_ptr(), None)
    assert rc == -1 and b"374 x 64" in lib.vppx_last_error()
    ep0 = _lib.VppxEvalParams(gt_scale=0)
    rc = lib.vppx_guided_metrics_dev(eng.ctx.handle, C.byref(ep0), 1, 374, 64, disp.data_ptr(), 374, 64, disp.data_ptr(),
                                     disp.data_ptr(), out.data_ptr(), None)
    assert rc == -1 and b"gt_scale" in lib.vppx_last_error()
    h = np.zeros((1, 375, 64), np.float32)
    rec = _lib.VppxMetrics()
    rc = lib.vppx_guided_metrics_host(eng.ctx.handle, None, 1, 374, 64, h.ctypes.data, 375, 64, h.ctypes.data, h.ctypes.data,
                                      C.byref(rec), None)
    assert rc == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 5.0).all()             # nothing was launched
    # the evaluating call: H = 375, iscale 2, oscale 1
    b = synth.make_batch(1, 375, 64, 64, 0.05, seed=2)
    t = lambda a: torch.from_numpy(a).to(eng.device)
    g = t(b["gt"])
    with pytest.raises(ValueError, match="374 x 64"):
        eng.vpp_rsgm(t(b["left"]), t(b["right"]), t(b["hints"]), rsgm_kw=dict(dmax=64), iscale=2, oscale=1, gt=g, validgt=g)
    with pytest.raises(ValueError, match="go together"):
        eng.vpp_rsgm(t(b["left"]), t(b["right"]), t(b["hints"]), rsgm_kw=dict(dmax=64), gt=g)
    vp, rp, sp = _lib.vpp_params(), _lib.rsgm_params(dmax=64), _lib.scale_params(iscale=2, oscale=1)
    d = torch.zeros((1, 374, 64), dtype=torch.float32, device=eng.device)
    rc = lib.vppx_occ_vpp_rsgm_eval_dev(eng.ctx.handle, None, C.byref(vp), C.byref(rp), C.byref(sp), C.byref(ep), 1, 375, 64, 3,
                                        t(b["left"]).data_ptr(), t(b["right"]).data_ptr(), t(b["hints"]).data_ptr(), None, None,
                                        g.data_ptr(), g.data_ptr(), None, None, None, d.data_ptr(), None, out.data_ptr(), None)
    assert rc == -1 and b"374 x 64" in lib.vppx_last_error()


def test_the_references_own_numbers(eng):
    """The committed cases of the reference's float32 results, at the tolerance the oracle itself is held to (test_oracle_glue.py)."""
    here = os.path.dirname(os.path.abspath(__file__))
    G = np.load(os.path.join(here, "golden", "glue_cases.npz"))
    recs = _run(eng, G["gm_disp"][None], G["gm_gt"][None], G["gm_valid"][None])
    assert np.allclose(recs[0][:6], G["gm_out"], rtol=1e-6, atol=1e-7)
    F = np.load(os.path.join(here, "golden", "frontend_cases.npz"))
    recs, em = _run(eng, F["met_disp"][None], F["met_gt"][None], F["met_valid"][None], errormap=True)
    want = [F["met_" + k.replace(" ", "_").replace(".", "p")] for k in KEYS]
    assert np.allclose(recs[0][:6], np.asarray(want, np.float64), rtol=1e-6, atol=1e-7)
    assert _same_bits(em[0], F["met_errormap"])


@pytest.mark.parametrize("H,W", [(540, 960), (375, 1242), (7, 13)])
def test_a_frames_record_does_not_depend_on_its_batch(eng, H, W):
    """As bytes: frame k of a batch of 32 equals the same frame alone (and at another, unaligned place in a batch of 3), and two
    runs of one batch give the same bytes."""
    disp, gt, valid = _data(32, H, W, seed=77)
    a = _run(eng, disp, gt, valid)
    b = _run(eng, disp, gt, valid)
    assert a.tobytes() == b.tobytes()
    for k in (0, 17, 31):
        one = _run(eng, disp[k:k + 1], gt[k:k + 1], valid[k:k + 1])
        assert one[0].tobytes() == a[k].tobytes(), k
    three = _run(eng, disp[16:19], gt[16:19], valid[16:19])
    assert three[1].tobytes() == a[17].tobytes()


def test_host_entry_point_and_run_frame(eng):
    from vppstereo_amd import _lib, pipeline, vpp_standalone
    disp, gt, valid = _data(3, 33, 47, seed=21)
    lib = _lib.load()
    recs = (_lib.VppxMetrics * 3)()
    em = np.empty_like(disp)
    _lib.check(lib.vppx_guided_metrics_host(eng.ctx.handle, None, 3, 33, 47, disp.ctypes.data, 33, 47, gt.ctypes.data,
                                            valid.ctypes.data, recs, em.ctypes.data))
    host = np.frombuffer(bytes(recs), np.float64).reshape(3, 8)
    assert host.tobytes() == _run(eng, disp, gt, valid).tobytes()
    assert _same_bits(em, _numpy_errormap(disp, gt, valid))
    # run_frame: the numpy convenience returns (result as without gt, the reference's dict)
    fr = synth.make_frame(48, 112, 64, 0.05, seed=4)
    vgt = (np.random.default_rng(1).random((48, 112)) < 0.8).astype(np.float32)
    for iscale, oscale in ((1, 1), (2, 2), (2, 1)):
        vpp_standalone.init_rand(5)
        plain = pipeline.run_frame(fr["left"], fr["right"], fr["hints"], maskocc=True, rsgm_kw=dict(dmax=64), iscale=iscale, oscale=oscale)
        vpp_standalone.init_rand(5)
        d, m = pipeline.run_frame(fr["left"], fr["right"], fr["hints"], maskocc=True, rsgm_kw=dict(dmax=64), iscale=iscale, oscale=oscale,
                                  gt=fr["gt"], validgt=vgt, return_errormap=True)
        assert np.array_equal(plain, d)
        assert list(m) == list(KEYS) + ['errormap']
        s = oscale
        gs = (fr["gt"][::s, ::s][:d.shape[0], :d.shape[1]] / np.float32(s)).astype(np.float32)
        vs = np.ascontiguousarray(vgt[::s, ::s][:d.shape[0], :d.shape[1]])
        rec = np.array([m[k] for k in KEYS] + [float((vs > 0).sum()), 0.0])
        _check_record(rec, d, gs, vs, tag=f"run_frame {iscale}/{oscale}")
        assert _same_bits(m['errormap'], _numpy_errormap(d, gs, vs))


# ---- the evaluating call: Engine.vpp_rsgm(..., gt=, validgt=) ----------------------------------------------------------------

def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update({k: str(v) for k, v in env.items()})
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _eval_case(e, B, H, W, D, seed, iscale=1, oscale=1, guided=False, pipelined=False, side_stream=False, repeats=1, want_parts=None,
               want_vert=None):
    """`out` of the evaluating call is bit-equal to the same call without gt; the metrics are within the bound of the oracle on
    out[f] and the ground truth decimated by numpy."""
    import contextlib
    import torch
    b = synth.make_batch(B, H, W, D, 0.05, seed=seed)
    rng = np.random.default_rng(seed)
    vgt = rng.choice(np.array([0, 1, 0.5, -1], np.float32), size=(B, H, W), p=[0.2, 0.5, 0.2, 0.1]).astype(np.float32)
    vh = (b["hints"] > 0).astype(np.float32) if guided else None
    side = torch.cuda.Stream(device=e.device) if side_stream else None
    with torch.cuda.stream(side) if side_stream else contextlib.nullcontext():
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(e.device)
        args = (t(b["left"]), t(b["right"]), t(b["hints"]))
        kw = dict(g_occ="occlusion_heuristic", seed=6, rsgm_kw=dict(dmax=D), validhints=t(vh) if guided else None, iscale=iscale, oscale=oscale)
        tg, tv = t(b["gt"]), t(vgt)
        torch.cuda.current_stream(e.device).synchronize()
        plain = e.vpp_rsgm(*args, **kw).clone()
        torch.cuda.current_stream(e.device).synchronize()
        if want_vert is not None:
            assert e.uses_vert() == want_vert
        results = []
        # repeated calls write the same buffers (graph mode replays only a call with identical pointers)
        out_buf = torch.empty_like(plain)
        m_buf = torch.empty((B, 8), dtype=torch.float64, device=e.device)
        for r in range(repeats):
            ev = None
            if pipelined:
                ev = torch.cuda.Event()
                ev.record()
            out_buf.fill_(-3.0)
            m_buf.fill_(-3.0)
            out, m = e.vpp_rsgm(*args, **kw, gt=tg, validgt=tv, inputs_ready=ev, out=out_buf, metrics_out=m_buf)
            assert out is out_buf and m is m_buf
            if want_parts is not None and r == 0:
                assert e.last_call_parts() > 1, e.last_call_parts()
            results.append((out.clone(), m.clone()))
        torch.cuda.current_stream(e.device).synchronize()
        e.synchronize()
    s = oscale
    for out, m in results:
        assert torch.equal(out, plain)
        o = out.cpu().numpy()
        Ho, Wo = o.shape[1:]
        gs = (b["gt"][:, ::s, ::s][:, :Ho, :Wo] / np.float32(s)).astype(np.float32)
        vs = np.ascontiguousarray(vgt[:, ::s, ::s][:, :Ho, :Wo])
        recs = m.cpu().numpy()
        for f in range(B):
            _check_record(recs[f], o[f], gs[f], vs[f], tag=f"eval B{B} {H}x{W} i{iscale} o{oscale} f{f}")
        # and as bytes the standalone call on the same map
        alone = e.guided_metrics(out, tg, tv, gt_scale=s)
        torch.cuda.synchronize()
        assert alone.cpu().numpy().tobytes() == recs.tobytes()
    return results


def test_eval_call_unguided_on_the_fused_layout():
    from vppstereo_amd.engine import Engine
    _eval_case(Engine(), 8, 80, 192, 192, seed=31, want_vert=3)


def test_eval_call_guided():
    from vppstereo_amd.engine import Engine
    _eval_case(Engine(), 3, 46, 172, 64, seed=32, guided=True)


def test_eval_call_iscale_2_oscale_2_and_iscale_2_oscale_1_on_an_even_shape():
    from vppstereo_amd.engine import Engine
    e = Engine()
    r22 = _eval_case(e, 3, 92, 172, 64, seed=33, iscale=2, oscale=2)
    assert tuple(r22[0][0].shape) == (3, 46, 86)
    r21 = _eval_case(e, 3, 92, 172, 64, seed=33, iscale=2, oscale=1)
    assert tuple(r21[0][0].shape) == (3, 92, 172)
    assert "scale_restore" in e.last_routes()


def test_eval_call_pipelined_with_inputs_ready():
    from vppstereo_amd.engine import Engine
    e = Engine()
    e.set_pipeline(True)
    try:
        _eval_case(e, 4, 60, 150, 64, seed=34, pipelined=True, repeats=3)
        _eval_case(e, 3, 92, 172, 64, seed=35, iscale=2, oscale=1, pipelined=True, repeats=2)
    finally:
        e.set_pipeline(False)


def test_eval_call_on_a_batch_that_runs_in_parts():
    from vppstereo_amd.engine import Engine

    def run():
        _eval_case(Engine(), 7, 46, 172, 64, seed=36, want_parts=True)
    _with_env({"VPPX_CHUNK": 3}, run)


def test_eval_call_in_graph_mode_on_a_side_stream():
    from vppstereo_amd.engine import Engine
    e = Engine()
    e.set_graph_mode(True)
    try:
        r0 = e.graph_replays()
        _eval_case(e, 2, 60, 112, 64, seed=37, side_stream=True, repeats=4)
        assert e.graph_replays() - r0 >= 2          # the metrics were captured with the rest and replayed
    finally:
        e.set_graph_mode(False)
