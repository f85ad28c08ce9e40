"""GPU parity of the evaluating frame stream (pipeline.FrameStream(metrics=True) over vppx_fstream_create_eval / _push_eval /
_pop_eval): every popped frame's map equals `run_frame` with seed + f, as tests/test_gpu_stream.py checks for the plain stream,
and its metrics equal -- as bytes -- the standalone metrics call (Engine.guided_metrics) on that map and the frame's ground
truth, which tests/test_gpu_metrics.py holds to the oracle.  The ring carries validgt as one byte per pixel: same numbers."""
import ctypes as C
import os

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu


def _frames(n, H, W, D, seed):
    """(left, right, hints, gt, validgt) with a distinct ground truth and float mask (0, 1, 0.5, -1) per frame."""
    out = []
    for f in range(n):
        fr = synth.make_frame(H, W, D, 0.05, seed=seed + f)
        rng = np.random.default_rng(seed + f)
        gt = (fr["gt"] + rng.normal(0, 1.0, (H, W))).astype(np.float32)
        vgt = rng.choice(np.array([0, 1, 0.5, -1], np.float32), size=(H, W), p=[0.25, 0.45, 0.2, 0.1]).astype(np.float32)
        out.append((fr["left"], fr["right"], fr["hints"], gt, vgt))
    return out


def _valid(h):
    return (h > 0).astype(np.float32)


@pytest.fixture(scope="module")
def eng():
    from vppstereo_amd.engine import Engine
    return Engine()


def _standalone(eng, disp, gt, vgt, s):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)[None]).to(eng.device)
    m = eng.guided_metrics(t(disp), t(gt), t(vgt), gt_scale=s)
    torch.cuda.synchronize()
    return m.cpu().numpy()[0]


def _stream(frames, H, W, batch, seed, D, guided=False, iscale=1, oscale=1, return_disp=True, flush_at=None, **kw):
    from vppstereo_amd.pipeline import FrameStream
    got, recs = [], []
    with FrameStream(H, W, 3, batch=batch, seed=seed, maskocc=True, rsgm_kw=dict(dmax=D), guided=guided, iscale=iscale, oscale=oscale,
                     metrics=True, return_disp=return_disp, **kw) as fs:
        def take():
            r = fs.pop()
            if r is None:
                return False
            got.append(r)
            recs.append(fs.last_metrics_record.copy())
            return True
        for f, (l, r, h, g, v) in enumerate(frames):
            fs.push_eval(l, r, h, validhints=_valid(h) if guided else None, gt=g, validgt=v)
            if f == flush_at:
                fs.flush()
                take()
        fs.flush()
        while take():
            pass
        assert fs.pop() is None and fs.pending == 0
        counts = fs.counts()
    return got, recs, counts


@pytest.mark.parametrize("guided,iscale,oscale", [(False, 1, 1), (True, 1, 1), (False, 2, 1), (False, 2, 2), (True, 2, 2)])
def test_eval_stream_equals_run_frame_and_the_standalone_metrics(eng, guided, iscale, oscale):
    """Two and a half batches of 4 with a flush in the middle (4 + 2 | 4): maps as run_frame, metrics as the standalone call."""
    from vppstereo_amd import pipeline, vpp_standalone
    H, W, D, seed, n = 52, 176, 64, 13, 10
    frames = _frames(n, H, W, D, 400)
    got, recs, _ = _stream(frames, H, W, 4, seed, D, guided=guided, iscale=iscale, oscale=oscale, flush_at=5)
    assert len(got) == n
    for f, (l, r, h, g, v) in enumerate(frames):
        vpp_standalone.init_rand(seed + f)
        want = pipeline.run_frame(l, r, h, maskocc=True, rsgm_kw=dict(dmax=D), validhints=_valid(h) if guided else None, iscale=iscale,
                                  oscale=oscale)
        disp, md = got[f]
        assert disp.shape == want.shape and np.array_equal(disp, want), f
        alone = _standalone(eng, disp, g, v, oscale)
        assert recs[f].tobytes() == alone.tobytes(), (f, recs[f], alone)
        assert list(md) == ['bad 1.0', 'bad 2.0', 'bad 3.0', 'bad 4.0', 'avgerr', 'rms']
        assert [md[k] for k in md] == recs[f][:6].tolist()
        assert recs[f][6] > 0 and np.isfinite(recs[f][:6]).all()
    assert len({r.tobytes() for r in recs}) == n        # distinct ground truths: distinct records


@pytest.mark.parametrize("iscale,oscale", [(1, 1), (2, 2)])
def test_return_disp_false_returns_the_same_metric_bytes(iscale, oscale):
    H, W, D, seed, n = 52, 176, 64, 5, 10
    frames = _frames(n, H, W, D, 600)
    a, ra, _ = _stream(frames, H, W, 4, seed, D, iscale=iscale, oscale=oscale, flush_at=5)
    b, rb, _ = _stream(frames, H, W, 4, seed, D, iscale=iscale, oscale=oscale, flush_at=2, return_disp=False)
    assert len(b) == n and all(isinstance(x, dict) for x in b)
    for f in range(n):
        assert ra[f].tobytes() == rb[f].tobytes(), f
        assert b[f] == a[f][1]


def test_eval_stream_with_patterns_mask_and_batch_sizes():
    """return_patterns with metrics: ((disp, lc, rc, conf), metrics); the records do not depend on the batch size."""
    H, W, D, seed, n = 40, 96, 192, 3, 9
    frames = _frames(n, H, W, D, 800)
    base, rbase, _ = _stream(frames, H, W, 9, seed, D)
    for batch, depth in ((1, 2), (4, 3)):
        got, recs, _ = _stream(frames, H, W, batch, seed, D, return_patterns=True, depth=depth)
        for f in range(n):
            (disp, lc, rc, conf), md = got[f]
            assert np.array_equal(disp, base[f][0]) and lc.shape == (H, W, 3) and conf.shape == (H, W)
            assert recs[f].tobytes() == rbase[f].tobytes(), (batch, f)


def test_eval_stream_reruns_the_metrics_with_a_batch_after_a_lost_lock_step():
    """VPPX_V3_SPIN_LIMIT=1 (the hook tests/test_gpu_stream.py uses) makes the fused aggregation give up: the batch's map is void (NaN)
    and so are the metrics computed behind it; the pop notices, re-runs batch AND metrics: what comes out is finite and right."""
    from vppstereo_amd.pipeline import FrameStream
    H, W, D, n, batch = 40, 96, 192, 20, 8
    frames = _frames(n, H, W, D, 900)
    want, rwant, _ = _stream(frames, H, W, batch, 9, D)
    old = {k: os.environ.get(k) for k in ("VPPX_VERT", "VPPX_V3_SPIN_LIMIT")}
    os.environ["VPPX_VERT"], os.environ["VPPX_V3_SPIN_LIMIT"] = "3", "1"
    try:
        fs = FrameStream(H, W, batch=batch, depth=3, seed=9, maskocc=True, rsgm_kw=dict(dmax=D), metrics=True)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    got, recs = [], []
    with fs:
        for r in fs.run((l, r_, h, None, None, g, v) for l, r_, h, g, v in frames):
            got.append(r)
            recs.append(fs.last_metrics_record.copy())
        assert fs.counts()[3] >= 1 and fs._ctx.lockstep_failures >= 1
    assert len(got) == n
    for f in range(n):
        assert np.array_equal(got[f][0], want[f][0]) and not np.isnan(got[f][0]).any(), f
        assert recs[f].tobytes() == rwant[f].tobytes() and np.isfinite(recs[f]).all(), f


def test_eval_stream_refuses_the_other_push_kinds_and_a_map_it_does_not_have():
    from vppstereo_amd import _lib
    from vppstereo_amd.pipeline import FrameStream
    lib = _lib.load()
    H, W = 32, 64
    l, r, h, g, v = _frames(1, H, W, 64, 1)[0]
    p = lambda a: a.ctypes.data
    d = np.empty((H, W), np.float32)
    got, rec = C.c_int(0), _lib.VppxMetrics()
    with FrameStream(H, W, batch=2, depth=2, rsgm_kw=dict(dmax=64), metrics=True, return_disp=False) as fs:
        with pytest.raises(ValueError, match="push_eval"):
            fs.push(l, r, h)
        with pytest.raises(ValueError, match="gt and validgt"):
            fs.push_eval(l, r, h, gt=g)
        with pytest.raises(ValueError, match="shape"):
            fs.push_eval(l, r, h, gt=g[:-1], validgt=v)
        assert lib.vppx_fstream_push(fs._h, p(l), p(r), p(h), None) == -1 and b"vppx_fstream_push_eval" in lib.vppx_last_error()
        assert lib.vppx_fstream_push_guided(fs._h, p(l), p(r), p(h), None, p(v)) == -1 and b"vppx_fstream_push_eval" in lib.vppx_last_error()
        assert lib.vppx_fstream_push_eval(fs._h, p(l), p(r), p(h), None, p(v), p(g), p(v)) == -1    # validhints on an unguided stream
        assert lib.vppx_fstream_push_eval(fs._h, p(l), p(r), p(h), None, None, p(g), None) == -1    # no validgt
        assert fs.counts()[0] == 0
        fs.push_eval(l, r, h, gt=g, validgt=v)
        fs.flush()
        # VPPX_FS_NO_DISP: the map was not copied out
        assert lib.vppx_fstream_pop(fs._h, p(d), None, None, None, None, C.byref(got)) == -1 and b"VPPX_FS_NO_DISP" in lib.vppx_last_error()
        assert lib.vppx_fstream_pop_eval(fs._h, p(d), None, None, None, None, C.byref(rec), C.byref(got)) == -1
        # the plain pop keeps working on an eval stream (the metrics are simply not returned)
        _lib.check(lib.vppx_fstream_pop(fs._h, None, None, None, None, None, C.byref(got)))
        assert got.value == 1
    with FrameStream(H, W, batch=2, depth=2, rsgm_kw=dict(dmax=64), metrics=True) as fs:
        fs.push_eval(l, r, h, gt=g, validgt=v)
        fs.flush()
        _lib.check(lib.vppx_fstream_pop(fs._h, p(d), None, None, None, None, C.byref(got)))     # plain pop: the map, no metrics
        assert got.value == 1 and np.isfinite(d).all()
    with FrameStream(H, W, batch=2, depth=2, rsgm_kw=dict(dmax=64)) as fs:
        with pytest.raises(ValueError, match="metrics=True"):
            fs.push_eval(l, r, h, gt=g, validgt=v)
        assert lib.vppx_fstream_push_eval(fs._h, p(l), p(r), p(h), None, None, p(g), p(v)) == -1 and b"without VPPX_FS_METRICS" in lib.vppx_last_error()
        fs.push(l, r, h)
        fs.flush()
        assert lib.vppx_fstream_pop_eval(fs._h, p(d), None, None, None, None, C.byref(rec), C.byref(got)) == -1
        _lib.check(lib.vppx_fstream_pop_eval(fs._h, p(d), None, None, None, None, None, C.byref(got)))
        assert got.value == 1
    # creation: the flags go with the entry point, gt_scale with the shape
    vp, rp, ep = _lib.vpp_params(), _lib.rsgm_params(dmax=64), _lib.eval_params(gt_scale=2)
    ctx = _lib.Context()
    hnd = C.c_void_p()
    assert lib.vppx_fstream_create(ctx.handle, None, C.byref(vp), C.byref(rp), 2, 2, H, W, 3, _lib.FS_METRICS, 1, C.byref(hnd)) == -1
    assert lib.vppx_fstream_create_eval(ctx.handle, None, C.byref(vp), C.byref(rp), None, None, 2, 2, H, W, 3, 0, 1, C.byref(hnd)) == -1
    assert lib.vppx_fstream_create_eval(ctx.handle, None, C.byref(vp), C.byref(rp), None, C.byref(ep), 2, 2, H, W, 3, _lib.FS_METRICS, 1,
                                        C.byref(hnd)) == -1 and b"gt_scale 2" in lib.vppx_last_error()
    assert not hnd.value
    ctx.close()
