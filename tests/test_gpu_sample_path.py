"""GPU parity of the whole path on hints sampled on the device: `Engine.vpp_rsgm(sample=...)` (vppx_occ_vpp_rsgm_sampled_dev),
`pipeline.run_frame(sample=...)`, `FrameStream(sample=...)` (vppx_fstream_create_sampled / _push_sampled) and the same stream
from plain C.  The oracle for the hints is torch on the CPU (``torch.manual_seed(s + f); losses.sample_hints``); everything
behind the hints is the existing call on those hints, which the other test files hold to the reference: the sampled call must
return the same bytes -- disparities, metrics records and the sampled maps themselves."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import synth
from vppstereo_amd import losses

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 64
P = 0.05


@pytest.fixture(scope="module")
def eng():
    from vppstereo_amd.engine import Engine
    return Engine()


def oracle(src, valid, p, seed):
    hs, vs = [], []
    for f in range(src.shape[0]):
        torch.manual_seed(int(seed) + f)
        h, v = losses.sample_hints(torch.from_numpy(np.array(src[f])), torch.from_numpy(np.array(valid[f])) > 0, p)
        hs.append(h.numpy())
        vs.append(v.numpy())
    return np.stack(hs), np.stack(vs)


_BATCHES = {}


def batch(B, H, W):
    """left, right, gt, validgt (a float mask of 0, 1, 0.5, -1) and a `raw` source pair distinct from the ground truth; made once."""
    key = (B, H, W)
    if key not in _BATCHES:
        b = synth.make_batch(B, H, W, D, 0.05, seed=900 + B)
        rng = np.random.default_rng(B * 1000 + H)
        b["validgt"] = rng.choice(np.array([0, 1, 0.5, -1], np.float32), size=(B, H, W), p=[0.2, 0.5, 0.2, 0.1]).astype(np.float32)
        b["gt"] = np.ascontiguousarray(b["gt"], np.float32)
        b["raw"] = (b["gt"] + rng.normal(0, 0.5, (B, H, W))).astype(np.float32).clip(0.5, D - 2)
        b["validraw"] = (rng.random((B, H, W)) < 0.6).astype(np.float32)
        for k in b:
            b[k].setflags(write=False)
        _BATCHES[key] = b
    return _BATCHES[key]


def T(eng, a):
    return torch.from_numpy(np.array(a)).to(eng.device)


MODES = {
    "plain": dict(),
    "guided": dict(guided=True),
    "maskocc": dict(g_occ="occlusion_heuristic"),
    "scaled": dict(iscale=2, oscale=2),
    "eval": dict(evaluate=True),
    "guided_eval_scaled": dict(guided=True, evaluate=True, iscale=2, oscale=2, g_occ="occlusion_heuristic"),
}


def both_calls(eng, b, mode, src_key="raw", sample_seed=2 ** 32 - 2, p=P, src_none=False):
    """(sampled call, the same call on the oracle's hints), each (disp, metrics or None), and the sampled maps."""
    m = dict(MODES[mode])
    guided, evaluate = m.pop("guided", False), m.pop("evaluate", False) or src_none
    B, H, W = b["gt"].shape
    l, r = T(eng, b["left"]), T(eng, b["right"])
    src, vsrc = (b["gt"], b["validgt"]) if src_none else (b[src_key], b["valid" + src_key])
    kw = dict(seed=3, rsgm_kw=dict(dmax=D), **m)
    if evaluate:
        kw.update(gt=T(eng, b["gt"]), validgt=T(eng, b["validgt"]))
    ho, vo = torch.empty((B, H, W), dtype=torch.float32, device=eng.device), torch.empty((B, H, W), dtype=torch.float32, device=eng.device)
    smp = dict(probability=p, seed=sample_seed, guided=guided, hints_out=ho, validhints_out=vo)
    if not src_none:
        smp.update(src=T(eng, src), validsrc=T(eng, vsrc))
    got = eng.vpp_rsgm(l, r, sample=smp, **kw)
    eng.synchronize()
    wh, wv = oracle(src, vsrc, p, sample_seed)
    want = eng.vpp_rsgm(l, r, T(eng, wh), validhints=T(eng, wv) if guided else None, **kw)
    eng.synchronize()
    split = lambda x: (x[0].cpu(), x[1].cpu()) if evaluate else (x.cpu(), None)
    return split(got), split(want), (ho.cpu().numpy(), vo.cpu().numpy()), (wh, wv)


@pytest.mark.parametrize("B,H,W", [(1, 48, 80), (3, 40, 136), (5, 48, 80)])
@pytest.mark.parametrize("mode", list(MODES))
def test_sampled_call_equals_the_call_on_the_oracles_hints(eng, mode, B, H, W):
    (gd, gm), (wd, wm), (ho, vo), (wh, wv) = both_calls(eng, batch(B, H, W), mode)
    assert np.array_equal(ho, wh) and np.array_equal(vo, wv) and 0 < wv.sum() < wv.size
    assert gd.shape == wd.shape and torch.equal(gd, wd)
    if gm is not None:
        assert gm.numpy().tobytes() == wm.numpy().tobytes() and np.isfinite(gm.numpy()[:, :6]).all()


def test_a_guided_sampled_batch_that_runs_in_parts():
    """VPPX_GUIDED_PART_MB (read when the context is created) makes five small guided frames run as three parts: the batch is
    sampled once, in front of them, frame f with seed + f."""
    from vppstereo_amd.engine import Engine
    old = os.environ.get("VPPX_GUIDED_PART_MB")
    os.environ["VPPX_GUIDED_PART_MB"] = "8"
    try:
        e = Engine()
    finally:
        os.environ.pop("VPPX_GUIDED_PART_MB", None) if old is None else os.environ.__setitem__("VPPX_GUIDED_PART_MB", old)
    (gd, _), (wd, _), (ho, vo), (wh, wv) = both_calls(e, batch(5, 48, 80), "guided")
    assert e.last_call_parts() > 1
    assert np.array_equal(ho, wh) and np.array_equal(vo, wv) and torch.equal(gd, wd)


def test_src_none_samples_the_ground_truth(eng):
    b = batch(3, 40, 136)
    (gd, gm), (wd, wm), (ho, vo), (wh, wv) = both_calls(eng, b, "plain", src_none=True)
    assert np.array_equal(ho, wh) and np.array_equal(vo, wv) and torch.equal(gd, wd) and gm.numpy().tobytes() == wm.numpy().tobytes()
    assert np.array_equal(ho[vo > 0], b["gt"][vo > 0]) and not (vo > 0)[~(b["validgt"] > 0)].any()
    l, r = T(eng, b["left"]), T(eng, b["right"])
    with pytest.raises(ValueError, match="gt / validgt"):
        eng.vpp_rsgm(l, r, sample=dict(probability=P))
    with pytest.raises(ValueError, match="hints=None"):
        eng.vpp_rsgm(l, r, T(eng, b["gt"]), sample=dict(probability=P, src=T(eng, b["gt"]), validsrc=T(eng, b["validgt"])))
    with pytest.raises(ValueError, match="sample=dict"):
        eng.vpp_rsgm(l, r)


def test_probability_zero_is_the_call_without_hints(eng):
    b = batch(3, 40, 136)
    (gd, _), (wd, _), (ho, vo), _ = both_calls(eng, b, "plain", p=0.0)
    assert not ho.any() and not vo.any() and torch.equal(gd, wd)


def test_pipelined_calls_alternate_their_sampled_maps():
    """Engine.set_pipeline: the sampling is the first kernel of the front stage and consecutive calls write two sets of maps in turn.
    Four calls queued without a synchronisation in between, each with its own seed and outputs, equal the unpipelined calls."""
    from vppstereo_amd.engine import Engine
    b = batch(3, 40, 136)
    plain, piped = Engine(), Engine()
    res = {e: (T(e, b["raw"]), T(e, b["validraw"])) for e in (plain, piped)}     # resident inputs: they outlive the queued calls
    args = lambda e, s, ho: dict(seed=3, rsgm_kw=dict(dmax=D), g_occ="occlusion_heuristic",
                                 sample=dict(probability=P, seed=s, src=res[e][0], validsrc=res[e][1], guided=s % 2 == 1, hints_out=ho))
    want = []
    for s in (10, 11, 12, 13):
        ho = torch.empty((3, 40, 136), dtype=torch.float32, device=plain.device)
        d = plain.vpp_rsgm(T(plain, b["left"]), T(plain, b["right"]), **args(plain, s, ho))
        plain.synchronize()
        want.append((d.cpu(), ho.cpu()))
    piped.set_pipeline(True)
    l, r = T(piped, b["left"]), T(piped, b["right"])
    got = []
    for s in (10, 11, 12, 13):
        ho = torch.empty((3, 40, 136), dtype=torch.float32, device=piped.device)
        got.append((piped.vpp_rsgm(l, r, **args(piped, s, ho)), ho))
    piped.synchronize()
    for (gd, gh), (wd, wh) in zip(got, want):
        assert torch.equal(gd.cpu(), wd) and torch.equal(gh.cpu(), wh)
    assert len({w[1].numpy().tobytes() for w in want}) == 4
    piped.set_pipeline(False)


def test_library_refuses_bad_arguments_before_it_launches(eng):
    from vppstereo_amd import _lib
    b = batch(1, 48, 80)
    l, r, g, v = T(eng, b["left"]), T(eng, b["right"]), T(eng, b["gt"]), T(eng, b["validgt"])
    out = torch.full((1, 48, 80), 5.0, dtype=torch.float32, device=eng.device)
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
    vp, rp, smp = _lib.vpp_params(), _lib.rsgm_params(dmax=D), _lib.sample_params()
    eng._bind_stream()

    def call(smp_=smp, B=1, H=48, W=80, src=g, vsrc=v, gt=None, vgt=None, disp=out, met=None):
        return eng.lib.vppx_occ_vpp_rsgm_sampled_dev(eng.ctx.handle, None, C.byref(vp), C.byref(rp), None, None,
                                                     C.byref(smp_) if smp_ is not None else None, B, H, W, 3, p(l), p(r), p(src), p(vsrc), 0,
                                                     None, p(gt), p(vgt), None, None, None, p(disp), None, p(met), None, None, None)
    for kw in (dict(smp_=None), dict(B=0), dict(H=0), dict(W=-16), dict(vsrc=None), dict(src=None, vsrc=None), dict(disp=None),
               dict(gt=g), dict(gt=g, vgt=v)):
        assert call(**kw) == -1 and eng.lib.vppx_last_error(), kw
    eng.synchronize()
    assert bool((out == 5.0).all())
    assert call() == 0
    eng.synchronize()
    assert not bool((out == 5.0).all())


def test_run_frame_equals_the_batched_call(eng):
    from vppstereo_amd import pipeline, vpp_standalone
    b = batch(3, 40, 136)
    for guided in (False, True):
        (gd, gm), _, _, _ = both_calls(eng, b, "guided_eval_scaled" if guided else "eval", sample_seed=40)
        for f in range(3):
            vpp_standalone.init_rand(3 + f)
            kw = dict(maskocc=True, iscale=2, oscale=2) if guided else {}
            disp, md = pipeline.run_frame(b["left"][f], b["right"][f], rsgm_kw=dict(dmax=D), gt=b["gt"][f], validgt=b["validgt"][f],
                                          sample=dict(probability=P, seed=40 + f, src=b["raw"][f], validsrc=b["validraw"][f], guided=guided), **kw)
            assert np.array_equal(disp, gd[f].numpy()), (guided, f)
            assert [md[k] for k in md] == gm[f].numpy()[:6].tolist()
    # src=None: the frame's own gt
    (gd, _), _, _, _ = both_calls(eng, b, "plain", sample_seed=7, src_none=True)
    vpp_standalone.init_rand(3)
    disp, _ = pipeline.run_frame(b["left"][0], b["right"][0], rsgm_kw=dict(dmax=D), gt=b["gt"][0], validgt=b["validgt"][0],
                                 sample=dict(probability=P, seed=7))
    assert np.array_equal(disp, gd[0].numpy())


def _frames(n, H, W):
    b = batch(5, H, W)
    return [(b["left"][f % 5], b["right"][f % 5], np.roll(b["gt"][f % 5], f // 5, 0), np.roll(b["validgt"][f % 5], f // 5, 1),
             np.roll(b["raw"][f % 5], f // 5, 0), b["validraw"][f % 5]) for f in range(n)]


def _want_frame(fr, f, seed, sseed, with_src, guided=False, scale=1):
    from vppstereo_amd import pipeline, vpp_standalone
    l, r, g, v, raw, vraw = fr
    vpp_standalone.init_rand(seed + f)
    smp = dict(probability=P, seed=sseed + f, guided=guided)
    if with_src:
        smp.update(src=raw, validsrc=vraw)
    return pipeline.run_frame(l, r, maskocc=True, rsgm_kw=dict(dmax=D), gt=g, validgt=v, sample=smp, iscale=scale, oscale=scale)


def test_sampling_eval_stream_equals_run_frame_whatever_the_batch_size():
    """2.5 batches with a flush in the middle, two batch sizes, src=None (sampled from the gt in the ring): frame f equals run_frame
    with init_rand(seed + f) and sampling seed sample_seed + f; return_disp=False returns the same records."""
    from vppstereo_amd.pipeline import FrameStream
    H, W, n, seed, sseed = 48, 80, 10, 13, 2 ** 32 - 4
    frames = _frames(n, H, W)
    want = [_want_frame(fr, f, seed, sseed, False) for f, fr in enumerate(frames)]
    recs = {}
    for bs, flush_at in ((4, 5), (3, 1)):
        got = []
        with FrameStream(H, W, 3, batch=bs, seed=seed, maskocc=True, rsgm_kw=dict(dmax=D), metrics=True, sample=P, sample_seed=sseed) as fs:
            rr = []

            def take():
                r = fs.pop()
                if r is not None:
                    got.append(r)
                    rr.append(fs.last_metrics_record.copy())
                return r is not None
            for f, (l, r, g, v, _, _) in enumerate(frames):
                fs.push_sampled(l, r, gt=g, validgt=v)
                if f == flush_at:
                    fs.flush()
                    take()
            fs.flush()
            while take():
                pass
            assert fs.pending == 0
        recs[bs] = rr
        assert len(got) == n
        for f in range(n):
            assert np.array_equal(got[f][0], want[f][0]), (bs, f)
            assert got[f][1] == want[f][1], (bs, f)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(recs[4], recs[3]))
    assert len({w[0].tobytes() for w in want}) == n
    with FrameStream(H, W, 3, batch=4, seed=seed, maskocc=True, rsgm_kw=dict(dmax=D), metrics=True, sample=P, sample_seed=sseed,
                     return_disp=False) as fs:
        mds = list(fs.run((l, r, None, None, None, g, v) for l, r, g, v, _, _ in frames))
    assert mds == [w[1] for w in want]


def test_sampling_stream_with_src_mixed_with_gt_frames_and_guided():
    """An evaluating stream whose frames bring src / validsrc, some of them none (a batch samples from one kind of source: the
    stream starts a new one where the kind changes); then the same guided, and with --iscale 2 --oscale 2 (the sampling in front of
    the resize in the pipelined front stage); sample_seed=None is the stream's seed."""
    from vppstereo_amd.pipeline import FrameStream
    H, W, n, seed = 40, 136, 7, 21
    frames = _frames(n, H, W)
    with_src = [True, True, False, False, False, True, True]
    for guided, scale in ((False, 1), (True, 1), (False, 2)):
        want = [_want_frame(fr, f, seed, seed, with_src[f], guided, scale) for f, fr in enumerate(frames)]
        with FrameStream(H, W, 3, batch=3, seed=seed, maskocc=True, rsgm_kw=dict(dmax=D), metrics=True, sample=P, guided=guided,
                         iscale=scale, oscale=scale) as fs:
            got = list(fs.run((l, r, None, raw if s else None, vraw if s else None, g, v) for (l, r, g, v, raw, vraw), s in zip(frames, with_src)))
        assert len(got) == n
        for f in range(n):
            assert np.array_equal(got[f][0], want[f][0]) and got[f][1] == want[f][1], (guided, scale, f)


def test_non_evaluating_sampling_stream_with_src():
    from vppstereo_amd import pipeline, vpp_standalone
    H, W, n, seed, sseed = 48, 80, 6, 5, 77
    frames = _frames(n, H, W)
    with pipeline.FrameStream(H, W, 3, batch=4, seed=seed, rsgm_kw=dict(dmax=D), sample=P, sample_seed=sseed) as fs:
        got = list(fs.run((l, r, None, raw, vraw) for l, r, _, _, raw, vraw in frames))
    assert len(got) == n
    for f, (l, r, _, _, raw, vraw) in enumerate(frames):
        vpp_standalone.init_rand(seed + f)
        want = pipeline.run_frame(l, r, rsgm_kw=dict(dmax=D), sample=dict(probability=P, seed=sseed + f, src=raw, validsrc=vraw))
        assert np.array_equal(got[f], want), f


def test_wrong_push_calls_are_refused():
    from vppstereo_amd import _lib
    from vppstereo_amd.pipeline import FrameStream
    lib = _lib.load()
    H, W = 48, 80
    l, r, g, v, raw, vraw = _frames(1, H, W)[0]
    p = lambda a: a.ctypes.data
    with FrameStream(H, W, batch=2, depth=2, rsgm_kw=dict(dmax=D), metrics=True, sample=P) as fs:
        with pytest.raises(ValueError, match="push_sampled"):
            fs.push(l, r, g)
        with pytest.raises(ValueError, match="push_sampled"):
            fs.push_eval(l, r, g, gt=g, validgt=v)
        with pytest.raises(ValueError, match="gt and validgt"):
            fs.push_sampled(l, r, src=raw, validsrc=vraw)
        assert lib.vppx_fstream_push(fs._h, p(l), p(r), p(g), None) == -1 and b"vppx_fstream_push_sampled" in lib.vppx_last_error()
        assert lib.vppx_fstream_push_guided(fs._h, p(l), p(r), p(g), None, p(v)) == -1 and b"vppx_fstream_push_sampled" in lib.vppx_last_error()
        assert lib.vppx_fstream_push_eval(fs._h, p(l), p(r), p(g), None, None, p(g), p(v)) == -1 and b"vppx_fstream_push_sampled" in lib.vppx_last_error()
        assert lib.vppx_fstream_push_sampled(fs._h, p(l), p(r), None, p(raw), None, p(g), p(v)) == -1 and b"go together" in lib.vppx_last_error()
        assert lib.vppx_fstream_push_sampled(fs._h, p(l), p(r), None, None, None, None, None) == -1
        assert fs.counts()[0] == 0
        fs.push_sampled(l, r, gt=g, validgt=v)
        fs.flush()
        assert fs.pop() is not None
    with FrameStream(H, W, batch=2, depth=2, rsgm_kw=dict(dmax=D), sample=P) as fs:     # not evaluating: there is no gt to sample from
        assert lib.vppx_fstream_push_sampled(fs._h, p(l), p(r), None, None, None, None, None) == -1 and b"VPPX_FS_METRICS" in lib.vppx_last_error()
        assert lib.vppx_fstream_push_sampled(fs._h, p(l), p(r), None, p(raw), p(vraw), p(g), p(v)) == -1
        assert fs.counts()[0] == 0
    with FrameStream(H, W, batch=2, depth=2, rsgm_kw=dict(dmax=D), metrics=True) as fs:
        with pytest.raises(ValueError, match="without sample="):
            fs.push_sampled(l, r, gt=g, validgt=v)
        assert lib.vppx_fstream_push_sampled(fs._h, p(l), p(r), None, None, None, p(g), p(v)) == -1 and b"without VPPX_FS_SAMPLE" in lib.vppx_last_error()
        assert fs.counts()[0] == 0
    # creation: the flag goes with the entry point
    vp, rp, ep, smp = _lib.vpp_params(), _lib.rsgm_params(dmax=D), _lib.eval_params(), _lib.sample_params()
    ctx = _lib.Context()
    hnd = C.c_void_p()
    assert lib.vppx_fstream_create(ctx.handle, None, C.byref(vp), C.byref(rp), 2, 2, H, W, 3, _lib.FS_SAMPLE, 1, C.byref(hnd)) == -1
    assert lib.vppx_fstream_create_eval(ctx.handle, None, C.byref(vp), C.byref(rp), None, C.byref(ep), 2, 2, H, W, 3,
                                        _lib.FS_METRICS | _lib.FS_SAMPLE, 1, C.byref(hnd)) == -1
    assert lib.vppx_fstream_create_sampled(ctx.handle, None, C.byref(vp), C.byref(rp), None, None, C.byref(smp), 2, 2, H, W, 3, 0, 1,
                                           C.byref(hnd)) == -1
    assert lib.vppx_fstream_create_sampled(ctx.handle, None, C.byref(vp), C.byref(rp), None, None, None, 2, 2, H, W, 3, _lib.FS_SAMPLE, 1,
                                           C.byref(hnd)) == -1
    assert lib.vppx_fstream_create_sampled(ctx.handle, None, C.byref(vp), C.byref(rp), None, None, C.byref(smp), 2, 2, H, W, 3,
                                           _lib.FS_SAMPLE | _lib.FS_METRICS, 1, C.byref(hnd)) == -1      # METRICS without ep
    assert not hnd.value
    ctx.close()


def _fnv1a(b):
    h = 1469598103934665603
    for v in b:
        h = ((h ^ v) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_c_program_pushes_sampled_frames_and_gets_the_python_streams_results(tmp_path):
    from test_cabi_c import _lcg_frames
    from test_cabi_eval_c import _lcg_gt
    from vppstereo_amd.pipeline import FrameStream
    libdir = os.path.join(ROOT, "vppstereo_amd")
    exe = str(tmp_path / "fstream_sample_demo")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "fstream_sample_demo.c"), "-o", exe, "-L", libdir, "-lvppx", "-Wl,-rpath," + libdir])
    n, H, W, batch, seed, sseed, p = 7, 24, 48, 3, 11, 4294967293, 0.25
    r = subprocess.run([exe, str(n), str(H), str(W), str(D), str(batch), str(seed), str(sseed), repr(p)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
    got = [line.split() for line in r.stdout.strip().splitlines()]
    assert [int(g[0]) for g in got] == list(range(n))
    frames, gts = _lcg_frames(n, H, W), _lcg_gt(n, H, W)
    with FrameStream(H, W, 3, batch=batch, seed=seed, maskocc=True, rsgm_kw=dict(dmax=D), metrics=True, sample=p, sample_seed=sseed) as fs:
        for f, (disp, md) in enumerate(fs.run((l, r_, None, None, None, g, v) for (l, r_, _), (g, v) in zip(frames, gts))):
            assert int(got[f][1], 16) == _fnv1a(disp.tobytes()), f
            words = np.array([int(w, 16) for w in got[f][2:10]], np.uint64)
            assert words.tobytes() == fs.last_metrics_record.tobytes(), f
    assert len({g[1] for g in got}) > 1
