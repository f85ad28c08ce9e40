"""--iscale / --oscale on the device path (test.py:136-148, :154, :247-248), bit for bit.  The yardstick of every case is the
composition of the numpy restatement of the resize (tests/_scale_ref.py, DESIGN section 5 rule 1), torch on the CPU for the hint
decimation and the restore (the reference's own expressions), and the CPU oracle's occlusion_heuristic / init_rand / vpp /
compute_rsgm at the scaled shape."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import oracle
import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _scale_ref as ref  # noqa: E402


def _valid(hints):
    return (hints > 0).astype(np.float32)


_scale_hints, _decimate, _restore = ref.scale_hints, ref.decimate, ref.restore   # torch's own expressions, on the CPU


def _want(left, right, hints, valid, iscale, oscale, seed, D, maskocc=False, g_occ=None, vpp_kw=None, rsgm_kw=None):
    """One frame: (restored map, map at (h, w), left pattern, right pattern, mask or None)."""
    H, W = hints.shape
    h, w = H // iscale, W // iscale
    ls, rs = (ref.resize_u8(left, w, h), ref.resize_u8(right, w, h)) if iscale != 1 else (left, right)
    hs = _scale_hints(hints, iscale)
    vs = _decimate(valid, iscale) if valid is not None else None
    assert hs.shape == (h, w)
    if maskocc:
        g_occ = oracle.occlusion_heuristic(hs)[1]
    oracle.init_rand(seed)
    lo, ro = oracle.vpp(ls, rs, hs, g_occ=g_occ, **(vpp_kw or {}))
    if vs is not None:
        d = oracle.compute_rsgm(ls, lo, ro, hints=hs, validhints=vs, dmax=D, **(rsgm_kw or {}))
    else:
        d = oracle.compute_rsgm(ls, lo, ro, dmax=D, **(rsgm_kw or {}))
    return _restore(d, iscale, oscale), d, lo, ro, (g_occ if maskocc else None)


def _t(eng, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def _engine_call(eng, b, iscale, oscale, seed, D, mask=None, guided=False, vpp_kw=None, rsgm_kw=None, sync=True):
    """Engine.vpp_rsgm with every output the scaled call has: (out, disp_small, l_vpp, r_vpp, occ_out or None)."""
    import torch
    from vppstereo_amd import pipeline
    B, H, W = b["hints"].shape
    Cc = b["left"].shape[3]
    h, w, Ho, Wo = pipeline.scaled_shape(H, W, iscale, oscale)
    dev = eng.device
    lv = torch.empty((B, h, w, Cc), dtype=torch.uint8, device=dev)
    rv = torch.empty_like(lv)
    ds = torch.empty((B, h, w), dtype=torch.float32, device=dev)
    occ_out = torch.empty((B, h, w), dtype=torch.uint8, device=dev) if isinstance(mask, str) else None
    g_occ = _t(eng, mask) if isinstance(mask, np.ndarray) else mask
    ek = dict(vpp_kw or {})   # the reference's keywords -> VppxVppParams fields
    if "method" in ek:
        ek["method"] = 1 if ek["method"] == "maxDistance" else 0
    out = eng.vpp_rsgm(_t(eng, b["left"]), _t(eng, b["right"]), _t(eng, b["hints"]), g_occ=g_occ, l_vpp=lv, r_vpp=rv, seed=seed,
                       vpp_kw=ek, rsgm_kw=dict(dmax=D, **(rsgm_kw or {})), occ_out=occ_out,
                       validhints=_t(eng, _valid(b["hints"])) if guided else None, iscale=iscale, oscale=oscale, disp_small=ds)
    assert tuple(out.shape) == (B, Ho, Wo)
    if not sync:
        return out, ds, lv, rv, occ_out
    torch.cuda.synchronize()
    eng.status()
    cpu = lambda x: None if x is None else x.cpu().numpy()
    return cpu(out), cpu(ds), cpu(lv), cpu(rv), cpu(occ_out)


def _check_batch(b, got, iscale, oscale, seed, D, mask=None, guided=False, vpp_kw=None, rsgm_kw=None):
    out, ds, lv, rv, occ = got
    B = b["hints"].shape[0]
    for f in range(B):
        l, r = b["left"][f], b["right"][f]
        if l.shape[2] == 1:
            l, r = l[..., 0], r[..., 0]
        g_occ = mask[f] if isinstance(mask, np.ndarray) else None
        wd, wds, lo, ro, wocc = _want(l, r, b["hints"][f], _valid(b["hints"][f]) if guided else None, iscale, oscale, seed + f, D,
                                      maskocc=isinstance(mask, str), g_occ=g_occ, vpp_kw=vpp_kw, rsgm_kw=rsgm_kw)
        assert np.array_equal(lv[f].reshape(lo.shape), lo) and np.array_equal(rv[f].reshape(ro.shape), ro), f
        if wocc is not None:
            assert np.array_equal(occ[f], wocc), f
        assert np.array_equal(ds[f], wds), f
        assert out[f].shape == wd.shape and np.array_equal(out[f], wd), f


def _batch(B, H, W, D, p, seed, C=3):
    return synth.make_batch(B, H, W, D, p, seed=seed, channels=C)


@pytest.mark.parametrize("s", [2, 3, 4])
@pytest.mark.parametrize("C", [1, 3])
def test_resize_alone_through_the_patterned_pair_of_a_call_without_hints(s, C):
    """All-zero hints: VPP leaves the pair as it is, so the patterned pair of the call IS the resized pair."""
    from vppstereo_amd.engine import Engine
    eng = Engine()
    for H, W in ((48, 160), (49, 163), (61, 177)):
        b = _batch(2, H, W, 64, 0.0, seed=H + s, C=C)
        b["hints"][:] = 0
        _, _, lv, rv, _ = _engine_call(eng, b, s, 1, 5, 64)
        for f in range(2):
            want_l = ref.resize_u8(b["left"][f], W // s, H // s)
            assert np.array_equal(lv[f], want_l), (H, W, f)
            assert np.array_equal(rv[f], ref.resize_u8(b["right"][f], W // s, H // s)), (H, W, f)
            if s == 2 and H % 2 == 0 and W % 2 == 0:   # exactly 2x: OpenCV's INTER_AREA fast path gives the same
                assert np.array_equal(lv[f], ref.area_fast_2x(b["left"][f]))


GRID = [
    # (iscale, oscale, C, H, W, mask, guided, vpp_kw)
    (2, 1, 3, 45, 170, "occlusion_heuristic", False, None),
    (3, 1, 1, 46, 171, "tensor", True, None),
    (4, 2, 3, 52, 176, None, True, dict(c_occ=0.1)),
    (3, 2, 3, 47, 165, "occlusion_heuristic", True, dict(method="maxDistance")),
    (2, 2, 1, 44, 168, "tensor", False, None),
    (2, 1, 3, 41, 161, None, False, dict(use_bilateral_patch=True)),
    (3, 2, 1, 45, 170, "occlusion_heuristic", False, dict(wsize=5)),
    (4, 2, 1, 49, 175, "occlusion_heuristic", True, None),
    (2, 1, 1, 40, 160, None, True, None),
]


@pytest.mark.parametrize("iscale,oscale,C,H,W,mask,guided,vpp_kw", GRID)
def test_scaled_call_equals_the_oracle(iscale, oscale, C, H, W, mask, guided, vpp_kw):
    from vppstereo_amd.engine import Engine
    D, seed = 64, 21
    b = _batch(2, H, W, D, 0.06, seed=H * W + iscale, C=C)
    h, w = H // iscale, W // iscale
    m = (np.random.default_rng(H).random((2, h, w)) < 0.2).astype(np.uint8) if mask == "tensor" else mask
    eng = Engine()
    got = _engine_call(eng, b, iscale, oscale, seed, D, mask=m, guided=guided, vpp_kw=vpp_kw, rsgm_kw=dict(p1=9))
    _check_batch(b, got, iscale, oscale, seed, D, mask=m, guided=guided, vpp_kw=vpp_kw, rsgm_kw=dict(p1=9))
    routes = eng.last_routes()
    assert routes[0] == f"scale_front<{C}>"
    assert (routes[-1] == "scale_restore") == (iscale != oscale)


def _rand_consumed():
    from vppstereo_amd import _lib
    s, c = C.c_uint32(), C.c_uint64()
    _lib.check(_lib.load().vppx_rand_state(_lib.default_context().handle, C.byref(s), C.byref(c)))
    return int(c.value)


@pytest.mark.parametrize("iscale,oscale,maskocc,guided", [(2, 1, True, False), (3, 2, False, True), (2, 2, True, True)])
def test_run_frame_scaled_equals_the_oracle_and_draws_like_the_unscaled_call(iscale, oscale, maskocc, guided):
    from vppstereo_amd import pipeline, vpp_standalone
    H, W, D = 47, 181, 64
    fr = synth.make_frame(H, W, D, 0.06, seed=31)
    v = _valid(fr["hints"]) if guided else None
    vpp_standalone.init_rand(9)
    d, lc, rc, conf = pipeline.run_frame(fr["left"], fr["right"], fr["hints"], maskocc=maskocc, validhints=v, rsgm_kw=dict(dmax=D),
                                         return_patterns=True, iscale=iscale, oscale=oscale)
    draws = _rand_consumed()
    wd, _, lo, ro, wocc = _want(fr["left"], fr["right"], fr["hints"], v, iscale, oscale, 9, D, maskocc=maskocc)
    assert np.array_equal(lc, lo) and np.array_equal(rc, ro)
    assert np.array_equal(d, wd)
    if maskocc:
        assert np.array_equal(conf, wocc)
    # the same frame resized by the restatement through the unscaled call: the same number of rand() draws
    h, w = H // iscale, W // iscale
    vpp_standalone.init_rand(9)
    pipeline.run_frame(ref.resize_u8(fr["left"], w, h), ref.resize_u8(fr["right"], w, h), _scale_hints(fr["hints"], iscale),
                       maskocc=maskocc, validhints=_decimate(v, iscale) if guided else None, rsgm_kw=dict(dmax=D))
    assert draws == _rand_consumed() and draws > 0


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


def test_fused_layout_batch_and_a_batch_in_parts():
    """8 frames at D = 192 take the fused aggregation layout; 7 frames with VPPX_CHUNK=3 run as parts.  Frame f equals the oracle
    with seed + f either way."""
    from vppstereo_amd.engine import Engine
    D = 192
    b = _batch(8, 80, 193, D, 0.05, seed=77)
    eng = Engine()
    got = _engine_call(eng, b, 2, 1, 4, D, mask="occlusion_heuristic")
    assert eng.uses_vert() == 3 and eng.last_call_parts() == 1
    _check_batch(b, got, 2, 1, 4, D, mask="occlusion_heuristic")
    b7 = _batch(7, 46, 171, 64, 0.05, seed=78)

    def parts():
        e = Engine()
        g = _engine_call(e, b7, 3, 2, 6, 64, guided=True)
        return g, e.last_call_parts()
    got, nparts = _with_env({"VPPX_CHUNK": 3}, parts)
    assert nparts > 1
    _check_batch(b7, got, 3, 2, 6, 64, guided=True)


def test_iscale_1_through_the_new_entry_point_equals_the_old_one():
    import torch
    from vppstereo_amd.engine import Engine
    b = _batch(3, 40, 120, 64, 0.05, seed=3)
    eng = Engine()
    t = lambda a: _t(eng, a)
    for guided in (False, True):
        vh = t(_valid(b["hints"])) if guided else None
        old = eng.vpp_rsgm(t(b["left"]), t(b["right"]), t(b["hints"]), g_occ="occlusion_heuristic", seed=8, rsgm_kw=dict(dmax=64),
                           validhints=vh)
        ds = torch.empty((3, 40, 120), dtype=torch.float32, device=eng.device)
        new = eng.vpp_rsgm(t(b["left"]), t(b["right"]), t(b["hints"]), g_occ="occlusion_heuristic", seed=8, rsgm_kw=dict(dmax=64),
                           validhints=vh, disp_small=ds)
        torch.cuda.synchronize()
        assert torch.equal(old, new) and torch.equal(new, ds)
        assert not any(r.startswith("scale_") for r in eng.last_routes())


def test_two_pipelined_scaled_calls_equal_the_unpipelined_results():
    import torch
    from vppstereo_amd.engine import Engine
    bs = [_batch(2, 46, 172, 64, 0.05, seed=90 + k) for k in range(3)]
    eng = Engine()
    want = [_engine_call(eng, b, 2, 1, 10 + k, 64, mask="occlusion_heuristic", guided=k == 1) for k, b in enumerate(bs)]
    eng.set_pipeline(True)
    try:
        pend = [_engine_call(eng, b, 2, 1, 10 + k, 64, mask="occlusion_heuristic", guided=k == 1, sync=False) for k, b in enumerate(bs)]
        torch.cuda.synchronize()
        eng.status()
    finally:
        eng.set_pipeline(False)
    for k in range(3):
        for a, x in zip(want[k], pend[k]):
            assert np.array_equal(a, x.cpu().numpy()), k


@pytest.mark.parametrize("guided", [False, True])
def test_frame_stream_iscale_2_equals_run_frame_frame_by_frame(guided):
    from vppstereo_amd import pipeline, vpp_standalone
    H, W, D, seed = 50, 178, 64, 13
    frames = [synth.make_frame(H, W, D, 0.05, seed=200, frame=f) for f in range(7)]
    want = []
    for f, fr in enumerate(frames):
        vpp_standalone.init_rand(seed + f)
        want.append(pipeline.run_frame(fr["left"], fr["right"], fr["hints"], maskocc=True, rsgm_kw=dict(dmax=D), return_patterns=True,
                                       validhints=_valid(fr["hints"]) if guided else None, iscale=2))
    got = []
    with pipeline.FrameStream(H, W, 3, batch=3, seed=seed, maskocc=True, rsgm_kw=dict(dmax=D), return_patterns=True, guided=guided,
                              iscale=2) as fs:
        for f, fr in enumerate(frames):
            fs.push(fr["left"], fr["right"], fr["hints"], validhints=_valid(fr["hints"]) if guided else None)
            if f == 4:
                fs.flush()          # mid-batch: 3 + 2 + 2
        fs.flush()
        while True:
            r = fs.pop()
            if r is None:
                break
            got.append(r)
    assert len(got) == 7
    for f in range(7):
        for a, x in zip(want[f], got[f]):
            assert a.shape == x.shape and np.array_equal(a, x), f
    assert got[0][0].shape == (50, 178) and got[0][1].shape == (25, 89, 3)


@pytest.mark.parametrize("H,W", [(540, 960), (375, 1242)])
def test_full_size_iscale_2(H, W):
    from vppstereo_amd.engine import Engine
    D = 192
    b = _batch(2, H, W, D, 0.03, seed=H)
    eng = Engine()
    got = _engine_call(eng, b, 2, 1, 2, D, mask="occlusion_heuristic")
    assert got[0].shape == (2, (H // 2) * 2, (W // 2) * 2)
    _check_batch(b, got, 2, 1, 2, D, mask="occlusion_heuristic")


def test_invalid_arguments_fail_with_a_message():
    import torch
    from vppstereo_amd import _lib
    from vppstereo_amd.engine import Engine
    eng = Engine()
    b = _batch(1, 40, 120, 64, 0.05, seed=1)
    t = lambda a: _t(eng, a)
    with pytest.raises(_lib.VppxError, match="positive"):
        eng.vpp_rsgm(t(b["left"]), t(b["right"]), t(b["hints"]), iscale=0)
    with pytest.raises(_lib.VppxError, match="positive"):
        eng.vpp_rsgm(t(b["left"]), t(b["right"]), t(b["hints"]), iscale=2, oscale=0)
    with pytest.raises(_lib.VppxError, match="frame too small"):      # 40 // 10 = 4 rows
        eng.vpp_rsgm(t(b["left"]), t(b["right"]), t(b["hints"]), iscale=10)
    with pytest.raises(ValueError, match="out"):
        eng.vpp_rsgm(t(b["left"]), t(b["right"]), t(b["hints"]), iscale=2, out=torch.empty((1, 20, 60), device=eng.device))
    # the C entry point itself: nothing launched, a message
    lib = _lib.load()
    vp, rp, sp = _lib.vpp_params(), _lib.rsgm_params(dmax=64), _lib.scale_params(iscale=-1)
    rc = lib.vppx_occ_vpp_rsgm_scaled_dev(eng.ctx.handle, None, C.byref(vp), C.byref(rp), C.byref(sp), 1, 40, 120, 3, None, None,
                                          None, None, None, None, None, None, None, None)
    assert rc == -1 and lib.vppx_last_error()
    with pytest.raises(Exception, match="positive"):
        from vppstereo_amd.pipeline import FrameStream
        FrameStream(40, 120, iscale=0)
