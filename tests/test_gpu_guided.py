"""--guided with the rSGM matcher on the batched device path (test.py:207-223): the hints drive both the virtual pattern and the
cost re-weighting of _guided_dsi (rsgm.py:116-127).  Every result is compared bit for bit with the CPU oracle:
init_rand(seed), vpp, then compute_rsgm(left, lv, rv, hints=..., validhints=...)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _valid(hints):
    return (hints > 0).astype(np.float32)


def _want(left, right, hints, valid, seed, D, maskocc=False, g_occ=None, vpp_kw=None, rsgm_kw=None):
    """The oracle of one frame: (disparity, left pattern, right pattern)."""
    if maskocc:
        g_occ = oracle.occlusion_heuristic(hints)[1]
    oracle.init_rand(seed)
    lo, ro = oracle.vpp(left, right, hints, g_occ=g_occ, **(vpp_kw or {}))
    d = oracle.compute_rsgm(left, lo, ro, hints=hints, validhints=valid, dmax=D, **(rsgm_kw or {}))
    return d, lo, ro


def _run_frame(l, r, h, v, seed, **kw):
    from vppstereo_amd import pipeline, vpp_standalone
    vpp_standalone.init_rand(seed)
    return pipeline.run_frame(l, r, h, validhints=v, return_patterns=True, **kw)


@pytest.mark.parametrize("H,W,D,ch,maskocc,method", [
    (45, 101, 64, 3, True, "rnd"),
    (37, 90, 96, 1, False, "maxDistance"),
    (40, 211, 192, 3, False, "rnd"),
    (33, 270, 256, 3, True, "maxDistance"),
    (48, 128, 64, 1, True, "rnd"),
])
def test_run_frame_guided_equals_the_oracle(H, W, D, ch, maskocc, method):
    fr = synth.make_frame(H, W, D, 0.05, seed=H + D, channels=ch)
    l, r, h = fr["left"], fr["right"], fr["hints"]
    if ch == 1:
        l, r = l[..., 0].copy(), r[..., 0].copy()
    v = _valid(h)
    vk = dict(method=method, c_occ=0.1)
    d, lc, rc, _ = _run_frame(l, r, h, v, 17, maskocc=maskocc, vpp_kw=vk, rsgm_kw=dict(dmax=D, p1=9))
    wd, lo, ro = _want(l, r, h, v, 17, D, maskocc=maskocc, vpp_kw=vk, rsgm_kw=dict(p1=9))
    assert np.array_equal(lc.reshape(lo.shape), lo) and np.array_equal(rc.reshape(ro.shape), ro)
    assert np.array_equal(d, wd)


def test_guided_hints_off_the_grid_out_of_range_and_disagreeing_with_their_mask():
    """Non-integer hints, hints above D, validhints == 1 where the hint is 0 (re-weighted, as rsgm.py:123 only looks at
    validhints) and hints > 0 with validhints == 0 (not re-weighted)."""
    H, W, D = 42, 120, 64
    fr = synth.make_frame(H, W, D, 0.08, seed=5)
    rng = np.random.default_rng(9)
    h = fr["hints"].copy()
    on = h > 0
    h[on] += rng.uniform(-0.49, 0.49, int(on.sum())).astype(np.float32)   # off the integer grid
    h[on & (rng.random((H, W)) < 0.2)] = np.float32(D + 37.5)               # above the search range
    v = _valid(h)
    v[on & (rng.random((H, W)) < 0.25)] = 0                                  # a hint that does not count
    v[(~on) & (rng.random((H, W)) < 0.03)] = 1                               # a valid pixel whose hint is 0
    assert ((v > 0) & (h == 0)).any() and ((v == 0) & (h > 0)).any()
    d, lc, rc, _ = _run_frame(fr["left"], fr["right"], h, v, 3, rsgm_kw=dict(dmax=D))
    wd, lo, ro = _want(fr["left"], fr["right"], h, v, 3, D)
    assert np.array_equal(lc, lo) and np.array_equal(rc, ro)
    assert np.array_equal(d, wd)


def _engine_batch(eng, b, seed, D, g_occ, vh, **kw):
    import torch
    dev = eng.device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    B, H, W = b["hints"].shape
    lv = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    rv = torch.empty_like(lv)
    out = eng.vpp_rsgm(t(b["left"]), t(b["right"]), t(b["hints"]), g_occ=t(g_occ) if isinstance(g_occ, np.ndarray) else g_occ,
                       l_vpp=lv, r_vpp=rv, seed=seed, rsgm_kw=dict(dmax=D), validhints=None if vh is None else t(vh), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), lv.cpu().numpy(), rv.cpu().numpy()


@pytest.mark.parametrize("B", [1, 3, 8, 17])
@pytest.mark.parametrize("mask", ["tensor", "occlusion_heuristic"])
def test_engine_vpp_rsgm_guided_batch_equals_the_oracle_frame_by_frame(B, mask):
    from vppstereo_amd.engine import Engine
    H, W, D, seed = 36, 84, 64, 40
    b = synth.make_batch(B, H, W, D, 0.05, seed=B)
    vh = _valid(b["hints"])
    masks = (np.random.default_rng(B).random((B, H, W)) < 0.2).astype(np.uint8)
    eng = Engine()
    out, lv, rv = _engine_batch(eng, b, seed, D, masks if mask == "tensor" else mask, vh)
    for f in range(B):
        wd, lo, ro = _want(b["left"][f], b["right"][f], b["hints"][f], vh[f], seed + f, D,
                           maskocc=mask != "tensor", g_occ=masks[f] if mask == "tensor" else None)
        assert np.array_equal(lv[f], lo) and np.array_equal(rv[f], ro), f
        assert np.array_equal(out[f], wd), f


def test_engine_rsgm_guided_equals_compute_rsgm():
    import torch
    from vppstereo_amd.engine import Engine
    B, H, W, D = 2, 44, 100, 128
    b = synth.make_batch(B, H, W, D, 0.06, seed=8)
    vh = _valid(b["hints"])
    eng = Engine()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    out = eng.rsgm(t(b["left"]), t(b["left"]), t(b["right"]), hints=t(b["hints"]), validhints=t(vh), dmax=D).cpu().numpy()
    plain = eng.rsgm(t(b["left"]), t(b["left"]), t(b["right"]), dmax=D).cpu().numpy()
    for f in range(B):
        want = oracle.compute_rsgm(b["left"][f], b["left"][f], b["right"][f], hints=b["hints"][f], validhints=vh[f], dmax=D)
        assert np.array_equal(out[f], want), f
    assert not np.array_equal(out, plain)
    with pytest.raises(ValueError):
        eng.rsgm(t(b["left"]), t(b["left"]), t(b["right"]), hints=t(b["hints"]), dmax=D)


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch, synth
from vppstereo_amd.engine import Engine
B, H, W, D = 8, 34, 70, 64
b = synth.make_batch(B, H, W, D, 0.05, seed=77)
eng = Engine()
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
out = eng.vpp_rsgm(t(b["left"]), t(b["right"]), t(b["hints"]), g_occ="occlusion_heuristic", seed=9, rsgm_kw=dict(dmax=D),
                   validhints=t((b["hints"] > 0).astype(np.float32)))
torch.cuda.synchronize()
np.save(sys.argv[2], out.cpu().numpy())
print("parts", eng.last_call_parts())
"""


def test_guided_batch_forced_into_parts_equals_the_whole_batch(tmp_path):
    """VPPX_CHUNK=3 (read when a context is created: a fresh child process) splits 8 frames into parts; frame f keeps
    srand(seed + f), so the results are those of the whole batch."""
    from vppstereo_amd.engine import Engine
    B, H, W, D = 8, 34, 70, 64
    b = synth.make_batch(B, H, W, D, 0.05, seed=77)
    whole, _, _ = _engine_batch(Engine(), b, 9, D, "occlusion_heuristic", _valid(b["hints"]))
    env = dict(os.environ, VPPX_CHUNK="3")
    dst = str(tmp_path / "parts.npy")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, dst], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert int(r.stdout.split("parts")[-1]) >= 2, r.stdout   # (2 + 3 + 3: a guided call's remainder is a part of its own)
    assert np.array_equal(np.load(dst), whole)


def _stream_frames(n, H, W, D, seed):
    out = []
    for f in range(n):
        fr = synth.make_frame(H, W, D, 0.05, seed=seed + f)
        out.append((fr["left"], fr["right"], fr["hints"], None, _valid(fr["hints"])))
    return out


@pytest.mark.parametrize("depth", [2, 3])
def test_guided_frame_stream_equals_run_frame_per_frame(depth):
    """37 frames in batches of 8 with a flush in the middle: each result equals its own run_frame call with seed + f."""
    from vppstereo_amd.pipeline import FrameStream
    H, W, D, seed = 44, 104, 64, 21
    frames = _stream_frames(37, H, W, D, 500)
    want = [_run_frame(l, r, h, v, seed + f, maskocc=True, rsgm_kw=dict(dmax=D))[0] for f, (l, r, h, _, v) in enumerate(frames)]
    got = []
    with FrameStream(H, W, 3, batch=8, depth=depth, seed=seed, maskocc=True, rsgm_kw=dict(dmax=D), guided=True) as fs:
        for fr in frames[:13]:
            fs.push(*fr)
        fs.flush()                      # 8 + 5 | 8 + 8 + 8
        got += [fs.pop() for _ in range(13)]
        got += list(fs.run(iter(frames[13:])))
    assert len(got) == 37
    for f in range(37):
        assert np.array_equal(got[f], want[f]), f


def test_guided_stream_refuses_missing_or_unexpected_validhints():
    from vppstereo_amd import _lib
    from vppstereo_amd.pipeline import FrameStream
    H, W, D = 24, 48, 64
    (l, r, h, _, v), = _stream_frames(1, H, W, D, 3)
    with FrameStream(H, W, 3, batch=2, seed=1, rsgm_kw=dict(dmax=D), guided=True) as fs:
        with pytest.raises(ValueError):
            fs.push(l, r, h)
        assert fs.counts()[0] == 0
        # the C entry point refuses the unguided push on a guided stream
        rc = fs._lib.vppx_fstream_push(fs._h, l.ctypes.data, r.ctypes.data, h.ctypes.data, None)
        assert rc == -1 and b"VPPX_FS_GUIDED" in fs._lib.vppx_last_error()
        assert fs.counts()[0] == 0
    with FrameStream(H, W, 3, batch=2, seed=1, rsgm_kw=dict(dmax=D)) as fs:
        with pytest.raises(ValueError):
            fs.push(l, r, h, None, v)
        rc = fs._lib.vppx_fstream_push_guided(fs._h, l.ctypes.data, r.ctypes.data, h.ctypes.data, None, v.ctypes.data)
        assert rc == -1 and b"without VPPX_FS_GUIDED" in fs._lib.vppx_last_error()
        assert fs.counts()[0] == 0
    assert _lib.ERR_NAMES[-1] == "VPPX_E_INVALID_ARG"


def test_guided_differs_from_unguided_on_the_same_inputs():
    from vppstereo_amd.engine import Engine
    B, H, W, D = 2, 40, 96, 64
    b = synth.make_batch(B, H, W, D, 0.06, seed=31)
    eng = Engine()
    g, lg, rg = _engine_batch(eng, b, 4, D, None, _valid(b["hints"]))
    u, lu, ru = _engine_batch(eng, b, 4, D, None, None)
    assert np.array_equal(lg, lu) and np.array_equal(rg, ru)     # the same patterns ...
    assert not np.array_equal(g, u)                              # ... but re-weighted costs
