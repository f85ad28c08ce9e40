"""GPU parity of the hint-sampling kernel (sample_kernels.hip behind vppx_sample_hints_dev / _host) with torch's CPU stream:
frame f of a call must equal ``torch.manual_seed(seed + f); losses.sample_hints(src, validsrc > 0, p)`` bit for bit -- the sign
of a zero included; a NaN source that is selected stays a NaN.  Shapes sit on the generator's seams (a word that depends on a
new word: 227; the first twist: 624), on the kernel's own (224 words per step, two steps per trip, 3584 per chunk, a ring of 8192) and one frame is
full size, to reach step counts the small ones do not."""
import ctypes as C

import numpy as np
import pytest
import torch

import synth
from vppstereo_amd import losses

pytestmark = pytest.mark.gpu

SEAMS = [1, 3, 4, 5, 223, 224, 225, 226, 227, 228, 396, 397, 398, 447, 448, 449, 623, 624, 625, 1247, 1248, 1249, 3583, 3584, 3585, 3808, 7167, 7168,
         7169, 8191, 8192, 8193]


@pytest.fixture(scope="module")
def eng():
    from vppstereo_amd.engine import Engine
    return Engine()


def oracle(src, valid, p, seed):
    """src, valid: float32 numpy [B,H,W]; torch on the CPU, one manual_seed per frame."""
    hs, vs = [], []
    for f in range(src.shape[0]):
        torch.manual_seed(int(seed) + f)
        h, v = losses.sample_hints(torch.from_numpy(src[f]), torch.from_numpy(valid[f]) > 0, p)
        hs.append(h.numpy())
        vs.append(v.numpy())
    return np.stack(hs), np.stack(vs)


def same(a, b):
    """Exact: the same bits wherever neither is a NaN, NaN where the other is."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def inputs(B, H, W, seed):
    rng = np.random.default_rng(seed)
    src = rng.uniform(0.5, 190.0, (B, H, W)).astype(np.float32)
    valid = rng.choice(np.array([0, 1, 0.5, -1, np.nan], np.float32), size=(B, H, W), p=[0.2, 0.5, 0.15, 0.1, 0.05]).astype(np.float32)
    return src, valid


def run(eng, src, valid, p, seed, want_valid=True):
    t = lambda a: torch.from_numpy(a).to(eng.device)
    if want_valid:
        h, v = eng.sample_hints(t(src), t(valid), p, seed)
        torch.cuda.synchronize()
        return h.cpu().numpy(), v.cpu().numpy()
    # validhints_out NULL: the C-ABI directly
    from vppstereo_amd import _lib
    s, vv = t(src), t(valid)
    out = torch.full_like(s, -7.0)
    smp = _lib.sample_params(probability=float(p), seed=int(seed) & 0xFFFFFFFF)
    eng._bind_stream()
    B, H, W = src.shape
    _lib.check(eng.lib.vppx_sample_hints_dev(eng.ctx.handle, C.byref(smp), B, H, W, C.c_void_p(s.data_ptr()), C.c_void_p(vv.data_ptr()),
                                             C.c_void_p(out.data_ptr()), None))
    torch.cuda.synchronize()
    return out.cpu().numpy(), None


def test_seams_of_the_generator_and_of_the_kernel(eng):
    for n in SEAMS:
        src, valid = inputs(1, 1, n, n)
        h, v = run(eng, src, valid, 0.5, 11)
        wh, wv = oracle(src, valid, 0.5, 11)
        assert same(h, wh) and same(v, wv), n
        assert n < 20 or 0 < v.sum() < n


@pytest.mark.parametrize("H,W", [(37, 53), (96, 130), (64, 80)])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_batches_frame_f_is_the_one_frame_call_with_seed_plus_f(eng, H, W, B):
    src, valid = inputs(B, H, W, 100 + B)
    h, v = run(eng, src, valid, 0.05, 21)
    wh, wv = oracle(src, valid, 0.05, 21)
    assert same(h, wh) and same(v, wv)
    for f in range(B):
        h1, v1 = run(eng, src[f:f + 1], valid[f:f + 1], 0.05, 21 + f)
        assert same(h1[0], h[f]) and same(v1[0], v[f]), f
    assert len({v[f].tobytes() for f in range(B)}) == B


def test_one_full_size_frame(eng):
    src, valid = inputs(1, 540, 960, 5)
    h, v = run(eng, src, valid, 0.05, 1)
    wh, wv = oracle(src, valid, 0.05, 1)
    assert same(h, wh) and same(v, wv)
    assert 0.02 < v.mean() < 0.05       # 5 % of the ~65 % valid pixels


@pytest.mark.parametrize("seed", [0, 1, 2 ** 32 - 1, 2 ** 32 + 5])
def test_seeds_wrap_at_two_to_the_32(eng, seed):
    src, valid = inputs(3, 37, 53, 7)
    h, v = run(eng, src, valid, 0.2, seed)
    wh, wv = oracle(src, valid, 0.2, seed)      # torch.manual_seed(2^32 - 1 + 1) seeds with 0, + 2 with 1
    assert same(h, wh) and same(v, wv)
    if seed == 2 ** 32 - 1:
        h0, _ = run(eng, src[1:], valid[1:], 0.2, 0)
        assert same(h0, h[1:])


@pytest.mark.parametrize("p", [0.0, 1.0, 0.05, 1e-9, 2.0, float("nan")])
def test_probabilities(eng, p):
    src, valid = inputs(2, 64, 80, 9)
    h, v = run(eng, src, valid, p, 3)
    wh, wv = oracle(src, valid, p, 3)
    assert same(h, wh) and same(v, wv)
    if p in (1.0, 2.0):
        assert np.array_equal(v, (valid > 0).astype(np.float32))
    if p == 0.0 or p != p:
        assert not v.any() and not h.any() and not np.signbit(h).any()


def test_odd_sources_pass_through_or_vanish(eng):
    """-0.0, negatives, inf and NaN in src, at selected and at unselected pixels; validsrc of 0, 0.5, -1 and NaN."""
    B, H, W = 2, 37, 53
    rng = np.random.default_rng(17)
    src = rng.choice(np.array([-0.0, 0.0, -3.5, 12.25, np.inf, -np.inf, np.nan], np.float32), size=(B, H, W)).astype(np.float32)
    valid = rng.choice(np.array([0, 1, 0.5, -1, np.nan], np.float32), size=(B, H, W)).astype(np.float32)
    h, v = run(eng, src, valid, 0.5, 4)
    wh, wv = oracle(src, valid, 0.5, 4)
    assert same(h, wh) and same(v, wv)
    sel = v > 0
    assert same(h[sel], src[sel])                                   # unchanged, the sign of -0.0 and the NaNs included
    assert np.isnan(h[sel]).any() and np.isinf(h[sel]).any() and np.signbit(h[sel][h[sel] == 0]).any()
    assert np.array_equal(h[~sel].view(np.uint32), np.zeros((~sel).sum(), np.uint32))   # +0.0 whatever src held there
    assert not np.isfinite(src[~sel]).all()
    assert not sel[~(valid > 0)].any() and set(np.unique(v)) == {0.0, 1.0}


def test_validhints_out_may_be_null(eng):
    src, valid = inputs(3, 37, 53, 23)
    h, _ = run(eng, src, valid, 0.3, 8, want_valid=False)
    assert same(h, oracle(src, valid, 0.3, 8)[0])


def test_host_twin_equals_dev(eng):
    from vppstereo_amd import pipeline
    for shape in ((3, 37, 53), (2, 64, 80)):
        src, valid = inputs(*shape, 31)
        h, v = run(eng, src, valid, 0.1, 2 ** 32 - 1)
        hh, hv = pipeline.sample_hints(src, valid, 0.1, 2 ** 32 - 1)
        assert same(hh, h) and same(hv, v)
    one, ov = pipeline.sample_hints(src[0], valid[0], 0.1, 2 ** 32 - 1)      # [H,W]
    assert one.shape == src[0].shape and same(one, h[0]) and same(ov, v[0])
    assert same(pipeline.sample_hints(src[0], valid[0], 0.1, 2 ** 32 - 1, return_valid=False), h[0])


def test_argument_checks_launch_nothing(eng):
    from vppstereo_amd import _lib
    lib, hnd = eng.lib, eng.ctx.handle
    t = torch.zeros((1, 8, 8), dtype=torch.float32, device=eng.device)
    out = torch.full_like(t, 5.0)
    p = lambda x: C.c_void_p(x.data_ptr())
    smp = _lib.sample_params()
    for args in ((None, 1, 8, 8, p(t), p(t), p(out), None), (C.byref(smp), 1, 8, 8, None, p(t), p(out), None),
                 (C.byref(smp), 1, 8, 8, p(t), None, p(out), None), (C.byref(smp), 1, 8, 8, p(t), p(t), None, None),
                 (C.byref(smp), 0, 8, 8, p(t), p(t), p(out), None), (C.byref(smp), 1, 0, 8, p(t), p(t), p(out), None),
                 (C.byref(smp), 1, 8, -1, p(t), p(t), p(out), None)):
        assert lib.vppx_sample_hints_dev(hnd, *args) == -1 and lib.vppx_last_error()
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())


def test_graph_mode_replayed_with_a_new_seed_equals_the_eager_call(eng):
    """vppx_set_graph_mode: the sampling is launched in front of the replayed graph, so a new sampling seed replays and is right."""
    from vppstereo_amd.engine import Engine
    B, H, W, D = 2, 48, 80, 64
    b = synth.make_batch(B, H, W, D, 0.05, seed=41)
    ref = Engine()
    t = lambda e, a: torch.from_numpy(a).to(e.device)
    valid = (b["gt"] > 0).astype(np.float32)
    want = {}
    for s in (5, 77):
        ho = torch.empty((B, H, W), dtype=torch.float32, device=ref.device)
        d = ref.vpp_rsgm(t(ref, b["left"]), t(ref, b["right"]), seed=3, rsgm_kw=dict(dmax=D),
                         sample=dict(probability=0.05, seed=s, src=t(ref, b["gt"]), validsrc=t(ref, valid), hints_out=ho))
        ref.synchronize()
        want[s] = (d.cpu(), ho.cpu())
        assert same(want[s][1].numpy(), oracle(b["gt"], valid, 0.05, s)[0])
    assert not torch.equal(want[5][1], want[77][1])
    g = Engine()
    side = torch.cuda.Stream(device=g.device)
    with torch.cuda.stream(side):
        l, r, src, vs = t(g, b["left"]), t(g, b["right"]), t(g, b["gt"]), t(g, valid)
        out = torch.empty((B, H, W), dtype=torch.float32, device=g.device)
        ho = torch.empty_like(out)
        side.synchronize()
        g.set_graph_mode(True)
        try:
            for s in (5, 5, 5, 77, 5):
                r0 = g.graph_replays()
                g.vpp_rsgm(l, r, out=out, seed=3, rsgm_kw=dict(dmax=D), sample=dict(probability=0.05, seed=s, src=src, validsrc=vs, hints_out=ho))
                g.synchronize()
                assert torch.equal(out.cpu(), want[s][0]) and torch.equal(ho.cpu(), want[s][1]), s
            assert g.graph_replays() - r0 == 1      # the last two calls, new seeds, launched the captured graph
        finally:
            g.set_graph_mode(False)
