"""The read-out kernels (readout_kernels.hip: PSMNet's upsample + softmax + regression, RAFT-Stereo's convex upsampling,
both with the crop) against the float64 referee of tests/_readout_ref.py.

No atol.  Every finite cell is held to the referee's limit(): the distance to the float64 value that a float32
implementation can reach in any association of the lerps and any order of the sums, with an expf within
DEVICE_EXP_ULPS of the true value (derivation in the referee; tests/test_gpu_handoff_ref.py says where the figure is
from).  A cell that is not finite must have the referee's class.  Sentinel words in front of and behind the output must
be intact.  What each case reaches is asserted on the CPU in tests/test_readout_ref_cpu.py, on these very arrays."""
import os

import numpy as np
import pytest

import _readout_ref as R
from _cells import INVALID, SENTINEL32, UNSUPPORTED, dev as _dev, guarded, guards_intact as _guards_intact, hold
import synth

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DEVICE_EXP_ULPS = 1.0
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "readout_cases.npz"))
_REFS = {}


@pytest.fixture(scope="module")
def eng():
    import torch
    from vppstereo_amd.engine import Engine
    assert torch.cuda.is_available()
    return Engine()


def _psm_ref(name):
    if ("psm", name) not in _REFS:
        c = R.psm_case(name)
        _REFS["psm", name] = (c, R.psm_readout(c.cost, c.D, c.H, c.W, c.crop, exp_ulps=DEVICE_EXP_ULPS))
    return _REFS["psm", name]


def _raft_ref(name):
    if ("raft", name) not in _REFS:
        c = R.raft_case(name)
        _REFS["raft", name] = (c, R.raft_upsample(c.flow, c.mask, c.f, c.negate, c.channels, c.crop, exp_ulps=DEVICE_EXP_ULPS))
    return _REFS["raft", name]


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _psm(eng, c, out=None, cost=None):
    cost = _dev(eng, c.cost, c.dtype) if cost is None else cost
    return eng.psmnet_disparity(cost, c.D, (c.H, c.W), crop=c.crop, out=out)


def _raft(eng, c, out=None):
    n = {1: 0, 2: 1, 4: 2, 8: 3}[c.f]
    return eng.raft_upsample(_dev(eng, c.flow, c.dtype), _dev(eng, c.mask, c.dtype), n, negate=c.negate, channels=c.channels, crop=c.crop,
                             out=out)


# ---- PSMNet -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.PSM_CASES))
def test_psm_readout_equals_the_referee(eng, name):
    import torch
    c, ref = _psm_ref(name)
    buf, out = guarded(eng, ref.value.shape, "float32")
    got = _psm(eng, c, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and got.dtype == torch.float32
    hold(R, got.cpu().numpy(), ref, f"psm {name}")
    assert _guards_intact(buf, ref.value.size)
    # a fresh output and the five-dimensional cost3 give the same bits
    five = _dev(eng, c.cost, c.dtype).unsqueeze(1)
    again = eng.psmnet_disparity(five, c.D, (c.H, c.W), crop=c.crop)
    assert again.shape == ref.value.shape and _same(again.cpu().numpy(), got.cpu().numpy())
    if name == "nonfinite":
        cls = R.classes(got.cpu().numpy())
        assert (cls == 1).any() and (cls == 0).any() and not (cls >= 2).any()


def test_psm_frames_of_a_batch_equal_one_frame_calls(eng):
    for name in ("x4", "x4_bf16"):
        c, _ = _psm_ref(name)
        both = _psm(eng, c).cpu().numpy()
        assert not _same(both[0], both[1])
        for f in range(c.B):
            one = eng.psmnet_disparity(_dev(eng, c.cost[f:f + 1], c.dtype), c.D, (c.H, c.W)).cpu().numpy()
            assert _same(one, both[f:f + 1]), (name, f)


def test_psm_crop_is_the_window_of_the_whole_map(eng):
    c, _ = _psm_ref("crop")
    top, left, Ho, Wo = R.window(c.H, c.W, c.crop)
    whole = eng.psmnet_disparity(_dev(eng, c.cost), c.D, (c.H, c.W)).cpu().numpy()
    assert _same(_psm(eng, c).cpu().numpy(), whole[:, top:top + Ho, left:left + Wo])


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_psm_golden_through_engine_and_drop_in(eng, tag):
    from vppstereo_amd.readout import psmnet_regress
    D, H, W = (int(v) for v in G[f"psm_{tag}_meta"])
    cost3 = G[f"psm_{tag}_cost3"]
    ref = R.psm_readout(cost3[:, 0], D, H, W, exp_ulps=DEVICE_EXP_ULPS)
    assert R.compare(G[f"psm_{tag}_pred"], ref)[1:] == (0, 0)
    got = eng.psmnet_disparity(_dev(eng, cost3), D, (H, W)).cpu().numpy()
    hold(R, got, ref, f"psm golden {tag}")
    drop = psmnet_regress(_dev(eng, cost3), D, (H, W))
    assert drop.shape == G[f"psm_{tag}_pred"].shape and _same(drop.cpu().numpy(), got)
    dist = np.abs(got.astype(F64) - G[f"psm_{tag}_pred"])
    print(f"psm golden {tag}: largest distance to the recording {dist.max():.3g} px")
    assert (dist <= 2 * ref.limit).all()         # both are within the limit of one value


# ---- RAFT-Stereo ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.RAFT_CASES))
def test_raft_upsample_equals_the_referee(eng, name):
    import torch
    c, ref = _raft_ref(name)
    buf, out = guarded(eng, ref.value.shape, "float32")
    got = _raft(eng, c, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    host = got.cpu().numpy()
    hold(R, host, ref, f"raft {name}")
    assert _guards_intact(buf, ref.value.size)
    # an output 4 bytes further into a larger buffer takes the float-by-float stores: the same bits
    buf1, out1 = guarded(eng, ref.value.shape, "float32", shift=1)
    assert out1.data_ptr() % 16 == 4
    _raft(eng, c, out=out1)
    torch.cuda.synchronize()
    assert _same(out1.cpu().numpy(), host) and _guards_intact(buf1, ref.value.size, shift=1)
    if c.negate:
        plain = eng.raft_upsample(_dev(eng, c.flow), _dev(eng, c.mask), 2, channels=c.channels, crop=c.crop).cpu().numpy()
        assert _same(-plain, host)


def test_raft_frames_of_a_batch_equal_one_frame_calls(eng):
    for name in ("two_by_two", "two_bf16"):
        c, _ = _raft_ref(name)
        both = _raft(eng, c).cpu().numpy()
        for f in range(c.B):
            one = eng.raft_upsample(_dev(eng, c.flow[f:f + 1], c.dtype), _dev(eng, c.mask[f:f + 1], c.dtype), 2).cpu().numpy()
            assert _same(one, both[f:f + 1]), (name, f)
        # channel 0 alone, read out of the two-channel tensor through its frame stride
        first = eng.raft_upsample(_dev(eng, c.flow, c.dtype), _dev(eng, c.mask, c.dtype), 2, channels=1).cpu().numpy()
        assert first.shape[1] == 1 and _same(first, both[:, :1])


def test_raft_non_finite_cells_stay_in_their_pixels(eng):
    c = R.raft_case("two_by_two")
    mask, flow = c.mask.copy(), c.flow.copy()
    f = c.f
    mask[1, 0 * f * f + 1 * f + 2, 1, 1] = np.nan           # k = 0, i = 1, j = 2 of source pixel (1, 1)
    mask[1, 3 * f * f + 0 * f + 0, 2, 3] = np.inf
    mask[1, 5 * f * f + 3 * f + 3, 0, 4] = -np.inf
    flow[0, 1, 1, 2] = np.inf                               # read by the 3x3 source pixels around it, channel 1
    ref = R.raft_upsample(flow, mask, f, exp_ulps=DEVICE_EXP_ULPS)
    cls = R.classes(ref.value)
    assert cls[1, 0, 4 + 1, 4 + 2] == 1 and cls[1, 1, 4 * 2, 4 * 3] == 1 and cls[1, 0, 3, 19] == 0
    assert (cls[1] == 1).sum() == 4 and (cls[0, 0] == 0).all() and (cls[0, 1] != 0).sum() == 9 * f * f
    got = eng.raft_upsample(_dev(eng, flow), _dev(eng, mask), 2).cpu().numpy()
    hold(R, got, ref, "raft non-finite")


@pytest.mark.parametrize("tag", ["a", "b", "c", "d", "e"])
def test_raft_golden_through_engine_and_drop_in(eng, tag):
    from vppstereo_amd.readout import upsample_flow
    n = int(G[f"raft_{tag}_meta"][0])
    flow, mask, up = G[f"raft_{tag}_flow"], G[f"raft_{tag}_mask"], G[f"raft_{tag}_up"]
    ref = R.raft_upsample(flow, mask, 2 ** n, exp_ulps=DEVICE_EXP_ULPS)
    assert R.compare(up, ref)[1:] == (0, 0)
    got = eng.raft_upsample(_dev(eng, flow), _dev(eng, mask), n).cpu().numpy()
    hold(R, got, ref, f"raft golden {tag}")
    drop = upsample_flow(_dev(eng, flow), _dev(eng, mask), n_downsample=n)
    assert drop.shape == up.shape and _same(drop.cpu().numpy(), got)
    assert (np.abs(got.astype(F64) - up) <= 2 * ref.limit).all()


# ---- refusals: before anything is launched, with no output byte touched -----------------------------------------
def test_refusals_leave_every_byte_alone(eng):
    import torch
    from vppstereo_amd._lib import VppxError
    lib, ctx = eng.lib, eng.ctx.handle
    inp = torch.full((8192,), 1.0, dtype=torch.float32, device=eng.device)
    out = torch.full((8192,), SENTINEL32, dtype=torch.int32, device=eng.device)
    p, o = inp.data_ptr(), out.data_ptr()
    eng._bind_stream()

    def psm(cost=p, B=1, D4=2, H4=2, W4=3, maxdisp=8, H=8, W=12, top=0, left=0, Hout=8, Wout=12, out_=o, dtype=0):
        return lib.vppx_psmnet_readout_dt_dev(ctx, cost, B, D4, H4, W4, maxdisp, H, W, top, left, Hout, Wout, out_, dtype)

    def raft(flow=p, stride=6, mask=p, B=1, C=1, H4=2, W4=3, f=2, mc=36, sign=1, top=0, left=0, Hout=4, Wout=6, out_=o, dtype=0):
        return lib.vppx_raft_upsample_dt_dev(ctx, flow, stride, mask, B, C, H4, W4, f, mc, sign, top, left, Hout, Wout, out_, dtype)

    bad = "bad arguments"
    table = (
        (lambda: psm(cost=None), INVALID, bad), (lambda: psm(out_=None), INVALID, bad), (lambda: psm(B=0), INVALID, bad),
        (lambda: psm(D4=0), INVALID, bad), (lambda: psm(H4=-1), INVALID, bad), (lambda: psm(W4=0), INVALID, bad),
        (lambda: psm(maxdisp=0), INVALID, bad), (lambda: psm(H=0, Hout=0), INVALID, bad), (lambda: psm(W=0), INVALID, bad),
        (lambda: psm(dtype=2), INVALID, "vppx_psmnet_readout: dtype 2 is neither VPPX_DT_F32 (0) nor VPPX_DT_BF16 (1)"),
        (lambda: psm(dtype=-1), INVALID, "dtype -1"),
        (lambda: psm(top=-1), INVALID, "is not inside the 8x12 map"), (lambda: psm(left=-1), INVALID, "is not inside"),
        (lambda: psm(Hout=0), INVALID, "is not inside"), (lambda: psm(Wout=0), INVALID, "is not inside"),
        (lambda: psm(top=1), INVALID, "vppx_psmnet_readout: the window of 8x12 pixels at row 1, column 0 is not inside the 8x12 map"),
        (lambda: psm(left=2, Wout=11), INVALID, "is not inside"), (lambda: psm(top=0x7FFFFFFF, Hout=2), INVALID, "is not inside"),
        (lambda: psm(D4=20000, maxdisp=4), UNSUPPORTED, "bytes of LDS"), (lambda: psm(maxdisp=5000), UNSUPPORTED, "bytes of LDS"),
        (lambda: psm(B=1 << 30, H=16, Hout=16), UNSUPPORTED, "more than one launch takes"),
        (lambda: raft(flow=None), INVALID, bad), (lambda: raft(mask=None), INVALID, bad), (lambda: raft(out_=None), INVALID, bad),
        (lambda: raft(B=0), INVALID, bad), (lambda: raft(C=0), INVALID, bad), (lambda: raft(H4=0), INVALID, bad),
        (lambda: raft(W4=-2), INVALID, bad), (lambda: raft(sign=0), INVALID, "vppx_raft_upsample: bad arguments (sign is +1 or -1)"),
        (lambda: raft(sign=2), INVALID, "sign is +1 or -1"),
        (lambda: raft(dtype=2), INVALID, "vppx_raft_upsample: dtype 2 is neither VPPX_DT_F32 (0) nor VPPX_DT_BF16 (1)"),
        (lambda: raft(f=3, mc=81), INVALID, "vppx_raft_upsample: factor 3 is not 1, 2, 4 or 8"), (lambda: raft(f=16, mc=2304), INVALID, "factor 16"),
        (lambda: raft(f=0, mc=0), INVALID, "factor 0"), (lambda: raft(f=-2, mc=36), INVALID, "factor -2"),
        (lambda: raft(mc=9), INVALID, "vppx_raft_upsample: the mask has 9 channels, factor 2 takes 9*2*2 = 36"),
        (lambda: raft(f=4, mc=36, Hout=8, Wout=12), INVALID, "takes 9*4*4 = 144"),
        (lambda: raft(stride=5), INVALID, "vppx_raft_upsample: flow_frame_stride 5 is less than 1 planes of 2x3"),
        (lambda: raft(C=2, stride=6), INVALID, "flow_frame_stride"),
        (lambda: raft(top=-1), INVALID, "is not inside the 4x6 map"),
        (lambda: raft(left=1), INVALID, "vppx_raft_upsample: the window of 4x6 pixels at row 0, column 1 is not inside the 4x6 map"),
        (lambda: raft(Hout=5), INVALID, "is not inside"), (lambda: raft(Wout=0), INVALID, "is not inside"),
        (lambda: raft(top=3, Hout=2), INVALID, "is not inside"),
        (lambda: raft(B=1 << 30, H4=1 << 10, W4=1, Hout=1 << 11, Wout=2, stride=1 << 10), UNSUPPORTED, "more than one launch takes"),
    )
    for n, (call, code, msg) in enumerate(table):
        rc = call()
        text = lib.vppx_last_error().decode()
        assert rc == code and msg in text, (n, rc, code, msg, text)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL32).all() and (inp.cpu().numpy() == 1.0).all()
    # what is allowed: the smallest of everything, and a window of one pixel in the last corner
    assert psm(D4=1, H4=1, W4=1, maxdisp=1, H=1, W=1, Hout=1, Wout=1) == 0
    assert raft(f=1, mc=9, H4=1, W4=1, stride=1, Hout=1, Wout=1) == 0
    assert raft(top=3, left=5, Hout=1, Wout=1, sign=-1) == 0
    torch.cuda.synchronize()
    assert (inp.cpu().numpy() == 1.0).all() and (out.cpu().numpy()[1:] == SENTINEL32).all()

    # through Engine
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=eng.device)            # noqa: E731
    with pytest.raises(ValueError, match="cost must be"):
        eng.psmnet_disparity(f32(1, 2, 3, 2, 2), 12, (8, 8))
    with pytest.raises(ValueError, match="cost: expected contiguous"):
        eng.psmnet_disparity(f32(1, 3, 2, 2).double(), 12, (8, 8))
    with pytest.raises(ValueError, match="cost: expected contiguous"):
        eng.psmnet_disparity(f32(1, 3, 2, 4)[..., ::2], 12, (8, 8))
    with pytest.raises(ValueError, match="leaves nothing"):
        eng.psmnet_disparity(f32(1, 3, 2, 2), 12, (8, 8), crop=[4, 4, 0, 0])
    with pytest.raises(ValueError, match="crop must be"):
        eng.psmnet_disparity(f32(1, 3, 2, 2), 12, (8, 8), crop=[1, 1, -1, 0])
    with pytest.raises(ValueError, match="out: expected shape"):
        eng.psmnet_disparity(f32(1, 3, 2, 2), 12, (8, 8), crop=[1, 1, 1, 1], out=f32(1, 8, 8))
    with pytest.raises(VppxError) as e:
        eng.psmnet_disparity(f32(1, 3, 2, 2), 5000, (8, 8))
    assert e.value.code == UNSUPPORTED
    with pytest.raises(ValueError, match="mask: expected shape"):
        eng.raft_upsample(f32(1, 2, 2, 3), f32(1, 36, 2, 3))
    with pytest.raises(ValueError, match="same dtype"):
        eng.raft_upsample(f32(1, 2, 2, 3), f32(1, 144, 2, 3).bfloat16())
    with pytest.raises(ValueError, match="n_downsample"):
        eng.raft_upsample(f32(1, 2, 2, 3), f32(1, 144, 2, 3), n_downsample=4)
    with pytest.raises(ValueError, match="channels must be"):
        eng.raft_upsample(f32(1, 2, 2, 3), f32(1, 144, 2, 3), channels=3)
    with pytest.raises(ValueError, match="out: expected shape"):
        eng.raft_upsample(f32(1, 2, 2, 3), f32(1, 144, 2, 3), channels=1, out=f32(1, 2, 8, 12))


# ---- one context ------------------------------------------------------------------------------------------------
def test_readouts_between_two_rsgm_calls_change_nothing(eng):
    """Both read-outs sit between two vpp_rsgm calls on one context: the vpp_rsgm results are the bits of runs without
    them, and the read-outs' are the bits of their first calls."""
    import torch
    from vppstereo_amd.engine import Engine
    B, H, W, D = 2, 60, 112, 64
    b = synth.make_batch(B, H, W, D, 0.04, seed=11)
    left, right, hints = (torch.from_numpy(b[k]).to(eng.device) for k in ("left", "right", "hints"))
    pc, _ = _psm_ref("crop")
    rc, _ = _raft_ref("test_py")
    first_psm, first_raft = _psm(eng, pc).cpu().numpy(), _raft(eng, rc).cpu().numpy()
    plain = Engine()
    try:
        want = [plain.vpp_rsgm(left, right, hints, seed=s, rsgm_kw=dict(dmax=D)).cpu().numpy() for s in (3, 4)]
    finally:
        torch.cuda.synchronize()
        plain.ctx.close()
    one = Engine()
    try:
        a = one.vpp_rsgm(left, right, hints, seed=3, rsgm_kw=dict(dmax=D))
        mid_psm, mid_raft = _psm(one, pc), _raft(one, rc)
        z = one.vpp_rsgm(left, right, hints, seed=4, rsgm_kw=dict(dmax=D))
        one.synchronize()
        assert _same(a.cpu().numpy(), want[0]) and _same(z.cpu().numpy(), want[1])
        assert _same(mid_psm.cpu().numpy(), first_psm) and _same(mid_raft.cpu().numpy(), first_raft)
    finally:
        torch.cuda.synchronize()
        one.ctx.close()


def test_cropped_disparity_goes_into_the_metrics_without_a_copy(eng):
    import torch
    c, ref = _psm_ref("crop")
    disp = _psm(eng, c)
    B, Ho, Wo = disp.shape
    rng = np.random.default_rng(5)
    gt = (ref.value + rng.uniform(-5, 5, ref.value.shape)).astype(F32)
    valid = (rng.random(ref.value.shape) < 0.7).astype(F32)
    direct = eng.guided_metrics(disp, _dev(eng, gt), _dev(eng, valid)).cpu().numpy()
    through_numpy = eng.guided_metrics(_dev(eng, disp.cpu().numpy()), _dev(eng, gt), _dev(eng, valid)).cpu().numpy()
    assert direct.shape == (B, 8) and np.array_equal(direct.view(np.uint64), through_numpy.view(np.uint64))
    assert direct[0, 6] == valid.sum() and direct[0, 4] > 0
    # RAFT's output, sliced to its channel, is taken the same way
    rc, _ = _raft_ref("test_py")
    up = _raft(eng, rc)[:, 0]
    assert up.is_contiguous()
    g2 = torch.zeros_like(up)
    m = eng.guided_metrics(up, g2, torch.ones_like(up)).cpu().numpy()
    assert m[0, 6] == up[0].numel()
