"""The referee of tests/_motion_ref.py against the recording of the reference's own lines, the planted mistakes against
the referee's limit on the very arrays tests/test_gpu_motion.py uploads, and the new symbol's binding.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import _corr_ref as CR
import _motion_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
F32, F64 = np.float32, np.float64
_REFS = {}


def _ref(name, dtype="float32"):
    if (name, dtype) not in _REFS:
        c = R.case(name)
        _REFS[name, dtype] = (c, R.case_ref(c, dtype))
    return _REFS[name, dtype]


def test_the_referee_holds_the_recording():
    """torch's CPU convolution is a float32 sum in some order too: the reference alone stays inside the bound."""
    c, cor1, flo1 = R.golden_case()
    # the referee's taps are the recorded lookup bit for bit, and its pyramid is the recorded one
    taps = R.taps_of(c.pyr, c.coords, c.radius)
    assert CR.same_bits(CR.channels_first(taps, c.B, c.H4, c.W2), c.lookup) == 0
    for a, b in zip(CR.pyramid(c.level0, 4), c.pyr):
        assert CR.same_bits(a, b) == 0
    ref_c, ref_f = R.front(c.pyr, c.coords, c.flow, c.wc, c.bias_c, c.wf, c.bias_f, c.radius)
    for what, got, ref in (("cor1", cor1, ref_c), ("flo1", flo1, ref_f)):
        worst, beyond, other = R.compare(got, ref)
        print(f"recording {what}: worst |got - value| / limit {worst:.3f}, {beyond} beyond, {other} of another class, "
              f"{int((got == 0).sum())} of {got.size} cells cut by the ReLU")
        assert beyond == 0 and other == 0
        assert 0.2 < (got == 0).mean() < 0.8                     # the ReLU cuts on both sides
    # the recording's coordinates reach outside the row on both sides, where every tap is +0
    zero = (taps.view(np.uint32) == 0).all(axis=1)
    assert zero.sum() >= 4
    want = np.maximum(c.bias_c, 0)
    assert all(np.array_equal(cor1.transpose(0, 2, 3, 1).reshape(c.N, -1)[n], want) for n in np.flatnonzero(zero))


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("name", list(R.CASES))
def test_every_planted_mistake_leaves_the_limit(name, dtype):
    """dtype is the pyramid's.  Per mistake: the share of cells of the output it touches that leave the float32 limit, and
    that leave the band of a bfloat16 output."""
    c, (ref_c, ref_f) = _ref(name, dtype)
    assert R.misses(R.case_ref(c, dtype)[0].value, ref_c) == 0
    for plant in R.PLANTED:
        pc, pf = R.planted(c, plant, dtype)
        sc, sf = (R.compare(pc, ref_c)[1] + R.compare(pc, ref_c)[2]) / pc.size, (R.compare(pf, ref_f)[1] + R.compare(pf, ref_f)[2]) / pf.size
        bc = sum(R.compare_bf16(R.BR.rne64(pc), ref_c)) / pc.size
        bf = sum(R.compare_bf16(R.BR.rne64(pf), ref_f)) / pf.size
        print(f"{name} [{dtype}] {plant}: cor1 {sc:.3f} (bfloat16 output {bc:.3f}), flo1 {sf:.3f} (bfloat16 output {bf:.3f}) of the cells leave")
        if plant == "tap_order":
            assert (sc > 0.3 and bc > 0.3 and sf == 0) if c.levels > 1 and c.radius > 0 else sc == 0      # one level or one tap: no order
        elif plant == "taps_bf16":
            assert sc > 0.3 and sf == 0
            assert bc > 0.0 if name != "k1_ks1" else True       # a bfloat16 output hides most of it: the float32 output is the check
        elif plant == "flipped":
            assert (sf > 0.3 and bf > 0.3 and sc == 0) if c.ks > 1 else sf == 0
        elif plant == "replicate":
            assert (sf > 0.2 and bf > 0.2 and sc == 0) if c.ks > 1 else sf == 0
        elif plant == "flow_swapped":
            assert sf > 0.3 and bf > 0.3 and sc == 0
        elif plant == "no_bias":
            assert sc > 0.2 and sf > 0.2 and bc > 0.2 and bf > 0.2
        elif plant == "no_relu":
            assert sc > 0.2 and sf > 0.2 and bc > 0.2 and bf > 0.2


def test_what_the_cases_reach():
    for name, (B, H4, W2, W3, levels, radius, ks, Cc, Cf) in R.CASES.items():
        c, (ref_c, ref_f) = _ref(name)
        assert c.K == levels * (2 * radius + 1)
        # every class of directed coordinate is there, one pixel each, and the far ones give relu(bias) exactly
        d = np.concatenate(list(CR.directed_coords(W3).values()))
        assert np.array_equal(c.coords.reshape(-1)[:len(d)].view(np.uint32), d.view(np.uint32))
        zero = R.zero_tap_pixels(c)
        far = sum(len(CR.directed_coords(W3)[k]) for k in ("far_outside", "huge", "inf", "nan"))
        assert zero.sum() >= far
        v = ref_c.value.transpose(0, 2, 3, 1)[zero]
        assert np.array_equal(v, np.broadcast_to(np.maximum(c.bias_c.astype(F64), 0), v.shape))
        for ref in (ref_c, ref_f):                               # the ReLU cuts on both sides
            assert 0.2 < (ref.value == 0).mean() < 0.8
            assert (ref.limit[ref.value > 0] < 1e-4 * ref.value[ref.value > 0].max()).all()
    assert R.CASES["k15_ks3"][4] * (2 * R.CASES["k15_ks3"][5] + 1) % 4 == 3 and R.case("k1_ks1").K == 1
    assert R.CASES["low_map"][1] < R.CASES["low_map"][6] and R.CASES["low_map"][2] % 16 == 3
    assert R.CASES["w2_ne_w3"][2] != R.CASES["w2_ne_w3"][3] and R.case("w2_ne_w3").N > 2 * 128 and R.case("w2_ne_w3").N % 128
    t = R.CASES["tiles"]
    assert t[2] == 16 and (t[1] * t[2]) % 8 == 0 and t[0] * t[1] * t[2] < 128 and t[3] >> 3 == 2
    # the flow's planted NaN reaches exactly its window, the inf as well, with the sign of its weight under the ReLU
    c = R.case("low_map", nonfinite=True)
    _, ref_f = R.case_ref(c)
    b, ch, y, x = R.NONFINITE_FLOW["nan"]
    nan = np.isnan(ref_f.value)
    want = np.zeros_like(nan)
    want[b, :, max(y - 3, 0):y + 4, max(x - 3, 0):x + 4] = True
    assert np.array_equal(nan, want)
    b, ch, y, x = R.NONFINITE_FLOW["inf"]
    cls = R.classes(ref_f.value)
    assert (cls == 2).sum() > 100 and ((cls == 2).sum(axis=(0, 1))[max(y - 3, 0):y + 4, max(x - 3, 0):x + 4] > 0).all() and (cls == 3).sum() == 0


def test_the_new_symbol_is_exported_and_bound():
    from vppstereo_amd import _lib
    lib = _lib.load()
    i, vp, i64 = C.c_int, C.c_void_p, C.c_int64
    name = "vppx_raft_motion_front_dt_dev"
    assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.vppx_raft_motion_front_dt_dev.argtypes == [vp, vp, vp, vp, i64, vp, i64, vp, vp, i, vp, vp, i, i, i, i, i, i, i, i, vp, i64, vp,
                                                          i64, i, i]
    assert (_lib.MOTION_MAX_CH, _lib.MOTION_MAX_KS) == (64, 7)
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "vppx.h")).read()
    assert "#define VPPX_MOTION_MAX_CH 64" in hdr and "#define VPPX_MOTION_MAX_KS 7" in hdr
    assert "BasicMotionEncoder convc1 / convf1" in hdr and "update.py:80,82" in hdr
