"""The referee of the 3x3 convolution and the ConvGRU made of it (tests/_gruconv_ref.py), held to the recording of the
reference's own ConvGRU.forward (tests/golden/gruconv_cases.npz), and its planted mistakes on the arrays tests/test_gpu_gruconv.py
uploads; and the new entry points in the header, the library and the derived binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _gruconv_ref as R

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vppx_raft_conv3x3_packed_bytes", "vppx_raft_conv3x3_pack_dev", "vppx_raft_conv3x3_dt_dev", "vppx_raft_gru_zr_dt_dev",
           "vppx_raft_gru_q_dt_dev")
# planted mistake -> the cases of the GPU file that claim to catch it
CONV_CATCHES = {"flipped": ("1x9", "9x1", "odd", "tiles"), "replicate": ("1x1", "1x9", "9x1", "odd", "tiles"),
                "transposed": ("1x1", "1x9", "9x1"), "swapped": ("odd",), "no_bias": ("1x1", "1x9", "9x1", "odd", "tiles")}
GRU_CATCHES = {"zr_swapped": ("odd",), "h_into_q": ("odd",), "z_complement": ("odd",)}
_REFS = {}


def _conv_ref(name):
    if name not in _REFS:
        c = R.case(name)
        _REFS[name] = (c, R.case_ref(c))
    return _REFS[name]


def _gru_ref(name):
    if ("gru", name) not in _REFS:
        c = R.gru_case(name)
        _REFS["gru", name] = (c, R.gru_case_ref(c))
    return _REFS["gru", name]


def test_the_convolution_is_torchs():
    """The float64 convolution against F.conv2d on the CPU, two sources, with and without the bias and the ReLU."""
    import torch
    import torch.nn.functional as F
    c, ref = _conv_ref("odd")
    x = torch.from_numpy(np.concatenate([c.x0, c.x1], axis=1))
    want = F.conv2d(x.double(), torch.from_numpy(c.w).double(), torch.from_numpy(c.bias).double(), padding=1).numpy()
    assert np.abs(ref.value - want).max() <= 1e-12 and (ref.limit > 0).all() and ref.limit.max() < 1e-3       # K + 1 = 289 roundings of sums of order 20
    got32 = F.conv2d(x, torch.from_numpy(c.w), torch.from_numpy(c.bias), padding=1).numpy()
    assert R.misses(got32, ref) == 0                     # a float32 evaluation lies inside the limit
    plain = R.conv3x3(c.x0, c.x1, c.w, None, relu=True)
    want = F.relu(F.conv2d(x.double(), torch.from_numpy(c.w).double(), padding=1)).numpy()
    assert np.abs(plain.value - want).max() <= 1e-12
    # bfloat16 storage: the weights are rounded once, the products are then exact in float32
    cb = R.case("odd", "bfloat16")
    refb = R.case_ref(cb)
    xb = torch.from_numpy(np.concatenate([cb.x0, cb.x1], axis=1)).double()
    wantb = F.conv2d(xb, torch.from_numpy(R.to_bf16(cb.w)).double(), torch.from_numpy(cb.bias).double(), padding=1).numpy()
    assert np.abs(refb.value - wantb).max() <= 1e-12
    assert np.abs(refb.value - F.conv2d(xb, torch.from_numpy(cb.w).double(), torch.from_numpy(cb.bias).double(), padding=1).numpy()).max() > 1e-4


def test_the_referee_reproduces_the_recording():
    g = R.load_recording()
    assert all(a.dtype == F32 for a in g.values()) and os.path.getsize(R.GOLDEN) < 466584
    for name, n_x in R.RECORDED.items():
        h0, ctx, xs, W = R.recorded_case(g, name)
        assert len(xs) == n_x and h0.shape[1] == 16 and ctx.shape[1] == 48
        x = np.concatenate(xs, axis=1)
        calls = R.recorded_ref(g, name)
        h = h0
        for k, ref in enumerate(calls, start=1):
            for cv in ("convz", "convr"):
                a = R.conv3x3(h, x, W[f"{cv}_weight"], W[f"{cv}_bias"])
                assert R.misses(g[f"{name}_call{k}_{cv}_out"], a) == 0, (name, k, cv)
            rec = g[f"{name}_h{k}"]
            worst, beyond, other = R.compare(rec, ref)
            print(f"{name} call {k}: recorded h against the referee, worst |h - value| / limit {worst:.3f}")
            assert beyond == 0 and other == 0, (name, k, worst)
            # convq's recorded output: its input is cat([r*h, x]) with the recorded r
            r = 1.0 / (1.0 + np.exp(-(g[f"{name}_call{k}_convr_out"].astype(F64) + ctx[:, 16:32])))
            aq = R.conv3x3(r * h, x, W["convq_weight"], W["convq_bias"], x0_limit=4 * R.U * np.abs(r * h))
            assert R.misses(g[f"{name}_call{k}_convq_out"], aq) == 0, (name, k)
            h = rec


def test_the_recorded_gates_do_not_all_saturate():
    g = R.load_recording()
    for name in R.RECORDED:
        cz, cr, _ = np.split(g[f"{name}_ctx"].astype(F64), 3, axis=1)
        for k in (1, 2):
            for cv, c in (("convz", cz), ("convr", cr)):
                gate = 1.0 / (1.0 + np.exp(-(g[f"{name}_call{k}_{cv}_out"] + c)))
                assert ((gate > 0.05) & (gate < 0.95)).mean() >= 0.25, (name, k, cv)


@pytest.mark.parametrize("planted", list(CONV_CATCHES))
def test_a_planted_convolution_leaves_the_limit(planted):
    for name in CONV_CATCHES[planted]:
        c, ref = _conv_ref(name)
        wrong = R.case_ref(c, **R.CONV_KW[planted]).value
        assert R.misses(wrong, ref) > 0, (planted, name)
        assert R.misses(ref.value, ref) == 0


@pytest.mark.parametrize("planted", list(GRU_CATCHES))
def test_a_planted_gru_leaves_the_limit(planted):
    for name in GRU_CATCHES[planted]:
        c, ref = _gru_ref(name)
        wrong = R.gru_case_ref(c, **{planted: True})
        assert R.misses(wrong.value, ref) > 0, (planted, name)
        if planted == "zr_swapped":
            assert R.misses(wrong.z.value, ref.z) > 0 and R.misses(wrong.rh.value, ref.rh) > 0
        if planted == "h_into_q":                       # the zr call is right, the q call reads the wrong buffer
            assert R.misses(wrong.z.value, ref.z) == 0 and R.misses(wrong.rh.value, ref.rh) == 0


def test_the_planted_mistakes_are_all_claimed():
    assert set(R.PLANTED) == set(CONV_CATCHES) | set(GRU_CATCHES)
    for name in set(sum(CONV_CATCHES.values(), ())):
        assert name in R.CASES
    # on the recording too: a wrong convolution does not hide behind the gates
    g = R.load_recording()
    ref = R.recorded_ref(g, "a")
    for planted in ("flipped", "replicate", "swapped", "no_bias"):
        wrong = R.recorded_ref(g, "a", **R.CONV_KW[planted])
        assert R.misses(wrong[1].value, ref[1]) > 0, planted
    for planted in GRU_CATCHES:
        assert R.misses(R.recorded_ref(g, "a", **{planted: True})[1].value, ref[1]) > 0, planted


def test_the_gate_plants_saturate_without_nan():
    c, ref = _gru_ref("odd")
    cz, cr, cq = np.split(c.ctx, 3, axis=1)
    assert ref.z.value[0, 0, 0, 1] == 1.0 and ref.z.value[0, 1, 1, 2] == 0.0 and ref.rh.value[0, 2, 3, 4] == 0.0
    assert ref.rh.value[0, 0, 2, 3] == c.h[0, 0, 2, 3] and ref.value[0, 1, 1, 2] == c.h[0, 1, 1, 2]      # r = 1;  z = 0 there
    assert np.isfinite(ref.value).all() and np.isfinite(ref.z.value).all()
    assert ref.z.limit[0, 0, 0, 1] == 0.0


def test_the_new_entry_points_are_declared_exported_and_bound():
    from vppstereo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vppx.h")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.EXPORTS and name in _lib.ABI.protos, name
        assert getattr(lib, name).argtypes is not None
    assert lib.vppx_raft_conv3x3_packed_bytes.restype is C.c_size_t
    assert lib.vppx_raft_conv3x3_packed_bytes.argtypes == [C.c_int, C.c_int, C.c_int]
    assert lib.vppx_raft_gru_zr_dt_dev.argtypes[-1] is C.c_void_p and len(lib.vppx_raft_gru_zr_dt_dev.argtypes) == 23
    assert len(lib.vppx_raft_gru_q_dt_dev.argtypes) == 21 and len(lib.vppx_raft_conv3x3_dt_dev.argtypes) == 16
    assert (_lib.CONV_MAX_CIN, _lib.CONV_MAX_COUT) == (512, 256)
    # the size is host arithmetic: one promise (it serves any B, H, W), and 0 for what is not built
    size = lib.vppx_raft_conv3x3_packed_bytes
    assert size(256, 384, _lib.DT_BF16) > 256 * 384 * 9 * 2 and size(256, 384, _lib.DT_F32) > 256 * 384 * 9 * 4
    assert size(16, 16, _lib.DT_BF16) >= 16 * 16 * 9 * 2 + 16 * 4
    for bad in ((8, 16, 0), (16, 8, 0), (272, 16, 0), (16, 528, 1), (16, 16, 2), (0, 16, 0), (16, -16, 1)):
        assert size(*bad) == 0, bad
    # a NULL context: the context is checked first, as everywhere
    assert lib.vppx_raft_conv3x3_pack_dev(None, None, 16, 16, 0, None, None) == -7 and b"context is NULL" in lib.vppx_last_error()
