"""CPU: the float64 referee of the encoders' glue (tests/_norm_ref.py) against the arrays the reference's own lines produced
(tests/golden/extractor_cases.npz), the planted mistakes on those very arrays, and what of the new entry points needs no
device: the exports, the NULL-handle sweep, vppx_norm_stats_pieces, and what FusedEncoder refuses."""
import ctypes as C

import numpy as np
import pytest
import torch

import _norm_ref as N
from vppstereo_amd import _header, _lib

G = N.load_recording()
NEW = ("vppx_raft_norm_stats_dt_dev", "vppx_raft_norm_apply_dt_dev", "vppx_norm_stats_pieces")


def _held(unit, plant=None):
    """-> (stages compared, cells beyond limit_any_f32 or of another class) of a unit's recorded norm-stage results."""
    stages = N.unit_stages(G, unit, any_f32=True, plant=plant)
    bad = 0
    for key, ref in stages.items():
        rec = N.recorded_stage(G, unit, key)
        ref = N._ns(ref.value[:rec.shape[0]], ref.limit[:rec.shape[0]])        # dual_inp: the heads read the first half
        _, beyond, other = N.compare(rec, ref)
        bad += beyond + other
    return len(stages), bad


@pytest.mark.parametrize("unit", N.UNITS)
def test_the_referee_reproduces_the_recording(unit):
    n, bad = _held(unit)
    assert n >= 2 and bad == 0, (unit, n, bad)


def test_the_recording_reaches_every_branch():
    assert len(N.unit_stages(G, "basic")) == 1 + 2 * 6 and len(N.unit_stages(G, "multi")) == 1 + 2 * 14
    for unit in ("rb_in_s2", "rb_bn_s2"):
        assert f"{unit}/downsample.0/out" in G.files
    assert "rb_bn_s2/norm3/running_var" in G.files and "rb_in_s2/norm3/running_var" not in G.files
    for k in ("running_mean", "running_var", "weight", "bias"):                 # away from (0, 1, 1, 0)
        a = G[f"multi/norm1/{k}"]
        assert np.abs(a - {"running_mean": 0, "running_var": 1, "weight": 1, "bias": 0}[k]).mean() > 0.1
    # dual_inp: three lists of two heads and the full-batch v; the list input of the basic encoder splits in two
    assert [G[f"multi/result/{i}/{j}"].shape[0] for i in range(3) for j in range(2)] == [1] * 6 and G["multi/result/3"].shape[0] == 2
    assert G["basic/result/0"].shape == G["basic/result/1"].shape == (1, 16, 2, 1)
    assert conv_cells("multi", "layer5.0.conv1") == 2                           # layer5 still reads more than one cell


def conv_cells(unit, path):
    a = N.conv_in(G, unit, path)
    return a.shape[2] * a.shape[3]


# which recorded units a planted mistake has to show on
PLANT_UNITS = {"unbiased": ("rb_in_s1", "rb_in_s2", "basic"), "eps_outside": ("rb_in_s1", "rb_bn_s1", "multi"),
               "no_inner_relu": N.UNITS, "relu_first": N.UNITS, "no_norm3": ("rb_in_s2", "rb_bn_s2", "basic", "multi"),
               "per_batch": ("rb_in_s1", "rb_in_s2", "basic"), "batch_stats": ("rb_bn_s1", "rb_bn_s2", "multi")}


@pytest.mark.parametrize("plant", N.PLANTS)
def test_a_planted_mistake_leaves_the_limit(plant):
    for unit in PLANT_UNITS[plant]:
        assert _held(unit, plant)[1] > 0, (plant, unit)


def test_the_limit_is_derived_not_loose():
    """limit() (the library's arithmetic) is far inside limit_any_f32() and both are relative: no floor under small values."""
    y = N.conv_out(G, "rb_in_s1", "conv1")
    tight, wide = N.apply(y, N.stats(y)), N.apply(y, N.stats(y, unit=N.U), any_f32=True)
    assert np.array_equal(tight.value, wide.value)
    pos = tight.value > 0
    assert (tight.limit[pos] < wide.limit[pos]).all() and (tight.limit[pos] / tight.value[pos]).max() < 1e-4
    s = N.stats(np.full((1, 1, 1, 1), 3.0, np.float32))
    assert s.mean[0, 0] == 3.0 and abs(s.rstd[0, 0] - 1 / np.sqrt(1e-5)) < 1e-9 and s.drstd[0, 0] < 1e-4
    for bad in (np.nan, np.inf):                       # a non-finite cell takes its plane, and only its plane
        x = np.ones((1, 2, 2, 2), np.float32)
        x[0, 1, 0, 0] = bad
        v = N.apply(x, N.stats(x)).value
        assert np.isnan(v[0, 1]).all() and np.isfinite(v[0, 0]).all()


def test_exports_and_null_sweep():
    lib = _lib.load()
    assert all(n in _lib.EXPORTS and hasattr(lib, n) for n in NEW)
    for name in NEW[:2]:
        fn = getattr(lib, name)
        assert fn.argtypes[-1] is C.c_void_p and fn.restype is C.c_int             # the context goes last
        rc = fn(*[0.0 if t in (C.c_float, C.c_double) else 0 if t in _header.SCALARS.values() else None for t in fn.argtypes])
        assert rc == _lib._K["VPPX_E_NO_DEVICE"] and b"context is NULL" in lib.vppx_last_error(), name
    vp, i, i64, d = C.c_void_p, C.c_int, C.c_int64, C.c_double
    assert list(lib.vppx_raft_norm_stats_dt_dev.argtypes) == [vp, i64, i, i, i, i, d, vp, i, vp]
    assert list(lib.vppx_raft_norm_apply_dt_dev.argtypes) == [vp, i64, vp, i64, vp, vp, i, vp, i64, vp, i64, vp, vp, vp, i64, i, i, i, i, i, vp]
    assert list(lib.vppx_norm_stats_pieces.argtypes) == [i64, i64]


def test_norm_stats_pieces():
    f = _lib.load().vppx_norm_stats_pieces
    assert f(4096, 64) == 1 and f(128 * 64, 35) == 1 and f(1 << 20, 1 << 20) == 1       # many planes: one piece each
    assert f(128, 544 * 960) >= 2 and f(2, 40200) >= 3 and f(1, 1 << 30) >= 2           # few large planes
    assert f(1, 1) == 1 and f(1, 16) == 1                                               # small planes are never cut
    for planes, cells in ((0, 0), (-1, 5), (5, -1), (1 << 40, 1 << 40), (1, 1 << 62)):
        assert f(planes, cells) >= 1
    cells = [1, 7, 16384, 16385, 40200, 10 ** 5, 544 * 960, 10 ** 7, 10 ** 9]
    planes = [1, 2, 3, 64, 128, 512, 2048, 2049, 10 ** 6]
    for p in planes:
        row = [f(p, c) for c in cells]
        assert row == sorted(row) and min(row) >= 1, (p, row)                           # not decreasing in the cells
    for c in cells:
        col = [f(p, c) for p in planes]
        assert col == sorted(col, reverse=True), (c, col)                               # not increasing in the planes


class _Block(torch.nn.Module):
    def __init__(self, norm):
        super().__init__()
        self.conv1, self.conv2 = torch.nn.Conv2d(4, 4, 3, padding=1), torch.nn.Conv2d(4, 4, 3, padding=1)
        self.norm1, self.norm2, self.downsample = norm(), norm(), None


class _Encoder(torch.nn.Module):
    def __init__(self, norm, dropout=None):
        super().__init__()
        self.conv1, self.norm1, self.conv2 = torch.nn.Conv2d(3, 4, 3, padding=1), norm(), torch.nn.Conv2d(4, 4, 1)
        self.layer1, self.layer2, self.layer3 = (torch.nn.Sequential(_Block(norm)) for _ in range(3))
        self.dropout = dropout


def test_fused_encoder_refuses_what_it_does_not_compute():
    from vppstereo_amd.extractor import FusedEncoder
    inst, batch = (lambda: torch.nn.InstanceNorm2d(4)), (lambda: torch.nn.BatchNorm2d(4))
    FusedEncoder(_Encoder(inst))                                                        # wrapping needs no device
    FusedEncoder(_Encoder(lambda: torch.nn.InstanceNorm2d(4, affine=True)))
    FusedEncoder(_Encoder(batch).eval())
    FusedEncoder(_Encoder(inst, torch.nn.Dropout2d(0.5)).eval())
    with pytest.raises(TypeError, match="GroupNorm"):
        FusedEncoder(_Encoder(lambda: torch.nn.GroupNorm(1, 4)))
    with pytest.raises(TypeError, match="training mode"):
        FusedEncoder(_Encoder(batch))                                                   # a fresh module is in training mode
    with pytest.raises(TypeError, match="running statistics"):
        FusedEncoder(_Encoder(lambda: torch.nn.InstanceNorm2d(4, track_running_stats=True)))
    with pytest.raises(TypeError, match="Sequential"):
        FusedEncoder(_Encoder(lambda: torch.nn.Sequential()))                           # norm_fn='none'
    with pytest.raises(TypeError, match="dropout"):
        FusedEncoder(_Encoder(inst, torch.nn.Dropout2d(0.5)))
    enc = _Encoder(batch).eval()
    enc.layer2[0].norm2.train()                                                         # one norm deep inside
    with pytest.raises(TypeError, match="layer2.0.norm2"):
        FusedEncoder(enc)
    with pytest.raises(TypeError, match="conv1"):
        FusedEncoder(torch.nn.Sequential())
    wrapped = FusedEncoder(_Encoder(inst))
    assert wrapped.conv1 is wrapped.encoder.conv1 and set(wrapped.state_dict()) == {"encoder." + k for k in wrapped.encoder.state_dict()}
