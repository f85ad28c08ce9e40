"""CPU-side checks of the hint-sampling layer (losses.sample_hints on the device, include/vppx.h "hint sampling").

The device kernel reproduces torch's CPU random stream, so the first thing pinned here is what that stream IS: a numpy model of
it (MT19937 seeded with init_genrand(seed mod 2^32), one tempered word per element, 24 bits kept) must equal torch.rand_like.
If that fails on another torch build the oracle has drifted, not the kernel.  Then: the threshold rule against the float32
compare over the whole 2^24 lattice, the struct, the bindings, and the refusals that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from vppstereo_amd import _lib, losses, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vppx_sample_params_default", "vppx_sample_threshold", "vppx_sample_hints_dev", "vppx_sample_hints_host",
       "vppx_occ_vpp_rsgm_sampled_dev", "vppx_fstream_create_sampled", "vppx_fstream_push_sampled"]
SEEDS = [0, 1, 7, 2 ** 32 - 1, 2 ** 32 + 5, 2 ** 63 + 11, 123456789]
SHAPES = [(3, 5), (1, 227), (1, 624), (25, 25), (37, 53), (64, 80), (540, 960)]
PROBS = [0.0, 1e-9, 0.01, 0.03, 0.05, 0.2, 1.0 / 3.0, 0.5, 0.9999999999, 1.0]


class StreamModel:
    """torch's CPU generator as the kernel models it: raw MT19937 words from numpy's implementation of the same generator
    (RandomState(s) seeds with init_genrand(s)), k = word & 0xFFFFFF, rand = k * 2^-24; consecutive calls continue the stream."""

    def __init__(self, seed):
        self.bg = np.random.RandomState(int(seed) % 2 ** 32)._bit_generator

    def k(self, n):
        return (self.bg.random_raw(n) & 0xFFFFFF).astype(np.uint32)

    def rand(self, shape):
        return (self.k(int(np.prod(shape))).astype(np.float32) * np.float32(2.0 ** -24)).reshape(shape)


def model_sample_hints(src, validsrc, p, seed):
    """The rule of include/vppx.h for one frame."""
    k = StreamModel(seed).k(src.size).reshape(src.shape)
    sel = (validsrc > 0) & (k < _lib.sample_threshold(p))
    return np.where(sel, src, np.float32(0)), sel.astype(np.float32)


@pytest.mark.parametrize("seed", SEEDS)
def test_the_numpy_model_is_torchs_cpu_stream(seed):
    for shape in SHAPES:
        torch.manual_seed(seed)
        m = StreamModel(seed)
        for call in range(2):   # consecutive calls continue the stream
            want = torch.rand_like(torch.empty(shape), dtype=torch.float32).numpy()
            assert np.array_equal(m.rand(shape), want), (seed, shape, call)


def test_the_model_of_a_frame_is_losses_sample_hints():
    rng = np.random.default_rng(3)
    for shape, seed, p in (((37, 53), 5, 0.05), ((64, 80), 2 ** 32 - 1, 0.5), ((3, 5), 0, 1.0), ((25, 25), 9, 0.0)):
        src = rng.uniform(-3, 90, shape).astype(np.float32)
        valid = rng.choice(np.array([0, 0.5, 1, -1, np.nan], np.float32), shape)
        torch.manual_seed(seed)
        want = losses.sample_hints(torch.from_numpy(src), torch.from_numpy(valid) > 0, p)
        h, v = model_sample_hints(src, valid, p, seed)
        assert torch.equal(torch.from_numpy(h), want[0]) and torch.equal(torch.from_numpy(v), want[1].float())


@pytest.fixture(scope="module")
def lattice():
    return torch.arange(2 ** 24, dtype=torch.float32) * 2.0 ** -24


@pytest.mark.parametrize("p", PROBS + [2.0, -1.0, float("inf"), float("nan")])
def test_threshold_is_the_float32_compare_over_the_whole_lattice(lattice, p):
    T = _lib.sample_threshold(p)
    assert 0 <= T <= 2 ** 24
    assert T == int((lattice < p).sum())                     # the selected k are exactly 0 .. T-1 ...
    assert T == 0 or bool((lattice[:T] < p).all())           # ... a prefix of the lattice
    assert T == _lib.load().vppx_sample_threshold(p)         # the library's own rule is the same one


def test_new_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "vppx.h")).read()
    declared = set(re.findall(r"\b(vppx_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name
    assert "#define VPPX_FS_SAMPLE 64" in hdr and _lib.FS_SAMPLE == 64
    assert re.search(r"sample_hints\(\)\s+losses\.py:5-10", hdr)
    assert lib.vppx_version() == 100


def test_struct_defaults_equal_the_headers():
    hdr = open(os.path.join(ROOT, "include", "vppx.h")).read()
    body = re.search(r"typedef struct VppxSampleParams \{(.*?)\} VppxSampleParams;", hdr, re.S).group(1)
    stated = dict(re.findall(r"(\w+);\s*/\* \[([0-9.]+)\]", body))
    assert set(stated) == {"probability", "seed"}
    p = _lib.VppxSampleParams(probability=9.0, seed=77, reserved0=5, reserved1=6)
    _lib.load().vppx_sample_params_default(C.byref(p))
    assert (p.probability, p.seed, p.reserved0, p.reserved1) == (float(stated["probability"]), int(stated["seed"]), 0, 0)
    assert C.sizeof(_lib.VppxSampleParams) == 24
    q = _lib.sample_params(probability=0.2, seed=2 ** 32 - 1)
    assert (q.probability, q.seed) == (0.2, 2 ** 32 - 1)
    with pytest.raises(TypeError, match="reserved0"):
        _lib.sample_params(reserved0=1)


def test_the_header_is_c99_and_states_the_size_a_c_compiler_sees(tmp_path):
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("needs gcc")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "vppx.h"\nint main(void) { printf("%d %d\\n", (int)sizeof(VppxSampleParams), '
                   'VPPX_FS_SAMPLE); return 0; }\n')
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    assert subprocess.check_output([exe], text=True).split() == ["24", "64"]


def test_new_calls_without_a_context_fail_with_a_message():
    lib = _lib.load()
    d = np.zeros((1, 4, 4), np.float32)
    smp = _lib.sample_params()
    rc = lib.vppx_sample_hints_host(C.c_void_p(), C.byref(smp), 1, 4, 4, d.ctypes.data, d.ctypes.data, d.ctypes.data, None)
    assert rc == -7 and b"context is NULL" in lib.vppx_last_error()
    rc = lib.vppx_sample_hints_dev(C.c_void_p(), C.byref(smp), 1, 4, 4, None, None, None, None)
    assert rc == -7 and b"context is NULL" in lib.vppx_last_error()
    rc = lib.vppx_occ_vpp_rsgm_sampled_dev(C.c_void_p(), None, None, None, None, None, C.byref(smp), 1, 4, 4, 3, *([None] * 4), 0,
                                           *([None] * 12))
    assert rc == -7 and b"context is NULL" in lib.vppx_last_error()
    h = C.c_void_p()
    rc = lib.vppx_fstream_create_sampled(C.c_void_p(), None, None, None, None, None, C.byref(smp), 4, 3, 32, 64, 3, 64, 1, C.byref(h))
    assert rc == -7 and b"context is NULL" in lib.vppx_last_error() and not h
    rc = lib.vppx_fstream_push_sampled(C.c_void_p(), None, None, None, None, None, None, None)
    assert rc == -1 and b"stream is NULL" in lib.vppx_last_error()


def _unopened_stream(sample, metrics):
    """A FrameStream that never opened a device: what its push calls refuse first needs none."""
    fs = object.__new__(pipeline.FrameStream)
    fs._sample, fs._metrics, fs._h = sample, metrics, None
    return fs


def test_stream_refusals_need_no_device():
    l = np.zeros((32, 64, 3), np.uint8)
    h = np.zeros((32, 64), np.float32)
    # sample together with pushed hints
    for metrics in (False, True):
        fs = _unopened_stream(True, metrics)
        with pytest.raises(ValueError, match="sampled on the device"):
            fs.push(l, l, h)
        with pytest.raises(ValueError, match="sampled on the device"):
            fs.push_eval(l, l, h, gt=h, validgt=h)
    # src=None without metrics=True
    with pytest.raises(ValueError, match="metrics=True"):
        _unopened_stream(True, False).push_sampled(l, l)
    # src without validsrc (and the other way round)
    with pytest.raises(ValueError, match="go together"):
        _unopened_stream(True, True).push_sampled(l, l, src=h, gt=h, validgt=h)
    with pytest.raises(ValueError, match="go together"):
        _unopened_stream(True, False).push_sampled(l, l, validsrc=h)
    # push_sampled on a stream that does not sample
    with pytest.raises(ValueError, match="without sample="):
        _unopened_stream(False, True).push_sampled(l, l, src=h, validsrc=h, gt=h, validgt=h)
    with pytest.raises(ValueError, match="without sample="):
        _unopened_stream(False, True).push_sampled(l, l, gt=h, validgt=h)
    # the constructor's own refusals still come first
    with pytest.raises(ValueError, match="metrics=True"):
        pipeline.FrameStream(32, 64, sample=0.05, return_disp=False)


def test_run_frame_refusals_need_no_device():
    l = np.zeros((30, 64, 3), np.uint8)
    h = np.zeros((30, 64), np.float32)
    with pytest.raises(ValueError, match="hints=None"):
        pipeline.run_frame(l, l, h, sample=dict(probability=0.05, src=h, validsrc=h))
    with pytest.raises(ValueError, match="go together"):
        pipeline.run_frame(l, l, sample=dict(src=h))
    with pytest.raises(ValueError, match="gt / validgt"):
        pipeline.run_frame(l, l, sample=dict(probability=0.05))
    with pytest.raises(TypeError, match="unknown keys"):
        pipeline.run_frame(l, l, sample=dict(p=0.05))
    with pytest.raises(ValueError, match="sample=dict"):
        pipeline.run_frame(l, l)


def test_shards_sample_with_the_global_frame_index():
    from vppstereo_amd import dist
    s = dict(probability=0.05, seed=2 ** 32 - 2)
    assert dist.shard_sample(s, 0)["seed"] == 2 ** 32 - 2 and dist.shard_sample(s, 5)["seed"] == 3
    assert dist.shard_sample(dict(probability=0.1), 4) == dict(probability=0.1, seed=5) and s["seed"] == 2 ** 32 - 2
