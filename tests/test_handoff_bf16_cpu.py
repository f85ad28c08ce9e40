"""tests/_handoff_bf16_ref.py without a GPU: the two rounding helpers against each other and against torch, the band
against the float32 referee and the reference's expression in torch, the band against three wrong kernels, every
coverage claim tests/test_gpu_handoff_bf16.py makes about its inputs (asserted on those inputs), and the C-ABI's new
names in the header, the library and the binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _handoff_bf16_ref as BR
import _handoff_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_EXP_ULPS = 1.0           # tests/test_gpu_handoff_ref.py's figure for the device's expf
TORCH_EXP_ULPS = 1.0            # tests/test_handoff_ref_cpu.py's figure for torch's float32 exp on the CPU (Sleef)


@pytest.fixture(scope="module")
def psm():
    """name -> (case, referee), computed once and left unchanged."""
    out = {}
    for name in BR.PSM_NAMES:
        c = BR.psm_case(name)
        out[name] = (c, BR.psm_ref(c))
    return out


@pytest.fixture(scope="module")
def raft():
    out = {}
    for name in R.RAFT_CASES:
        c = BR.raft_case(name)
        out[name] = (c, BR.raft_ref(c))
    return out


# ---- rounding ---------------------------------------------------------------------------------------------
def _float32_samples():
    rng = np.random.default_rng(61)
    u = rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32)
    edge = np.array([0x00000000, 0x80000000, 0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x00017FFF, 0x007F8000,
                     0x007FFFFF, 0x00800000, 0x3F808000, 0x3F818000, 0x3F808001, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0x7F800000,
                     0xFF800000, 0xFF7F8000, 0x7FC00000, 0x7F800001, 0xFFC12345, 0x7F80FFFF], np.uint32)
    return np.concatenate([edge, u]).view(np.float32)


def test_the_two_roundings_and_torch_agree_on_float32():
    import torch
    x = _float32_samples()
    a = BR.bf16_rne_f32(x)
    nan = np.isnan(x)
    assert np.isnan(a[nan]).all() and not np.isnan(a[~nan]).any()
    assert not (a.view(np.uint32) & 0xFFFF).any()
    with np.errstate(invalid="ignore"):                         # signalling NaNs among the samples
        b = BR.rne64(x.astype(np.float64))
    assert np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))
    t = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(BR.bits(a)[~nan], t[~nan])
    assert (np.isnan(BR.widen(t[nan]))).all()
    # overflow and the subnormal grid, by hand
    top = float(BR.BF16_MAX)
    assert BR.rne64(top + 2.0 ** 119 - 2.0 ** 80) == BR.BF16_MAX and np.isinf(BR.rne64(top + 2.0 ** 119))     # the tie goes to even
    assert BR.rne64(2.0 ** -134) == 0 and BR.rne64(2.0 ** -134 + 2.0 ** -180) == np.float32(2.0 ** -133)
    assert BR.rne64(3 * 2.0 ** -134) == np.float32(2.0 ** -132) and BR.rne64(-2.0 ** -133) == np.float32(-2.0 ** -133)


def test_rne64_is_one_rounding_where_two_would_differ():
    """1 + 2^-8 + 2^-30 lies above the tie between 1 and 1 + 2^-7: a rounding to float32 first lands on the tie, and
    the second rounding then goes to even, down."""
    x = 1.0 + 2.0 ** -8 + 2.0 ** -30
    assert BR.rne64(x) == np.float32(1 + 2.0 ** -7)
    assert BR.bf16_rne_f32(np.array([x], np.float32))[0] == np.float32(1.0)
    # against the rounding done in exact rational arithmetic
    import math
    from fractions import Fraction
    rng = np.random.default_rng(67)
    d = rng.standard_normal(4000) * np.exp2(rng.integers(-140, 129, 4000))
    got = BR.rne64(d)
    for x, g in zip(d.tolist(), got.tolist()):
        q = max(math.frexp(x)[1] - 8, -133)
        n = Fraction(abs(x)) / Fraction(2) ** q
        f = math.floor(n)
        f += 1 if n - f > Fraction(1, 2) or (n - f == Fraction(1, 2) and f % 2) else 0
        r = f * Fraction(2) ** q
        want = math.inf if r > Fraction(float(BR.BF16_MAX)) else float(r)
        assert g == math.copysign(want, x), (x, g, want)
    assert np.isinf(got).any() and (np.abs(got[got != 0]) < 2.0 ** -126).any()


# ---- the band ---------------------------------------------------------------------------------------------
def _count(ref, got32):
    cells = BR.modulated_normal(ref)
    return int(cells.sum()), int((BR.outside(got32, ref, DEVICE_EXP_ULPS) & cells).sum()), int((BR.two_valued(ref, DEVICE_EXP_ULPS) & cells).sum())


def test_the_referee_rounded_once_is_inside_the_band(psm, raft):
    for what, table in (("psm", psm), ("raft", raft)):
        total = [0, 0, 0]
        for name, (c, ref) in table.items():
            got = BR.bf16_rne_f32(ref.out)
            assert not BR.outside(got, ref, DEVICE_EXP_ULPS).any(), (what, name)      # every modulated cell, small ones included
            total = [a + b for a, b in zip(total, _count(ref, got))]
        print(f"{what}: {total[0]} modulated cells of normal size, {total[1]} outside, {total[2]} with a band of two values")
        assert total[0] > 10000 and total[1] == 0
        assert total[2] < total[0] / 100                         # the band is one value nearly everywhere: it is a bit-exact check there


def _torch_psm(c):
    """psmnet.py:157-197 written out in torch float32 on the CPU (tools/bench_handoff.py::torch_ref), cast once."""
    import torch
    fl, fr, hints, valid = (torch.from_numpy(np.array(a)) for a in (c.fl, c.fr, c.hints, c.valid))
    B, Cc, H4, W4 = fl.shape
    D4 = c.maxdisp // 4
    cost = torch.zeros((B, 2 * Cc, D4, H4, W4))
    for i in range(min(D4, W4)):
        if i > 0:
            cost[:, :Cc, i, :, i:] = fl[:, :, :, i:]
            cost[:, Cc:, i, :, i:] = fr[:, :, :, :-i]
        else:
            cost[:, :Cc, i], cost[:, Cc:, i] = fl, fr
    h = torch.nn.functional.interpolate(hints, size=[c.H // 4, c.W // 4], mode="nearest").squeeze(1)
    v = torch.nn.functional.interpolate(valid, size=[c.H // 4, c.W // 4], mode="nearest").squeeze(1)
    h = (h * v / 4.0).unsqueeze(1).unsqueeze(2).expand(-1, 2 * Cc, D4, -1, -1)
    v = v.unsqueeze(1).unsqueeze(2).expand(-1, 2 * Cc, D4, -1, -1)
    d = torch.linspace(0, D4 - 1, D4).view(1, 1, -1, 1, 1).expand(B, 2 * Cc, -1, H4, W4)
    out = cost * ((1 - v) + v * 10.0 * torch.exp(-(d - h) ** 2 / (2 * 0.25 ** 2)))
    return out.to(torch.bfloat16).float().numpy()


def _torch_raft(c):
    """corr.py:160-178 in torch float32 on the CPU, cast once."""
    import torch
    corr, hints, valid = (torch.from_numpy(np.array(a)) for a in (c.corr, c.hints, c.valid))
    B, H4, W2, _, W3 = corr.shape
    h = torch.nn.functional.interpolate(hints, size=[H4, W2], mode="nearest").squeeze(1)
    v = torch.nn.functional.interpolate(valid, size=[H4, W2], mode="nearest").squeeze(1)
    x = torch.arange(W2, dtype=torch.float32).view(1, 1, -1).expand(B, H4, -1)
    t = (x * v - h * v / 4.0)[..., None, None]
    v = v[..., None, None]
    k = torch.arange(W3, dtype=torch.float32).view(1, 1, 1, 1, -1)
    out = corr * ((1 - v) + v * 10.0 * torch.exp(-(k - t) ** 2 / (2 * 1.0 ** 2)))
    return out.to(torch.bfloat16).float().numpy()


def test_the_references_expression_in_torch_cast_once_is_inside_the_band(psm, raft):
    for name, (c, ref) in psm.items():
        got = _torch_psm(c)
        assert not BR.outside(got, ref, TORCH_EXP_ULPS).any(), name
        keep = (ref.v == 0) & ~np.isnan(ref.out64)               # finite hints: times exactly 1
        assert np.array_equal(got[keep], ref.plain[keep]), name
    for name, (c, ref) in raft.items():
        assert not BR.outside(_torch_raft(c), ref, TORCH_EXP_ULPS).any(), name


@pytest.mark.parametrize("mutant", ["truncate", "bf16_factor", "strict_cut"])
def test_the_band_rejects_a_wrong_kernel(psm, raft, mutant):
    """More than 1 % of the modulated normal-size cells leave the band (a condition set beforehand, not a measurement)."""
    fn = getattr(BR, "mutant_" + mutant)
    for what, table in (("psm", psm), ("raft", raft)):
        if what == "raft" and mutant == "strict_cut":
            continue                                             # the RAFT kernel has no cut
        cells = out = 0
        for name, (c, ref) in table.items():
            m = BR.modulated_normal(ref)
            cells += int(m.sum())
            out += int((BR.outside(fn(ref), ref, DEVICE_EXP_ULPS) & m).sum())
        print(f"{mutant} on {what}: {out} of {cells} cells outside the band")
        assert out > cells / 100, (what, out, cells)


# ---- what the inputs reach --------------------------------------------------------------------------------
def test_inputs_are_bf16_values_and_every_v_occurs(psm, raft):
    seen = set()
    for table in (psm, raft):
        for name, (c, ref) in table.items():
            for a in ((c.fl, c.fr) if hasattr(c, "fl") else (c.corr,)):
                assert not (np.ascontiguousarray(a).view(np.uint32) & 0xFFFF).any(), name
            seen |= {(float(v), bool(np.signbit(v))) for v in np.unique(c.v4)} | ({(0.0, True)} if np.signbit(c.v4[c.v4 == 0]).any() else set())
    for v in R.VALUES_OF_V:
        assert (float(v), bool(np.signbit(v))) in seen, v


def test_the_new_widths_reach_the_vector_positions_claimed(psm):
    def route(c):
        return "wide" if c.W4 % 8 == 0 else "narrow"
    c, ref = psm["w16_d24"]
    assert route(c) == "wide" and c.D4 == 24 and c.W4 == 16
    # planes 1..7 cut the first vector at every position, 9..15 the second; 16.. leave nothing
    assert {i % 8 for i in range(1, c.D4) if i < c.W4} == set(range(8)) and c.D4 > c.W4
    # the right feature's window starts at every offset of an aligned vector
    assert {(x0 - i) & 7 for i in range(c.D4) for x0 in (0, 8)} == set(range(8))
    live = ~BR.left_of_cut(ref.out.shape) & (ref.v != 0)
    for i in range(1, 16):
        assert live[0, :, i, :, i:].any(), i                     # a modulated cell right of every cut
    c, _ = psm["w72"]
    assert route(c) == "wide" and c.W4 // 8 * c.H4 == 270 > 256
    c, _ = psm["w12"]
    assert route(c) == "narrow" and c.W4 % 4 == 0
    assert {route(psm[n][0]) for n in R.PSM_CASES} == {"wide", "narrow"}
    assert max(psm[n][0].W4 * psm[n][0].H4 for n in BR.PSM_NAMES if route(psm[n][0]) == "narrow") > 256      # its second block too


def test_the_overflow_and_nan_cells_are_what_they_claim(psm):
    c, ref = psm["overflow"]
    o = BR.OVERFLOW_AT
    cell = (0, o["ch"], o["i"], o["y"], o["x"])
    assert c.fl[0, o["ch"], o["y"], o["x"]] == BR.BF16_MAX and ref.v[cell] == 1 and o["x"] >= o["i"]
    assert ref.mod64[cell] == 10.0 and ref.out64[cell] == 10.0 * float(BR.BF16_MAX) > float(BR.BF16_MAX) * (1 + 2.0 ** -8)
    lo, hi = BR.band(ref, DEVICE_EXP_ULPS)
    assert np.isposinf(lo[cell]) and np.isposinf(hi[cell])
    c, ref = psm["nan_feature"]
    n = BR.NAN_AT
    assert np.isnan(ref.out64[0, n["ch"], :n["x"] + 1, n["y"], n["x"]]).all() and (ref.v[0, n["ch"], :, n["y"], n["x"]] == 1).all()
    assert np.isnan(ref.out64).sum() == min(n["x"] + 1, c.D4)


def test_the_copy_case_and_the_raft_sentinel_hold_their_patterns(raft):
    c = BR.copy_case()
    for m in (c.flb, c.frb):
        assert set(BR.COPY_PATTERNS.tolist()) <= set(m.reshape(-1).tolist())
    assert c.W4 % 8 == 0
    want = BR.psm_plain_bits(c.flb, c.frb, c.maxdisp)
    assert set(BR.COPY_PATTERNS.tolist()) <= set(want[:, :c.C].reshape(-1).tolist())
    assert set(BR.COPY_PATTERNS.tolist()) <= set(want[:, c.C:, 1:].reshape(-1).tolist())     # through a shifted window too
    assert (want[BR.left_of_cut(want.shape)] == 0).all()
    plain = R.psm_plain(BR.widen(c.flb), BR.widen(c.frb), c.maxdisp)
    num = ~np.isnan(plain)
    assert np.array_equal(BR.widen(want)[num], plain[num])
    odd_rows = 0
    for name, (rc, ref) in raft.items():
        s = BR.raft_sentinel_bits(rc)
        rows = rc.v4 == 0
        assert np.isnan(BR.widen(s[rows])).all() and np.array_equal(s[~rows], BR.bits(rc.corr)[~rows]), name
        start = (np.arange(rows.size).reshape(rows.shape) * rc.W3) % 2 == 1
        odd_rows += int((start & ~rows).sum())
    assert odd_rows > 50                                         # modulated rows that start on an odd element (odd W3)


# ---- the C-ABI's new names ---------------------------------------------------------------------------------
def test_dt_entries_are_declared_exported_and_bound():
    from vppstereo_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "vppx.h")).read()
    declared = set(re.findall(r"\b(vppx_[a-z0-9_]+)\s*\(", hdr))
    i, vp = C.c_int, C.c_void_p
    want = {"vppx_psmnet_cost_volume_dt_dev": [vp] * 5 + [i] * 7 + [vp, i], "vppx_raft_corr_modulate_dt_dev": [vp] * 4 + [i] * 7}
    for name, argtypes in want.items():
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
        assert list(getattr(lib, name).argtypes) == argtypes, name
        old = getattr(lib, name.replace("_dt_dev", "_dev"))
        assert list(old.argtypes) == argtypes[:-1], name         # the float32 entries keep their signatures
        # the header's parameter list has as many parameters, the last one `int dtype`
        params = re.search(name + r"\s*\((.*?)\);", hdr, re.S).group(1).split(",")
        assert len(params) == len(argtypes) and params[-1].split() == ["int", "dtype"], name
    assert re.search(r"VPPX_DT_F32\s*=\s*0\b", hdr) and re.search(r"VPPX_DT_BF16\s*=\s*1\b", hdr)
    assert (_lib.DT_F32, _lib.DT_BF16) == (0, 1)
    assert "rounded to\n *     bfloat16 ONCE, to nearest even" in hdr


def test_dt_entries_without_a_context_fail_with_a_message():
    from vppstereo_amd import _lib
    lib = _lib.load()
    rc = lib.vppx_raft_corr_modulate_dt_dev(None, None, None, None, 1, 1, 1, 1, 4, 4, 1)
    assert rc == -7 and b"context is NULL" in lib.vppx_last_error()
    rc = lib.vppx_psmnet_cost_volume_dt_dev(None, None, None, None, None, 1, 1, 1, 1, 4, 4, 4, None, 1)
    assert rc == -7 and b"context is NULL" in lib.vppx_last_error()
