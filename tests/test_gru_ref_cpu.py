"""The referee of the update block's glue (tests/_gru_ref.py) held to the reference's recording and to torch on the
CPU, and its planted mistakes shown to leave the limit on the arrays tests/test_gpu_gru.py uploads.  No GPU.

(a) the recorded tensors of BasicMultiUpdateBlock.forward (tests/golden/gru_cases.npz) and torch's composition of the
    same lines lie inside limit() at every cell, with torch's CPU exp taken as within TORCH_EXP_ULPS of the true value
    (the figure of tests/test_handoff_ref_cpu.py);
(b) every planted wrong implementation lies outside it at some cell;
(c) the library exports the three entry points.
"""
import numpy as np
import pytest

import _gru_ref as R
import _readout_ref as RR

F32, F64 = np.float32, np.float64
TORCH_EXP_ULPS = 1.0


def _inside(got, ref, what):
    worst, beyond, other = R.compare(got, ref)
    print(f"{what}: worst |got - value| / limit {worst:.3f}")
    assert (beyond, other) == (0, 0), (what, worst, beyond, other)


def _leaves(got, ref, what):
    worst, beyond, other = R.compare(np.asarray(got, F64), ref)
    print(f"{what}: {beyond} cells beyond, {other} of another class, worst ratio {worst:.3g}")
    assert beyond + other > 0, what


# ---- (a) ------------------------------------------------------------------------------------------------------------
def test_interp_indices_and_weights_are_torchs_bit_for_bit():
    """A one-hot row interpolated along one axis returns the weight of its cell at every output position: the products
    with 1 and 0 and the sums with 0 are exact."""
    import torch
    import torch.nn.functional as F
    for n_in, n_out in ((1, 1), (1, 7), (3, 5), (4, 7), (2, 3), (3, 3), (5, 1), (6, 11), (60, 120), (34, 68), (7, 240)):
        i0, i1, l0, l1 = RR.lin_src(n_in, n_out, align_corners=True)
        want = np.zeros((n_in, n_out), F32)
        for d in range(n_out):
            want[i0[d], d] += l0[d]
            if i1[d] != i0[d]:
                want[i1[d], d] += l1[d]
            else:
                want[i0[d], d] = F32(l0[d] + l1[d])
        eye = torch.eye(n_in).reshape(n_in, 1, 1, n_in)
        along_w = F.interpolate(eye, (1, n_out), mode="bilinear", align_corners=True)[:, 0, 0].numpy()
        along_h = F.interpolate(eye.reshape(n_in, 1, n_in, 1), (n_out, 1), mode="bilinear", align_corners=True)[:, 0, :, 0].numpy()
        assert np.array_equal(along_w, want) and np.array_equal(along_h, want), (n_in, n_out)


@pytest.mark.parametrize("name", list(R.ASSEMBLE_CASES))
def test_torch_assembles_inside_the_limit(name):
    import torch
    import torch.nn.functional as F
    c = R.assemble_case(name)
    ref = R.assemble_ref(c)
    parts = []
    for s in c.sources:
        x = torch.from_numpy(np.ascontiguousarray(R.source_view(s)))
        parts.append(x if s[4] == "copy" else F.avg_pool2d(x, 3, stride=2, padding=1) if s[4] == "pool2x" else
                     F.interpolate(x, (c.H, c.W), mode="bilinear", align_corners=True))
    got = torch.cat(parts, dim=1).numpy()
    assert got.shape == ref.value.shape == (c.B, c.channels, c.H, c.W)
    _inside(got, ref, f"torch assemble {name}")
    assert (ref.limit[:, :c.sources[0][1]] == 0).all()          # the copied source is exact


@pytest.mark.parametrize("name", list(R.GATE_CASES))
def test_torch_gates_inside_the_limit(name):
    import torch
    c = R.gate_case(name)
    t = torch.from_numpy
    r = torch.sigmoid(t(c.ar) + t(c.cr)) * t(c.h)
    _inside(r.numpy(), R.reset(c.ar, c.cr, c.h, TORCH_EXP_ULPS), f"torch reset {name}")
    z = torch.sigmoid(t(c.az) + t(c.cz))
    q = torch.tanh(t(c.aq) + t(c.cq))
    _inside(((1 - z) * t(c.h) + z * q).numpy(), R.update(c.az, c.cz, c.aq, c.cq, c.h, TORCH_EXP_ULPS), f"torch update {name}")
    # what the case is said to hold
    ref = R.update(c.az, c.cz, c.aq, c.cq, c.h)
    cls = R.classes(ref.value)
    assert (cls == 1).any() and (cls == 2).any() and (cls == 0).sum() > 0.9 * cls.size
    assert R.classes(R.reset(c.ar, c.cr, c.h).value).max() >= 2
    with np.errstate(invalid="ignore"):
        v = np.abs(c.az.astype(F64) + c.cz)
    assert (v[np.isfinite(v)] > 88).any() and (v < 0.5).any()     # saturated where expf overflows, and near 0


def test_the_recording_lies_inside_the_limit():
    G = R.load_recording()
    for call in R.CALLS:
        ref = R.block_ref(G, call, TORCH_EXP_ULPS)
        flags = R.CALL_FLAGS[call]
        levels = [("gru32", 2)] * flags["iter32"] + [("gru16", 1)] * flags["iter16"] + [("gru08", 0)] * flags["iter08"]
        for tag, i in levels:
            _inside(G[f"{call}_{tag}.convz_in"], ref[f"{tag}.hx"], f"{call} {tag} hx")
            _inside(G[f"{call}_{tag}.convq_in"], ref[f"{tag}.rhx"], f"{call} {tag} [r*h, x]")
            _inside(G[f"{call}_net{i}_out"], ref[f"net{i}"], f"{call} net{i}")
        for i in range(3):
            if not any(i == j for _, j in levels):
                assert np.array_equal(G[f"{call}_net{i}_out"], G[f"{call}_net{i}_in"])
        if flags["update"]:
            _inside(G[f"{call}_flow_head_in"], ref["net0"], f"{call} flow_head input")
            _inside(G[f"{call}_mask_in"], ref["net0"], f"{call} mask input")
            assert np.array_equal(G[f"{call}_mask"], F32(0.25) * G[f"{call}_mask_out"])
            assert np.array_equal(G[f"{call}_delta"], G[f"{call}_flow_head_out"])
    # the second iteration runs on the first one's states
    for i in range(3):
        assert np.array_equal(G["it1_net%d_in" % i], G["it0_net%d_out" % i])
    assert sum(G[k].nbytes for k in G.files) < 400 * 1024


# ---- (b) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.GATE_CASES))
def test_planted_gate_mistakes_leave_the_limit(name):
    c = R.gate_case(name)
    up, rs = R.update(c.az, c.cz, c.aq, c.cq, c.h), R.reset(c.ar, c.cr, c.h)
    _leaves(R.update(c.az, c.cz, c.aq, c.cq, c.h, swap_z=True).value, up, "z and 1 - z swapped")
    _leaves(R.update(c.az, c.cr, c.aq, c.cq, c.h).value, up, "cr in the place of cz (update)")
    _leaves(R.reset(c.ar, c.cz, c.h).value, rs, "cz in the place of cr (reset)")
    _leaves(R.update(c.az, c.cz, c.aq, c.cq, c.h, q_gate="sigmoid").value, up, "tanh replaced by sigmoid")
    _leaves(R.reset(c.ar, c.cr, c.h, gated=False).value, rs, "r * h left as h")
    # out is h: a kernel that read h again after writing it would blend the new state
    again = R.update(c.az, c.cz, c.aq, c.cq, np.nan_to_num(up.value, nan=0.0, posinf=0.0, neginf=0.0)).value
    _leaves(again, up, "the new h where the old one belongs")


def test_planted_assembly_mistakes_leave_the_limit():
    for name in ("odd_a", "odd_b", "aligned", "wide_hx"):
        c = R.assemble_case(name)
        ref = R.assemble_ref(c)

        def planted(**how):
            srcs = []
            for s in c.sources:
                x = R.source_view(s)
                srcs.append(x if s[4] == "copy" else R.pool2x(x, **{k: v for k, v in how.items() if k != "align_corners"})[0]
                            if s[4] == "pool2x" else R.interp(x, c.H, c.W, **{k: v for k, v in how.items() if k == "align_corners"})[0])
            return np.concatenate(srcs, axis=1)

        assert R.compare(planted(), ref)[1:] == (0, 0)
        _leaves(planted(divisor="inside"), ref, f"{name}: the pool divisor as the count of cells inside the map")
        _leaves(planted(shift=1), ref, f"{name}: the pool window shifted by one")
        if any(s[4] == "interp" and s[2] * s[3] > 1 for s in c.sources):
            _leaves(planted(align_corners=False), ref, f"{name}: align_corners=False")
        if any(s[0].shape[1] != s[1] * s[2] * s[3] for s in c.sources):
            _leaves(R.assemble_stride_ignored(c), ref, f"{name}: a frame stride ignored")
    # the order of the sources, where two of them have the same number of channels
    c = R.assemble_case("odd_a")
    ref = R.assemble_ref(c)
    views = [(R.source_view(s), s[4]) for s in c.sources]
    _leaves(R.assemble([views[0], views[1], views[3], views[2]], c.H, c.W).value, ref, "the source order in hx permuted")


def test_planted_block_mistakes_leave_the_limit_of_the_recording():
    G = R.load_recording()
    good = R.block_ref(G, "it1")
    # gru32 of the second iteration reading the NEW net[1] (the call's output) where the old one belongs
    bad = R.block_ref(G, "it1", old_net1_from="it1")
    _leaves(bad["gru32.hx"].value, good["gru32.hx"], "gru32 reads the new net[1]")
    # gru16's hx as [h, interp(net2), pool2x(net0)]
    bad = R.block_ref(G, "it1", hx_order=(1, 0))
    _leaves(bad["gru16.hx"].value, good["gru16.hx"], "gru16's sources permuted")
    # gru16 reading the OLD net[2] where the new one belongs
    H, W = G["it1_net1_in"].shape[2:]
    old = R.assemble([(G["it1_net1_in"], "copy"), (G["it1_net0_in"], "pool2x"), (G["it1_net2_in"], "interp")], H, W)
    _leaves(old.value, good["gru16.hx"], "gru16 reads the old net[2]")


# ---- (c) ------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_three_calls():
    from vppstereo_amd import _lib
    lib = _lib.load()
    for name in ("vppx_raft_gru_assemble_dt_dev", "vppx_raft_gru_reset_dt_dev", "vppx_raft_gru_update_dt_dev"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    import ctypes as C
    assert C.sizeof(_lib.VppxGruSource) == 32 and _lib.GRU_MODES == {"copy": 0, "pool2x": 1, "interp": 2}
    null = C.c_void_p()
    assert lib.vppx_raft_gru_reset_dt_dev(null, null, 0, null, 0, null, 0, null, 0, 1, 1, 1, 1, 1, 0) == -7
    assert b"context is NULL" in lib.vppx_last_error()
