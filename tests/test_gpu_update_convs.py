"""FusedUpdate(block, convs=True): the motion encoder's convc2 / convf2 / conv, the flow head and the mask head with its `.25 *` as
seven launches of Engine.raft_conv, on the stand-in model of tests/_raft_loop.py (its motion encoder ends in 14 channels, its flow
head in 2, its mask head is a 3x3 and a 1x1 to 144), inside the composed loop of tests/test_gpu_raft_loop.py, whose model, inputs,
yardsticks and bound these tests share:
        max |fused - f64|  <=  4 * max |plain - f64|          per returned tensor,
the factor being that file's, for the reasons given there.  Stagewise, every spied raft_conv launch is held to the float64 referee
of tests/_conv_ref.py on the inputs the device actually had.  docs/NOTEBOOK.md has the ratios an MI355X gave."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest

import _conv_ref as CR
import _raft_loop as L
import test_gpu_raft_loop as T
from _cells import hold

pytestmark = pytest.mark.gpu

B, H, W, ITERS, CROP = T.B, T.H, T.W, T.ITERS, T.CROP
SEVEN = ("convc2", "convf2", "conv", "flow_head.0", "flow_head.2", "mask.0", "mask.2")
RELU = (True, True, True, True, False, True, False)
SCALE = (1.0, 1.0, 1.0, 1.0, 1.0, 1.0, .25)
FLAGS = [dict(motion_front=True, gru_conv=True, convs=True), dict(convs=True)]


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda", torch.cuda.current_device())


def _seven(model):
    blk = model.update_block
    enc = blk.encoder
    return [enc.convc2, enc.convf2, enc.conv, blk.flow_head[0], blk.flow_head[2], blk.mask[0], blk.mask[2]]


def _wrap(model, **flags):
    from vppstereo_amd.extractor import FusedEncoder
    from vppstereo_amd.update import FusedUpdate
    return SimpleNamespace(fnet=FusedEncoder(model.fnet), cnet=FusedEncoder(model.cnet), update=FusedUpdate(model.update_block, **flags))


class _MaskInTheLastIterationOnly:
    """The `test_mode` line of INTEGRATION.md around an update block: mask=(itr == iters - 1)."""

    def __init__(self, update, iters):
        self.update, self.iters, self.k = update, iters, 0

    def __call__(self, net, inp, corr=None, flow=None, **flags):
        if flags.get("update", True):
            self.k += 1
            flags["mask"] = self.k == self.iters
        return self.update(net, inp, corr, flow, **flags)


def _hooked(model, ran):
    return [m.register_forward_hook(lambda m_, i, o, name=name: ran.append(name)) for name, m in zip(SEVEN, _seven(model))]


def _check_convs(spy, model, what):
    """Every raft_conv record against tests/_conv_ref.conv with the live module's weights: the seven come in SEVEN's order."""
    recs = spy.of("raft_conv")
    mods = _seven(model)
    assert len(recs) % 7 == 0
    for k, rec in enumerate(recs):
        j = k % 7
        x0, cout, ksize = rec.args[0], rec.args[2], rec.args[3]
        m = mods[j]
        assert (cout, ksize) == (m.out_channels, m.kernel_size[0]) and bool(rec.kwargs["relu"]) == RELU[j] and rec.kwargs["scale"] == SCALE[j], (k, SEVEN[j])
        assert (rec.kwargs.get("x1") is not None) == (j == 2)                    # encoder.conv reads cor and flo as two sources
        dtype = L._dt(x0)
        ref = CR.conv(L._np(x0), L._np(rec.kwargs.get("x1")), m.weight.detach().float().cpu().numpy(), m.bias.detach().float().cpu().numpy(), dtype,
                      relu=RELU[j], scale=SCALE[j])
        hold(CR, L._np(rec.result), ref, f"{what} launch {k} {SEVEN[j]}", dtype)
    return len(recs)


# ---- stagewise --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("flags", FLAGS, ids=["all", "convs_alone"])
def test_torch_runs_none_of_the_seven_and_every_launch_equals_its_referee(dev, flags, dtype):
    import torch
    model, inputs, eng = T._model(dtype, dev), T._inputs(dtype, dev), T._eng(dev)
    ran = []
    hooks = _hooked(model, ran)
    try:
        with L.LaunchSpy(eng, names=L.SPIED + ("raft_conv",)) as spy:
            res = L.fused_forward(model, _wrap(model, **flags), *inputs, iters=ITERS, crop=CROP)
            torch.cuda.synchronize()
        assert ran == [], f"torch ran {ran}"
        c = spy.counts()
        assert c["raft_conv"] == 7 * ITERS
        full = bool(flags.get("gru_conv"))
        assert (c["raft_gru_zr"], c["raft_gru_q"], c["raft_motion_front"]) == ((3 * ITERS, 3 * ITERS, ITERS) if full else (0, 0, 0))
        per_iteration = [r.name for r in spy.records if r.name in ("raft_conv", "raft_motion_front", "raft_gru_assemble")]
        front = ["raft_motion_front"] if full else []
        assert per_iteration == (["raft_gru_assemble"] * 2 + front + ["raft_conv"] * 3 + ["raft_gru_assemble"] + ["raft_conv"] * 4) * ITERS
        assert _check_convs(spy, model, f"{dtype}") == 7 * ITERS
        # the mask in the last iteration only: five launches in the others, and the bits of the run above
        with L.LaunchSpy(eng, names=("raft_conv",)) as spy:
            w = _wrap(model, **flags)
            w.update = _MaskInTheLastIterationOnly(w.update, ITERS)
            last = L.fused_forward(model, w, *inputs, iters=ITERS, crop=CROP)
            torch.cuda.synchronize()
        assert ran == [] and spy.counts()["raft_conv"] == 5 * (ITERS - 1) + 7
        for a, b in zip(T._named(res).values(), T._named(last).values()):
            assert torch.equal(a, b)
    finally:
        for h in hooks:
            h.remove()
    assert vars(eng).keys().isdisjoint(L.SPIED + ("raft_conv",))


def test_mask_false_returns_none_and_the_same_bits(dev):
    import torch
    from vppstereo_amd.update import FusedUpdate
    model = T._model("float32", dev)
    gen = torch.Generator().manual_seed(6501)
    sizes = L.map_sizes(H, W)
    rnd = lambda *s: torch.randn(s, generator=gen).to(dev)                                  # noqa: E731
    net = [torch.tanh(rnd(B, L.HIDDEN, *s)) for s in sizes]
    inp = [list(rnd(B, 3 * L.HIDDEN, *s).split(L.HIDDEN, dim=1)) for s in sizes]
    corr, flow = rnd(B, L.LEVELS * (2 * L.RADIUS + 1), *sizes[0]), rnd(B, 2, *sizes[0])
    for flags in (dict(convs=True), dict()):
        fused = FusedUpdate(model.update_block, **flags)
        n1, m1, d1 = fused([t.clone() for t in net], inp, corr, flow)
        n2, m2, d2 = fused([t.clone() for t in net], inp, corr, flow, mask=False)
        assert m2 is None and tuple(m1.shape) == (B, 144) + sizes[0] and tuple(d1.shape) == (B, 2) + sizes[0]
        assert torch.equal(d1, d2) and all(torch.equal(a, b) for a, b in zip(n1, n2))
        assert d1.data_ptr() != d2.data_ptr()                                               # results are tensors of their own
        assert sorted(fused._bufs) == (["cor2", "flo2", "flow_head", "mask", "motion"] if flags else [])


# ---- end to end -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", T.REGIMES)
@pytest.mark.parametrize("flags", FLAGS, ids=["all", "convs_alone"])
def test_the_loop_with_the_convolutions_is_as_close_to_float64_as_plain_torch(dev, flags, regime):
    import torch
    model, inputs = T._model(regime, dev), T._inputs(regime, dev)
    ref, plain = T._yard(regime, dev)
    ran = []
    hooks = _hooked(model, ran)
    try:
        res = L.fused_forward(model, _wrap(model, **flags), *inputs, iters=ITERS, autocast=regime == "autocast", crop=CROP)
        torch.cuda.synchronize()
    finally:
        for h in hooks:
            h.remove()
    assert ran == [], f"torch ran {ran}"
    T._hold_end_to_end(T._host64(res), plain, ref, f"convs {'+ front + gru_conv' if len(flags) > 1 else 'alone'} {regime}")
    stored = torch.float32 if regime == "float32" else torch.bfloat16
    assert [t.dtype for t in res.net] == [stored] * 3 and res.flow.dtype == torch.float32 and res.disparity.dtype == torch.float32


# ---- the weights follow the module --------------------------------------------------------------------------------------------------
def test_the_weights_follow_the_module(dev):
    """encoder.conv's weight (126 -> here 14 channels out, the two-source call) and mask[2]'s (the 1x1) are replaced behind the
    wrapper's back by `p.data = new` and by load_state_dict; each time the next forward is that of the NEW weights."""
    import torch
    model = copy.deepcopy(T._model("float32", dev))
    inputs = T._inputs("float32", dev)
    wrapped = _wrap(model, **FLAGS[0])
    enc_conv, mask2 = model.update_block.encoder.conv, model.update_block.mask[2]
    run = lambda: T._host64(L.fused_forward(model, wrapped, *inputs, iters=ITERS, crop=CROP))        # noqa: E731
    old = T._f64(model, inputs)
    plain = T._host64(L.plain_forward(model, *inputs, iters=ITERS, crop=CROP))
    T._hold_end_to_end(run(), plain, old, "before any change")
    packed = {id(m): wrapped.update._packed[id(m)][1] for m in (enc_conv, mask2)}
    run()
    assert all(wrapped.update._packed[k][1] is p for k, p in packed.items()) and len(wrapped.update._packed) == 3 + 7
    gen = torch.Generator().manual_seed(6502)
    for how in ("data", "load_state_dict"):
        new = [(torch.randn(m.weight.shape, generator=gen) * m.weight.std().cpu() * 1.5).to(dev) for m in (enc_conv, mask2)]
        for m, w in zip((enc_conv, mask2), new):
            if how == "data":
                m.weight.data = w
            else:
                m.load_state_dict({"weight": w, "bias": m.bias.detach().clone()})
            assert torch.equal(m.weight, w)
        ref = T._f64(model, inputs)
        plain = T._host64(L.plain_forward(model, *inputs, iters=ITERS, crop=CROP))
        T._hold_end_to_end(run(), plain, ref, f"after {how}", other=old)
        old = ref
    assert len(wrapped.update._packed) == 3 + 7
    wrapped.update.forget_weights()
    assert wrapped.update._packed == {}


# ---- a head that is not plain falls back ------------------------------------------------------------------------------------------------
def test_a_head_that_is_not_plain_falls_back(dev):
    import torch
    model = copy.deepcopy(T._model("float32", dev))
    inputs, eng = T._inputs("float32", dev), T._eng(dev)
    model.update_block.flow_head[0].padding_mode = "replicate"        # F.pad(mode="replicate") and a convolution without padding
    ref = T._f64(model, inputs)
    plain = T._host64(L.plain_forward(model, *inputs, iters=ITERS, crop=CROP))
    assert np.abs(plain["flow"] - T._yard("float32", dev)[1]["flow"]).max() > 1e-4      # the padding mode matters to plain torch
    ran = []
    hooks = _hooked(model, ran)
    try:
        with L.LaunchSpy(eng, names=("raft_conv",)) as spy:
            res = L.fused_forward(model, _wrap(model, **FLAGS[0]), *inputs, iters=ITERS, crop=CROP)
            torch.cuda.synchronize()
    finally:
        for h in hooks:
            h.remove()
    assert ran == ["flow_head.0"] * ITERS and spy.counts()["raft_conv"] == 6 * ITERS
    T._hold_end_to_end(T._host64(res), plain, ref, "flow_head[0] with replicate padding")
