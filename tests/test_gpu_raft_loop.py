"""The composed RAFT-Stereo loop with the patch of INTEGRATION.md applied as a whole (tests/_raft_loop.py): FusedEncoder around both
encoders, CorrBlock1DFused, the deferred lookup, FusedUpdate(motion_front=True, gru_conv=True) and Engine.raft_upsample, on one
live stand-in model, three iterations.

Stagewise: every launch of one forward is spied and held to the float64 referee of that launch, on the inputs the device actually
had, within that referee's own derived limit (bfloat16: its band).  End to end: the yardstick is the same loop in plain torch
operations on the device in the same dtype regime; both are compared with the float64 run of the same weights on the CPU and
        max |fused - f64|  <=  4 * max |plain - f64|          per returned tensor.
The factor is not a measured tolerance: both sides evaluate one graph in one storage precision and differ in summation order, in
fused multiply-adds and in where a bfloat16 tensor is rounded; each side is a maximum over a few thousand cells of errors of like
size, and four covers the spread of two such maxima.  tests/test_raft_loop_cpu.py shows that a wrong source, order, gate, sign or
buffer lies orders of magnitude beyond it.  docs/NOTEBOOK.md has the ratios an MI355X gave.

Shapes: B = 2, 3 x 40 x 72 images; maps of 10 x 18, 5 x 9 and 3 x 5; correlation widths 18 / 9 / 4 / 2.  The convolution kernel's
tile is 8 rows x 32 columns (tests/_gruconv_ref.CASES "tiles"): 10 rows are one whole tile and a partial one, 18 columns a partial
one, two frames; the 5 x 9 and 3 x 5 maps are one partial tile each.  The motion front works on 16 pixels of a row at a time
(tests/_motion_ref.CASES "low_map": a row tail): 18 leaves a tail of 2.  These sizes reach both.
The second size of the across-calls test is 32 x 64 and not 32 x 48: a map 12 wide leaves level 3 of the pyramid one cell wide,
which the correlation calls refuse (W3 >> (levels - 1) < 2), as the reference divides by zero there; 64 is the nearest width that
is a multiple of 16 with a 2-wide last level."""
import copy

import numpy as np
import pytest

import _raft_loop as L

pytestmark = pytest.mark.gpu

B, H, W, ITERS, CROP = 2, 40, 72, 3, (3, 5, 2, 6)
FACTOR = 4
REGIMES = ("float32", "bfloat16", "autocast")
NAMES = ("flow", "net0", "net1", "net2", "disparity")
_CACHE = {}

assert L.map_sizes(H, W) == [(10, 18), (5, 9), (3, 5)]
assert 10 % 8 and 10 > 8 and 18 % 32 and 18 % 16 and 18 > 16        # a partial tile of the conv kernel, a row tail of the motion front


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda", torch.cuda.current_device())


def _eng(dev):
    from vppstereo_amd.corr import _engine
    return _engine(dev)


def _model(regime, dev):
    """The seeded model in the regime's storage on the device, made once per regime (tests that change weights copy it)."""
    key = ("model", regime)
    if key not in _CACHE:
        m = L.build_model()
        L.assert_no_fallback(m)
        _CACHE[key] = (m.bfloat16() if regime == "bfloat16" else m).to(dev)
    return _CACHE[key]


def _inputs(regime, dev, size=(B, H, W)):
    """(image0, image2, image3, hints, validhints) on the device: bfloat16 images in the bfloat16 regime, float32 hints always."""
    import torch
    key = ("inputs", regime == "bfloat16", size)
    if key not in _CACHE:
        a = L.inputs(*size)
        idt = torch.bfloat16 if regime == "bfloat16" else torch.float32
        _CACHE[key] = [torch.from_numpy(getattr(a, k)).to(dev).to(idt) for k in ("image0", "image2", "image3")] + \
                      [torch.from_numpy(getattr(a, k)).to(dev) for k in ("hints", "validhints")]
    return _CACHE[key]


def _named(res):
    return {"flow": res.flow, "net0": res.net[0], "net1": res.net[1], "net2": res.net[2], "disparity": res.disparity}


def _host64(res):
    return {k: v.double().cpu().numpy() for k, v in _named(res).items()}


def _f64(model, inputs, schedule="default"):
    """The float64 run on the CPU of the weights and inputs as they are stored (bfloat16 ones widened: exact)."""
    m = copy.deepcopy(model).cpu().double()
    res = L.plain_forward(m, *(t.cpu().double() for t in inputs), iters=ITERS, schedule=schedule, crop=CROP)
    return _host64(res)


def _yard(regime, dev, schedule="default"):
    """-> (the float64 run, the plain run on the device in the regime), made once and left unchanged."""
    key = ("yard", regime, schedule)
    if key not in _CACHE:
        model, inputs = _model(regime, dev), _inputs(regime, dev)
        ref = _f64(model, inputs, schedule)
        plain = L.plain_forward(model, *inputs, iters=ITERS, schedule=schedule, autocast=regime == "autocast", crop=CROP)
        _CACHE[key] = (ref, _host64(plain))
    return _CACHE[key]


def _hold_end_to_end(fused, plain, ref, what, other=None):
    """max |fused - f64| <= FACTOR * max |plain - f64| per tensor, with a yardstick that is not vacuous.  other: a float64 run the
    fused one must lie BEYOND the bound of (the weights of before), which plain torch separates by more than ten bounds."""
    for k in NAMES:
        assert np.isfinite(fused[k]).all() and np.isfinite(plain[k]).all(), (what, k)
        assert fused[k].shape == ref[k].shape
        e_fused, e_plain = float(np.abs(fused[k] - ref[k]).max()), float(np.abs(plain[k] - ref[k]).max())
        print(f"{what} {k}: max |fused - f64| {e_fused:.3e}, max |plain - f64| {e_plain:.3e}, ratio {e_fused / e_plain if e_plain else float('inf'):.3f}")
        assert e_plain > 0, (what, k)
        assert e_fused <= FACTOR * e_plain, f"{what} {k}: {e_fused:.3e} is more than {FACTOR} x {e_plain:.3e}"
        if other is not None:
            apart = float(np.abs(plain[k] - other[k]).max())
            assert apart > 10 * FACTOR * e_plain, f"{what} {k}: plain torch separates the two sets of weights by {apart:.3e} only"
            assert float(np.abs(fused[k] - other[k]).max()) > FACTOR * e_plain, f"{what} {k}: within the bound of the OLD weights"


def _norm_launches(model):
    """(statistics launches, apply launches) one forward of both encoders takes: one statistics launch per InstanceNorm2d (a
    frozen BatchNorm2d has none), and one apply launch per norm except a downsample path's, which goes into its block's second."""
    import torch
    stats = sum(isinstance(m, torch.nn.InstanceNorm2d) for m in model.fnet.modules())
    norms = sum(isinstance(m, (torch.nn.InstanceNorm2d, torch.nn.BatchNorm2d)) for enc in (model.fnet, model.cnet) for m in enc.modules())
    folded = sum(getattr(m, "downsample", None) is not None for enc in (model.fnet, model.cnet) for m in enc.modules())
    return stats, norms - folded


# ---- stagewise -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_every_launch_of_the_composed_loop_equals_its_referee(dev, dtype):
    import torch
    model, inputs, eng = _model(dtype, dev), _inputs(dtype, dev), _eng(dev)
    blk = model.update_block
    ran, hooks = [], []
    watched = [(f"{g}.{cv}", getattr(getattr(blk, g), cv)) for g in ("gru08", "gru16", "gru32") for cv in ("convz", "convr", "convq")]
    watched += [("convc1", blk.encoder.convc1), ("convf1", blk.encoder.convf1)]
    for name, conv in watched:
        hooks.append(conv.register_forward_hook(lambda m, i, o, name=name: ran.append(name)))
    try:
        with L.LaunchSpy(eng) as spy:
            res = L.fused_forward(model, L.wrap(model), *inputs, iters=ITERS, crop=CROP)
            torch.cuda.synchronize()
    finally:
        for h in hooks:
            h.remove()
    assert ran == [], f"torch ran {ran}"
    counts = spy.counts()
    print(f"launches of one forward of {ITERS} iterations [{dtype}]: " + ", ".join(f"{k} {v}" for k, v in counts.items()))
    stats, applies = _norm_launches(model)
    assert (stats, applies) == (15, 42)
    want = dict(raft_norm_stats=stats, raft_norm_apply=applies, raft_corr_fused=1, raft_corr_pyramid=0, raft_corr_lookup=0,
                raft_motion_front=ITERS, raft_gru_assemble=3 * ITERS, raft_gru_reset=0, raft_gru_update=0, raft_gru_zr=3 * ITERS,
                raft_gru_q=3 * ITERS, raft_upsample=1)
    assert counts == want
    per_iteration = [r.name for r in spy.records if r.name.startswith(("raft_motion", "raft_gru"))]
    one = ["raft_gru_assemble", "raft_gru_zr", "raft_gru_q"]
    assert per_iteration == (one + one + ["raft_motion_front"] + one) * ITERS      # gru32, gru16, the motion front, gru08
    assert L.check_all(spy, model, L.map_sizes(H, W)) == len(spy.records) == sum(want.values())
    tdt = torch.bfloat16 if dtype == "bfloat16" else torch.float32
    assert all(t.dtype == tdt for t in res.net) and res.flow.dtype == res.disparity.dtype == torch.float32
    assert tuple(res.disparity.shape) == (B, 1, H - CROP[2] - CROP[3], W - CROP[0] - CROP[1])
    assert vars(eng).keys().isdisjoint(L.SPIED)                                    # the spy is gone


# ---- end to end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", REGIMES)
def test_the_composed_loop_is_as_close_to_float64_as_plain_torch(dev, regime):
    import torch
    model, inputs = _model(regime, dev), _inputs(regime, dev)
    ref, plain = _yard(regime, dev)
    res = L.fused_forward(model, L.wrap(model), *inputs, iters=ITERS, autocast=regime == "autocast", crop=CROP)
    torch.cuda.synchronize()
    _hold_end_to_end(_host64(res), plain, ref, regime)
    stored = torch.float32 if regime == "float32" else torch.bfloat16
    # the dtypes the docstrings of update.py and extractor.py promise: a convolution's output under autocast is bfloat16 and so
    # are the hidden states; the flow and the disparity are float32
    assert [t.dtype for t in res.net] == [stored] * 3 and res.flow.dtype == torch.float32 and res.disparity.dtype == torch.float32
    assert (res.flow[:, 1] == 0).all()


# ---- the flags -------------------------------------------------------------------------------------------------------------------
FLAGS = [(True, True, "fused", "default"), (True, False, "fused", "default"), (False, True, "fused", "default"),
         (False, False, "fused", "default"), (True, True, "plain", "default"), (True, True, "fused", "slow_fast"),
         (False, False, "fused", "slow_fast")]


@pytest.mark.parametrize("motion_front,gru_conv,corr_block,schedule", FLAGS)
def test_every_flag_combination_holds_the_bound(dev, motion_front, gru_conv, corr_block, schedule):
    import torch
    model, inputs, eng = _model("float32", dev), _inputs("float32", dev), _eng(dev)
    ref, plain = _yard("float32", dev, schedule)
    with L.LaunchSpy(eng) as spy:
        res = L.fused_forward(model, L.wrap(model, motion_front, gru_conv), *inputs, iters=ITERS, schedule=schedule, crop=CROP,
                              corr_block=corr_block)
        torch.cuda.synchronize()
    _hold_end_to_end(_host64(res), plain, ref, f"motion_front={motion_front} gru_conv={gru_conv} {corr_block} {schedule}")
    c = spy.counts()
    grus = (6 if schedule == "slow_fast" else 3) * ITERS            # slow-fast: gru32 three times, gru16 twice, gru08 once
    assert c["raft_gru_assemble"] == grus
    assert (c["raft_gru_zr"], c["raft_gru_q"], c["raft_gru_reset"], c["raft_gru_update"]) == ((grus, grus, 0, 0) if gru_conv else (0, 0, grus, grus))
    assert (c["raft_motion_front"], c["raft_corr_lookup"]) == ((ITERS, 0) if motion_front else (0, ITERS))
    assert (c["raft_corr_fused"], c["raft_corr_pyramid"]) == ((1, 0) if corr_block == "fused" else (0, 1))


# ---- one wrapped model across calls ---------------------------------------------------------------------------------------------
def test_one_wrapped_model_across_calls(dev):
    """B = 2 at 40 x 72, B = 1 at 32 x 64, the first again, through the same FusedEncoder / FusedUpdate objects."""
    import torch
    model = _model("float32", dev)
    small = (1, 32, 64)
    a, b = _inputs("float32", dev), _inputs("float32", dev, small)
    wrapped = L.wrap(model)
    bits = lambda res: [v.cpu().numpy().view(np.int32) for v in _named(res).values()]      # noqa: E731
    run = lambda w, x: L.fused_forward(model, w, *x, iters=ITERS, crop=CROP)                # noqa: E731
    first = bits(run(wrapped, a))
    packed = {g: wrapped.update._packed[id(getattr(model.update_block, g))][1] for g in ("gru08", "gru16", "gru32")}
    second = bits(run(wrapped, b))
    sizes = L.map_sizes(*small[1:])
    assert sizes == [(8, 16), (4, 8), (2, 4)]
    for level, size, channels in ((8, sizes[0], 48), (16, sizes[1], 48), (32, sizes[2], 32)):
        assert tuple(wrapped.update._hx[level].shape) == (1, channels) + size
        assert tuple(wrapped.update._gates[level, "z"].shape) == tuple(wrapped.update._gates[level, "rh"].shape) == (1, 16) + size
    third = bits(run(wrapped, a))
    fresh = bits(run(L.wrap(model), b))
    torch.cuda.synchronize()
    for k, x, y, z, f in zip(NAMES, first, second, third, fresh):
        assert np.array_equal(x, z), f"{k}: the third call is not the first"
        assert np.array_equal(y, f), f"{k}: the second call is not a freshly wrapped model's"
    assert not np.array_equal(first[1][0], first[1][1])                             # the two frames differ
    sizes = L.map_sizes(H, W)
    for level, size, channels in ((8, sizes[0], 48), (16, sizes[1], 48), (32, sizes[2], 32)):
        assert tuple(wrapped.update._hx[level].shape) == (B, channels) + size
        assert tuple(wrapped.update._gates[level, "z"].shape) == (B, 16) + size
    assert sorted(wrapped.update._hx) == [8, 16, 32] and len(wrapped.update._gates) == 6
    for g, p in packed.items():                                                      # the packed weights were made once
        assert wrapped.update._packed[id(getattr(model.update_block, g))][1] is p, g
    assert len(wrapped.update._packed) == 3


# ---- the weights follow the module -----------------------------------------------------------------------------------------------
def _replace(how, conv, bn, w, var):
    import torch
    if how == "data":
        conv.weight.data = w
        bn.running_var.data = var
    elif how == "copy_":
        with torch.no_grad():
            conv.weight.copy_(w)
            bn.running_var.copy_(var)
    else:
        kw = dict(assign=True) if how == "assign" else {}
        conv.load_state_dict({"weight": w, "bias": conv.bias.detach().clone()}, **kw)
        sd = {k: v.detach().clone() for k, v in bn.state_dict().items()}
        sd["running_var"] = var
        bn.load_state_dict(sd, **kw)


def test_the_weights_follow_the_module(dev):
    """gru16.convq's weight and the running variance of one BatchNorm2d of the context encoder are replaced in four ways behind
    the wrappers' backs; each time the next forward is that of the NEW weights."""
    import torch
    model = copy.deepcopy(_model("float32", dev))
    inputs = _inputs("float32", dev)
    wrapped = L.wrap(model)
    conv, bn = model.update_block.gru16.convq, model.cnet.layer1[0].norm1
    run = lambda: _host64(L.fused_forward(model, wrapped, *inputs, iters=ITERS, crop=CROP))        # noqa: E731
    old = _f64(model, inputs)
    plain = _host64(L.plain_forward(model, *inputs, iters=ITERS, crop=CROP))
    _hold_end_to_end(run(), plain, old, "before any change")
    gen = torch.Generator().manual_seed(6100)
    for how in ("data", "load_state_dict", "assign", "copy_"):
        w = (torch.randn(conv.weight.shape, generator=gen) * conv.weight.std().cpu() * 1.5).to(dev)
        var = (torch.rand(bn.num_features, generator=gen) * 2.0 + 0.1).to(dev)
        _replace(how, conv, bn, w, var)
        assert torch.equal(conv.weight, w) and torch.equal(bn.running_var, var) and not conv.weight.requires_grad
        new = _f64(model, inputs)
        plain = _host64(L.plain_forward(model, *inputs, iters=ITERS, crop=CROP))
        _hold_end_to_end(run(), plain, new, f"after {how}", other=old)
        old = new
    assert len(wrapped.update._packed) == 3
