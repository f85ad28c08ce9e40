"""FusedEncoder(encoder, convs=True) (vppstereo_amd/extractor.py): every convolution of an encoder that the convolution kernel
takes as one launch of Engine.raft_conv, at stride 1 or 2, on the small seeded encoders of tests/_enc_models.py.

Stagewise: every raft_conv launch of one forward is spied (tests/_raft_loop.LaunchSpy) and held to the float64 referee of
tests/_strided_ref.py on the tensors the device actually had; the number of launches is the number of plain convolutions, and only
the stem runs in torch.  End to end, the bound of tests/test_gpu_raft_loop.py: with the float64 run of the same weights on the CPU,
        max |fused - f64|  <=  4 * max |plain - f64|          per returned tensor,
plain being the encoder in torch operations on the device in the same regime (float32, bfloat16 storage, autocast).
docs/NOTEBOOK.md has the ratios an MI355X gave."""
import copy

import numpy as np
import pytest

import _enc_models as EM
import _raft_loop as L
import _strided_ref as SR

pytestmark = pytest.mark.gpu

FACTOR = 4
REGIMES = ("float32", "bfloat16", "autocast")
KINDS = {"basic": EM.basic, "multi": EM.multi}
_CACHE = {}


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda", torch.cuda.current_device())


def _eng(dev):
    from vppstereo_amd.corr import _engine
    return _engine(dev)


def _model(kind, regime, dev):
    key = (kind, regime == "bfloat16")
    if key not in _CACHE:
        m = KINDS[kind]()
        _CACHE[key] = (m.bfloat16() if regime == "bfloat16" else m).to(dev)
    return _CACHE[key]


def _image(regime, dev, shape=EM.INPUT):
    import torch
    x = EM.image(dev, shape=shape)
    return x.to(torch.bfloat16) if regime == "bfloat16" else x


def _forward(fused, x, regime):
    import torch
    with torch.no_grad(), L._autocast(x.device, regime == "autocast"):
        return EM.flat(fused(x, num_layers=3) if fused.multi else fused(x))


def _plain(enc, x, regime):
    import torch
    with torch.no_grad(), L._autocast(x.device, regime == "autocast"):
        return EM.plain(enc, x)


def _f64(enc, x):
    import torch
    with torch.no_grad():
        return [t.numpy() for t in EM.plain(copy.deepcopy(enc).cpu().double(), x.cpu().double())]


def _hold(fused, plain, ref, what):
    """max |fused - f64| <= FACTOR * max |plain - f64| per output -> the largest ratio."""
    assert len(fused) == len(plain) == len(ref)
    worst = 0.0
    for k, (a, b, r) in enumerate(zip(fused, plain, ref)):
        a, b = a.double().cpu().numpy(), b.double().cpu().numpy()
        assert a.shape == r.shape and np.isfinite(a).all() and np.isfinite(b).all(), (what, k)
        e_fused, e_plain = float(np.abs(a - r).max()), float(np.abs(b - r).max())
        print(f"{what} output {k} {a.shape}: max |fused - f64| {e_fused:.3e}, max |plain - f64| {e_plain:.3e}, ratio {e_fused / e_plain:.3f}")
        assert e_plain > 0 and e_fused <= FACTOR * e_plain, f"{what} output {k}: {e_fused:.3e} is more than {FACTOR} x {e_plain:.3e}"
        worst = max(worst, e_fused / e_plain)
    return worst


class _Watch:
    """The convolutions torch ran (forward hooks) and the modules whose packed weights were asked for, in order."""

    def __init__(self, fused):
        import torch
        self.torch_ran, self.packed_for, self.fused = [], [], fused
        self.hooks = [m.register_forward_hook(lambda m_, i, o: self.torch_ran.append(m_)) for m in fused.encoder.modules()
                      if isinstance(m, torch.nn.Conv2d)]
        inner = fused._packed_conv

        def spied(eng, conv, dtype, device):
            self.packed_for.append(conv)
            return inner(eng, conv, dtype, device)

        fused._packed_conv = spied

    def close(self):
        for h in self.hooks:
            h.remove()
        del self.fused._packed_conv


# ---- stagewise, and end to end ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("kind", list(KINDS))
def test_every_plain_convolution_is_one_launch_that_meets_its_referee(dev, kind, regime):
    import torch
    from vppstereo_amd.extractor import FusedEncoder
    enc, x, eng = _model(kind, regime, dev), _image(regime, dev), _eng(dev)
    fused = FusedEncoder(enc, convs=True)
    watch = _Watch(fused)
    try:
        with L.LaunchSpy(eng, names=("raft_conv",)) as spy:
            got = _forward(fused, x, regime)
            torch.cuda.synchronize()
    finally:
        watch.close()
    plain_convs = EM.convs_of(enc)
    assert len(spy.records) == len(plain_convs) == (15 if kind == "basic" else 38)
    assert watch.torch_ran == [enc.conv1], "only the stem runs in torch"
    assert len(watch.packed_for) == len(spy.records) and set(map(id, watch.packed_for)) == set(map(id, plain_convs))
    want = torch.float32 if regime == "float32" else torch.bfloat16                        # under autocast the stem returns bfloat16
    strides = set()
    for k, (rec, conv) in enumerate(zip(spy.records, watch.packed_for)):
        assert rec.args[0].dtype == rec.result.dtype == want, k
        strides.add((conv.kernel_size[0], rec.kwargs["stride"]))
        SR.check_launch(rec, conv, f"{kind} [{regime}] launch {k}: {conv.in_channels} -> {conv.out_channels} k{conv.kernel_size[0]} s{conv.stride[0]}")
    assert strides >= {(3, 1), (3, 2), (1, 2)} and all(t.dtype == want for t in got)
    assert len(fused._packed) == len(plain_convs)
    worst = _hold(got, _plain(enc, x, regime), _f64(enc, x), f"{kind} [{regime}]")
    print(f"{kind} [{regime}]: the largest ratio {worst:.3f}")


@pytest.mark.parametrize("kind", list(KINDS))
def test_convs_false_is_todays_path(dev, kind):
    import torch
    from vppstereo_amd.extractor import FusedEncoder
    enc, x, eng = _model(kind, "float32", dev), _image("float32", dev), _eng(dev)
    n_convs = sum(isinstance(m, torch.nn.Conv2d) for m in enc.modules())
    outs = []
    for fused in (FusedEncoder(enc), FusedEncoder(enc, convs=False)):
        watch = _Watch(fused)
        try:
            with L.LaunchSpy(eng, names=("raft_conv",)) as spy:
                outs.append(_forward(fused, x, "float32"))
        finally:
            watch.close()
        assert spy.records == [] and watch.packed_for == [] and len(watch.torch_ran) == n_convs and fused._packed == {}
    assert all(torch.equal(a, b) for a, b in zip(*outs))


@pytest.mark.parametrize("regime", ["float32", "autocast"])
def test_across_calls_of_changing_size_and_a_replaced_weight(dev, regime):
    """One wrapper: the first size, a smaller odd one (maps of 21 x 45, 11 x 23, 6 x 12, 3 x 6, 2 x 3), the first again; then a weight of
    a strided convolution replaced (`p.data = new`) and one written in place.  What a wrapper keeps from call to call (packed
    weights, norm constants) must not show: every call gives the bits of a wrapper made for that call alone.  The end-to-end bound
    is held at the first size only: its factor is argued for maxima over thousands of cells, which a [1,16,2,3] output is not."""
    import torch
    from vppstereo_amd.extractor import FusedEncoder
    enc = copy.deepcopy(_model("multi", regime, dev))
    fused = FusedEncoder(enc, convs=True)
    fresh = lambda x: _forward(FusedEncoder(enc, convs=True), x, regime)                # noqa: E731
    small = (1, 3, 21, 45)
    first = None
    for shape in (EM.INPUT, small, EM.INPUT):
        x = _image(regime, dev, shape)
        got = _forward(fused, x, regime)
        assert tuple(got[-1].shape[2:]) == ((3, 4) if shape == EM.INPUT else (2, 3))
        assert all(torch.equal(a, b) for a, b in zip(got, fresh(x))), f"{shape}: not the bits of a fresh wrapper"
        if shape == EM.INPUT:
            if first is None:
                _hold(got, _plain(enc, x, regime), _f64(enc, x), f"multi [{regime}] {shape}")
            first = got
    packed = {k: v[1] for k, v in fused._packed.items()}
    assert len(packed) == 38
    gen = torch.Generator().manual_seed(6801)
    c1, dn = enc.layer2[0].conv1, enc.layer4[0].downsample[0]
    c1.weight.data = (torch.randn(c1.weight.shape, generator=gen) * 0.1).to(c1.weight)
    with torch.no_grad():
        dn.weight.copy_((torch.randn(dn.weight.shape, generator=gen) * 0.2).to(dn.weight))
    x = _image(regime, dev)
    got = _forward(fused, x, regime)
    assert all(torch.equal(a, b) for a, b in zip(got, fresh(x))), "the new weights were not followed"
    assert not any(torch.equal(a, b) for a, b in zip(got, first))
    again = {k for k, v in fused._packed.items() if v[1] is not packed[k]}
    assert again == {id(c1), id(dn)}, "exactly the two convolutions were packed again"
