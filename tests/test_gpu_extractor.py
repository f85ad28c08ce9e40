"""vppstereo_amd.extractor.FusedEncoder around stand-in encoders whose convolutions replay the recording of the reference's
own forward passes (tests/golden/extractor_cases.npz): a ResidualBlock of either norm kind with and without the downsample
path, BasicEncoder('instance') on a list of two images, MultiBasicEncoder('batch').eval() with dual_inp.

Every tensor the wrapper hands to a convolution, and what it returns, is held to the recorded one within the referee's
limit_any_f32() (tests/_norm_ref.py; the recording is torch's CPU arithmetic), where a block's result inherits the bound its
residual arrived with, and to the referee's own value within limit(), the residual being the tensor the wrapper itself
handed on.  No atol.  In bfloat16 every handed tensor lies in the band a single rounding allows."""
import numpy as np
import pytest
import torch

import _norm_ref as N

pytestmark = pytest.mark.gpu

F32 = np.float32
G = N.load_recording()
DEV = "cuda"


class Replay(torch.nn.Module):
    """A convolution that logs what it is handed and returns its recorded output (a fresh tensor every call)."""

    def __init__(self, unit, path, dtype, log):
        super().__init__()
        self.path, self.log = path, log
        self.out = torch.from_numpy(N.conv_out(G, unit, path)).to(DEV).to(dtype)

    def forward(self, x):
        assert self.path not in self.log, self.path
        self.log[self.path] = x.detach().clone()
        return self.out.clone()


def stand_in(unit, dtype, log):
    """The recorded unit as modules: Replay convolutions, and norms of the recorded kind with the recorded parameters."""
    has = lambda path: f"{unit}/{path}/out" in G.files                                  # noqa: E731
    conv = lambda path: Replay(unit, path, dtype, log)                                  # noqa: E731

    def norm(path, channels):
        if f"{unit}/{path}/running_mean" not in G.files:
            return torch.nn.InstanceNorm2d(channels)
        m = torch.nn.BatchNorm2d(channels)
        with torch.no_grad():
            for k in ("running_mean", "running_var", "weight", "bias"):
                getattr(m, k).copy_(torch.from_numpy(G[f"{unit}/{path}/{k}"]))
        return m.eval()

    def block(prefix):
        b = torch.nn.Module()
        Cc = G[f"{unit}/{prefix}conv1/out"].shape[1]
        b.conv1, b.conv2 = conv(prefix + "conv1"), conv(prefix + "conv2")
        b.norm1, b.norm2 = norm(prefix + "norm1", Cc), norm(prefix + "norm2", Cc)
        b.downsample = torch.nn.Sequential(conv(prefix + "downsample.0"), norm(prefix + "norm3", Cc)) if has(prefix + "downsample.0") else None
        return b

    if unit in N.BLOCK_UNITS:
        return block("")
    enc = torch.nn.Module()
    enc.conv1, enc.norm1 = conv("conv1"), norm("norm1", G[f"{unit}/conv1/out"].shape[1])
    for k in range(1, 6 if has("layer4.0.conv1") else 4):
        setattr(enc, f"layer{k}", torch.nn.Sequential(block(f"layer{k}.0."), block(f"layer{k}.1.")))
    if has("conv2"):
        enc.conv2 = conv("conv2")
    else:
        for name in ("outputs08", "outputs16"):
            setattr(enc, name, torch.nn.ModuleList([torch.nn.Sequential(block(f"{name}.{k}.0."), conv(f"{name}.{k}.1")) for k in range(2)]))
        enc.outputs32 = torch.nn.ModuleList([conv(f"outputs32.{k}") for k in range(2)])
    return enc.eval()


def _host(t):
    return t.float().cpu().numpy()


def _source(unit, path):
    """The convolution whose recorded input `path` reads (itself, unless the recording stores it once under another)."""
    return path if f"{unit}/{path}/in" in G.files else str(G[f"{unit}/{path}/in_of"])


def _hold(got, ref, what, dtype):
    got = _host(got)
    ref = N._ns(ref.value[:got.shape[0]], ref.limit[:got.shape[0]])                     # dual_inp: the heads read the first half
    if dtype == torch.bfloat16:
        beyond, other = N.compare_bf16(got, ref)
        worst = float("nan")
    else:
        worst, beyond, other = N.compare(got, ref)
    print(f"{what}: {got.size} cells, worst |got - value| / limit {worst:.3f}, {beyond} beyond, {other} of another class")
    assert beyond == 0 and other == 0, (what, beyond, other)


def _check_blocks(unit, log, dtype, results=None, also=None):
    """Every norm-stage tensor in `log` (and a block unit's result) against the recording and against the referee.
    also: (block prefix, tensor, recorded array) -- a block's full result where no convolution reads all of it."""
    handed = lambda path: log[path]                                                    # noqa: E731
    inherited = {}                              # convolution path -> the bound its handed input carries against the recorded one
    n = 0
    if unit not in N.BLOCK_UNITS:
        y = N.conv_out(G, unit, "conv1")
        for any_f32 in (True, False):
            s, w, b = N._norm_of(G, unit, "norm1", y, any_f32, None)
            ref = N.apply(y, s, w, b, any_f32=any_f32)
            if any_f32:
                inherited["layer1.0.conv1"] = ref.limit
                if dtype == torch.float32:
                    _hold(handed("layer1.0.conv1"), N._ns(N.conv_in(G, unit, "layer1.0.conv1"), ref.limit), f"{unit} stem vs recording", dtype)
            else:
                _hold(handed("layer1.0.conv1"), ref, f"{unit} stem vs referee", dtype)
        n += 1
    for prefix in N.block_prefixes(G, unit):
        src = _source(unit, prefix + "conv1")
        x_handed = _host(handed(prefix + "conv1"))
        nxt = N.consumer_of(G, unit, prefix) if unit not in N.BLOCK_UNITS else None
        got_out = results if unit in N.BLOCK_UNITS else handed(nxt)
        rl = inherited.get(src)
        anyf = N.block_stages(G, unit, prefix, any_f32=True, res_limit=None if rl is None else rl[:x_handed.shape[0]])
        if dtype == torch.float32:
            _hold(handed(prefix + "conv2"), N._ns(N.conv_in(G, unit, prefix + "conv2"), anyf[prefix + "conv2"].limit),
                  f"{unit} {prefix}conv2 vs recording", dtype)
            rec = G[f"{unit}/result"] if unit in N.BLOCK_UNITS else N.conv_in(G, unit, nxt)
            _hold(got_out, N._ns(rec, anyf[prefix + "out"].limit), f"{unit} {prefix}out vs recording", dtype)
        if nxt is not None:
            inherited[nxt] = anyf[prefix + "out"].limit
        tight = N.block_stages(G, unit, prefix, any_f32=False, res=x_handed)
        _hold(handed(prefix + "conv2"), tight[prefix + "conv2"], f"{unit} {prefix}conv2 vs referee", dtype)
        _hold(got_out, tight[prefix + "out"], f"{unit} {prefix}out vs referee", dtype)
        if also is not None and also[0] == prefix:
            if dtype == torch.float32:
                _hold(also[1], N._ns(also[2], anyf[prefix + "out"].limit), f"{unit} {prefix}out (whole) vs recording", dtype)
            _hold(also[1], tight[prefix + "out"], f"{unit} {prefix}out (whole) vs referee", dtype)
        n += 2
    return n


@pytest.fixture
def no_torch_glue(monkeypatch):
    """torch's norm, ReLU and add raise while the wrapper runs."""
    def raiser(name):
        def fn(*a, **k):
            raise AssertionError(f"the wrapper called torch's {name}")
        return fn
    for name in ("instance_norm", "batch_norm", "relu"):
        monkeypatch.setattr(torch.nn.functional, name, raiser(name))
    for name in ("relu", "add", "instance_norm", "batch_norm"):
        monkeypatch.setattr(torch, name, raiser(name))


def _image(a, dtype):
    return torch.from_numpy(a).to(DEV).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("unit", N.BLOCK_UNITS)
def test_a_residual_block(unit, dtype, no_torch_glue):
    """FusedEncoder's block step (the stride-1 block adds its input, the stride-2 block its normalised downsample path)."""
    from vppstereo_amd.corr import _engine
    from vppstereo_amd.extractor import FusedEncoder
    log = {}
    blk = stand_in(unit, dtype, log)
    x = _image(N.to_bf16(G[f"{unit}/x"]) if dtype == torch.bfloat16 else G[f"{unit}/x"], dtype)
    host = torch.nn.Module()                                                            # a wrapper to borrow the block step from
    host.conv1, host.norm1, host.conv2 = blk.conv1, blk.norm1, blk.conv2
    host.layer1 = host.layer2 = host.layer3 = torch.nn.Sequential(blk)
    with torch.no_grad():
        out = FusedEncoder(host)._block(_engine(x.device), blk, x)
    assert out.dtype == dtype and tuple(out.shape) == G[f"{unit}/result"].shape
    assert torch.equal(log["conv1"], x) and ("downsample.0" in log) == (unit.endswith("s2"))
    assert _check_blocks(unit, log, dtype, out) == 2


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_basic_encoder_on_a_list(dtype, no_torch_glue):
    from vppstereo_amd.extractor import FusedEncoder
    log = {}
    enc = FusedEncoder(stand_in("basic", dtype, log))
    pair = [_image(G["basic/x0"], dtype), _image(G["basic/x1"], dtype)]
    out = enc(pair)
    assert isinstance(out, tuple) and len(out) == 2                                     # the list input splits again
    for k in range(2):
        assert out[k].dtype == dtype and torch.equal(out[k].float().cpu(), torch.from_numpy(G[f"basic/result/{k}"]))
    assert torch.equal(log["conv1"], torch.cat(pair, dim=0))
    assert list(log) == N.conv_paths(G, "basic")                                        # every convolution, in the reference's order
    assert _check_blocks("basic", log, dtype) == 13


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_multi_encoder_dual_inp(dtype, no_torch_glue):
    from vppstereo_amd.extractor import FusedEncoder
    log = {}
    enc = FusedEncoder(stand_in("multi", dtype, log))
    x = _image(G["multi/x"], dtype)
    out = enc(x, dual_inp=True, num_layers=3)
    assert isinstance(out, tuple) and len(out) == 4 and [type(o) for o in out[:3]] == [list] * 3 and [len(o) for o in out[:3]] == [2] * 3
    for i in range(3):
        for j in range(2):                                                              # a head's last convolution is replayed: exact
            assert torch.equal(out[i][j].float().cpu(), torch.from_numpy(G[f"multi/result/{i}/{j}"])), (i, j)
    assert tuple(out[3].shape) == G["multi/result/3"].shape and out[3].shape[0] == 2 * out[0][0].shape[0]
    assert torch.equal(out[3][:1], log["outputs08.0.0.conv1"]) and torch.equal(log["conv1"], x)
    assert list(log) == N.conv_paths(G, "multi")
    assert _check_blocks("multi", log, dtype, also=("layer3.1.", out[3], G["multi/result/3"])) == 29     # v: the full batch
    for layers, want in ((1, 2), (2, 3)):                                               # the shorter returns of the reference
        log.clear()
        short = enc(x, dual_inp=True, num_layers=layers)
        assert len(short) == want and tuple(short[-1].shape) == G["multi/result/3"].shape and all(len(o) == 2 for o in short[:-1])


def test_frozen_statistics_follow_the_module():
    """The [C,2] tensor of a frozen BatchNorm is built once and again when the module's buffers change."""
    from vppstereo_amd.extractor import FusedEncoder
    log = {}
    enc = FusedEncoder(stand_in("multi", torch.float32, log))
    m = enc.encoder.norm1
    dev = torch.device(DEV, torch.cuda.current_device())
    a = enc._norm_consts(m, dev)
    assert enc._norm_consts(m, dev)[0] is a[0] and a[0].shape == (64, 2)
    want = torch.stack([m.running_mean.double(), 1 / torch.sqrt(m.running_var.double() + m.eps)], dim=1).float()
    assert torch.equal(a[0].cpu(), want)
    with torch.no_grad():
        m.running_var.mul_(4.0)
    b = enc._norm_consts(m, dev)
    assert b[0] is not a[0] and torch.allclose(b[0][:, 1].cpu(), want[:, 1] / 2, rtol=1e-4)
    m.train()
    with pytest.raises(RuntimeError, match="training mode"):
        enc(torch.from_numpy(G["multi/x"]).to(DEV), dual_inp=True)
