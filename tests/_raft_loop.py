"""The composed RAFT-Stereo loop for tests/test_gpu_raft_loop.py and tests/test_raft_loop_cpu.py: a live stand-in model, the
loop twice over the same modules (plain torch, and with the patch of INTEGRATION.md applied), a spy on the Engine's launches
and adapters from a spied launch to the float64 referee of that launch.

TEST INFRASTRUCTURE ONLY.  torch is imported where it is used; nothing here needs a GPU to import.

The model is written from the interfaces vppstereo_amd/extractor.py, corr.py, update.py and readout.py document, out of
torch.nn modules, seeded: a basic encoder with InstanceNorm2d, a multi encoder with BatchNorm2d in eval mode (seeded running
statistics and affine parameters), three context convolutions, an update block in the shape of `_block()` of
tests/test_gpu_gruconv.py with real convolutions everywhere, a flow head and a mask of 9 * 4 * 4 channels.  Widths are narrow
but taken by every kernel: hidden sizes of 16 at the three levels make the GRUs' inputs 32, 48 and 48 channels (multiples of 16
within CONV_MAX_CIN / CONV_MAX_COUT), convc1 and convf1 have 16 outputs (a multiple of 16 within VPPX_MOTION_MAX_CH, convf1 7x7 =
VPPX_MOTION_MAX_KS), and the feature dimension is 32 (raft_corr_fused takes any D > 0).  `assert_no_fallback` checks it.

What is float32 in every regime: the coordinates, the flow handed on from iteration to iteration, the correlation volume (the
feature maps go through `.float()`, as the reference's do) and the disparity.  The update block gets the flow in the weights'
dtype.  The mask is widened to the flow's dtype before the read-out in both forwards: `Engine.raft_upsample` wants both of one
dtype, and widening a bfloat16 cell is exact.
"""
import contextlib
from types import SimpleNamespace

import numpy as np

F32, F64 = np.float32, np.float64
HIDDEN = 16
FEATURES = 32
MOTION = 14                       # the motion encoder's output channels: with the flow's two, 16
LEVELS, RADIUS = 4, 4
SPIED = ("raft_norm_stats", "raft_norm_apply", "raft_corr_fused", "raft_corr_pyramid", "raft_corr_lookup", "raft_motion_front",
         "raft_gru_assemble", "raft_gru_reset", "raft_gru_update", "raft_gru_zr", "raft_gru_q", "raft_upsample")
MISTAKES = ("gru16_reads_new_net0", "gru08_reads_old_net1", "pool_interp_exchanged", "no_reset", "flow_sign", "no_hints", "stale_hx")


# ---------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------
def _res_block(nn, cin, cout, norm, stride):
    b = nn.Module()
    b.conv1 = nn.Conv2d(cin, cout, 3, padding=1, stride=stride)
    b.conv2 = nn.Conv2d(cout, cout, 3, padding=1)
    b.norm1, b.norm2 = norm(cout), norm(cout)
    b.downsample = None if stride == 1 and cin == cout else nn.Sequential(nn.Conv2d(cin, cout, 1, stride=stride), norm(cout))
    return b


def _trunk(nn, enc, norm):
    """conv1 (7x7, stride 2), norm1 and layer1..3 of two residual blocks each: 1/4 of the image, 16 channels."""
    enc.conv1, enc.norm1 = nn.Conv2d(3, 8, 7, stride=2, padding=3), norm(8)
    enc.layer1 = nn.Sequential(_res_block(nn, 8, 8, norm, 1), _res_block(nn, 8, 8, norm, 1))
    enc.layer2 = nn.Sequential(_res_block(nn, 8, 12, norm, 2), _res_block(nn, 12, 12, norm, 1))
    enc.layer3 = nn.Sequential(_res_block(nn, 12, 16, norm, 1), _res_block(nn, 16, 16, norm, 1))


def build_model(seed=6001):
    """-> an nn.Module in eval mode, float32, on the CPU: fnet, cnet, context_zqr_convs, update_block."""
    import torch
    nn = torch.nn
    torch.manual_seed(seed)
    inorm = lambda c: nn.InstanceNorm2d(c)                                              # noqa: E731
    bnorm = lambda c: nn.BatchNorm2d(c)                                                 # noqa: E731
    model = nn.Module()
    model.fnet = nn.Module()
    _trunk(nn, model.fnet, inorm)
    model.fnet.conv2 = nn.Conv2d(16, FEATURES, 1)
    cnet = model.cnet = nn.Module()
    _trunk(nn, cnet, bnorm)
    cnet.layer4 = nn.Sequential(_res_block(nn, 16, 16, bnorm, 2), _res_block(nn, 16, 16, bnorm, 1))
    cnet.layer5 = nn.Sequential(_res_block(nn, 16, 16, bnorm, 2), _res_block(nn, 16, 16, bnorm, 1))
    head = lambda: nn.Sequential(_res_block(nn, 16, 16, bnorm, 1), nn.Conv2d(16, HIDDEN, 3, padding=1))     # noqa: E731
    cnet.outputs08 = nn.ModuleList([head(), head()])
    cnet.outputs16 = nn.ModuleList([head(), head()])
    cnet.outputs32 = nn.ModuleList([nn.Conv2d(16, HIDDEN, 3, padding=1), nn.Conv2d(16, HIDDEN, 3, padding=1)])
    model.context_zqr_convs = nn.ModuleList([nn.Conv2d(HIDDEN, 3 * HIDDEN, 3, padding=1) for _ in range(3)])

    def gru(inp):
        g = nn.Module()
        g.convz, g.convr, g.convq = (nn.Conv2d(HIDDEN + inp, HIDDEN, 3, padding=1) for _ in range(3))
        return g

    blk = model.update_block = nn.Module()
    blk.n_gru_layers = 3
    enc = blk.encoder = nn.Module()
    K = LEVELS * (2 * RADIUS + 1)
    enc.convc1, enc.convc2 = nn.Conv2d(K, 16, 1), nn.Conv2d(16, 16, 3, padding=1)
    enc.convf1, enc.convf2 = nn.Conv2d(2, 16, 7, padding=3), nn.Conv2d(16, 16, 3, padding=1)
    enc.conv = nn.Conv2d(32, MOTION, 3, padding=1)
    blk.gru08, blk.gru16, blk.gru32 = gru(MOTION + 2 + HIDDEN), gru(2 * HIDDEN), gru(HIDDEN)
    blk.flow_head = nn.Sequential(nn.Conv2d(HIDDEN, 16, 3, padding=1), nn.ReLU(), nn.Conv2d(16, 2, 3, padding=1))
    blk.mask = nn.Sequential(nn.Conv2d(HIDDEN, 32, 3, padding=1), nn.ReLU(), nn.Conv2d(32, 9 * 4 * 4, 1))
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in blk.modules():                 # as tests/test_gpu_gruconv.py's _block(): the gates move
            if isinstance(m, nn.Conv2d):
                m.weight.mul_(2.0)
        for m in model.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=gen) * 0.2)
                m.running_var.copy_(torch.rand(m.num_features, generator=gen) * 0.5 + 0.2)
                m.weight.copy_(torch.rand(m.num_features, generator=gen) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=gen) * 0.2)
    for p in model.parameters():
        p.requires_grad_(False)
    return model.eval()


def inputs(B, H, W, seed=6002, density=0.05):
    """-> namespace(image0, image2, image3 [B,3,H,W] in [0, 1], hints, validhints [B,1,H,W]) float32 numpy: hints on about
    `density` of the pixels, and on one in five of the pixels the sub-sampling reads, so that rows are modulated at any size."""
    rng = np.random.default_rng([seed, B, H, W])
    img = lambda: rng.random((B, 3, H, W)).astype(F32)                                  # noqa: E731
    valid = (rng.random((B, 1, H, W)) < density).astype(F32)
    valid[:, :, ::4, ::4] = (rng.random((B, 1, (H + 3) // 4, (W + 3) // 4)) < 0.2).astype(F32)
    hints = (rng.uniform(0.0, W / 2.0, (B, 1, H, W)).astype(F32) * valid).astype(F32)
    return SimpleNamespace(image0=img(), image2=img(), image3=img(), hints=hints, validhints=valid)


def map_sizes(H, W):
    """The three levels' map sizes of an H x W image."""
    out = [(H // 4, W // 4)]
    for _ in range(2):
        out.append(tuple((v - 1) // 2 + 1 for v in out[-1]))
    return out


def assert_no_fallback(model):
    """Every stage of the model is one the kernels take."""
    from vppstereo_amd import _lib
    from vppstereo_amd.update import GruGlue
    blk = model.update_block
    for gru, channels in ((blk.gru08, 3 * HIDDEN), (blk.gru16, 3 * HIDDEN), (blk.gru32, 2 * HIDDEN)):
        assert GruGlue._conv_takes(gru, HIDDEN, channels), channels
    for conv in (blk.encoder.convc1, blk.encoder.convf1):
        assert conv.out_channels % 16 == 0 and conv.out_channels <= _lib.MOTION_MAX_CH
    assert blk.encoder.convf1.kernel_size[0] <= _lib.MOTION_MAX_KS and LEVELS <= _lib.CORR_MAX_LEVELS and RADIUS <= _lib.CORR_MAX_RADIUS


# ---------------------------------------------------------------------------------------------------
# plain torch
# ---------------------------------------------------------------------------------------------------
def _autocast(device, on):
    import torch
    return torch.autocast(device.type, dtype=torch.bfloat16) if on else contextlib.nullcontext()


def _plain_block(blk, x):
    import torch
    y = torch.relu(blk.norm1(blk.conv1(x)))
    y = torch.relu(blk.norm2(blk.conv2(y)))
    if blk.downsample is not None:
        x = blk.downsample(x)
    return torch.relu(x + y)


def _plain_trunk(enc, x):
    import torch
    x = torch.relu(enc.norm1(enc.conv1(x)))
    for layer in (enc.layer1, enc.layer2, enc.layer3):
        for blk in layer:
            x = _plain_block(blk, x)
    return x


def _plain_cnet(enc, x):
    x = _plain_trunk(enc, x)
    o08 = [f[1](_plain_block(f[0], x)) for f in enc.outputs08]
    y = x
    for blk in enc.layer4:
        y = _plain_block(blk, y)
    o16 = [f[1](_plain_block(f[0], y)) for f in enc.outputs16]
    z = y
    for blk in enc.layer5:
        z = _plain_block(blk, z)
    return o08, o16, [f(z) for f in enc.outputs32]


def plain_volume(fmap2, fmap3, hints, validhints):
    """All-pairs correlation along the row / sqrt(D) and the hint modulation -> [B,H4,W2,W3] in the maps' dtype."""
    import torch
    import torch.nn.functional as Fn
    D = fmap2.shape[1]
    corr = torch.einsum("bdhi,bdhj->bhij", fmap2, fmap3) / torch.sqrt(torch.tensor(float(D), dtype=fmap2.dtype, device=fmap2.device))
    if hints is None:
        return corr
    B, H4, W2, W3 = corr.shape
    v = Fn.interpolate(validhints.to(corr.dtype), size=(H4, W2), mode="nearest")[:, 0]
    h = Fn.interpolate(hints.to(corr.dtype), size=(H4, W2), mode="nearest")[:, 0] * v / 4
    x = torch.arange(W2, dtype=corr.dtype, device=corr.device)
    target = (x * v - h)[..., None]
    k = torch.arange(W3, dtype=corr.dtype, device=corr.device)
    return corr * ((1 - v)[..., None] + (10 * v)[..., None] * torch.exp(-(k - target) ** 2 / 2))


def plain_pyramid(level0, levels=LEVELS):
    out = [level0]
    for _ in range(1, levels):
        w = out[-1].shape[-1] // 2
        out.append((out[-1][..., 0:2 * w:2] + out[-1][..., 1:2 * w:2]) / 2)
    return out


def plain_lookup(pyr, cx, radius=RADIUS):
    """pyr: levels [B,H4,W2,Wi]; cx [B,H4,W2] -> [B, levels*(2r+1), H4, W2]: linear taps at cx / 2^i + t, zero outside."""
    import torch
    t = torch.arange(-radius, radius + 1, dtype=cx.dtype, device=cx.device)
    outs = []
    for i, lev in enumerate(pyr):
        W = lev.shape[-1]
        x = cx[..., None] / 2 ** i + t
        x0 = torch.floor(x)
        w1 = x - x0
        taps = 0
        for xi, wi in ((x0, 1 - w1), (x0 + 1, w1)):
            inside = (xi >= 0) & (xi <= W - 1)
            val = torch.gather(lev, -1, xi.clamp(0, W - 1).long())
            taps = taps + torch.where(inside, val * wi, torch.zeros_like(val))
        outs.append(taps)
    return torch.cat(outs, dim=-1).permute(0, 3, 1, 2).contiguous()


def _pool2x(x):
    import torch.nn.functional as Fn
    return Fn.avg_pool2d(x, 3, stride=2, padding=1)


def _interp(x, dest):
    import torch.nn.functional as Fn
    return Fn.interpolate(x, dest.shape[2:], mode="bilinear", align_corners=True)


def _plain_gru(gru, h, ctx, xs, mistake=None, stale=None, tag=None):
    import torch
    cz, cr, cq = ctx
    x = torch.cat(xs, dim=1)
    hx = torch.cat([h.to(x.dtype) if x.dtype != h.dtype else h, x], dim=1)
    if mistake == "stale_hx" and stale is not None and tag == 8:
        if tag in stale:
            hx, fresh = stale[tag], hx
            stale[tag] = fresh
            x = hx[:, h.shape[1]:]
        else:
            stale[tag] = hx
    z = torch.sigmoid(gru.convz(hx) + cz)
    r = torch.sigmoid(gru.convr(hx) + cr)
    rh = h if mistake == "no_reset" else r * h
    q = torch.tanh(gru.convq(torch.cat([rh.to(x.dtype), x], dim=1)) + cq)
    return ((1 - z) * h + z * q).to(h.dtype)


def _plain_update(blk, net, inp, corr=None, flow=None, iter08=True, iter16=True, iter32=True, update=True, mistake=None, stale=None):
    import torch
    old0, old1 = net[0], net[1]
    if iter32:
        net[2] = _plain_gru(blk.gru32, net[2], inp[2], [_pool2x(net[1])], mistake)
    if iter16:
        xs = [_pool2x(net[0]), _interp(net[2], net[1])]
        if mistake == "pool_interp_exchanged":
            xs = xs[::-1]
        net[1] = _plain_gru(blk.gru16, net[1], inp[1], xs, mistake)
    if iter08:
        enc = blk.encoder
        cor = torch.relu(enc.convc2(torch.relu(enc.convc1(corr))))
        flo = torch.relu(enc.convf2(torch.relu(enc.convf1(flow))))
        out = torch.relu(enc.conv(torch.cat([cor, flo], dim=1)))
        up = old1 if mistake == "gru08_reads_old_net1" else net[1]
        net[0] = _plain_gru(blk.gru08, net[0], inp[0], [out, flow, _interp(up, net[0])], mistake, stale, 8)
        if mistake == "gru16_reads_new_net0" and iter16:
            net[1] = _plain_gru(blk.gru16, old1, inp[1], [_pool2x(net[0]), _interp(net[2], old1)], mistake)
    if not update:
        return net
    return net, .25 * blk.mask(net[0]), blk.flow_head(net[0])


def plain_upsample(flow, mask, negate=True, crop=None, factor=4):
    """Convex upsampling of channel 0 of `flow` with the softmax of `mask` over its 9 taps -> [B,1,Hout,Wout]."""
    import torch
    import torch.nn.functional as Fn
    B, _, H, W = flow.shape
    m = torch.softmax(mask.view(B, 1, 9, factor, factor, H, W), dim=2)
    taps = Fn.unfold(factor * flow[:, :1], [3, 3], padding=1).view(B, 1, 9, 1, 1, H, W)
    up = torch.sum(m * taps, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(B, 1, factor * H, factor * W)
    if negate:
        up = -up
    if crop is not None:
        left, right, top, bottom = crop
        up = up[:, :, top:factor * H - bottom, left:factor * W - right]
    return up.contiguous()


def _coords(B, H, W, dtype, device):
    import torch
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dtype, device=device), torch.arange(W, dtype=dtype, device=device), indexing="ij")
    return torch.stack([xs, ys], dim=0)[None].repeat(B, 1, 1, 1)


def _wdtype(model):
    return model.update_block.gru08.convz.weight.dtype


def _loop(model, update, corr_of, upsample, image, hints, iters, schedule, autocast, net, inp):
    """The iterations both forwards share: `update(net, inp, corr, flow, **flags)`, `corr_of(coords1)` and `upsample(flow, mask)`
    are the three places where they differ."""
    import torch
    assert schedule in ("default", "slow_fast")
    wdtype = _wdtype(model)
    cdtype = torch.float64 if wdtype == torch.float64 else torch.float32
    B, _, H4, W4 = net[0].shape
    coords0 = _coords(B, H4, W4, cdtype, image.device)
    coords1 = coords0.clone()
    mask = None
    for _ in range(iters):
        coords1 = coords1.detach()
        corr = corr_of(coords1)
        flow = coords1 - coords0
        with _autocast(image.device, autocast):
            if schedule == "slow_fast":
                net = update(net, inp, iter32=True, iter16=False, iter08=False, update=False)
                net = update(net, inp, iter32=True, iter16=True, iter08=False, update=False)
            net, mask, delta = update(net, inp, corr, flow.to(wdtype))
        delta[:, 1] = 0.0
        coords1 = coords1 + delta
    flow = coords1 - coords0
    return SimpleNamespace(flow=flow, net=list(net), disparity=upsample(flow, mask.to(flow.dtype)))


def plain_forward(model, image0, image2, image3, hints=None, validhints=None, iters=3, schedule="default", autocast=False, crop=None,
                  mistake=None):
    """The composition in plain torch operations, in the model's dtype on the images' device (`.double()` on the CPU: the
    float64 run).  -> namespace(flow [B,2,H4,W4], net [three hidden states], disparity [B,1,Hout,Wout]).  `mistake`: one of
    MISTAKES, planted into the composition."""
    import torch
    assert mistake is None or mistake in MISTAKES
    with torch.no_grad():
        with _autocast(image0.device, autocast):
            cnet = _plain_cnet(model.cnet, image0)
            both = model.fnet.conv2(_plain_trunk(model.fnet, torch.cat([image2, image3], dim=0)))
            fmap2, fmap3 = both.split(image2.shape[0], dim=0)
            net = [torch.tanh(x[0]) for x in cnet]
            inp = [torch.relu(x[1]) for x in cnet]
            inp = [list(conv(i).split(HIDDEN, dim=1)) for i, conv in zip(inp, model.context_zqr_convs)]
        if _wdtype(model) != torch.float64:
            fmap2, fmap3 = fmap2.float(), fmap3.float()
        no_hints = hints is None or mistake == "no_hints"
        pyr = plain_pyramid(plain_volume(fmap2, fmap3, None if no_hints else hints, None if no_hints else validhints))
        wdtype, stale = _wdtype(model), {}

        def corr_of(coords1):
            return plain_lookup(pyr, coords1[:, 0]).to(wdtype)

        def update(net, inp, corr=None, flow=None, **flags):
            return _plain_update(model.update_block, net, inp, corr, flow, mistake=mistake, stale=stale, **flags)

        def upsample(flow, mask):
            return plain_upsample(flow, mask, negate=mistake != "flow_sign", crop=crop)

        return _loop(model, update, corr_of, upsample, image0, hints, iters, schedule, autocast, net, inp)


# ---------------------------------------------------------------------------------------------------
# the patch of INTEGRATION.md
# ---------------------------------------------------------------------------------------------------
def wrap(model, motion_front=True, gru_conv=True):
    """The wrappers of INTEGRATION.md around the model's own modules -> namespace(fnet, cnet, update)."""
    from vppstereo_amd.extractor import FusedEncoder
    from vppstereo_amd.update import FusedUpdate
    return SimpleNamespace(fnet=FusedEncoder(model.fnet), cnet=FusedEncoder(model.cnet),
                           update=FusedUpdate(model.update_block, motion_front=motion_front, gru_conv=gru_conv))


def fused_forward(model, wrapped, image0, image2, image3, hints=None, validhints=None, iters=3, schedule="default", autocast=False,
                  crop=None, corr_block="fused"):
    """The same loop with the patch applied: FusedEncoder around both encoders, CorrBlock1DFused (or CorrBlock1D) on the
    `.float()` feature maps, `corr_fn.deferred(coords1)`, FusedUpdate, and `raft_upsample(..., negate=True, channels=1, crop=)`.
    -> what plain_forward returns."""
    import torch
    from vppstereo_amd.corr import CorrBlock1D, CorrBlock1DFused, _engine
    with torch.no_grad():
        with _autocast(image0.device, autocast):
            cnet = wrapped.cnet(image0, num_layers=3)
            fmap2, fmap3 = wrapped.fnet([image2, image3])
            net = [torch.tanh(x[0]) for x in cnet]
            inp = [torch.relu(x[1]) for x in cnet]
            inp = [list(conv(i).split(HIDDEN, dim=1)) for i, conv in zip(inp, model.context_zqr_convs)]
        block = CorrBlock1DFused if corr_block == "fused" else CorrBlock1D
        if hints is not None:
            corr_fn = block(fmap2.float(), fmap3.float(), hints=hints, validhints=validhints, radius=RADIUS, num_levels=LEVELS)
        else:
            corr_fn = block(fmap2.float(), fmap3.float(), radius=RADIUS, num_levels=LEVELS)
        eng = _engine(image0.device)

        def upsample(flow, mask):
            return eng.raft_upsample(flow, mask, negate=True, channels=1, crop=crop)

        return _loop(model, wrapped.update, corr_fn.deferred, upsample, image0, hints, iters, schedule, autocast, net, inp)


# ---------------------------------------------------------------------------------------------------
# the spy
# ---------------------------------------------------------------------------------------------------
def _host_copy(a):
    """Tensors anywhere in a (lists, tuples, dicts) as host copies of their own; everything else as it is."""
    if hasattr(a, "detach") and hasattr(a, "cpu"):
        return a.detach().cpu().clone()
    if isinstance(a, (list, tuple)):
        return type(a)(_host_copy(v) for v in a)
    if isinstance(a, dict):
        return {k: _host_copy(v) for k, v in a.items()}
    return a


class LaunchSpy:
    """`with LaunchSpy(eng) as spy:` wraps the SPIED methods on that Engine INSTANCE and restores them on exit, also after an
    exception.  Per call `spy.records` gains namespace(name, args, kwargs, result, out): host copies of every tensor argument
    taken BEFORE the call (several launches work in place), and host copies of the result and of every buffer handed in to be
    written (`out=`, `z=`, `rh=`) taken after it."""
    WRITTEN = ("out", "z", "rh")

    def __init__(self, eng, names=SPIED):
        self.eng, self.names, self.records, self._saved = eng, tuple(names), [], {}

    def _wrap(self, name, fn):
        def spied(*args, **kwargs):
            rec = SimpleNamespace(name=name, args=_host_copy(args), kwargs=_host_copy(kwargs), result=None, out={})
            res = fn(*args, **kwargs)
            rec.result = _host_copy(res)
            rec.out = {k: _host_copy(kwargs[k]) for k in self.WRITTEN if kwargs.get(k) is not None}
            self.records.append(rec)
            return res
        return spied

    def __enter__(self):
        for name in self.names:
            self._saved[name] = (name in vars(self.eng), vars(self.eng).get(name))
            setattr(self.eng, name, self._wrap(name, getattr(self.eng, name)))
        return self

    def __exit__(self, *exc):
        for name, (had, val) in self._saved.items():
            if had:
                setattr(self.eng, name, val)
            else:
                delattr(self.eng, name)
        self._saved.clear()
        return False

    def of(self, name):
        return [r for r in self.records if r.name == name]

    def counts(self):
        return {name: len(self.of(name)) for name in self.names}


# ---------------------------------------------------------------------------------------------------
# adapters: a spied launch against the referee of that launch, on the inputs the device actually had
# ---------------------------------------------------------------------------------------------------
def _np(t):
    """A host tensor of either dtype as float32 (exact), None as None."""
    return None if t is None else t.float().numpy()


def _dt(t):
    import torch
    return "bfloat16" if t.dtype == torch.bfloat16 else "float32"


def _arg(rec, k, name, default=None):
    """Positional argument k of a record, or its keyword."""
    return rec.args[k] if len(rec.args) > k else rec.kwargs.get(name, default)


def _given(st):
    """Statistics handed in as float32 numbers: the kernel reads exactly these, so they carry no bound (as
    tests/test_gpu_norm.py takes them)."""
    st = np.asarray(st, F64)
    st = st[None] if st.ndim == 2 else st
    return SimpleNamespace(mean=st[..., 0], rstd=st[..., 1], dmean=np.zeros(st.shape[:2]), drstd=np.zeros(st.shape[:2]))


def check_norm_stats(rec, what):
    import _norm_ref as N
    from _cells import hold
    x = _arg(rec, 0, "x")
    ref = N.stats_value(N.stats(_np(x), _arg(rec, 1, "eps", 1e-5)))
    hold(N, _np(rec.result), ref, what, "float32")


def check_norm_apply(rec, what):
    import _norm_ref as N
    from _cells import hold
    x, st = _arg(rec, 0, "x"), _arg(rec, 1, "stats")
    kw = rec.kwargs
    rs = kw.get("residual_stats")
    ref = N.apply(_np(x), _given(_np(st)), _np(_arg(rec, 2, "weight")), _np(_arg(rec, 3, "bias")), relu_inner=bool(_arg(rec, 4, "relu", True)),
                  res=_np(kw.get("residual")), res_stats=None if rs is None else _given(_np(rs)), res_weight=_np(kw.get("residual_weight")),
                  res_bias=_np(kw.get("residual_bias")))
    hold(N, _np(rec.result), ref, what, _dt(x))


def check_corr_fused(rec, what):
    """Level 0 within `_corr_fused_ref.bound` as tests/test_gpu_corr_fused.py holds random features to it; the levels above are
    the pyramid rule on level 0 as stored, bit for bit."""
    import _corr_fused_ref as FR
    import _corr_ref as CR
    f2, f3 = _arg(rec, 0, "fmap2"), _arg(rec, 1, "fmap3")
    hints, valid = _arg(rec, 2, "hints"), _arg(rec, 3, "validhints")
    bf16 = _dt(f2) == "bfloat16"
    got = [_np(t).reshape(t.shape[0], t.shape[-1]) for t in rec.result]
    c64, lim = FR.bound(_np(f2), _np(f3), _np(hints), _np(valid), bf16)
    dist = np.abs(got[0].astype(F64) - c64)
    beyond = ~(dist <= lim) & (got[0] != 0)
    worst = float(np.max(np.where(lim > 0, dist / np.where(lim > 0, lim, 1.0), 0.0)))
    print(f"{what} [{_dt(f2)}]: {got[0].size} cells, worst distance / bound {worst:.4f}, {int(beyond.sum())} beyond")
    assert np.isfinite(got[0]).all() and not beyond.any(), f"{what}: {int(beyond.sum())} cells beyond the bound"
    level0 = FR.bf16_round(got[0]) if bf16 else got[0]
    want = CR.widened(CR.pyramid(level0, len(got)))
    for i in range(1, len(got)):
        assert CR.same_bits(got[i], want[i]) == 0, f"{what}: level {i} is not the pooled level below"


def check_motion_front(rec, what):
    import _motion_ref as M
    from _cells import hold
    pyr, coords, flow = rec.args[0], rec.args[1], rec.args[2]
    wc, bc, wf, bf = (_np(t) for t in rec.args[3:7])
    radius = _arg(rec, 7, "radius", 4)
    levels = []
    for t in pyr:
        a = _np(t).reshape(t.shape[0], t.shape[-1])
        levels.append(M.BR.bits(a) if _dt(t) == "bfloat16" else a)
    cx = _np(coords)
    cx = cx[:, 0] if cx.ndim == 4 else cx
    ref_c, ref_f = M.front(levels, np.ascontiguousarray(cx), _np(flow), wc, bc, wf, bf, radius)
    hold(M, _np(rec.result[0]), ref_c, f"{what}: cor1", _dt(rec.result[0]))
    hold(M, _np(rec.result[1]), ref_f, f"{what}: flo1", _dt(rec.result[1]))


def check_assemble(rec, what):
    import _gru_ref as G
    from _cells import hold
    out = rec.out["out"] if "out" in rec.out else rec.result
    ref = G.assemble([(_np(t), mode) for t, mode in rec.args[0]], out.shape[2], out.shape[3])
    hold(G, _np(out), ref, what, _dt(out))


def gru_weights(gru):
    """The live module's weights as the referee takes them: float32 numpy."""
    return {f"{cv}_{p}": getattr(getattr(gru, cv), p).detach().float().cpu().numpy() for cv in ("convz", "convr", "convq")
            for p in ("weight", "bias")}


def check_gru_zr(rec, W, what):
    import _gruconv_ref as R
    from _cells import hold
    hx, cz, cr, h = rec.args[0], rec.args[2], rec.args[3], rec.args[4]
    x1 = rec.kwargs.get("x1")
    dtype = _dt(h)
    z, rh = R.zr(_np(hx), _np(x1), W["convz_weight"], W["convz_bias"], W["convr_weight"], W["convr_bias"], _np(cz), _np(cr), _np(h), dtype)
    hold(R, _np(rec.result[0]), z, f"{what}: z", dtype)
    hold(R, _np(rec.result[1]), rh, f"{what}: r*h", dtype)


def check_gru_q(rec, W, what):
    import _gruconv_ref as R
    from _cells import hold
    rh, cq, z, h = rec.args[0], rec.args[2], rec.args[3], rec.args[4]
    dtype = _dt(h)
    ref = R.q(_np(rh), _np(rec.kwargs.get("x1")), W["convq_weight"], W["convq_bias"], _np(cq), _np(z), _np(h), dtype)
    hold(R, _np(rec.result), ref, what, dtype)


def check_upsample(rec, what):
    import _readout_ref as RO
    import _referee
    from _cells import hold
    flow, mask = rec.args[0], rec.args[1]
    kw = rec.kwargs
    f = 2 ** int(_arg(rec, 2, "n_downsample", 2))
    ref = RO.raft_upsample(_np(flow), _np(mask), f, negate=bool(kw.get("negate", False)), channels=kw.get("channels"), crop=kw.get("crop"))
    hold(_referee, _np(rec.result), ref, what, "float32")


def check_all(spy, model, sizes):
    """Every spied launch against its referee.  sizes: the three levels' (H, W), which tell a GRU record's level."""
    blk = model.update_block
    weights = {sizes[0]: gru_weights(blk.gru08), sizes[1]: gru_weights(blk.gru16), sizes[2]: gru_weights(blk.gru32)}
    level = {sizes[0]: "gru08", sizes[1]: "gru16", sizes[2]: "gru32"}
    n = 0
    for k, rec in enumerate(spy.records):
        what = f"launch {k} {rec.name}"
        if rec.name == "raft_norm_stats":
            check_norm_stats(rec, what)
        elif rec.name == "raft_norm_apply":
            check_norm_apply(rec, what)
        elif rec.name == "raft_corr_fused":
            check_corr_fused(rec, what)
        elif rec.name == "raft_motion_front":
            check_motion_front(rec, what)
        elif rec.name == "raft_gru_assemble":
            check_assemble(rec, what)
        elif rec.name in ("raft_gru_zr", "raft_gru_q"):
            size = tuple(rec.args[4].shape[2:])
            (check_gru_zr if rec.name == "raft_gru_zr" else check_gru_q)(rec, weights[size], f"{what} {level[size]}")
        elif rec.name == "raft_upsample":
            check_upsample(rec, what)
        else:
            raise AssertionError(f"{what}: no referee is wired to this launch")
        n += 1
    return n
