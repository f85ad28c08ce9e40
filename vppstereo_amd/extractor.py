"""RAFT-Stereo's encoders with the work between their convolutions on the device (INTEGRATION.md has the patch).

`FusedEncoder(encoder)` wraps a loaded `BasicEncoder` or `MultiBasicEncoder` (models/raft_stereo/extractor.py:122-300): any
module with `conv1`, `norm1`, `layer1` .. `layer3` (and `conv2` for the basic encoder; `layer4`, `layer5`, `outputs08`,
`outputs16`, `outputs32` for the multi encoder) whose blocks have `conv1`, `conv2`, `norm1`, `norm2` and `downsample`.  It
holds the encoder and calls every convolution as it is, so the weights and the `state_dict` are untouched; what it replaces
are the norm, ReLU and sum lines of `forward` (:181-183, :276-278) and of `ResidualBlock.forward` (:48-60).  Per norm one
statistics call (`Engine.raft_norm_stats`; none for a frozen BatchNorm, whose (running_mean, 1 / sqrt(running_var + eps))
are built once) and one launch that normalises, applies the ReLU and, behind a block's second convolution, adds the residual
-- normalised itself on the downsample path -- and applies the last ReLU (`Engine.raft_norm_apply`), in place over the
convolution's output.  include/vppx.h has the arithmetic.

Norms taken: `InstanceNorm2d` without running statistics, affine or not, and `BatchNorm2d` in eval mode.  Anything else
(GroupNorm, the empty Sequential of norm_fn='none', a BatchNorm in training mode, dropout while training) is a TypeError
when wrapping.  Inference only, as `FusedUpdate`: float32 or bfloat16; a tensor of another dtype than the first
convolution's output is converted to it, and a dtype the kernels do not store (float16) is an error.

`FusedEncoder(encoder, convs=True)` takes the convolutions too, as `FusedUpdate(block, convs=True)` does for the update block:
every convolution of the trunk and the blocks (conv1, conv2 and downsample[0] of each ResidualBlock, extractor.py:10-11,45),
the basic encoder's conv2 (:149), the second element of every outputs08 / outputs16 head and the outputs32 convolutions
(:231,240,247) runs as one launch of `Engine.raft_conv` in the dtype of its input, at stride 1 or 2.  Each convolution is decided
on its own: one that is not a plain nn.Conv2d (k 1 or 3, padding k // 2, stride (1, 1) or (2, 2), dilation 1, groups 1, zero
padding, Cin a positive multiple of 16 up to CONV_MAX_CIN, Cout up to CONV_MAX_COUT) runs in torch -- the 7x7 stem on three
channels always does --, as does one whose input is of a dtype the kernel does not store.  Under autocast the stem returns
bfloat16 and everything behind it runs in bfloat16 with weights rounded once when they are packed; a float32 model runs the
float32 matrix path.  The packed weights follow FusedUpdate's cache rule (`PackedWeights` of _convs.py, `forget_weights()`
included).  It is opt-in: README.md has what was measured.
"""
import torch

from ._convs import PackedWeights, conv_plain
from .corr import _engine
from .update import _as


def _blocks_of(encoder):
    """Every (name, ResidualBlock) the forward of the encoder runs."""
    names = ["layer1", "layer2", "layer3"] + (["layer4", "layer5"] if hasattr(encoder, "outputs08") else [])
    for name in names:
        if not hasattr(encoder, name):
            raise TypeError(f"FusedEncoder: the encoder has no {name!r}")
        for k, blk in enumerate(getattr(encoder, name)):
            yield f"{name}.{k}", blk
    for name in ("outputs08", "outputs16"):
        for k, head in enumerate(getattr(encoder, name, ())):
            yield f"{name}.{k}.0", head[0]


def _check_norm(m, where):
    if isinstance(m, torch.nn.InstanceNorm2d):
        if m.track_running_stats:
            raise TypeError(f"FusedEncoder: {where} is an InstanceNorm2d with running statistics")
    elif isinstance(m, torch.nn.BatchNorm2d):
        if m.training:
            raise TypeError(f"FusedEncoder: {where} is a BatchNorm2d in training mode; call .eval() first (inference only)")
        if m.running_mean is None or m.running_var is None:
            raise TypeError(f"FusedEncoder: {where} is a BatchNorm2d without running statistics")
    else:
        raise TypeError(f"FusedEncoder: {where} is a {type(m).__name__}; InstanceNorm2d and BatchNorm2d in eval mode are taken")


class FusedEncoder(torch.nn.Module, PackedWeights):
    """A module, so that it can take the encoder's place as `fnet` / `cnet` of a RAFTStereo; the encoder is its only child
    (`state_dict` keys gain the prefix `encoder.`: wrap after the weights are loaded)."""

    def __init__(self, encoder, convs=False):
        torch.nn.Module.__init__(self)
        PackedWeights.__init__(self)
        self.convs = bool(convs)
        for name in ("conv1", "norm1"):
            if not hasattr(encoder, name):
                raise TypeError(f"FusedEncoder: the encoder has no {name!r}")
        self.multi = hasattr(encoder, "outputs08")
        if self.multi:
            for name in ("outputs16", "outputs32"):
                if not hasattr(encoder, name):
                    raise TypeError(f"FusedEncoder: the encoder has no {name!r}")
        elif not hasattr(encoder, "conv2"):
            raise TypeError("FusedEncoder: the encoder has neither 'conv2' nor 'outputs08'")
        _check_norm(encoder.norm1, "norm1")
        for where, blk in _blocks_of(encoder):
            for name in ("conv1", "conv2", "norm1", "norm2", "downsample"):
                if not hasattr(blk, name):
                    raise TypeError(f"FusedEncoder: {where} has no {name!r}")
            _check_norm(blk.norm1, f"{where}.norm1"), _check_norm(blk.norm2, f"{where}.norm2")
            if blk.downsample is not None:
                _check_norm(blk.downsample[1], f"{where}.downsample.1")
        if getattr(encoder, "dropout", None) is not None and encoder.training:
            raise TypeError("FusedEncoder: the encoder has dropout and is in training mode; call .eval() first (inference only)")
        self.encoder = encoder
        self._consts = {}                  # id(norm) -> (what it was built from, (stats, weight, bias))

    def __getattr__(self, name):           # conv1, layer1, norm_fn, ...: the encoder's own
        try:
            return super().__getattr__(name)
        except AttributeError:
            enc = self.__dict__.get("_modules", {}).get("encoder")
            if enc is None:
                raise
            return getattr(enc, name)

    # ---- one norm ----
    def _norm_consts(self, m, device):
        """(stats or None, weight, bias) of a norm as float32 tensors on `device`: the affine parameters, and for a frozen
        BatchNorm its [C,2] (running_mean, 1 / sqrt(running_var + eps)), the square root taken in float64.  Built once,
        and again when a buffer or parameter of the module has changed or moved."""
        src = [t for t in (getattr(m, "running_mean", None), getattr(m, "running_var", None), m.weight, m.bias) if t is not None]
        key = (device, m.eps) + tuple((t.data_ptr(), t._version) for t in src)
        hit = self._consts.get(id(m))
        if hit is not None and hit[0] == key:
            return hit[1]
        f32 = lambda t: None if t is None else t.detach().to(device=device, dtype=torch.float32).contiguous()  # noqa: E731
        stats = None
        if isinstance(m, torch.nn.BatchNorm2d):
            rstd = 1.0 / torch.sqrt(m.running_var.detach().double() + float(m.eps))
            stats = torch.stack([m.running_mean.detach().double(), rstd], dim=1).to(device=device, dtype=torch.float32).contiguous()
        out = (stats, f32(m.weight), f32(m.bias))
        self._consts[id(m)] = (key, out)
        return out

    def _stats(self, eng, m, x):
        if isinstance(m, torch.nn.BatchNorm2d) and m.training:
            raise RuntimeError("FusedEncoder: a BatchNorm2d went back to training mode; the wrapper is inference only")
        stats, w, b = self._norm_consts(m, x.device)
        if stats is None:
            stats = eng.raft_norm_stats(x, eps=m.eps)
        return stats, w, b

    def _norm_relu(self, eng, m, x):
        """relu(norm(x)), in place over x (a convolution's output)."""
        stats, w, b = self._stats(eng, m, x)
        return eng.raft_norm_apply(x, stats, w, b, relu=True, out=x)

    @staticmethod
    def _conv_plain(conv, cin):
        """Whether Engine.raft_conv takes this module on `cin` input channels: FusedUpdate's rule, with stride (2, 2) as well."""
        return conv_plain(conv, cin, strides=((1, 1), (2, 2)))

    def _conv(self, conv, x, dtype):
        """conv(x) in the working dtype (None: whatever the convolution returns).  convs=True: one launch of Engine.raft_conv in
        the dtype of x where the kernel takes the module."""
        if self.convs and x.dtype in (torch.float32, torch.bfloat16) and self._conv_plain(conv, x.shape[1]):
            eng = _engine(x.device)
            x = _as(x, x.dtype)
            y = eng.raft_conv(x, self._packed_conv(eng, conv, x.dtype, x.device), conv.out_channels, conv.kernel_size[0],
                              stride=conv.stride[0])
            return _as(y, dtype or y.dtype)
        y = conv(x)
        if y.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"FusedEncoder: a convolution returned {y.dtype}; the kernels store float32 and bfloat16")
        return _as(y, dtype or y.dtype)

    def _block(self, eng, blk, x):
        """ResidualBlock.forward (extractor.py:48-60) in three launches (four with the downsample path's statistics)."""
        dtype = x.dtype
        y = self._norm_relu(eng, blk.norm1, self._conv(blk.conv1, x, dtype))
        y = self._conv(blk.conv2, y, dtype)
        stats, w, b = self._stats(eng, blk.norm2, y)
        if blk.downsample is None:
            return eng.raft_norm_apply(y, stats, w, b, relu=True, residual=x, out=y)
        r = self._conv(blk.downsample[0], x, dtype)
        rstats, rw, rb = self._stats(eng, blk.downsample[1], r)
        return eng.raft_norm_apply(y, stats, w, b, relu=True, residual=r, residual_stats=rstats, residual_weight=rw, residual_bias=rb,
                                   out=y)

    def _layer(self, eng, layer, x):
        for blk in layer:
            x = self._block(eng, blk, x)
        return x

    @torch.no_grad()
    def forward(self, x, dual_inp=False, num_layers=3):
        enc = self.encoder
        is_list = isinstance(x, (tuple, list))
        if is_list and not self.multi:     # BasicEncoder: if input is list, combine batch dimension (extractor.py:176-179)
            batch_dim = x[0].shape[0]
            x = torch.cat(x, dim=0)
        eng = _engine(x.device)
        x = self._norm_relu(eng, enc.norm1, self._conv(enc.conv1, x, None))
        x = self._layer(eng, enc.layer1, x)
        x = self._layer(eng, enc.layer2, x)
        x = self._layer(eng, enc.layer3, x)
        if not self.multi:
            x = self._conv(enc.conv2, x, None) if self.convs else enc.conv2(x)
            if is_list:
                x = x.split(split_size=batch_dim, dim=0)
            return x
        if dual_inp:
            v = x
            x = x[:(x.shape[0] // 2)]
        head = (lambda conv, t: self._conv(conv, t, None)) if self.convs else (lambda conv, t: conv(t))     # noqa: E731
        outputs08 = [head(f[1], self._block(eng, f[0], x)) for f in enc.outputs08]
        if num_layers == 1:
            return (outputs08, v) if dual_inp else (outputs08,)
        y = self._layer(eng, enc.layer4, x)
        outputs16 = [head(f[1], self._block(eng, f[0], y)) for f in enc.outputs16]
        if num_layers == 2:
            return (outputs08, outputs16, v) if dual_inp else (outputs08, outputs16)
        z = self._layer(eng, enc.layer5, y)
        outputs32 = [head(f, z) for f in enc.outputs32]
        return (outputs08, outputs16, outputs32, v) if dual_inp else (outputs08, outputs16, outputs32)
