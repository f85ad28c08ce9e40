"""PSMNet's feature_extraction and 3-D regularization on the library's kernels (INTEGRATION.md has the patch): FusedFeatureExtraction,
and FusedRegularization further down.

`FusedFeatureExtraction(fe, dtype=None)` wraps a loaded `feature_extraction` (models/psmnet/submodule.py:131-253): any module
with `firstconv`, `layer1` .. `layer4`, `branch1` .. `branch4` and `lastconv` of the reference's structure -- convbn groups
`Sequential(Conv2d, BatchNorm2d)`, BasicBlocks with `conv1` = `Sequential(convbn, ReLU)`, `conv2` = convbn and `downsample` =
None or a convbn, branches `Sequential(AvgPool2d, convbn, ReLU)`, and `lastconv` = `Sequential(convbn, ReLU, Conv2d)`.  It holds
the module, so the weights and the `state_dict` are untouched, and runs its forward as:

  * the stem: `firstconv[0]` (3 input channels) with its BatchNorm and ReLU in torch; the result is converted to `dtype`
    (torch.float32 or torch.bfloat16; None keeps what the stem returns, bfloat16 under autocast);
  * every other convolution the kernel takes (`conv_plain` of _convs.py with dilation (2, 2) as well) as one launch of
    `Engine.conv2d` with its frozen BatchNorm folded into the weights (`fold_bn`), its ReLU and, for a block's second
    convolution, the residual in the epilogue: a BasicBlock is 2 launches, 3 with a `downsample`, whose launch runs first and
    whose output is the residual.  A convolution the kernel does not take runs in torch with its BatchNorm, decided per
    convolution;
  * the 320-channel tensor without a `cat` and without a copy: the last block of `layer2` stores `output_raw` into the first
    channels of one [B,320,H4,W4] buffer (`layer3` reads it there through its frame stride), the last block of `layer4`
    stores `output_skip` behind it, one `Engine.psm_spp_pool` makes the four pooled maps, four folded 1x1 convolutions with ReLU
    run on them, and one `Engine.raft_gru_assemble` interpolates the four into the last channels in the reference's order
    branch4, branch3, branch2, branch1; `lastconv` reads the buffer as one source.

-> [B,32,H4,W4] in `dtype`, ready for `Engine.psmnet_cost_volume`.  For the reference's module that is `launches()` = 62
launches per call.  Inference only, under `torch.no_grad()`; a BatchNorm in training mode or without running statistics is a
TypeError when wrapping.  The packed weights follow `PackedWeights`' cache rule over the convolution's and the norm's tensors
(`forget_weights()` included).  It is opt-in: README.md has what was measured.
"""
import torch

from ._convs import PackedWeights, conv3d_plain, conv_plain, frozen_bn, frozen_bn3d
from .corr import _engine
from .update import _as

_WHO = "FusedFeatureExtraction"
_STRIDES, _DILATIONS = ((1, 1), (2, 2)), ((1, 1), (2, 2))


def _check_convbn(pair, where):
    """A convbn group: Sequential(Conv2d, BatchNorm2d in eval mode with running statistics)."""
    if not isinstance(pair, torch.nn.Sequential) or len(pair) != 2:
        raise TypeError(f"{_WHO}: {where} is not a Sequential(Conv2d, BatchNorm2d)")
    if not isinstance(pair[0], torch.nn.Conv2d):
        raise TypeError(f"{_WHO}: {where}[0] is {type(pair[0]).__name__}, not a Conv2d")
    frozen_bn(pair[1], f"{_WHO}: {where}[1]")
    if pair[1].num_features != pair[0].out_channels:
        raise TypeError(f"{_WHO}: {where}[1] normalises {pair[1].num_features} channels, {where}[0] makes {pair[0].out_channels}")


def _check_relu(m, where):
    if not isinstance(m, torch.nn.ReLU):
        raise TypeError(f"{_WHO}: {where} is {type(m).__name__}, not a ReLU")


def _check_seq(m, n, where):
    if not isinstance(m, torch.nn.Sequential) or len(m) != n:
        raise TypeError(f"{_WHO}: {where} is not a Sequential of {n}")


class FusedFeatureExtraction(torch.nn.Module, PackedWeights):
    """A module, so that it can take the place of `feature_extraction` in a PSMNet; the wrapped module is its only child
    (`state_dict` keys gain the prefix `fe.`: wrap after the weights are loaded)."""

    def __init__(self, fe, dtype=None):
        torch.nn.Module.__init__(self)
        PackedWeights.__init__(self)
        if dtype not in (None, torch.float32, torch.bfloat16):
            raise TypeError(f"{_WHO}: dtype is {dtype}; the kernels store float32 and bfloat16")
        for name in ("firstconv", "layer1", "layer2", "layer3", "layer4", "branch1", "branch2", "branch3", "branch4", "lastconv"):
            if not hasattr(fe, name):
                raise TypeError(f"{_WHO}: the module has no {name!r}")
        _check_seq(fe.firstconv, 6, "firstconv")
        for k in (0, 2, 4):
            _check_convbn(fe.firstconv[k], f"firstconv[{k}]"), _check_relu(fe.firstconv[k + 1], f"firstconv[{k + 1}]")
        for name in ("layer1", "layer2", "layer3", "layer4"):
            layer = getattr(fe, name)
            if not isinstance(layer, torch.nn.Sequential) or len(layer) < 1:
                raise TypeError(f"{_WHO}: {name} is not a Sequential of blocks")
            for k, blk in enumerate(layer):
                where = f"{name}[{k}]"
                for part in ("conv1", "conv2", "downsample"):
                    if not hasattr(blk, part):
                        raise TypeError(f"{_WHO}: {where} has no {part!r}")
                _check_seq(blk.conv1, 2, f"{where}.conv1")
                _check_convbn(blk.conv1[0], f"{where}.conv1[0]"), _check_relu(blk.conv1[1], f"{where}.conv1[1]")
                _check_convbn(blk.conv2, f"{where}.conv2")
                if blk.downsample is not None:
                    _check_convbn(blk.downsample, f"{where}.downsample")
        for name in ("branch1", "branch2", "branch3", "branch4"):
            br = getattr(fe, name)
            _check_seq(br, 3, name)
            pool = br[0]
            if not isinstance(pool, torch.nn.AvgPool2d):
                raise TypeError(f"{_WHO}: {name}[0] is {type(pool).__name__}, not an AvgPool2d")
            ks, st = torch.nn.modules.utils._pair(pool.kernel_size), torch.nn.modules.utils._pair(pool.stride)
            if ks[0] != ks[1] or st != ks or torch.nn.modules.utils._pair(pool.padding) != (0, 0) or pool.ceil_mode or pool.divisor_override:
                raise TypeError(f"{_WHO}: {name}[0] is not an AvgPool2d((k, k), stride=(k, k)) without padding")
            _check_convbn(br[1], f"{name}[1]"), _check_relu(br[2], f"{name}[2]")
            if br[1][0].kernel_size != (1, 1) or br[1][0].stride != (1, 1):
                raise TypeError(f"{_WHO}: {name}[1][0] is not a 1x1 convolution at stride 1")
        _check_seq(fe.lastconv, 3, "lastconv")
        _check_convbn(fe.lastconv[0], "lastconv[0]"), _check_relu(fe.lastconv[1], "lastconv[1]")
        if not isinstance(fe.lastconv[2], torch.nn.Conv2d):
            raise TypeError(f"{_WHO}: lastconv[2] is {type(fe.lastconv[2]).__name__}, not a Conv2d")
        self._channels = (fe.layer2[-1].conv2[0].out_channels, fe.layer4[-1].conv2[0].out_channels,
                          tuple(getattr(fe, f"branch{k}")[1][0].out_channels for k in (4, 3, 2, 1)))
        total = self._channels[0] + self._channels[1] + sum(self._channels[2])
        if fe.lastconv[0][0].in_channels != total:
            raise TypeError(f"{_WHO}: lastconv[0][0] takes {fe.lastconv[0][0].in_channels} channels, layer2, layer4 and the branches make {total}")
        self.fe = fe
        self.dtype = dtype

    def launches(self):
        """Engine launches of one forward where the kernel takes every convolution behind the stem."""
        fe = self.fe
        blocks = sum(2 + (blk.downsample is not None) for name in ("layer1", "layer2", "layer3", "layer4") for blk in getattr(fe, name))
        return 2 + blocks + 1 + 4 + 1 + 2

    # ---- one convolution ----
    def _convbn(self, eng, pair, x, relu=False, residual=None, out=None):
        """[relu](bn(conv(x)) [+ residual]), into `out` where there is one: one launch with the norm folded, or torch."""
        conv, bn = pair[0], pair[1]
        if conv_plain(conv, x.shape[1], strides=_STRIDES, dilations=_DILATIONS):
            packed = self._packed_conv_bn(eng, conv, bn, x.dtype, x.device)
            return eng.conv2d(x, packed, conv.out_channels, conv.kernel_size[0], stride=conv.stride[0], dilation=conv.dilation[0],
                              residual=residual, relu=relu, out=out)
        if bn.training:
            raise RuntimeError(f"{_WHO}: a BatchNorm2d went back to training mode; the wrapper is inference only")
        y = bn.to(x.dtype)(conv.to(x.dtype)(x)) if conv.weight.dtype != x.dtype else bn(conv(x))
        return self._finish(y, x.dtype, relu, residual, out)

    @staticmethod
    def _finish(y, dtype, relu, residual, out):
        y = _as(y, dtype)
        if residual is not None:
            y = y + residual
        if relu:
            y = torch.relu_(y)
        if out is not None:
            out.copy_(y)
            return out
        return y

    def _conv(self, eng, conv, x):
        """A convolution without a norm behind it (lastconv[2])."""
        if conv_plain(conv, x.shape[1], strides=_STRIDES, dilations=_DILATIONS):
            return eng.conv2d(x, self._packed_conv(eng, conv, x.dtype, x.device), conv.out_channels, conv.kernel_size[0], stride=conv.stride[0],
                              dilation=conv.dilation[0])
        return _as(conv(x.to(conv.weight.dtype)), x.dtype)

    def _block(self, eng, blk, x, out=None):
        """BasicBlock.forward (submodule.py:75-84): out = conv2(conv1(x)); out += downsample(x) or x -- no ReLU behind the sum."""
        res = x if blk.downsample is None else self._convbn(eng, blk.downsample, x)
        h = self._convbn(eng, blk.conv1[0], x, relu=True)
        return self._convbn(eng, blk.conv2, h, residual=res, out=out)

    def _layer(self, eng, layer, x, last_out=None):
        """Every block of a layer; last_out(shape of the last block's input, that block) -> the buffer its output goes into."""
        for k, blk in enumerate(layer):
            out = last_out(x, blk) if last_out is not None and k == len(layer) - 1 else None
            x = self._block(eng, blk, x, out)
        return x

    def forward(self, x):
        with torch.no_grad():
            return self._forward(x)

    def _forward(self, x):
        fe = self.fe
        stem = fe.firstconv[0]
        if stem[1].training:
            raise RuntimeError(f"{_WHO}: a BatchNorm2d went back to training mode; the wrapper is inference only")
        x = torch.relu_(stem[1](stem[0](x)))
        dtype = x.dtype if self.dtype is None else self.dtype
        if dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"{_WHO}: the stem returns {dtype}; the kernels store float32 and bfloat16 (pass dtype=)")
        x = _as(x, dtype)
        eng = _engine(x.device)
        x = self._convbn(eng, fe.firstconv[2], x, relu=True)
        x = self._convbn(eng, fe.firstconv[4], x, relu=True)
        x = self._layer(eng, fe.layer1, x)
        c_raw, c_skip, c_br = self._channels
        feat = []

        def raw_slot(xin, blk):
            s = blk.conv1[0][0].stride
            B, _, H, W = xin.shape
            feat.append(torch.empty((B, c_raw + c_skip + sum(c_br), (H - 1) // s[0] + 1, (W - 1) // s[1] + 1), dtype=dtype, device=xin.device))
            return feat[0][:, :c_raw]

        raw = self._layer(eng, fe.layer2, x, raw_slot)
        buf = feat[0]
        x = self._layer(eng, fe.layer3, raw)
        self._layer(eng, fe.layer4, x, lambda xin, blk: buf[:, c_raw:c_raw + c_skip])
        x = self._convbn(eng, fe.lastconv[0], self._tail(eng, buf), relu=True)
        return self._conv(eng, fe.lastconv[2], x)

    def _tail(self, eng, buf):
        """The pyramid pooling (submodule.py:208-250) over a feature buffer that holds output_raw and output_skip: the four
        branches into its last channels, in the order branch4, branch3, branch2, branch1.  -> buf."""
        c_raw, c_skip, _ = self._channels
        branches = [getattr(self.fe, f"branch{k}") for k in (4, 3, 2, 1)]
        ks = [torch.nn.modules.utils._pair(br[0].kernel_size)[0] for br in branches]
        pooled = eng.psm_spp_pool(buf[:, c_raw:c_raw + c_skip], ks)
        small = [(self._convbn(eng, br[1], p, relu=True), "interp") for br, p in zip(branches, pooled)]
        eng.raft_gru_assemble(small, out=buf[:, c_raw + c_skip:])
        return buf


# ---------------------------------------------------------------------------------------------------
# the 3-D regularization: dres0 .. dres4 and classif1 .. classif3 (models/psmnet/psmnet.py:93-128, 199-213)
# ---------------------------------------------------------------------------------------------------
_WHO3 = "FusedRegularization"


def _autocast_bf16():
    """Whether torch would run a convolution on the device in bfloat16 here."""
    if hasattr(torch, "get_autocast_dtype"):
        return torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16
    return torch.is_autocast_enabled() and torch.get_autocast_gpu_dtype() == torch.bfloat16


def _check_convbn3d(pair, where, conv_type=torch.nn.Conv3d):
    """A convbn_3d group: Sequential(Conv3d, BatchNorm3d in eval mode with running statistics); conv5 and conv6 of an hourglass
    have a ConvTranspose3d in the convolution's place."""
    name = conv_type.__name__
    if not isinstance(pair, torch.nn.Sequential) or len(pair) != 2:
        raise TypeError(f"{_WHO3}: {where} is not a Sequential({name}, BatchNorm3d)")
    if not isinstance(pair[0], conv_type):
        raise TypeError(f"{_WHO3}: {where}[0] is {type(pair[0]).__name__}, not a {name}")
    frozen_bn3d(pair[1], f"{_WHO3}: {where}[1]")
    if pair[1].num_features != pair[0].out_channels:
        raise TypeError(f"{_WHO3}: {where}[1] normalises {pair[1].num_features} channels, {where}[0] makes {pair[0].out_channels}")


def _check_seq3(m, kinds, where):
    """A Sequential whose members are, in order, "convbn" groups, "relu"s and "conv"s (a Conv3d without a norm)."""
    if not isinstance(m, torch.nn.Sequential) or len(m) != len(kinds):
        raise TypeError(f"{_WHO3}: {where} is not a Sequential of {len(kinds)}")
    for k, kind in enumerate(kinds):
        if kind == "convbn":
            _check_convbn3d(m[k], f"{where}[{k}]")
        elif kind == "relu":
            if not isinstance(m[k], torch.nn.ReLU):
                raise TypeError(f"{_WHO3}: {where}[{k}] is {type(m[k]).__name__}, not a ReLU")
        elif not isinstance(m[k], torch.nn.Conv3d):
            raise TypeError(f"{_WHO3}: {where}[{k}] is {type(m[k]).__name__}, not a Conv3d")


class FusedRegularization(torch.nn.Module, PackedWeights):
    """PSMNet's 3-D regularization with its stride-1 convolutions on the convolution kernel (INTEGRATION.md has the composition).

    `FusedRegularization(model, dtype=None)` wraps a loaded PSMNet, or any module with `dres0` .. `dres4` and `classif1` ..
    `classif3` of the reference's structure (models/psmnet/psmnet.py:15-128): `dres0` = Sequential(convbn_3d, ReLU, convbn_3d,
    ReLU), `dres1` = Sequential(convbn_3d, ReLU, convbn_3d), three hourglasses with `conv1`, `conv3`, `conv4` =
    Sequential(convbn_3d, ReLU), `conv2` = convbn_3d and `conv5`, `conv6` = Sequential(ConvTranspose3d, BatchNorm3d), and
    classifiers Sequential(convbn_3d, ReLU, Conv3d).  It holds the module, so the weights and the `state_dict` are untouched.

    `forward(cost) -> cost3` [B,1,D,H,W], which `Engine.psmnet_disparity` takes, follows psmnet.py:199-213 and
    `hourglass.forward` line for line.  Every convolution `conv3d_plain` of _convs.py accepts is one launch of `Engine.conv3d`
    with its frozen BatchNorm3d folded (`fold_bn3d`), its ReLU and the sum that follows it directly in the epilogue:
    `dres1(cost0) + cost0`, the hourglass's `relu(conv2(out) + postsqu)`, `classif2(out2) + cost1`, `classif3(out3) + cost2`.
    Out of scope, and run in torch in the volume's dtype, decided per convolution: the hourglasses' two Conv3d at stride 2 and
    two ConvTranspose3d with the sums behind them (`relu(conv5 + presqu)`, `out + cost0`), and any convolution `conv3d_plain`
    refuses.  For the reference's module that is `launches()` = 16 launches per call.  `dtype`: torch.float32 or
    torch.bfloat16; None keeps the volume's (bfloat16 under autocast).  Inference only, under `torch.no_grad()`; a BatchNorm3d in
    training mode is a TypeError when wrapping.  The packed weights follow `PackedWeights`' cache rule.  Opt-in: README.md has
    what was measured."""

    def __init__(self, model, dtype=None):
        torch.nn.Module.__init__(self)
        PackedWeights.__init__(self)
        if dtype not in (None, torch.float32, torch.bfloat16):
            raise TypeError(f"{_WHO3}: dtype is {dtype}; the kernels store float32 and bfloat16")
        for name in ("dres0", "dres1", "dres2", "dres3", "dres4", "classif1", "classif2", "classif3"):
            if not hasattr(model, name):
                raise TypeError(f"{_WHO3}: the module has no {name!r}")
        _check_seq3(model.dres0, ("convbn", "relu", "convbn", "relu"), "dres0")
        _check_seq3(model.dres1, ("convbn", "relu", "convbn"), "dres1")
        for name in ("dres2", "dres3", "dres4"):
            hg = getattr(model, name)
            for part in ("conv1", "conv2", "conv3", "conv4", "conv5", "conv6"):
                if not hasattr(hg, part):
                    raise TypeError(f"{_WHO3}: {name} has no {part!r}")
            for part in ("conv1", "conv3", "conv4"):
                _check_seq3(getattr(hg, part), ("convbn", "relu"), f"{name}.{part}")
            _check_convbn3d(hg.conv2, f"{name}.conv2")
            _check_convbn3d(hg.conv5, f"{name}.conv5", torch.nn.ConvTranspose3d)
            _check_convbn3d(hg.conv6, f"{name}.conv6", torch.nn.ConvTranspose3d)
        for name in ("classif1", "classif2", "classif3"):
            _check_seq3(getattr(model, name), ("convbn", "relu", "conv"), name)
        self.model = model
        self.dtype = dtype

    def _plan(self):
        """(convolution, its input channels) of everything forward() hands to _convbn / _conv, in its order."""
        m = self.model
        chain = lambda pairs, cin: [(p[0], c) for p, c in zip(pairs, [cin] + [p[0].out_channels for p in pairs[:-1]])]   # noqa: E731
        plan = chain([m.dres0[0], m.dres0[2], m.dres1[0], m.dres1[2]], m.dres0[0][0].in_channels)
        for hg in (m.dres2, m.dres3, m.dres4):
            plan += chain([hg.conv1[0], hg.conv2, hg.conv3[0], hg.conv4[0]], hg.conv1[0][0].in_channels)
        for cl in (m.classif1, m.classif2, m.classif3):
            plan += [(cl[0][0], cl[0][0].in_channels), (cl[2], cl[0][0].out_channels)]
        return plan

    def launches(self):
        """Engine.conv3d launches of one forward: the convolutions conv3d_plain accepts."""
        return sum(1 for conv, cin in self._plan() if conv3d_plain(conv, cin))

    # ---- one convolution ----
    @staticmethod
    def _torch(m, x):
        """A module of the wrapped model on x, in x's dtype whatever the parameters' is."""
        wd = next(m.parameters()).dtype
        if wd == x.dtype:
            y = m(x)
        elif x.dtype == torch.bfloat16:
            with torch.autocast(x.device.type, dtype=torch.bfloat16):
                y = m(x)
        else:
            y = m(x.to(wd))
        return y.to(x.dtype).contiguous()

    def _convbn(self, eng, pair, x, relu=False, residual=None):
        """[relu](bn(conv(x)) [+ residual]): one launch with the norm folded, or torch."""
        conv, bn = pair[0], pair[1]
        if conv3d_plain(conv, x.shape[1]):
            return eng.conv3d(x, self._packed_conv3d_bn(eng, conv, bn, x.dtype, x.device), conv.out_channels, residual=residual, relu=relu)
        if bn.training:
            raise RuntimeError(f"{_WHO3}: a BatchNorm3d went back to training mode; the wrapper is inference only")
        y = self._torch(pair, x)
        if residual is not None:
            y = y + residual
        return torch.relu_(y) if relu else y

    def _conv(self, eng, conv, x, residual=None):
        """A convolution without a norm behind it (a classifier's last) [+ residual]."""
        if conv3d_plain(conv, x.shape[1]):
            return eng.conv3d(x, self._packed_conv3d(eng, conv, x.dtype, x.device), conv.out_channels, residual=residual)
        y = self._torch(conv, x)
        return y if residual is None else y + residual

    def _hourglass(self, eng, hg, x, presqu, postsqu):
        """hourglass.forward (psmnet.py:64-83)."""
        out = self._convbn(eng, hg.conv1[0], x, relu=True)                           # in:1/4 out:1/8 (stride 2: torch)
        pre = self._convbn(eng, hg.conv2, out, relu=True, residual=postsqu)         # relu(conv2(out) + postsqu), or relu(conv2(out))
        out = self._convbn(eng, hg.conv3[0], pre, relu=True)                         # in:1/8 out:1/16 (stride 2: torch)
        out = self._convbn(eng, hg.conv4[0], out, relu=True)
        if hg.conv5[1].training or hg.conv6[1].training:
            raise RuntimeError(f"{_WHO3}: a BatchNorm3d went back to training mode; the wrapper is inference only")
        post = torch.relu_(self._torch(hg.conv5, out) + (presqu if presqu is not None else pre))
        return self._torch(hg.conv6, post), pre, post

    def _classif(self, eng, cl, x, residual=None):
        return self._conv(eng, cl[2], self._convbn(eng, cl[0], x, relu=True), residual=residual)

    def forward(self, cost):
        with torch.no_grad():
            return self._forward(cost)

    def _forward(self, cost):
        m = self.model
        if cost.dim() != 5:
            raise ValueError(f"{_WHO3}: cost is {tuple(cost.shape)}; expected [B,C,D,H,W]")
        dtype = self.dtype
        if dtype is None:
            dtype = torch.bfloat16 if cost.is_cuda and _autocast_bf16() else cost.dtype
        if dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"{_WHO3}: the volume is {dtype}; the kernels store float32 and bfloat16 (pass dtype=)")
        cost = cost.to(dtype).contiguous()
        eng = _engine(cost.device)
        cost0 = self._convbn(eng, m.dres0[2], self._convbn(eng, m.dres0[0], cost, relu=True), relu=True)
        cost0 = self._convbn(eng, m.dres1[2], self._convbn(eng, m.dres1[0], cost0, relu=True), residual=cost0)

        out1, pre1, post1 = self._hourglass(eng, m.dres2, cost0, None, None)
        out1 = out1 + cost0

        out2, pre2, post2 = self._hourglass(eng, m.dres3, out1, pre1, post1)
        out2 = out2 + cost0

        out3, pre3, post3 = self._hourglass(eng, m.dres4, out2, pre1, post2)
        out3 = out3 + cost0

        cost1 = self._classif(eng, m.classif1, out1)
        cost2 = self._classif(eng, m.classif2, out2, residual=cost1)
        return self._classif(eng, m.classif3, out3, residual=cost2)
