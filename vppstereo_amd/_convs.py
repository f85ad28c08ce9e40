"""What FusedUpdate (update.py), FusedEncoder (extractor.py), FusedFeatureExtraction and FusedRegularization (psmnet.py) share around
`Engine.raft_conv` / `Engine.conv2d` / `Engine.conv3d`: the decision whether the kernel takes a convolution, the fold of a frozen
BatchNorm into a convolution's weights, and the one cache of packed weights.
"""
import weakref

import torch


def conv_plain(conv, cin, strides=((1, 1),), dilations=((1, 1),)):
    """Whether Engine.raft_conv (Engine.conv2d, with `dilations`) takes this module on `cin` input channels: an nn.Conv2d whose
    forward is nn.Conv2d's, 1x1 or 3x3, a stride of `strides`, a dilation d of `dilations` (dilation 1 unless the caller names
    others; (2, 2) goes with stride (1, 1) only), groups 1, zeros outside the map, padding d * (k // 2), within the channel
    counts that are built."""
    from . import _lib
    if not isinstance(conv, torch.nn.Conv2d) or type(conv).forward is not torch.nn.Conv2d.forward:
        return False
    k, d = conv.kernel_size[0], tuple(conv.dilation)
    return (tuple(conv.kernel_size) in ((1, 1), (3, 3)) and tuple(conv.weight.shape) == (conv.out_channels, cin, k, k)
            and d in dilations and d in ((1, 1), (2, 2)) and conv.padding == (d[0] * (k // 2), d[0] * (k // 2))
            and tuple(conv.stride) in strides and (d == (1, 1) or tuple(conv.stride) == (1, 1)) and conv.groups == 1
            and conv.padding_mode == "zeros" and cin % 16 == 0 and 0 < cin <= _lib.CONV_MAX_CIN
            and 0 < conv.out_channels <= _lib.CONV_MAX_COUT)


def frozen_bn(bn, what):
    """Raise the TypeError of a wrapper for a norm that cannot be folded: anything but a BatchNorm2d in eval mode with running
    statistics."""
    if not isinstance(bn, torch.nn.BatchNorm2d):
        raise TypeError(f"{what} is {type(bn).__name__}, not a BatchNorm2d")
    if bn.training:
        raise TypeError(f"{what} is in training mode; only a frozen BatchNorm2d (model.eval()) folds into its convolution")
    if bn.running_mean is None or bn.running_var is None:
        raise TypeError(f"{what} keeps no running statistics (track_running_stats=False): there is nothing to fold")


def fold_bn(conv, bn):
    """(weight [Cout,Cin,k,k], bias [Cout]) float32 of the convolution that equals bn(conv(x)) for a BatchNorm2d in eval mode,
    computed in float64 and rounded to float32 once each:
        s = gamma / sqrt(running_var + eps);   w' = w * s[m];   b' = beta + (conv_bias - running_mean) * s
    (gamma 1 and beta 0 for a norm without affine parameters)."""
    frozen_bn(bn, "the norm")
    f64 = lambda t: t.detach().double()                                                  # noqa: E731
    s = 1.0 / torch.sqrt(f64(bn.running_var) + float(bn.eps))
    if bn.weight is not None:
        s = f64(bn.weight) * s
    shift = -f64(bn.running_mean) if conv.bias is None else f64(conv.bias) - f64(bn.running_mean)
    b = shift * s
    if bn.bias is not None:
        b = f64(bn.bias) + b
    w = f64(conv.weight) * s[:, None, None, None]
    return w.to(torch.float32).contiguous(), b.to(torch.float32).contiguous()


def conv3d_plain(conv, cin):
    """Whether Engine.conv3d takes this module on `cin` input channels: an nn.Conv3d whose forward is nn.Conv3d's, kernel
    (3, 3, 3), stride 1, padding 1, dilation 1, groups 1, zeros outside the volume, `cin` a multiple of 16 with 3 * cin within the
    input channels that are built, and an output channel count that is built.  A stride of 2 and a ConvTranspose3d are not."""
    from . import _lib
    if not isinstance(conv, torch.nn.Conv3d) or type(conv).forward is not torch.nn.Conv3d.forward:
        return False
    return (tuple(conv.kernel_size) == (3, 3, 3) and tuple(conv.weight.shape) == (conv.out_channels, cin, 3, 3, 3)
            and tuple(conv.stride) == (1, 1, 1) and conv.padding == (1, 1, 1) and tuple(conv.dilation) == (1, 1, 1) and conv.groups == 1
            and conv.padding_mode == "zeros" and cin % 16 == 0 and 0 < 3 * cin <= _lib.CONV_MAX_CIN
            and 0 < conv.out_channels <= _lib.CONV_MAX_COUT)


def frozen_bn3d(bn, what):
    """frozen_bn for a BatchNorm3d: the TypeError of a wrapper for anything but a BatchNorm3d in eval mode with running statistics."""
    if not isinstance(bn, torch.nn.BatchNorm3d):
        raise TypeError(f"{what} is {type(bn).__name__}, not a BatchNorm3d")
    if bn.training:
        raise TypeError(f"{what} is in training mode; only a frozen BatchNorm3d (model.eval()) folds into its convolution")
    if bn.running_mean is None or bn.running_var is None:
        raise TypeError(f"{what} keeps no running statistics (track_running_stats=False): there is nothing to fold")


def fold_bn3d(conv, bn):
    """fold_bn for a Conv3d and a BatchNorm3d in eval mode: (weight [Cout,Cin,3,3,3], bias [Cout]) float32 of the convolution that
    equals bn(conv(x)), computed in float64 and rounded to float32 once each:
        s = gamma / sqrt(running_var + eps);   w' = w * s[m];   b' = beta + (conv_bias - running_mean) * s"""
    frozen_bn3d(bn, "the norm")
    f64 = lambda t: t.detach().double()                                                  # noqa: E731
    s = 1.0 / torch.sqrt(f64(bn.running_var) + float(bn.eps))
    if bn.weight is not None:
        s = f64(bn.weight) * s
    shift = -f64(bn.running_mean) if conv.bias is None else f64(conv.bias) - f64(bn.running_mean)
    b = shift * s
    if bn.bias is not None:
        b = f64(bn.bias) + b
    w = f64(conv.weight) * s[:, None, None, None, None]
    return w.to(torch.float32).contiguous(), b.to(torch.float32).contiguous()


class PackedWeights:
    """The packed weights of the modules a wrapper runs on the convolution kernel, kept per module: GruGlue's GRUs and both
    wrappers' single convolutions."""

    def __init__(self):
        self._packed = {}                  # the GRU's id -> (what they were made from, packed convz + convr, packed convq,
        #                                    a weak reference to the GRU, the parameter objects); a single convolution's id
        #                                    (convs=True) -> the same with its packed weights and None

    def _packed_conv(self, eng, conv, dtype, device):
        """The packed weights of one plain convolution (convs=True): the GRUs' rule, the convolution in the GRU's place.  A
        buffer serves either stride."""
        make = lambda: (eng.raft_conv_pack(conv.weight, conv.bias, dtype=dtype), None)      # noqa: E731
        return self._packed_for(conv, [conv.weight, conv.bias], make, dtype, device)[0]

    def _packed_conv_bn(self, eng, conv, bn, dtype, device):
        """The packed weights of `conv` with the frozen BatchNorm2d `bn` behind it folded in (fold_bn), kept under the
        convolution: the conv cache rule over the convolution's two parameters and the norm's four tensors and eps, which is
        what FusedEncoder._norm_consts looks at.  For bfloat16 the packing rounds the folded weights once more, as always."""
        if bn.training:
            raise RuntimeError("a BatchNorm2d went back to training mode; the wrapper is inference only")
        make = lambda: (eng.raft_conv_pack(*fold_bn(conv, bn), dtype=dtype), None)          # noqa: E731
        params = [conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var]
        return self._packed_for(conv, params, make, (dtype, float(bn.eps), id(bn)), device)[0]

    def _packed_conv3d(self, eng, conv, dtype, device):
        """_packed_conv for a Conv3d that conv3d_plain accepts (Engine.conv3d_pack)."""
        make = lambda: (eng.conv3d_pack(conv.weight, conv.bias, dtype=dtype), None)         # noqa: E731
        return self._packed_for(conv, [conv.weight, conv.bias], make, dtype, device)[0]

    def _packed_conv3d_bn(self, eng, conv, bn, dtype, device):
        """_packed_conv_bn for a Conv3d with the frozen BatchNorm3d `bn` behind it (fold_bn3d), under the same cache rule."""
        if bn.training:
            raise RuntimeError("a BatchNorm3d went back to training mode; the wrapper is inference only")
        make = lambda: (eng.conv3d_pack(*fold_bn3d(conv, bn), dtype=dtype), None)           # noqa: E731
        params = [conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var]
        return self._packed_for(conv, params, make, (dtype, float(bn.eps), id(bn)), device)[0]

    def _packed_for(self, owner, params, make, dtype, device):
        """The pair make() returns, kept under id(owner) while the device, the dtype and every parameter of `params` stay what they
        were; the rule is GruGlue._packed_weights'."""
        stamp = (device, dtype, tuple(None if p is None else (id(p), p.data_ptr(), p._version) for p in params))
        key = id(owner)
        kept = self._packed.get(key)
        if kept is not None and kept[3] is not None and kept[3]() is not owner:    # the entry of a module that is gone
            kept = None
        if kept is None or kept[0] != stamp:
            store = self._packed

            def gone(ref, key=key, store=store):     # the module was freed: its packed weights go with it
                hit = store.get(key)
                if hit is not None and hit[3] is ref:
                    del store[key]

            try:
                ref = weakref.ref(owner, gone)
            except TypeError:                        # an object that takes no weak reference: the held parameters still pin the ids
                ref = None
            first, second = make()
            kept = store[key] = (stamp, first, second, ref, tuple(params))
        return kept[1], kept[2]

    def forget_weights(self):
        """Drop every packed weight, the GRUs' and the single convolutions': the next call with conv=True or convs=True packs again.  For the one change _packed_weights cannot see,
        a write through `p.data` (`p.data.copy_(new)`, `p.data.mul_(2)`)."""
        self._packed.clear()
