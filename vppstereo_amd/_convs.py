"""What FusedUpdate (update.py) and FusedEncoder (extractor.py) share around `Engine.raft_conv`: the decision whether the
kernel takes a convolution, and the one cache of packed weights.
"""
import weakref

import torch


def conv_plain(conv, cin, strides=((1, 1),)):
    """Whether Engine.raft_conv takes this module on `cin` input channels: an nn.Conv2d whose forward is nn.Conv2d's, 1x1 or
    3x3, a stride of `strides`, dilation 1, groups 1, zeros outside the map, padding k // 2, within the channel counts that
    are built."""
    from . import _lib
    if not isinstance(conv, torch.nn.Conv2d) or type(conv).forward is not torch.nn.Conv2d.forward:
        return False
    k = conv.kernel_size[0]
    return (tuple(conv.kernel_size) in ((1, 1), (3, 3)) and tuple(conv.weight.shape) == (conv.out_channels, cin, k, k)
            and conv.padding == (k // 2, k // 2) and tuple(conv.stride) in strides and conv.dilation == (1, 1) and conv.groups == 1
            and conv.padding_mode == "zeros" and cin % 16 == 0 and 0 < cin <= _lib.CONV_MAX_CIN
            and 0 < conv.out_channels <= _lib.CONV_MAX_COUT)


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
