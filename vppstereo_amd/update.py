"""RAFT-Stereo's update block with the work between its convolutions on the device (INTEGRATION.md has the patch).

`FusedUpdate(block)` wraps an existing `BasicMultiUpdateBlock` (models/raft_stereo/update.py:99-142): any module with
`encoder`, `gru08` / `gru16` / `gru32` (each with `convz`, `convr`, `convq`), `flow_head`, `mask` and `n_gru_layers`.  It
holds the block and calls its convolutions as they are, so the block's weights and its `state_dict` are untouched; what it replaces is
the glue of `forward` and of the three `ConvGRU.forward` calls (:23-32): per GRU one launch assembles
hx = cat([h, *x]) with pool2x (:89-90) and interp (:95-97) applied on the way, one launch writes r * h over the h part of
that buffer, which convq then reads as cat([r*h, x]), and one launch makes the new hidden state
(`Engine.raft_gru_assemble`, `raft_gru_reset`, `raft_gru_update`; include/vppx.h has the arithmetic).  The encoder's
`cat([out, flow])` (:87) becomes two sources of gru08's hx.  The convolutions, their ReLUs, `flow_head`, `mask` and the
`.25 *` stay torch's (but see convs=True below).

`FusedUpdate(block, motion_front=True)` also takes the front of the motion encoder (update.py:80,82): given
`corr = corr_fn.deferred(coords1)` (vppstereo_amd.corr.DeferredCorr) instead of the lookup's result, one launch makes
relu(convc1(lookup)) and relu(convf1(flow)) (`Engine.raft_motion_front`) and the 36-channel tensor between the lookup and
convc1 is never written; convc2, convf2 and conv stay torch's.  It is opt-in: README.md has what was measured.

`FusedUpdate(block, gru_conv=True)` takes the nine gate convolutions too: a GRU is then the assembly and two launches,
convz + convr with their gates (`Engine.raft_gru_zr`) and convq with the rest of ConvGRU.forward (`Engine.raft_gru_q`), on the
matrix cores (bfloat16 MFMA for bfloat16 storage, the float32 matrix path for float32).  The packed weights are kept per GRU and
made again when a parameter, the dtype or the device changes; a GRU whose channel counts the kernel does not take runs as
without the flag.  It is opt-in: README.md has what was measured.  The cache rule: a parameter has changed when it is another
object, when its storage has moved (`p.data = new`, `.to()`, `load_state_dict(assign=True)`) or when its version counter has
(`p.copy_()` under no_grad, `load_state_dict`); an entry lives no longer than its GRU.  A write through `p.data`
(`p.data.copy_()`, `p.data.mul_()`) shows in neither and keeps the old packed weights: call `forget_weights()` after one.

`FusedUpdate(block, convs=True)` takes the seven convolutions that are left: convc2, convf2 and conv of the motion encoder
(update.py:81,83,86; conv reads cor and flo as two sources, so their `cat` is never written), conv1 and conv2 of the flow head
(:34-42) and the two of the mask head with its `.25 *` (:113-116, :141), each one launch of `Engine.raft_conv` with its ReLU or
its scale in the epilogue.  Each convolution is decided on its own: one that is not a plain nn.Conv2d (stride 1, dilation 1,
groups 1, zero padding of k // 2, k 1 or 3, channel counts within what include/vppx.h says is built) runs in torch, as does
everything when the hidden state is of a dtype the kernel does not store.  The packed weights follow the GRUs' cache rule, per
convolution.  It is independent of the other two flags and opt-in: README.md has what was measured.

A lookup that `_motion` itself materialises (a DeferredCorr with motion_front=False) is float32; for a bfloat16 block outside
autocast it is converted to bfloat16 on its way into convc1, which would refuse it otherwise.  A tensor the caller passes is left alone.

`forward(..., mask=False)` skips the mask head on either path and returns None in its place: in test_mode the reference
computes the mask in every iteration and uses the last one (raft_stereo.py:146-153).

Inference only: the hidden state of a level is overwritten inside a buffer that is reused from call to call, which
autograd cannot follow.  float32 or bfloat16; a tensor of another dtype than the hidden state's (a convolution's output
under autocast) is converted to it, and a dtype the kernels do not store (float16) is an error.
"""
import torch
import torch.nn.functional as F

from ._convs import PackedWeights, conv_plain
from .corr import DeferredCorr, _engine


def _as(t, dtype):
    """t in the working dtype, with contiguous frames (a channel slice stays a view; a channels-last tensor is copied)."""
    if t.dtype != dtype:
        t = t.to(dtype)
    _, C, H, W = t.shape
    want = (H * W, W, 1)
    if any(n > 1 and s != w for n, s, w in zip((C, H, W), t.stride()[1:], want)):
        t = t.contiguous()
    return t


class GruGlue(PackedWeights):
    """The three launches around one ConvGRU's convolutions, and the hx buffers they work in.  The packed weights live in
    PackedWeights (_convs.py), the cache FusedEncoder uses too."""

    def __init__(self):
        PackedWeights.__init__(self)       # self._packed
        self._hx = {}                      # level (or the GRU's id) -> the hx buffer of that GRU
        self._gates = {}                   # (level, "z" / "rh") -> the z and r*h buffers of that GRU (conv=True)
        self._bufs = {}                    # name -> a buffer between two convolutions of convs=True

    def _buffer(self, level, shape, dtype, device, kept=None):
        """The hx buffer of a level (or a buffer of `kept`): kept from call to call, made again when its shape, dtype or device
        changes."""
        kept = self._hx if kept is None else kept
        buf = kept.get(level)
        if buf is None or tuple(buf.shape) != tuple(shape) or buf.dtype != dtype or buf.device != device:
            buf = kept[level] = torch.empty(tuple(shape), dtype=dtype, device=device)
        return buf

    @staticmethod
    def _conv_takes(gru, hidden, channels):
        """Whether the convolution kernel takes this GRU: three plain 3x3 convolutions of `channels` -> `hidden` channels within
        what include/vppx.h says is built."""
        from . import _lib
        if hidden % 16 or channels % 16 or channels > _lib.CONV_MAX_CIN or 2 * hidden > _lib.CONV_MAX_COUT:
            return False
        for conv in (gru.convz, gru.convr, gru.convq):
            pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)        # noqa: E731
            if (tuple(conv.weight.shape) != (hidden, channels, 3, 3) or pair(getattr(conv, "padding", 1)) != (1, 1)
                    or pair(getattr(conv, "stride", 1)) != (1, 1) or pair(getattr(conv, "dilation", 1)) != (1, 1)
                    or getattr(conv, "groups", 1) != 1 or getattr(conv, "padding_mode", "zeros") != "zeros"):
                return False
        return True

    def _packed_weights(self, eng, gru, dtype, device):
        """(packed convz + convr, packed convq) of a GRU: made once, and again when the device, the dtype or a parameter changes.
        A parameter has changed when it is another object, when its storage lies elsewhere (`p.data = new`, `.to()`,
        `load_state_dict(assign=True)`: what FusedEncoder._norm_consts looks at too) or when its version counter has moved (an
        in-place write, `load_state_dict`).  A write THROUGH `p.data` (`p.data.copy_()`, `p.data.mul_()`) moves neither and cannot
        be seen: call forget_weights() after one.  The entry holds its parameter objects, so their ids cannot come back under
        other tensors while it lives, and it goes when its GRU does: a later GRU at the same address never meets it."""
        params = [p for conv in (gru.convz, gru.convr, gru.convq) for p in (conv.weight, conv.bias)]

        def make():
            wz, bz, wr, br, wq, bq = params
            bzr = None if bz is None and br is None else torch.cat([
                torch.zeros(w.shape[0], dtype=w.dtype, device=w.device) if b is None else b.detach() for w, b in ((wz, bz), (wr, br))])
            return (eng.raft_conv3x3_pack(torch.cat([wz.detach(), wr.detach()]), bzr, dtype=dtype),
                    eng.raft_conv3x3_pack(wq, bq, dtype=dtype))

        return self._packed_for(gru, params, make, dtype, device)

    def fused_gru(self, gru, h, cz, cr, cq, *x_list, level=None, conv=False):
        """One ConvGRU.forward (update.py:23-32).  An entry of x_list is a tensor, taken as it is, or (tensor, "pool2x")
        / (tensor, "interp"), resampled to h's size on its way into hx.  -> the new hidden state, a new tensor.
        conv=True: the three convolutions run on the library's kernel with the gates as their epilogues, two launches behind
        the assembly (`Engine.raft_gru_zr`, `raft_gru_q`); a GRU whose channel counts that kernel does not take runs as with
        conv=False."""
        dtype = h.dtype
        eng = _engine(h.device)
        h = _as(h, dtype)
        sources = [(h, "copy")]
        for x in x_list:
            t, mode = x if isinstance(x, (tuple, list)) else (x, "copy")
            sources.append((_as(t, dtype), mode))
        B, _, H, W = h.shape
        channels = sum(t.shape[1] for t, _ in sources)
        hx = self._buffer(id(gru) if level is None else level, (B, channels, H, W), dtype, h.device)
        eng.raft_gru_assemble(sources, out=hx)
        hidden = h.shape[1]
        if conv and dtype in (torch.float32, torch.bfloat16) and self._conv_takes(gru, hidden, channels):
            key = id(gru) if level is None else level
            packed_zr, packed_q = self._packed_weights(eng, gru, dtype, h.device)
            z = self._buffer((key, "z"), h.shape, dtype, h.device, self._gates)
            rh = self._buffer((key, "rh"), h.shape, dtype, h.device, self._gates)   # not the h part of hx: other tiles read it as halo
            eng.raft_gru_zr(hx, packed_zr, _as(cz, dtype), _as(cr, dtype), h, z=z, rh=rh)
            return eng.raft_gru_q(rh, packed_q, _as(cq, dtype), z, h, x1=hx[:, hidden:] if channels > hidden else None)
        az = _as(gru.convz(hx), dtype)
        ar = _as(gru.convr(hx), dtype)
        cz, cr, cq = _as(cz, dtype), _as(cr, dtype), _as(cq, dtype)
        eng.raft_gru_reset(ar, cr, h, hx)          # both convolutions above have read hx: same stream
        aq = _as(gru.convq(hx), dtype)             # reads cat([r*h, x])
        return eng.raft_gru_update(az, cz, aq, cq, h)


_glue = GruGlue()


def fused_gru(gru, h, cz, cr, cq, *x_list, conv=False):
    """`gru(h, cz, cr, cq, *x_list)` of a ConvGRU (update.py:23-32) with its glue on the device, and with conv=True its
    convolutions as well; see GruGlue.fused_gru."""
    with torch.no_grad():
        return _glue.fused_gru(gru, h, cz, cr, cq, *x_list, conv=conv)


class FusedUpdate(torch.nn.Module, GruGlue):
    """A module, so that it can take the block's place as `self.update_block` of a RAFTStereo; the block is its only child
    (`state_dict` keys gain the prefix `block.`: wrap after the weights are loaded)."""

    def __init__(self, block, motion_front=False, gru_conv=False, convs=False):
        torch.nn.Module.__init__(self)
        GruGlue.__init__(self)
        self.motion_front = bool(motion_front)
        self.gru_conv = bool(gru_conv)
        self.convs = bool(convs)
        for name in ("encoder", "gru08", "gru16", "gru32", "flow_head", "mask", "n_gru_layers"):
            if not hasattr(block, name):
                raise TypeError(f"FusedUpdate: the block has no {name!r}")
        self.block = block

    def __getattr__(self, name):           # encoder, gru08, n_gru_layers, ...: the block's own
        try:
            return super().__getattr__(name)
        except AttributeError:
            block = self.__dict__.get("block", None) or self.__dict__.get("_modules", {}).get("block")
            if block is None:
                raise
            return getattr(block, name)

    @staticmethod
    def _conv_plain(conv, cin):
        """Whether Engine.raft_conv takes this module on `cin` input channels: an nn.Conv2d whose forward is nn.Conv2d's, 1x1 or
        3x3, stride 1, dilation 1, groups 1, zeros outside the map, padding k // 2, within the channel counts that are built."""
        return conv_plain(conv, cin)

    def _conv(self, conv, dtype, x0, x1=None, relu=False, scale=1.0, keep=None):
        """[relu](conv(cat([x0, x1]))) [* scale]: one launch of Engine.raft_conv in `dtype` where the kernel takes the module,
        torch otherwise.  keep: the name of the kept buffer the launch writes; None makes a new tensor."""
        cin = x0.shape[1] + (0 if x1 is None else x1.shape[1])
        if dtype in (torch.float32, torch.bfloat16) and self._conv_plain(conv, cin):
            eng = _engine(x0.device)
            x0, x1 = _as(x0, dtype), None if x1 is None else _as(x1, dtype)
            out = None
            if keep is not None:
                out = self._buffer(keep, (x0.shape[0], conv.out_channels) + tuple(x0.shape[2:]), dtype, x0.device, self._bufs)
            return eng.raft_conv(x0, self._packed_conv(eng, conv, dtype, x0.device), conv.out_channels, conv.kernel_size[0], x1=x1,
                                 relu=relu, scale=scale, out=out)
        y = conv(x0 if x1 is None else torch.cat([x0, x1.to(x0.dtype)], dim=1))
        y = F.relu(y) if relu else y
        return y if scale == 1.0 else scale * y

    @staticmethod
    def _head_convs(head):
        """(first, second) convolution of a head that is second(relu(first(x))): the reference's FlowHead (conv1, conv2, relu) or
        an nn.Sequential(Conv2d, ReLU, Conv2d); None for anything else."""
        nn = torch.nn
        if isinstance(head, nn.Sequential):
            if len(head) == 3 and isinstance(head[0], nn.Conv2d) and isinstance(head[1], nn.ReLU) and isinstance(head[2], nn.Conv2d):
                return head[0], head[2]
            return None
        kids = dict(head.named_children()) if isinstance(head, nn.Module) else {}
        if (set(kids) == {"conv1", "conv2", "relu"} and isinstance(kids["conv1"], nn.Conv2d) and isinstance(kids["conv2"], nn.Conv2d)
                and isinstance(kids["relu"], nn.ReLU)):
            return kids["conv1"], kids["conv2"]
        return None

    def _head(self, head, x, dtype, name, scale=1.0):
        """head(x) [* scale] of the flow head or the mask head: two launches where the head is one _head_convs knows."""
        pair = self._head_convs(head) if self.convs else None
        if pair is None:
            y = head(x)
            return y if scale == 1.0 else scale * y
        return self._conv(pair[1], dtype, self._conv(pair[0], dtype, x, relu=True, keep=name), scale=scale)

    def _motion(self, flow, corr, dtype=None):
        """BasicMotionEncoder.forward (update.py:79-87) up to its last cat: -> (out [B,126,H,W], flow).  dtype: the working dtype of
        convs=True, the hidden state's."""
        enc = self.block.encoder
        if isinstance(corr, DeferredCorr) and self.motion_front:
            cor, flo = self._front(enc, corr, flow)
        else:
            if isinstance(corr, DeferredCorr):
                corr = corr.materialize()  # float32; convc1 of a bfloat16 block takes bfloat16 (autocast converts by itself)
                want = getattr(getattr(enc.convc1, "weight", None), "dtype", corr.dtype)
                if corr.dtype != want and want == torch.bfloat16 and not torch.is_autocast_enabled():
                    corr = corr.to(want)
            cor, flo = F.relu(enc.convc1(corr)), None
        return self._motion_tail(enc, cor, flo, dtype, flow), flow

    def _motion_tail(self, enc, cor, flo, dtype, flow=None):
        """update.py:81-86 on relu(convc1(.)) and relu(convf1(.)): with convs=True three launches and no cat.  flo None: convf1 runs
        here on `flow`, behind convc2 as the reference orders them."""
        if self.convs:
            cor = self._conv(enc.convc2, dtype, cor, relu=True, keep="cor2")
            if flo is None:
                flo = F.relu(enc.convf1(flow))
            flo = self._conv(enc.convf2, dtype, flo, relu=True, keep="flo2")
            return self._conv(enc.conv, dtype, cor, flo, relu=True, keep="motion")
        cor = F.relu(enc.convc2(cor))
        if flo is None:
            flo = F.relu(enc.convf1(flow))
        flo = F.relu(enc.convf2(flo))
        return F.relu(enc.conv(torch.cat([cor, flo], dim=1)))

    @staticmethod
    def _front(enc, corr, flow):
        """relu(convc1(lookup)) and relu(convf1(flow)) in one launch, in flow's dtype (float32 or bfloat16)."""
        if flow.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"FusedUpdate: flow is {flow.dtype}; the kernels store float32 and bfloat16")
        f32 = lambda t: None if t is None else t.detach().float().contiguous()        # noqa: E731
        c1, f1 = enc.convc1, enc.convf1
        return _engine(flow.device).raft_motion_front(corr.pyramid, corr.coords.contiguous(), flow.float().contiguous(), f32(c1.weight),
                                                      f32(c1.bias), f32(f1.weight), f32(f1.bias), corr.radius, out_dtype=flow.dtype)

    @torch.no_grad()
    def forward(self, net, inp, corr=None, flow=None, iter08=True, iter16=True, iter32=True, update=True, mask=True):
        blk = self.block
        n = blk.n_gru_layers
        if iter32:                         # reads the old net[1]
            net[2] = self.fused_gru(blk.gru32, net[2], *(inp[2]), (net[1], "pool2x"), level=32, conv=self.gru_conv)
        if iter16:                         # reads the old net[0] and the new net[2]
            x = [(net[0], "pool2x")] + ([(net[2], "interp")] if n > 2 else [])
            net[1] = self.fused_gru(blk.gru16, net[1], *(inp[1]), *x, level=16, conv=self.gru_conv)
        if iter08:                         # reads the new net[1]
            out, fl = self._motion(flow, corr, net[0].dtype)
            x = [out, fl] + ([(net[1], "interp")] if n > 1 else [])
            net[0] = self.fused_gru(blk.gru08, net[0], *(inp[0]), *x, level=8, conv=self.gru_conv)
        if not update:
            return net
        if self.convs:
            dtype = net[0].dtype
            delta_flow = self._head(blk.flow_head, net[0], dtype, "flow_head")
            return net, (self._head(blk.mask, net[0], dtype, "mask", scale=.25) if mask else None), delta_flow
        delta_flow = blk.flow_head(net[0])
        if not mask:                       # test_mode uses the last iteration's only (raft_stereo.py:146-153)
            return net, None, delta_flow
        mask = .25 * blk.mask(net[0])      # scale mask to balance gradients (update.py:140-141)
        return net, mask, delta_flow
