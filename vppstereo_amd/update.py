"""RAFT-Stereo's update block with the work between its convolutions on the device (INTEGRATION.md has the patch).

`FusedUpdate(block)` wraps an existing `BasicMultiUpdateBlock` (models/raft_stereo/update.py:99-142): any module with
`encoder`, `gru08` / `gru16` / `gru32` (each with `convz`, `convr`, `convq`), `flow_head`, `mask` and `n_gru_layers`.  It
holds the block and calls its convolutions as they are, so the block's weights and its `state_dict` are untouched; what it replaces is
the glue of `forward` and of the three `ConvGRU.forward` calls (:23-32): per GRU one launch assembles
hx = cat([h, *x]) with pool2x (:89-90) and interp (:95-97) applied on the way, one launch writes r * h over the h part of
that buffer, which convq then reads as cat([r*h, x]), and one launch makes the new hidden state
(`Engine.raft_gru_assemble`, `raft_gru_reset`, `raft_gru_update`; include/vppx.h has the arithmetic).  The encoder's
`cat([out, flow])` (:87) becomes two sources of gru08's hx.  The convolutions, their ReLUs, `flow_head`, `mask` and the
`.25 *` stay torch's.

`FusedUpdate(block, motion_front=True)` also takes the front of the motion encoder (update.py:80,82): given
`corr = corr_fn.deferred(coords1)` (vppstereo_amd.corr.DeferredCorr) instead of the lookup's result, one launch makes
relu(convc1(lookup)) and relu(convf1(flow)) (`Engine.raft_motion_front`) and the 36-channel tensor between the lookup and
convc1 is never written; convc2, convf2 and conv stay torch's.  It is opt-in: README.md has what was measured.

Inference only: the hidden state of a level is overwritten inside a buffer that is reused from call to call, which
autograd cannot follow.  float32 or bfloat16; a tensor of another dtype than the hidden state's (a convolution's output
under autocast) is converted to it, and a dtype the kernels do not store (float16) is an error.
"""
import torch
import torch.nn.functional as F

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


class GruGlue:
    """The three launches around one ConvGRU's convolutions, and the hx buffers they work in."""

    def __init__(self):
        self._hx = {}                      # level (or the GRU's id) -> the hx buffer of that GRU

    def _buffer(self, level, shape, dtype, device):
        """The hx buffer of a level: kept from call to call, made again when its shape, dtype or device changes."""
        buf = self._hx.get(level)
        if buf is None or tuple(buf.shape) != tuple(shape) or buf.dtype != dtype or buf.device != device:
            buf = self._hx[level] = torch.empty(tuple(shape), dtype=dtype, device=device)
        return buf

    def fused_gru(self, gru, h, cz, cr, cq, *x_list, level=None):
        """One ConvGRU.forward (update.py:23-32).  An entry of x_list is a tensor, taken as it is, or (tensor, "pool2x")
        / (tensor, "interp"), resampled to h's size on its way into hx.  -> the new hidden state, a new tensor."""
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
        az = _as(gru.convz(hx), dtype)
        ar = _as(gru.convr(hx), dtype)
        cz, cr, cq = _as(cz, dtype), _as(cr, dtype), _as(cq, dtype)
        eng.raft_gru_reset(ar, cr, h, hx)          # both convolutions above have read hx: same stream
        aq = _as(gru.convq(hx), dtype)             # reads cat([r*h, x])
        return eng.raft_gru_update(az, cz, aq, cq, h)


_glue = GruGlue()


def fused_gru(gru, h, cz, cr, cq, *x_list):
    """`gru(h, cz, cr, cq, *x_list)` of a ConvGRU (update.py:23-32) with its glue on the device; see GruGlue.fused_gru."""
    with torch.no_grad():
        return _glue.fused_gru(gru, h, cz, cr, cq, *x_list)


class FusedUpdate(torch.nn.Module, GruGlue):
    """A module, so that it can take the block's place as `self.update_block` of a RAFTStereo; the block is its only child
    (`state_dict` keys gain the prefix `block.`: wrap after the weights are loaded)."""

    def __init__(self, block, motion_front=False):
        torch.nn.Module.__init__(self)
        GruGlue.__init__(self)
        self.motion_front = bool(motion_front)
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

    def _motion(self, flow, corr):
        """BasicMotionEncoder.forward (update.py:79-87) up to its last cat: -> (out [B,126,H,W], flow)."""
        enc = self.block.encoder
        if isinstance(corr, DeferredCorr) and self.motion_front:
            cor, flo = self._front(enc, corr, flow)
        else:
            if isinstance(corr, DeferredCorr):
                corr = corr.materialize()
            cor, flo = F.relu(enc.convc1(corr)), None
        cor = F.relu(enc.convc2(cor))
        if flo is None:
            flo = F.relu(enc.convf1(flow))
        flo = F.relu(enc.convf2(flo))
        return F.relu(enc.conv(torch.cat([cor, flo], dim=1))), flow

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
    def forward(self, net, inp, corr=None, flow=None, iter08=True, iter16=True, iter32=True, update=True):
        blk = self.block
        n = blk.n_gru_layers
        if iter32:                         # reads the old net[1]
            net[2] = self.fused_gru(blk.gru32, net[2], *(inp[2]), (net[1], "pool2x"), level=32)
        if iter16:                         # reads the old net[0] and the new net[2]
            x = [(net[0], "pool2x")] + ([(net[2], "interp")] if n > 2 else [])
            net[1] = self.fused_gru(blk.gru16, net[1], *(inp[1]), *x, level=16)
        if iter08:                         # reads the new net[1]
            out, fl = self._motion(flow, corr)
            x = [out, fl] + ([(net[1], "interp")] if n > 1 else [])
            net[0] = self.fused_gru(blk.gru08, net[0], *(inp[0]), *x, level=8)
        if not update:
            return net
        delta_flow = blk.flow_head(net[0])
        mask = .25 * blk.mask(net[0])      # scale mask to balance gradients (update.py:140-141)
        return net, mask, delta_flow
