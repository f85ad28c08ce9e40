"""Drop-ins for the read-out of the two deep front-ends (INTEGRATION.md has the patches).

`psmnet_regress` replaces models/psmnet/psmnet.py:227-233 (the trilinear upsample of cost3, the squeeze, the softmax
and `disparityregression`), `upsample_flow` has the signature and the result shape of `RAFTStereo.upsample_flow`
(models/raft_stereo/raft_stereo.py:69-81).  Both are one launch in libvppx.so and return float32; the negation, the
channel slice and the crop of test.py:237-245 can go into the same launch through `Engine.psmnet_disparity` /
`Engine.raft_upsample`.  bfloat16 inputs are widened on load.
"""
from .corr import _engine


def psmnet_regress(cost3, maxdisp, size):
    """cost3 [B,1,D4,H4,W4] (or [B,D4,H4,W4]) -> pred3 float32 [B,H,W], (H, W) = size."""
    return _engine(cost3.device).psmnet_disparity(cost3.contiguous(), maxdisp, size)


def upsample_flow(flow, mask, n_downsample=2):
    """flow [N,D,H,W], mask [N,9*f*f,H,W] -> float32 [N,D,f*H,f*W], f = 2**n_downsample."""
    if mask.dtype != flow.dtype:     # under autocast the mask may arrive narrower than the flow
        mask = mask.to(flow.dtype)
    return _engine(flow.device).raft_upsample(flow.contiguous(), mask.contiguous(), n_downsample)
