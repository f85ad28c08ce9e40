"""Drop-in for `CorrBlock1D` of models/raft_stereo/corr.py:110-183 (the import in raft_stereo.py).

The GEMM and the division by sqrt(D) stay torch's; the hint modulation, the pyramid and the per-iteration lookup run
in libvppx.so: the constructor is one fused pass over the volume, `__call__` one launch (include/vppx.h has the
arithmetic, which is the reference's bit for bit in float32).  bfloat16 feature maps give a bfloat16 pyramid; the
lookup's result is float32 either way, as the reference's `.float()` makes it.
"""
from .engine import Engine

_engines = {}


def _engine(device):
    """One Engine per device for every block built in this process."""
    key = device.index
    if key not in _engines:
        _engines[key] = Engine(key)
    return _engines[key]


class CorrBlock1D:
    def __init__(self, fmap2, fmap3, hints=None, validhints=None, num_levels=4, radius=4):
        self.num_levels = num_levels
        self.radius = radius
        self._eng = _engine(fmap2.device)
        corr = self._eng.raft_corr(fmap2, fmap3)
        # num_levels entries: the reference pools once more (corr.py:122-124) into a level that nothing reads
        self.corr_pyramid = self._eng.raft_corr_pyramid(corr, hints, validhints, num_levels)

    def __call__(self, coords):
        return self._eng.raft_corr_lookup(self.corr_pyramid, coords.contiguous(), self.radius)

    @staticmethod
    def corr(fmap2, fmap3, hints=None, validhints=None):
        return _engine(fmap2.device).raft_corr(fmap2, fmap3, hints, validhints)
