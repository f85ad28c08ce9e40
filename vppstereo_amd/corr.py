"""Drop-in for `CorrBlock1D` of models/raft_stereo/corr.py:110-183 (the import in raft_stereo.py).

`CorrBlock1D` (the default): the GEMM and the division by sqrt(D) stay torch's; the hint modulation, the pyramid and the
per-iteration lookup run in libvppx.so: the constructor is one fused pass over the volume, `__call__` one launch.
`CorrBlock1DFused`, or `CorrBlock1D(..., fused=True)`: the GEMM runs in libvppx.so too, on the matrix cores, fused with
the division, the modulation and the pyramid: the constructor is one launch that reads the two feature maps and writes
the levels, and the volume is never read back.  include/vppx.h has the arithmetic, which is the reference's bit for bit in
float32 where the float32 GEMM is exact; the fused block divides by sqrt(D) with one IEEE division where torch on the
device multiplies by a reciprocal.  bfloat16 feature maps give a bfloat16 pyramid (in the fused block every cell of
level 0 is the float32 result rounded once); the lookup's result is float32 either way, as the reference's `.float()`
makes it.  `CorrBlock1D.corr` and `Engine.raft_corr` are torch's GEMM in both classes.
`deferred(coords)` hands the lookup on without running it: `FusedUpdate(block, motion_front=True)` fuses it into convc1.
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
    def __init__(self, fmap2, fmap3, hints=None, validhints=None, num_levels=4, radius=4, *, fused=False):
        self.num_levels = num_levels
        self.radius = radius
        self._eng = _engine(fmap2.device)
        if fused:
            self.corr_pyramid = self._eng.raft_corr_fused(fmap2.contiguous(), fmap3.contiguous(), hints, validhints, num_levels)
            return
        corr = self._eng.raft_corr(fmap2, fmap3)
        # num_levels entries: the reference pools once more (corr.py:122-124) into a level that nothing reads
        self.corr_pyramid = self._eng.raft_corr_pyramid(corr, hints, validhints, num_levels)

    def __call__(self, coords):
        return self._eng.raft_corr_lookup(self.corr_pyramid, coords.contiguous(), self.radius)

    def deferred(self, coords):
        """The lookup at `coords`, not made yet: what `FusedUpdate(block, motion_front=True)` takes as `corr` and fuses
        into convc1 (vppstereo_amd/update.py); `materialize()` is `self(coords)`."""
        return DeferredCorr(self, coords)

    @staticmethod
    def corr(fmap2, fmap3, hints=None, validhints=None):
        return _engine(fmap2.device).raft_corr(fmap2, fmap3, hints, validhints)


class DeferredCorr:
    """A lookup that has not run: the pyramid, the coordinates and the radius of `CorrBlock1D.deferred(coords)`."""

    def __init__(self, block, coords):
        self.block, self.pyramid, self.coords, self.radius = block, block.corr_pyramid, coords, block.radius

    def materialize(self):
        """Today's lookup: float32 [B, levels*(2*radius+1), H4, W2]."""
        return self.block(self.coords)


class CorrBlock1DFused(CorrBlock1D):
    """`CorrBlock1D` whose constructor is the one fused launch (`fused=True` by default), for the one-line import change
    of INTEGRATION.md.  tools/README.md and profiles/corr_fused.json have what it costs against the default block."""

    def __init__(self, fmap2, fmap3, hints=None, validhints=None, num_levels=4, radius=4, *, fused=True):
        super().__init__(fmap2, fmap3, hints, validhints, num_levels, radius, fused=fused)
