"""ctypes binding of libvppx.so (C-ABI in include/vppx.h).

There is no CPU fallback anywhere in this package: if the HIP library is missing or no
MI355X is visible, every compute call raises.  PyTorch is used only as plumbing (device
memory, streams, torch.distributed) by the optional tensor front-end.
"""
import ctypes as C
import os
import threading

import numpy as np

from . import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VPPX_LIB") or os.path.join(_HERE, "libvppx.so")  # VPPX_LIB: experiment builds

# include/vppx.h is the only description of the C-ABI: the structs, the constants and (in load()) every signature come from it
with open(os.path.join(_HERE, os.pardir, "include", "vppx.h")) as _f:
    ABI = _header.parse(_f.read())
_K = ABI.constants
VPPX_OK = _K["VPPX_OK"]
ERR_NAMES = {v: n for n, v in _K.items() if n.startswith("VPPX_E_")}
EXPORTS = list(ABI.protos)      # every function the header declares, in its order
CORR_MAX_LEVELS, CORR_MAX_RADIUS = _K["VPPX_CORR_MAX_LEVELS"], _K["VPPX_CORR_MAX_RADIUS"]
DT_F32, DT_BF16 = _K["VPPX_DT_F32"], _K["VPPX_DT_BF16"]
GRU_MAX_SOURCES = _K["VPPX_GRU_MAX_SOURCES"]
MOTION_MAX_CH, MOTION_MAX_KS = _K["VPPX_MOTION_MAX_CH"], _K["VPPX_MOTION_MAX_KS"]
CONV_MAX_CIN, CONV_MAX_COUT = _K["VPPX_CONV_MAX_CIN"], _K["VPPX_CONV_MAX_COUT"]
SPP_MAX_LEVELS, SPP_MAX_K = _K["VPPX_SPP_MAX_LEVELS"], _K["VPPX_SPP_MAX_K"]
GRU_MODES = {m: _K["VPPX_GRU_" + m.upper()] for m in ("copy", "pool2x", "interp")}
FS_PATTERNS, FS_MASK, FS_GOCC, FS_GUIDED, FS_METRICS, FS_NO_DISP, FS_SAMPLE = (
    _K["VPPX_FS_" + n] for n in ("PATTERNS", "MASK", "GOCC", "GUIDED", "METRICS", "NO_DISP", "SAMPLE"))
VIZ_KEYS = ('bad 1.0', 'bad 2.0', 'bad 3.0', 'bad 4.0', 'avgerr', 'rms')  # utils.guided_visualize's dict keys (utils.py:79), VPPX_VIZ_* bit order
VIZ_ALL, VIZ_MAX_DILATION = _K["VPPX_VIZ_ALL"], _K["VPPX_VIZ_MAX_DILATION"]
METRIC_KEYS = ('bad 1.0', 'bad 2.0', 'bad 3.0', 'bad 4.0', 'avgerr', 'rms')  # the reference's dict keys (losses.py:24), VppxMetrics order

VppxVppParams, VppxRsgmParams, VppxOccParams = (ABI.structs[n] for n in ("VppxVppParams", "VppxRsgmParams", "VppxOccParams"))
VppxScaleParams, VppxEvalParams, VppxSampleParams = (ABI.structs[n] for n in ("VppxScaleParams", "VppxEvalParams", "VppxSampleParams"))
VppxGruSource, VppxMetrics = ABI.structs["VppxGruSource"], ABI.structs["VppxMetrics"]


class VppxError(Exception):
    """Raised for every non-zero return of the C-ABI; .code is the VPPX_E_* value.  The
    message is the reference's own exception text where one exists (rsgm.py:19-40)."""

    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


_lib = None
_lock = threading.Lock()


def load():
    """Load libvppx.so; raises (never falls back) when it has not been built."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: the HIP library has not been built "
                "(run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C vppstereo_amd/csrc`). "
                "vppstereo_amd has no CPU fallback.")
        # torch bundles its own HIP runtime (same soname as /opt/rocm's): whichever is loaded first
        # serves the whole process, and torch only works with its own -> let torch go first.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        lib = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in ABI.protos.items():
            fn = getattr(lib, name, None)
            if fn is None:
                raise ImportError(f"{LIB_PATH} does not export {name}, which include/vppx.h declares: rebuild the library")
            fn.restype, fn.argtypes = restype, argtypes
        _lib = lib
        return lib


def split_routes(s):
    """Split vppx_last_routes' list at the commas outside <>."""
    out, depth, cur = [], 0, []
    for ch in s:
        if ch == "," and depth == 0:
            out.append("".join(cur))
            cur = []
            continue
        depth += (ch == "<") - (ch == ">")
        cur.append(ch)
    if cur:
        out.append("".join(cur))
    return out


def _route_list(fn, handle):
    n = check(fn(handle, None, 0))
    buf = C.create_string_buffer(n + 1)
    check(fn(handle, buf, n + 1))
    return split_routes(buf.value.decode())


def last_routes(lib, handle):
    return _route_list(lib.vppx_last_routes, handle)


def last_front_routes(lib, handle):
    return _route_list(lib.vppx_last_front_routes, handle)


def check(rc):
    """Turn a negative return code into the reference's `raise Exception(msg)`."""
    if rc is not None and rc < 0:
        msg = load().vppx_last_error().decode("utf-8", "replace")
        raise VppxError(rc, msg or ERR_NAMES.get(rc, f"vppx error {rc}"))
    return rc


def np_ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


class Context:
    """One vppx_ctx (one GPU, one stream, one workspace arena)."""

    def __init__(self, device=-1):
        self._lib = load()
        self._h = C.c_void_p()
        check(self._lib.vppx_create(C.byref(self._h), int(device)))

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            self._lib.vppx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        """Bind a hipStream_t handle; 0 / None = the legacy default stream (torch's default stream)."""
        if not stream_ptr:
            check(self._lib.vppx_set_stream_legacy(self._h))
        else:
            check(self._lib.vppx_set_stream(self._h, C.c_void_p(stream_ptr)))

    def use_own_stream(self):
        """Back to the context's private non-blocking stream (what a fresh context uses)."""
        check(self._lib.vppx_set_stream(self._h, None))

    def synchronize(self):
        """Wait for the context's stream; raises VppxError when a fused aggregation launch lost its lock step."""
        check(self._lib.vppx_synchronize(self._h))

    def status(self):
        """Non-blocking health check (vppx_status): raises VppxError for a lost lock step seen so far."""
        check(self._lib.vppx_status(self._h))

    @property
    def lockstep_failures(self):
        return int(self._lib.vppx_lockstep_failures(self._h))

    @property
    def device_name(self):
        return self._lib.vppx_device_name(self._h).decode()

    @property
    def workspace_bytes(self):
        return int(self._lib.vppx_workspace_bytes(self._h))


_default_ctx = None


def default_context():
    """Process-wide context used by the drop-in module-level functions (the reference's
    natives are free functions with global libc rand() state)."""
    global _default_ctx
    if _default_ctx is None:
        dev = -1
        lr = os.environ.get("LOCAL_RANK")
        if lr is not None:
            try:
                import torch
                if torch.cuda.device_count() > int(lr):
                    dev = int(lr)
            except Exception:
                dev = -1
        _default_ctx = Context(dev)
    return _default_ctx


def _fill(p, kw):
    # setattr on a ctypes.Structure silently creates a Python attribute for an unknown name: a misspelt or
    # reference-style keyword (blending=, wsizeAgg_x=) must not be ignored
    names = {f[0] for f in p._fields_ if not f[0].startswith("reserved")}
    for k, v in kw.items():
        if k not in names:
            raise TypeError(f"{type(p).__name__}: unknown parameter {k!r} (fields: {sorted(names)})")
        setattr(p, k, v)
    return p


def vpp_params(**kw):
    p = VppxVppParams()
    load().vppx_vpp_params_default(C.byref(p))
    return _fill(p, kw)


def occ_params(**kw):
    p = VppxOccParams()
    load().vppx_occ_params_default(C.byref(p))
    return _fill(p, kw)


def rsgm_params(**kw):
    p = VppxRsgmParams()
    load().vppx_rsgm_params_default(C.byref(p))
    return _fill(p, kw)


def scale_params(**kw):
    """VppxScaleParams: iscale / oscale of test.py:36-37 (defaults 1, 1)."""
    p = VppxScaleParams()
    load().vppx_scale_params_default(C.byref(p))
    return _fill(p, kw)


def eval_params(**kw):
    """VppxEvalParams: gt_scale = --oscale of test.py:150-152 (default 1)."""
    p = VppxEvalParams()
    load().vppx_eval_params_default(C.byref(p))
    return _fill(p, kw)


def sample_params(**kw):
    """VppxSampleParams: probability = --guideperc (default 0.05), seed (default 1)."""
    p = VppxSampleParams()
    load().vppx_sample_params_default(C.byref(p))
    return _fill(p, kw)


def sample_threshold(p):
    """T of the sampling rule (include/vppx.h): torch's ``rand < p`` on float32 rand = k * 2**-24 is exactly ``k < T`` with
    T = clamp(ceil(float64(float32(p)) * 2**24), 0, 2**24); NaN selects nothing.  Host arithmetic, no library call."""
    pf = float(np.float32(p))
    if not pf > 0.0:
        return 0
    if pf >= 1.0:
        return 1 << 24
    return min(int(np.ceil(pf * 16777216.0)), 1 << 24)


def check_gt_shape(Hg, Wg, gt_scale, Ho, Wo, what="gt"):
    """What the library checks before it launches anything (vppx_guided_metrics_dev): gt_scale takes gt to the map's shape."""
    s = int(gt_scale)
    if s < 1:
        raise ValueError(f"gt_scale {s} (>= 1)")
    if (Hg // s, Wg // s) != (Ho, Wo):
        raise ValueError(f"{what} of {Hg} x {Wg} at gt_scale {s} is {Hg // s} x {Wg // s}, the disparity map is {Ho} x {Wo}")


def metrics_dict(rec):
    """One VppxMetrics record (ctypes struct or a sequence of its 8 doubles) -> the reference's dict (losses.py:24)."""
    v = [rec.bad1, rec.bad2, rec.bad3, rec.bad4, rec.avgerr, rec.rms] if isinstance(rec, VppxMetrics) else [float(x) for x in rec[:6]]
    return dict(zip(METRIC_KEYS, v))


def viz_which(which):
    """`which` of guided_visualize: None (all six), a VPPX_VIZ_* bit mask, one of the reference's keys, or an iterable of keys."""
    if which is None:
        return VIZ_ALL
    if isinstance(which, str):
        which = [which]
    if isinstance(which, int):
        w = which
    else:
        w = 0
        for k in which:
            if k not in VIZ_KEYS:
                raise ValueError(f"which: unknown map {k!r} (one of {VIZ_KEYS})")
            w |= 1 << VIZ_KEYS.index(k)
    if w <= 0 or w & ~VIZ_ALL:
        raise ValueError(f"which: {which!r} selects no map of {VIZ_KEYS}")
    return w


def scaled_shape(H, W, iscale=1, oscale=1):
    """(h, w, Ho, Wo): the shape the matcher runs at and the shape of the returned map (vppx_scaled_shape)."""
    sp = scale_params(iscale=int(iscale), oscale=int(oscale))
    v = [C.c_int(0) for _ in range(4)]
    check(load().vppx_scaled_shape(int(H), int(W), C.byref(sp), *[C.byref(x) for x in v]))
    return tuple(int(x.value) for x in v)


def c_contig(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a
