"""test.py:154-225 as ONE call for numpy arrays (a convenience the reference does not have; `filter.occlusion_heuristic`,
`vpp_standalone.vpp` and `rsgm.compute_rsgm` remain the drop-ins for its three call sites).

    disp = run_frame(left, right, hints, maskocc=True)                      # test.py --vpp --maskocc --stereomodel rsgm
    disp = run_frame(left, right, hints, validhints=valid)                  # test.py --vpp --guided --stereomodel rsgm
    disp, lc, rc, conf = run_frame(..., return_patterns=True)
    disp = run_frame(left, right, hints, maskocc=True, iscale=2)            # test.py --iscale 2 (resize + restore on the device)

The pair, the hints and the mask cross PCIe once, the mask never leaves the device
between the occlusion heuristic and the scan, and only the disparity map comes back unless the patterned pair is asked for.
Arithmetic, random stream and results are those of the three separate calls (tests/test_gpu_vpp.py)."""
import ctypes as C

import numpy as np

from . import _lib
from .vpp_standalone import hint_range


def _vpp_params(vk, method, dmin, dmax):
    """Keywords of `vpp_standalone.vpp` (vpp_standalone.py:396-399) -> VppxVppParams; `vk` is consumed, leftovers raise."""
    p = _lib.vpp_params(method=1 if method == "maxDistance" else 0, wsize=int(vk.pop("wsize", 3)), wsize_agg_x=int(vk.pop("wsizeAgg_x", 64)),
                        wsize_agg_y=int(vk.pop("wsizeAgg_y", 3)), direction=1 if vk.pop("left2right", True) else 0,
                        uniform_color=int(bool(vk.pop("uniform_color", False))), discard_occluded=int(bool(vk.pop("discard_occ", False))),
                        interpolate=int(bool(vk.pop("interpolate", True))), c=float(vk.pop("blending", 0.4)), c_occ=float(vk.pop("c_occ", 0.0)),
                        use_distance_patch=int(bool(vk.pop("use_distance_patch", False))), distance_gamma=float(vk.pop("distance_gamma", 0.3)),
                        dmin=dmin, dmax=dmax, use_bilateral_patch=int(bool(vk.pop("use_bilateral_patch", False))),
                        bilateral_o_xy=float(vk.pop("bilateral_o_xy", 2)), bilateral_o_i=float(vk.pop("bilateral_o_i", 1)),
                        bilateral_th=float(vk.pop("bilateral_th", .001)))
    if vk:
        raise TypeError(f"unknown vpp keyword(s): {sorted(vk)}")
    return p


def scaled_shape(H, W, iscale=1, oscale=1):
    """--iscale / --oscale (test.py:142-148, :247-248): (h, w, Ho, Wo), the shape the matcher runs at, (H // iscale, W // iscale),
    and the shape of the returned map -- floor((h, w) * iscale / oscale) when iscale != 1 and iscale / oscale != 1, else (h, w)."""
    return _lib.scaled_shape(H, W, iscale, oscale)


def _scaled_hints(gt, iscale):
    """The hints vpp() sees at iscale (test.py:147): every iscale-th row and column, divided by iscale (float32)."""
    h, w = gt.shape[0] // iscale, gt.shape[1] // iscale
    return gt[::iscale, ::iscale][:h, :w] / np.float32(iscale)


def sample_hints(src, validsrc, probability=0.05, seed=1, return_valid=True):
    """losses.sample_hints (losses.py:5-10) of one frame or a batch of host arrays on the device (vppx_sample_hints_host): frame f
    equals ``torch.manual_seed(seed + f); sample_hints(src[f], validsrc[f] > 0, probability)`` on the CPU, bit for bit.  src,
    validsrc: float [H,W] or [B,H,W].  Returns (hints, validhints) float32, or hints alone with return_valid=False."""
    src = np.ascontiguousarray(np.asarray(src, dtype=np.float32))
    validsrc = np.ascontiguousarray(np.asarray(validsrc, dtype=np.float32))
    if src.ndim not in (2, 3) or validsrc.shape != src.shape:
        raise ValueError("src, validsrc: float arrays of one shape, [H,W] or [B,H,W]")
    B = 1 if src.ndim == 2 else src.shape[0]
    H, W = src.shape[-2:]
    hints = np.empty_like(src)
    valid = np.empty_like(src) if return_valid else None
    smp = _lib.sample_params(probability=float(probability), seed=int(seed) & 0xFFFFFFFF)
    lib, ctx = _lib.load(), _lib.default_context()
    _lib.check(lib.vppx_sample_hints_host(ctx.handle, C.byref(smp), B, H, W, _lib.np_ptr(src), _lib.np_ptr(validsrc), _lib.np_ptr(hints),
                                          _lib.np_ptr(valid)))
    return (hints, valid) if return_valid else hints


SAMPLE_KEYS = ("probability", "seed", "src", "validsrc", "guided")


def check_sampled_push(sampling, metrics, hints=None, validhints=None, src=None, validsrc=None):
    """What a push on a FrameStream refuses about sampling, before anything touches the device."""
    if sampling:
        if hints is not None or validhints is not None:
            raise ValueError("the stream was created with sample=: the hints are sampled on the device, no push brings any (push_sampled)")
        if (src is None) != (validsrc is None):
            raise ValueError("src and validsrc go together")
        if src is None and not metrics:
            raise ValueError("src=None samples from the frame's gt: the stream needs metrics=True (or push src and validsrc)")
    elif src is not None or validsrc is not None:
        raise ValueError("src / validsrc given but the stream was created without sample=")


def run_frame(left, right, hints=None, maskocc=False, g_occ=None, occ_kw=None, vpp_kw=None, rsgm_kw=None, return_patterns=False,
              validhints=None, iscale=1, oscale=1, gt=None, validgt=None, return_errormap=False, sample=None):
    """left, right: uint8 [H,W,3] or [H,W]; hints: float [H,W] (0 = none).  maskocc: compute g_occ with the occlusion heuristic
    (test.py:154) -- else `g_occ` (uint8 [H,W] or None) is used as given.  vpp_kw: keywords of `vpp_standalone.vpp`
    (wsize, blending, c_occ, ...); rsgm_kw: keywords of `rsgm.compute_rsgm` (dmax, p1, ...).  validhints: float [H,W] or None;
    given, the call is --guided (test.py:207-223): `hints` also re-weight the matching costs of compute_rsgm wherever
    validhints > 0.  Returns the float32 disparity map, or (disparity, left_vpp, right_vpp, conf_map or None) with
    return_patterns.  iscale / oscale: --iscale / --oscale (test.py:136-148, :247-248): the full-size frame is resized on the
    device, the call runs at (h, w) = (H // iscale, W // iscale) -- g_occ and the returned patterns and mask have that shape --
    and the map comes back at (Ho, Wo) (`scaled_shape`).
    gt / validgt: float [H,W] (the full frame shape) or None.  Given, the frame's evaluation metrics (losses.guided_metrics,
    test.py:251-252, with the --oscale decimation of the ground truth, test.py:150-152) are computed on the device and the call
    returns ``(result_as_above, metrics)``: a dict with the reference's keys 'bad 1.0' ... 'bad 4.0', 'avgerr', 'rms' (floats),
    plus 'errormap' (float32 [Ho,Wo]) with return_errormap.
    sample: None, or dict(probability=0.05, seed=1, src=None, validsrc=None, guided=False): the hints are sampled on the device
    first (`sample_hints`; test.py:125-129) from src / validsrc or, without them, from gt / validgt; `hints` and `validhints` must
    then be None, and guided=True feeds the sampled mask as validhints (test.py:207-208)."""
    if sample is not None:
        sample = dict(sample)
        unknown = set(sample) - set(SAMPLE_KEYS)
        if unknown:
            raise TypeError(f"sample: unknown keys {sorted(unknown)} (keys: {list(SAMPLE_KEYS)})")
        if hints is not None or validhints is not None:
            raise ValueError("sample: the hints are sampled on the device; pass hints=None and validhints=None")
        s_src, s_valid = sample.get("src"), sample.get("validsrc")
        if (s_src is None) != (s_valid is None):
            raise ValueError("sample: src and validsrc go together")
        if s_src is None:
            if gt is None or validgt is None:
                raise ValueError("sample: without src / validsrc the hints are sampled from gt / validgt: pass them")
            s_src, s_valid = gt, validgt
        hints, s_mask = sample_hints(s_src, s_valid, sample.get("probability", 0.05), sample.get("seed", 1))
        if sample.get("guided"):
            validhints = s_mask
    elif hints is None:
        raise ValueError("hints: a float [H,W] array (or sample=dict(...) to sample them on the device)")
    vk = dict(vpp_kw or {})
    method = vk.pop("method", "rnd")
    assert method in ["rnd", "maxDistance"]
    evaluate = gt is not None or validgt is not None
    if evaluate and (gt is None or validgt is None):
        raise ValueError("gt and validgt go together")
    if return_errormap and not evaluate:
        raise ValueError("return_errormap needs gt and validgt")
    gt_eval, vgt_eval = gt, validgt
    left = np.ascontiguousarray(left, np.uint8)
    right = np.ascontiguousarray(right, np.uint8)
    gt = np.ascontiguousarray(np.asarray(hints, dtype=np.float32))   # (the hints: `g` / `gt` of vpp_core_opt.pyx:53)
    if left.shape != right.shape or left.shape[:2] != gt.shape:
        raise ValueError("left, right and hints must agree in height and width")
    vh = None
    if validhints is not None:
        vh = np.ascontiguousarray(np.asarray(validhints, dtype=np.float32))
        if vh.shape != gt.shape:
            raise ValueError("validhints must have the shape of hints")
    iscale, oscale = int(iscale), int(oscale)
    scaled = (iscale, oscale) != (1, 1)
    H, W = gt.shape
    h, w, Ho, Wo = scaled_shape(H, W, iscale, oscale) if scaled else (H, W, H, W)
    if evaluate:
        gt_eval = np.ascontiguousarray(np.asarray(gt_eval, dtype=np.float32))
        vgt_eval = np.ascontiguousarray(np.asarray(vgt_eval, dtype=np.float32))
        if gt_eval.shape != (H, W) or vgt_eval.shape != (H, W):
            raise ValueError(f"gt, validgt: expected shape {(H, W)}, got {gt_eval.shape}, {vgt_eval.shape}")
        _lib.check_gt_shape(H, W, oscale, Ho, Wo)
    ch = 1 if left.ndim == 2 else left.shape[2]
    dmin, dmax = hint_range(_scaled_hints(gt, iscale) if iscale != 1 else gt)
    no_hints = dmin is None
    if no_hints:
        dmin, dmax = 0.0, 0.0     # no hints: the scan leaves the pair as it is (vpp_standalone.py:407)
    p = _vpp_params(vk, method, dmin, dmax)
    if no_hints:
        p.use_distance_patch = 0  # vpp() returns the untouched pair before dmin / dmax are looked at (vpp_standalone.py:407)
    if p.use_distance_patch and not dmax > dmin:
        raise ZeroDivisionError("use_distance_patch needs two distinct hint values (vpp_standalone.py:8 divides by dmax-dmin)")
    rk = dict(rsgm_kw or {})
    if "subpixel" in rk:
        rk["subpixel"] = int(bool(rk["subpixel"]))
    rp = _lib.rsgm_params(**rk)
    op = _lib.occ_params(**(occ_kw or {})) if maskocc else None
    occ = None
    if not maskocc and g_occ is not None:
        occ = np.ascontiguousarray(np.asarray(g_occ) != 0, np.uint8)
        if occ.shape != (h, w):
            raise ValueError(f"g_occ: expected shape {(h, w)}, got {occ.shape}")
    lib, ctx = _lib.load(), _lib.default_context()
    seed, consumed = C.c_uint32(), C.c_uint64()
    _lib.check(lib.vppx_rand_state(ctx.handle, C.byref(seed), C.byref(consumed)))   # the stream vpp() and the scans share
    p.seed, p.rand_offset = seed.value, consumed.value
    disp = np.empty((Ho, Wo), np.float32)
    lc = rc = conf = None
    if return_patterns:
        lc, rc = np.empty((h, w, ch), np.uint8), np.empty((h, w, ch), np.uint8)
        conf = np.empty((h, w), np.uint8) if maskocc else None
    draws = (C.c_uint64 * 1)()
    try:
        if scaled:
            sp = _lib.scale_params(iscale=iscale, oscale=oscale)
            _lib.check(lib.vppx_occ_vpp_rsgm_scaled_host(ctx.handle, C.byref(op) if op is not None else None, C.byref(p), C.byref(rp),
                                                         C.byref(sp), 1, H, W, ch, _lib.np_ptr(left), _lib.np_ptr(right), _lib.np_ptr(gt),
                                                         _lib.np_ptr(occ), _lib.np_ptr(vh), _lib.np_ptr(conf), _lib.np_ptr(lc),
                                                         _lib.np_ptr(rc), _lib.np_ptr(disp), None, draws))
        elif vh is not None:
            _lib.check(lib.vppx_occ_vpp_rsgm_guided_host(ctx.handle, C.byref(op) if op is not None else None, C.byref(p), C.byref(rp), 1,
                                                         h, w, ch, _lib.np_ptr(left), _lib.np_ptr(right), _lib.np_ptr(gt), _lib.np_ptr(occ),
                                                         _lib.np_ptr(vh), _lib.np_ptr(conf), _lib.np_ptr(lc), _lib.np_ptr(rc),
                                                         _lib.np_ptr(disp), draws))
        else:
            _lib.check(lib.vppx_occ_vpp_rsgm_host(ctx.handle, C.byref(op) if op is not None else None, C.byref(p), C.byref(rp), 1, h, w,
                                                  ch, _lib.np_ptr(left), _lib.np_ptr(right), _lib.np_ptr(gt), _lib.np_ptr(occ),
                                                  _lib.np_ptr(conf), _lib.np_ptr(lc), _lib.np_ptr(rc), _lib.np_ptr(disp), draws))
    except _lib.VppxError as e:
        raise Exception(str(e)) from e   # the reference raises bare Exception(msg) (rsgm.py:31-40,166)
    if method == "rnd":
        _lib.check(lib.vppx_rand_advance(ctx.handle, int(draws[0])))
    result = (disp, lc, rc, conf) if return_patterns else disp
    if not evaluate:
        return result
    rec = _lib.VppxMetrics()
    emap = np.empty((Ho, Wo), np.float32) if return_errormap else None
    ep = _lib.eval_params(gt_scale=oscale)
    _lib.check(lib.vppx_guided_metrics_host(ctx.handle, C.byref(ep), 1, Ho, Wo, _lib.np_ptr(disp), H, W, _lib.np_ptr(gt_eval),
                                            _lib.np_ptr(vgt_eval), C.byref(rec), _lib.np_ptr(emap)))
    metrics = _lib.metrics_dict(rec)
    if return_errormap:
        metrics['errormap'] = emap
    return result, metrics


class FrameStream:
    """The hot path for a caller that holds ONE numpy frame at a time (test.py:291-311: a DataLoader with batch size 1, then
    :154-225 per frame) at the rate of the batched kernels: frames go in one at a time, results come out one at a time in
    input order, and in between the library batches them (libvppx `vppx_fstream_*`: one multi-threaded copy into a page-locked
    ring of `depth` batches, upload of batch k+1 under batch k's kernels, copy-out under batch k+1's sum / WTA kernel; depth 3 is
    what keeps the device busy, depth 2 saves a third of the ring's page-locked and device memory at ~10 % of the rate).

        with FrameStream(540, 960, maskocc=True, rsgm_kw=dict(dmax=192), seed=7) as fs:
            for disp in fs.run((l, r, hints) for l, r, hints in loader):     # input order
                ...
        # or: fs.push(l, r, hints); ...; fs.flush(); r = fs.pop()

    Frame f (counted from the stream's creation) draws its colours from srand(seed + f): its results equal
    `init_rand(seed + f); run_frame(...)` bit for bit whatever `batch`, wherever a flush falls.  (The reference's single libc
    stream running through all frames is a serial dependency between frames; per-frame streams are what lets frames be
    batched and sharded)  `use_distance_patch`: dmin / dmax are each frame's own, computed on the device
    (a frame whose hints all have ONE value, where the reference divides by zero, gets the full patch size).  batch=None: one round of the lock-step kernel for this shape (vppx_batch_quantum), else 16.
    Results: the float32 disparity map, or with return_patterns (disparity, left_vpp, right_vpp, conf_map or None); each a fresh
    array.  `draws` of the last popped frame (rand() calls it consumed) is in `last_draws`.
    guided=True: --guided (test.py:207-223); every push brings the frame's validhints, and the frame equals
    `run_frame(..., validhints=...)` with seed + f.
    iscale / oscale: --iscale / --oscale (test.py:136-148, :247-248): pushes take full-size frames (and, with_g_occ, masks of the
    scaled shape); disparities come back at (Ho, Wo), patterns and mask at (h, w) (`scaled_shape`), and frame f equals
    `run_frame(..., iscale=, oscale=)` with seed + f.  batch=None then takes the batch quantum of the scaled shape.
    metrics=True: an evaluating stream (test.py:251-252).  Frames go in through ``push_eval``, which also brings the frame's ground
    truth, ``gt=`` and ``validgt=`` (float [H,W], the full frame shape; > 0 is valid), the metrics of every batch are computed on the device behind its kernels
    (with the --oscale decimation of test.py:150-152) and each result becomes ``(result_as_above, metrics)`` -- metrics: the
    dict of `run_frame`, without an error map; `last_metrics_record` holds the popped frame's eight doubles (VppxMetrics).
    return_disp=False (needs metrics=True): the disparity maps stay on the device and each result is the metrics dict alone.
    sample=probability: the hints are sampled on the device (test.py:125-129, `sample_hints`): frames go in through
    ``push_sampled``, frame f samples with seed sample_seed + f (sample_seed=None: the stream's `seed`) and equals
    `run_frame(..., sample=dict(probability=, seed=sample_seed + f, ...))` with init_rand(seed + f)."""

    def __init__(self, height, width, channels=3, batch=None, depth=3, seed=1, maskocc=False, with_g_occ=False, occ_kw=None,
                 vpp_kw=None, rsgm_kw=None, return_patterns=False, copy_threads=-1, device=-1, guided=False, iscale=1, oscale=1,
                 metrics=False, return_disp=True, sample=None, sample_seed=None):
        self._sample = sample is not None
        if not return_disp and not metrics:
            raise ValueError("return_disp=False needs metrics=True (a stream that returns nothing)")
        if not return_disp and return_patterns:
            raise ValueError("return_disp=False returns the metrics alone: not with return_patterns")
        vk = dict(vpp_kw or {})
        method = vk.pop("method", "rnd")
        assert method in ["rnd", "maxDistance"]
        if maskocc and with_g_occ:
            raise ValueError("either maskocc (the mask is computed on the way) or with_g_occ (every push brings one)")
        p = _vpp_params(vk, method, 0.0, 0.0)
        p.seed = int(seed) & 0xFFFFFFFF
        rk = dict(rsgm_kw or {})
        if "subpixel" in rk:
            rk["subpixel"] = int(bool(rk["subpixel"]))
        rp = _lib.rsgm_params(**rk)
        op = _lib.occ_params(**(occ_kw or {})) if maskocc else None
        self.h, self.w, self.ch = int(height), int(width), int(channels)
        self._shape = (self.h, self.w) if self.ch == 1 else (self.h, self.w, self.ch)
        self.iscale, self.oscale = int(iscale), int(oscale)
        self._scaled = (self.iscale, self.oscale) != (1, 1)
        self._lib = _lib.load()
        if self._scaled:
            sp = _lib.scale_params(iscale=self.iscale, oscale=self.oscale)
            try:
                self.hs, self.ws, self.ho, self.wo = scaled_shape(self.h, self.w, self.iscale, self.oscale)
            except _lib.VppxError as e:
                raise Exception(str(e)) from e
        else:
            self.hs, self.ws, self.ho, self.wo = self.h, self.w, self.h, self.w
        self._shape_s = (self.hs, self.ws) if self.ch == 1 else (self.hs, self.ws, self.ch)
        self._metrics, self._return_disp = bool(metrics), bool(return_disp)
        if self._metrics:
            _lib.check_gt_shape(self.h, self.w, self.oscale, self.ho, self.wo)
        self._ctx = _lib.Context(device)
        if batch is None:
            batch = int(self._lib.vppx_batch_quantum(self._ctx.handle, self.hs, self.ws, int(rp.dmax))) or 16
        self.batch, self.depth = int(batch), int(depth)
        self._patterns, self._mask, self._gocc = bool(return_patterns), bool(maskocc and return_patterns), bool(with_g_occ)
        self._guided = bool(guided)
        flags = (_lib.FS_PATTERNS if self._patterns else 0) | (_lib.FS_MASK if self._mask else 0) | (_lib.FS_GOCC if self._gocc else 0)
        flags |= _lib.FS_GUIDED if self._guided else 0
        flags |= (_lib.FS_METRICS if self._metrics else 0) | (0 if self._return_disp else _lib.FS_NO_DISP)
        flags |= _lib.FS_SAMPLE if self._sample else 0
        self._fill_has_src = False
        self._h = C.c_void_p()
        self.last_metrics_record = None
        try:
            if self._sample:
                ep = _lib.eval_params(gt_scale=self.oscale) if self._metrics else None
                smp = _lib.sample_params(probability=float(sample), seed=int(seed if sample_seed is None else sample_seed) & 0xFFFFFFFF)
                _lib.check(self._lib.vppx_fstream_create_sampled(self._ctx.handle, C.byref(op) if op is not None else None, C.byref(p),
                                                                 C.byref(rp), C.byref(sp) if self._scaled else None,
                                                                 C.byref(ep) if ep is not None else None, C.byref(smp), self.batch, self.depth,
                                                                 self.h, self.w, self.ch, flags, int(copy_threads), C.byref(self._h)))
            elif self._metrics:
                ep = _lib.eval_params(gt_scale=self.oscale)
                _lib.check(self._lib.vppx_fstream_create_eval(self._ctx.handle, C.byref(op) if op is not None else None, C.byref(p),
                                                              C.byref(rp), C.byref(sp) if self._scaled else None, C.byref(ep), self.batch,
                                                              self.depth, self.h, self.w, self.ch, flags, int(copy_threads),
                                                              C.byref(self._h)))
            elif self._scaled:
                _lib.check(self._lib.vppx_fstream_create_scaled(self._ctx.handle, C.byref(op) if op is not None else None, C.byref(p),
                                                                C.byref(rp), C.byref(sp), self.batch, self.depth, self.h, self.w, self.ch,
                                                                flags, int(copy_threads), C.byref(self._h)))
            else:
                _lib.check(self._lib.vppx_fstream_create(self._ctx.handle, C.byref(op) if op is not None else None, C.byref(p), C.byref(rp),
                                                         self.batch, self.depth, self.h, self.w, self.ch, flags, int(copy_threads), C.byref(self._h)))
        except _lib.VppxError as e:
            self._ctx.close()
            raise Exception(str(e)) from e
        self._pushed = self._popped = self._fill = 0
        self._inflight = []       # frames not yet popped of every submitted batch, oldest first (at most `depth` batches)
        self._early = []          # results popped to make room, oldest first
        self.last_draws = 0

    # ---- context manager / lifetime ----
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if getattr(self, "_h", None):
            self._lib.vppx_fstream_destroy(self._h)
            self._h = C.c_void_p()
            self._ctx.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- one frame in ----
    def _arr(self, a, dtype, shape, name):
        a = np.asarray(a)
        if a.dtype != dtype or not a.flags.c_contiguous:
            a = np.ascontiguousarray(a, dtype)
        if a.shape != shape:
            raise ValueError(f"{name}: expected shape {shape}, got {a.shape}")
        return a

    def push(self, left, right, hints, g_occ=None, validhints=None):
        """One frame in (copied before the call returns).  The frame that completes a batch submits it; if that submit fails
        the push raises but HAS taken the frame, and the next push or `flush()` submits the batch again.  validhints: float
        [H,W], required on a guided stream and refused on any other.  A metrics=True stream takes its frames through
        `push_eval`, a sample= stream through `push_sampled`."""
        check_sampled_push(self._sample, self._metrics, hints, validhints)
        if self._metrics:
            raise ValueError("the stream was created with metrics=True: every push brings gt and validgt (push_eval)")
        self._push(left, right, hints, g_occ, validhints, None, None)

    def push_eval(self, left, right, hints, g_occ=None, validhints=None, gt=None, validgt=None):
        """`push` on a metrics=True stream (vppx_fstream_push_eval): the frame and its ground truth, gt and validgt, float [H,W]
        at the full frame shape (validgt > 0 is valid).  Refused on any other stream."""
        check_sampled_push(self._sample, self._metrics, hints, validhints)
        if not self._metrics:
            raise ValueError("gt / validgt given but the stream was created without metrics=True")
        if gt is None or validgt is None:
            raise ValueError("the stream was created with metrics=True: every push brings gt and validgt")
        self._push(left, right, hints, g_occ, validhints, gt, validgt)

    def push_sampled(self, left, right, g_occ=None, src=None, validsrc=None, gt=None, validgt=None):
        """One frame into a sample= stream (vppx_fstream_push_sampled): its hints are sampled on the device with probability
        `sample`, frame f of the stream with sampling seed sample_seed + f, from src / validsrc (float [H,W]) or -- src=None, on a
        metrics=True stream -- from the gt / validgt the push brings anyway (nothing else goes up for the hints then).  A guided=True
        stream feeds the sampled mask as validhints.  Refused on any other stream."""
        check_sampled_push(self._sample, self._metrics, None, None, src, validsrc)
        if not self._sample:
            raise ValueError("the stream was created without sample=: every push brings its hints (push / push_eval)")
        if self._metrics and (gt is None or validgt is None):
            raise ValueError("the stream was created with metrics=True: every push brings gt and validgt")
        if not self._metrics and (gt is not None or validgt is not None):
            raise ValueError("gt / validgt given but the stream was created without metrics=True")
        if src is not None:
            src = self._arr(src, np.float32, (self.h, self.w), "src")
            validsrc = self._arr(validsrc, np.float32, (self.h, self.w), "validsrc")
        if self._fill and self._fill_has_src != (src is not None):
            self.flush()   # a batch samples from one kind of source
        self._push(left, right, src, g_occ, validsrc, gt, validgt)

    def _push(self, left, right, hints, g_occ, validhints, gt, validgt):
        left = self._arr(left, np.uint8, self._shape, "left")
        right = self._arr(right, np.uint8, self._shape, "right")
        if not self._sample:
            hints = self._arr(hints, np.float32, (self.h, self.w), "hints")
        occ = None
        if self._gocc:
            if g_occ is None:
                raise ValueError("the stream was created with with_g_occ=True: every push brings a mask")
            occ = np.ascontiguousarray(np.asarray(g_occ) != 0, np.uint8)
            if occ.shape != (self.hs, self.ws):
                raise ValueError(f"g_occ: expected shape {(self.hs, self.ws)}")
        elif g_occ is not None:
            raise ValueError("g_occ given but the stream was created without with_g_occ=True")
        vh = None
        if self._sample:
            vh = validhints   # (the frame's validsrc, checked by push_sampled)
        elif self._guided:
            if validhints is None:
                raise ValueError("the stream was created with guided=True: every push brings validhints")
            vh = self._arr(validhints, np.float32, (self.h, self.w), "validhints")
        elif validhints is not None:
            raise ValueError("validhints given but the stream was created without guided=True")
        if self._metrics:
            gt = self._arr(gt, np.float32, (self.h, self.w), "gt")
            validgt = self._arr(validgt, np.float32, (self.h, self.w), "validgt")
        # a full batch whose submit failed (an earlier push raised, having taken its frame): submit it before anything else --
        # raises again, and takes nothing, if it still fails
        if self._fill == self.batch:
            self.flush()
        # the ring holds `depth` submitted batches: before the frame that would start one more, take the oldest batch's results
        if self._fill == 0:
            while len(self._inflight) >= self.depth:
                self._early.append(self._pop_native())
        try:
            occ_p = occ.ctypes.data if occ is not None else None
            if self._sample:
                if self._fill == 0:
                    self._fill_has_src = hints is not None
                _lib.check(self._lib.vppx_fstream_push_sampled(self._h, left.ctypes.data, right.ctypes.data, occ_p,
                                                               hints.ctypes.data if hints is not None else None,
                                                               vh.ctypes.data if vh is not None else None,
                                                               gt.ctypes.data if gt is not None else None,
                                                               validgt.ctypes.data if validgt is not None else None))
            elif self._metrics:
                _lib.check(self._lib.vppx_fstream_push_eval(self._h, left.ctypes.data, right.ctypes.data, hints.ctypes.data, occ_p,
                                                            vh.ctypes.data if vh is not None else None, gt.ctypes.data,
                                                            validgt.ctypes.data))
            elif vh is not None:
                _lib.check(self._lib.vppx_fstream_push_guided(self._h, left.ctypes.data, right.ctypes.data, hints.ctypes.data, occ_p,
                                                              vh.ctypes.data))
            else:
                _lib.check(self._lib.vppx_fstream_push(self._h, left.ctypes.data, right.ctypes.data, hints.ctypes.data, occ_p))
        except _lib.VppxError as e:
            # the native stream may have taken the frame and failed only to submit the batch it completed: stay in step
            if self.counts()[0] > self._pushed:
                self._pushed += 1
                self._fill += 1
            raise Exception(str(e)) from e
        self._pushed += 1
        self._fill += 1
        if self._fill == self.batch:
            self._inflight.append(self._fill)
            self._fill = 0

    def flush(self):
        """Submit the frames pushed so far as a smaller batch (end of the sequence, or a latency bound)."""
        try:
            _lib.check(self._lib.vppx_fstream_flush(self._h))
        except _lib.VppxError as e:
            raise Exception(str(e)) from e
        if self._fill:
            self._inflight.append(self._fill)
            self._fill = 0

    # ---- one frame out ----
    def _pop_native(self):
        disp = np.empty((self.ho, self.wo), np.float32) if self._return_disp else None
        rec = _lib.VppxMetrics() if self._metrics else None
        lc = rc = conf = None
        if self._patterns:
            lc, rc = np.empty(self._shape_s, np.uint8), np.empty(self._shape_s, np.uint8)
        if self._mask:
            conf = np.empty((self.hs, self.ws), np.uint8)
        draws, got = C.c_uint64(0), C.c_int(0)
        try:
            if self._metrics:
                _lib.check(self._lib.vppx_fstream_pop_eval(self._h, disp.ctypes.data if disp is not None else None,
                                                           lc.ctypes.data if lc is not None else None,
                                                           rc.ctypes.data if rc is not None else None,
                                                           conf.ctypes.data if conf is not None else None, C.byref(draws), C.byref(rec),
                                                           C.byref(got)))
            else:
                _lib.check(self._lib.vppx_fstream_pop(self._h, disp.ctypes.data, lc.ctypes.data if lc is not None else None,
                                                      rc.ctypes.data if rc is not None else None, conf.ctypes.data if conf is not None else None,
                                                      C.byref(draws), C.byref(got)))
        except _lib.VppxError as e:
            raise Exception(str(e)) from e
        if not got.value:
            return None
        self._popped += 1
        self._inflight[0] -= 1
        if self._inflight[0] == 0:
            self._inflight.pop(0)
        res = (disp, lc, rc, conf) if self._patterns else disp
        if self._metrics:
            record = np.array([rec.bad1, rec.bad2, rec.bad3, rec.bad4, rec.avgerr, rec.rms, rec.n_valid, rec.reserved], np.float64)
            md = _lib.metrics_dict(rec)
            res = (res, md) if self._return_disp else md
            return res, int(draws.value), record
        return res, int(draws.value), None

    def pop(self):
        """The next result in input order (waits for its batch), or None when nothing submitted is outstanding."""
        r = self._early.pop(0) if self._early else self._pop_native()
        if r is None:
            return None
        self.last_draws = r[1]
        self.last_metrics_record = r[2]
        return r[0]

    @property
    def pending(self):
        """Frames pushed whose results have not been popped."""
        return self._pushed - self._popped + len(self._early)

    def counts(self):
        """(frames pushed, frames of the batch being filled, frames submitted and not popped, batches re-run after a lost lock step)."""
        v = [C.c_int64(0) for _ in range(4)]
        _lib.check(self._lib.vppx_fstream_counts(self._h, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def run(self, frames):
        """Generator: results for an iterable of (left, right, hints[, g_occ]) in input order -- on a guided stream
        (left, right, hints, g_occ or None, validhints); on a metrics=True stream the two extra entries gt, validgt come at
        the end: (left, right, hints, g_occ or None, validhints or None, gt, validgt); on a sample= stream the arguments of
        `push_sampled`: (left, right[, g_occ, src, validsrc, gt, validgt]) -- keeps about `depth` batches in flight."""
        for fr in frames:
            (self.push_sampled if self._sample else self.push_eval if self._metrics else self.push)(*fr)
            # whole batches that must be complete by now: everything but the last depth - 1 submitted ones
            while self._early:
                yield self.pop()
            while len(self._inflight) >= self.depth:
                yield self.pop()
        self.flush()
        while True:
            r = self.pop()
            if r is None:
                return
            yield r


def run_stream(frames, **kw):
    """`FrameStream(...).run(frames)` with the shape taken from the first frame; keywords as for `FrameStream`."""
    it = iter(frames)
    try:
        first = next(it)
    except StopIteration:
        return
    l = np.asarray(first[0])
    ch = 1 if l.ndim == 2 else l.shape[2]

    def chain():
        yield first
        yield from it
    with FrameStream(l.shape[0], l.shape[1], ch, with_g_occ=kw.pop("with_g_occ", len(first) > 3 and first[3] is not None), **kw) as fs:
        yield from fs.run(chain())
