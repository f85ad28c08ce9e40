"""Batched, device-resident front-end of the hot path (test.py:158-225 for B frames at once).

torch is plumbing only: tensors own the HBM buffers, ``torch.cuda.current_stream`` orders the
work, ``torch.distributed`` shards frame batches (see dist.py).  Every method hands raw device
pointers to the C-ABI ``_dev`` entry points of libvppx.so.
"""
import ctypes as C

from . import _lib


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# The convolution's rule for output channels: multiples of 16 (raft_conv3x3* and the gates) or any count from 1 on (raft_conv*).
_OUT_16, _OUT_ANY = "out16", "any"


def _conv_built(rule):
    return (f"multiples of 16 up to {_lib.CONV_MAX_CIN} in and {'1 to ' if rule is _OUT_ANY else ''}{_lib.CONV_MAX_COUT} "
            "out are built")


class Engine:
    """One GPU's VPP+rSGM pipeline.  Inputs are CUDA tensors:
        left, right : uint8  [B,H,W,C]     hints : float32 [B,H,W]     g_occ : uint8 [B,H,W] or None
    """

    def __init__(self, device=None):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("vppstereo_amd.Engine needs an MI355X (no CPU fallback)")
        self.torch = torch
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.ctx = _lib.Context(self.device.index)
        self.lib = _lib.load()
        self._conv_sizes = {}              # (rule, Cout, Cin, ksize, VppxDtype) -> bytes of the packed weights

    def _bind_stream(self):
        """Run on torch's current stream, so that library kernels are ordered with the torch work around them.
        torch's default stream is the legacy null stream (handle 0): the context then launches on the null stream
        itself (vppx_set_stream_legacy); re-binding an unchanged stream costs nothing."""
        self.ctx.set_stream(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _chk(self, t, dtype, ndim, name, shape=None):
        """Every tensor handed to the C-ABI is checked here: the library trusts B/H/W/C and raw pointers."""
        if t.device != self.device or t.dtype != dtype or t.dim() != ndim or not t.is_contiguous():
            raise ValueError(f"{name}: expected contiguous {dtype} tensor with {ndim} dims on {self.device}")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")

    def _chk_pair(self, left, right, hints, g_occ=None):
        torch = self.torch
        self._chk(left, torch.uint8, 4, "left")
        B, H, W, Cc = left.shape
        if Cc not in (1, 3):
            raise ValueError("left: channels must be 1 or 3")
        self._chk(right, torch.uint8, 4, "right", left.shape)
        self._chk(hints, torch.float32, 3, "hints", (B, H, W))
        if g_occ is not None:
            self._chk(g_occ, torch.uint8, 3, "g_occ", (B, H, W))
        return B, H, W, Cc

    def vpp(self, left, right, hints, g_occ=None, seed=1, **kw):
        """In-place-free VPP: returns patterned copies (l_vpp, r_vpp) like vpp() does."""
        B, H, W, Cc = self._chk_pair(left, right, hints, g_occ)
        self._bind_stream()
        l, r = left.clone(), right.clone()
        p = _lib.vpp_params(seed=int(seed) & 0xFFFFFFFF, **kw)
        _lib.check(self.lib.vppx_vpp_dev(self.ctx.handle, C.byref(p), B, H, W, Cc, _ptr(l), _ptr(r), _ptr(hints),
                                         _ptr(g_occ), None, None))
        return l, r

    def rsgm(self, left, left_vpp, right_vpp, out=None, hints=None, validhints=None, **kw):
        """compute_rsgm for a batch; hints / validhints (float32 [B,H,W], both or neither): --guided (rsgm.py:265-268)."""
        torch = self.torch
        self._chk(left, torch.uint8, 4, "left")
        B, H, W, Cc = left.shape
        self._chk(left_vpp, torch.uint8, 4, "left_vpp", left.shape)
        self._chk(right_vpp, torch.uint8, 4, "right_vpp", left.shape)
        if (hints is None) != (validhints is None):
            raise ValueError("hints and validhints go together (--guided needs both)")
        if hints is not None:
            self._chk(hints, torch.float32, 3, "hints", (B, H, W))
            self._chk(validhints, torch.float32, 3, "validhints", (B, H, W))
        if out is None:
            out = torch.empty((B, H, W), dtype=torch.float32, device=self.device)
        self._chk(out, torch.float32, 3, "out", (B, H, W))
        self._bind_stream()
        p = _lib.rsgm_params(**kw)
        _lib.check(self.lib.vppx_rsgm_dev(self.ctx.handle, C.byref(p), B, H, W, Cc, _ptr(left), _ptr(left_vpp),
                                          _ptr(right_vpp), _ptr(hints), _ptr(validhints), _ptr(out)))
        return out

    def rsgm_post(self, disp_l_pad, disp_r_pad, h, w, subpixel=True, out=None):
        """Stage API: the post-processing of compute_rsgm (rsgm.py:275-292) on the padded left / right disparity maps
        [B, Hp, Wp] (Hp, Wp = h, w rounded up to multiples of 16): crop, left/right check, astype(uint8), filterSpeckles(0, 200,
        10), sub-pixel restore, _interpolate_background.  Returns [B, h, w] float32."""
        torch = self.torch
        self._chk(disp_l_pad, torch.float32, 3, "disp_l_pad")
        B, Hp, Wp = disp_l_pad.shape
        self._chk(disp_r_pad, torch.float32, 3, "disp_r_pad", disp_l_pad.shape)
        if (Hp, Wp) != (-(-int(h) // 16) * 16, -(-int(w) // 16) * 16):
            raise ValueError("padded maps must be [B, ceil16(h), ceil16(w)]")
        if out is None:
            out = torch.empty((B, int(h), int(w)), dtype=torch.float32, device=self.device)
        self._chk(out, torch.float32, 3, "out", (B, int(h), int(w)))
        self._bind_stream()
        _lib.check(self.lib.vppx_rsgm_post_dev(self.ctx.handle, B, int(h), int(w), _ptr(disp_l_pad), _ptr(disp_r_pad),
                                               int(bool(subpixel)), _ptr(out)))
        return out

    @staticmethod
    def _padded(h, w):
        return -(-int(h) // 16) * 16, -(-int(w) // 16) * 16

    def rsgm_front(self, left, left_vpp, right_vpp):
        """Stage API: the front stage of compute_rsgm (rsgm.py:254-263) through the one launch the whole call makes: reflect
        pad, gray, 5x5 census.  left / left_vpp / right_vpp: uint8 [B,H,W,C].  Returns (gray_left uint8, census_l uint32,
        census_r uint32), each [B,Hp,Wp]: the padded gray image of `left`, the census codes of the padded patterned pair."""
        torch = self.torch
        self._chk(left, torch.uint8, 4, "left")
        B, H, W, Cc = left.shape
        if Cc not in (1, 3):
            raise ValueError("left: channels must be 1 or 3")
        self._chk(left_vpp, torch.uint8, 4, "left_vpp", left.shape)
        self._chk(right_vpp, torch.uint8, 4, "right_vpp", left.shape)
        Hp, Wp = self._padded(H, W)
        gray = torch.empty((B, Hp, Wp), dtype=torch.uint8, device=self.device)
        cl = torch.empty((B, Hp, Wp), dtype=torch.uint32, device=self.device)
        cr = torch.empty((B, Hp, Wp), dtype=torch.uint32, device=self.device)
        self._bind_stream()
        _lib.check(self.lib.vppx_rsgm_front_dev(self.ctx.handle, B, H, W, Cc, _ptr(left), _ptr(left_vpp), _ptr(right_vpp),
                                                _ptr(gray), _ptr(cl), _ptr(cr)))
        return gray, cl, cr

    def rsgm_guided_rows(self, census_l, census_r, hints, validhints, dmax):
        """Stage API: the compact re-weighted cost rows of --guided (_guided_dsi, rsgm.py:116-127) through the launch the
        whole call makes.  census_l / census_r: uint32 [B,Hp,Wp]; hints / validhints: float32 [B,H,W] with Hp, Wp = H, W
        rounded up to multiples of 16.  Returns (gmap int32 [B,Hp,Wp], rows uint16 [B*H*W, dmax], count uint32 [1]): gmap is
        the row index of every pixel with validhints > 0 (-1 elsewhere), count the number of rows written."""
        torch = self.torch
        self._chk(hints, torch.float32, 3, "hints")
        B, H, W = hints.shape
        self._chk(validhints, torch.float32, 3, "validhints", hints.shape)
        Hp, Wp = self._padded(H, W)
        self._chk(census_l, torch.uint32, 3, "census_l", (B, Hp, Wp))
        self._chk(census_r, torch.uint32, 3, "census_r", (B, Hp, Wp))
        gmap = torch.empty((B, Hp, Wp), dtype=torch.int32, device=self.device)
        rows = torch.empty((B * H * W, int(dmax)), dtype=torch.uint16, device=self.device)
        count = torch.empty((1,), dtype=torch.uint32, device=self.device)
        self._bind_stream()
        _lib.check(self.lib.vppx_rsgm_guided_rows_dev(self.ctx.handle, B, H, W, int(dmax), _ptr(census_l), _ptr(census_r),
                                                      _ptr(hints), _ptr(validhints), _ptr(gmap), _ptr(rows), _ptr(count)))
        return gmap, rows, count

    def rsgm_mid(self, disp_l, disp_r):
        """Stage API: median3x3 -> _linear_interpolate(., 15, 3) -> clip (rsgm.py:145-151, 173-179) of the padded left /
        right disparity maps, float32 [B,Hp,Wp] with Hp, Wp multiples of 16, through the launch the whole call makes.
        Returns (out_l, out_r)."""
        torch = self.torch
        self._chk(disp_l, torch.float32, 3, "disp_l")
        B, Hp, Wp = disp_l.shape
        self._chk(disp_r, torch.float32, 3, "disp_r", disp_l.shape)
        out_l, out_r = torch.empty_like(disp_l), torch.empty_like(disp_r)
        self._bind_stream()
        _lib.check(self.lib.vppx_rsgm_mid_dev(self.ctx.handle, B, Hp, Wp, _ptr(disp_l), _ptr(disp_r), _ptr(out_l), _ptr(out_r)))
        return out_l, out_r

    def _chk_call(self, left, right, planes, scale, g_occ, heuristic, out, l_vpp, r_vpp, occ_out, disp_small=None, gt_scale=None,
                  errormap=None):
        """The tensors of one `vpp_rsgm` call, whatever its route.  left / right: uint8 [B,H,W,C]; planes: (tensor or None, name)
        pairs of the float32 [B,H,W] maps at the full frame shape (hints, validhints, gt, ...); scale: (iscale, oscale), or None
        for the unscaled call.  g_occ (a tensor), occ_out, l_vpp, r_vpp and disp_small have the shape (h, w) the call runs at,
        out -- allocated here when None -- and errormap the restored one (Ho, Wo); gt_scale: given, it must take (H, W) there.
        Returns (B, H, W, C, out)."""
        torch = self.torch
        self._chk(left, torch.uint8, 4, "left")
        B, H, W, Cc = left.shape
        if Cc not in (1, 3):
            raise ValueError("left: channels must be 1 or 3")
        self._chk(right, torch.uint8, 4, "right", left.shape)
        h, w, Ho, Wo = _lib.scaled_shape(H, W, *scale) if scale else (H, W, H, W)
        for t, n in planes:
            if t is not None:
                self._chk(t, torch.float32, 3, n, (B, H, W))
        if gt_scale is not None:
            _lib.check_gt_shape(H, W, gt_scale, Ho, Wo)
        if g_occ is not None and not heuristic:
            self._chk(g_occ, torch.uint8, 3, "g_occ", (B, h, w))
        if out is None:
            out = torch.empty((B, Ho, Wo), dtype=torch.float32, device=self.device)
        self._chk(out, torch.float32, 3, "out", (B, Ho, Wo))
        if disp_small is not None:
            self._chk(disp_small, torch.float32, 3, "disp_small", (B, h, w))
        for t, n in ((l_vpp, "l_vpp"), (r_vpp, "r_vpp")):
            if t is not None:
                self._chk(t, torch.uint8, 4, n, (B, h, w, Cc))
        if occ_out is not None:
            if not heuristic:
                raise ValueError("occ_out is the mask output of g_occ='occlusion_heuristic'")
            self._chk(occ_out, torch.uint8, 3, "occ_out", (B, h, w))
        if errormap is not None:
            self._chk(errormap, torch.float32, 3, "errormap", (B, Ho, Wo))
        return B, H, W, Cc, out

    def _call_params(self, seed, vpp_kw, rsgm_kw, g_occ, heuristic, inputs_ready):
        """Last step in front of the C entry point of a `vpp_rsgm` call: bind the stream, build the parameter blocks (vp, rp, op
        -- None without the heuristic) and hand over the inputs-ready event, which the next hot-path call consumes."""
        self._bind_stream()
        vp = _lib.vpp_params(seed=int(seed) & 0xFFFFFFFF, **(vpp_kw or {}))
        rp = _lib.rsgm_params(**(rsgm_kw or {}))
        op = _lib.occ_params(**(g_occ if isinstance(g_occ, dict) else {})) if heuristic else None
        if inputs_ready is not None:
            _lib.check(self.lib.vppx_inputs_ready_event(self.ctx.handle, C.c_void_p(inputs_ready.cuda_event)))
        return vp, rp, op

    def vpp_rsgm(self, left, right, hints=None, g_occ=None, out=None, l_vpp=None, r_vpp=None, seed=1, vpp_kw=None,
                 rsgm_kw=None, occ_out=None, inputs_ready=None, validhints=None, iscale=1, oscale=1, disp_small=None,
                 gt=None, validgt=None, metrics_out=None, errormap=None, sample=None):
        """The whole hot path for a batch: one call, no host round trips, no synchronisation.

        g_occ: None, a uint8 [B,H,W] mask tensor, or -- test.py:154 with --maskocc in the same call --
        ``"occlusion_heuristic"`` / a dict of its parameters (rx, ry, l, g, th_conf, th_filter): the mask is then
        computed on the way (vppx_occ_vpp_rsgm_dev) and also written to `occ_out` when given.
        inputs_ready: a ``torch.cuda.Event`` recorded after the work that produced this call's input tensors.  Only
        matters with `set_pipeline(True)`: the front stage then waits for that event instead of for everything queued on
        the current stream, and can overlap the previous call's tail (it then covers `validhints` too).
        validhints: float32 [B,H,W] or None.  Given, the call is --guided (test.py:207-223): `hints` also re-weight the
        matching costs wherever validhints > 0 (vppx_occ_vpp_rsgm_guided_dev), with either form of g_occ.
        iscale / oscale: --iscale / --oscale (test.py:136-148, :247-248, vppx_occ_vpp_rsgm_scaled_dev).  The inputs keep their
        full shape [B,H,W(,C)]; the call runs at (h, w) = (H // iscale, W // iscale), so g_occ, occ_out, l_vpp and r_vpp are of
        that shape, and `out` is [B,Ho,Wo] (pipeline.scaled_shape).  disp_small: float32 [B,h,w] or None, the map before the
        restore.  With the defaults the call is exactly the unscaled one.
        gt / validgt: float32 [B,H,W] (the full frame shape) or None.  Given, the call also computes losses.guided_metrics of
        its result on the device, behind the post stage on the same stream (vppx_occ_vpp_rsgm_eval_dev: test.py:136-252 in one
        call), with gt_scale = oscale (test.py:150-152), and returns ``(out, metrics)``: metrics is a float64 [B,8] tensor, a
        view of the VppxMetrics records (`guided_metrics`); metrics_out: such a tensor to write into; errormap: float32
        [B,Ho,Wo] or None, receives the reference's error map.  Without gt the call is today's, and returns `out`.
        sample: None, or a dict(probability=0.05, seed=1, src=None, validsrc=None, guided=False, hints_out=None,
        validhints_out=None): the hints are sampled on the device on the way (vppx_occ_vpp_rsgm_sampled_dev; `sample_hints`
        describes the stream), frame f with sampling seed `seed + f`, from src / validsrc (float32 [B,H,W]) or, without them,
        from gt / validgt.  `hints` and `validhints` must then be None; guided=True is --guided with the sampled mask
        (test.py:207-208); hints_out / validhints_out: float32 [B,H,W] tensors that receive the sampled maps."""
        if sample is not None:
            if hints is not None or validhints is not None:
                raise ValueError("sample: the hints are sampled on the device; pass hints=None and validhints=None")
            heuristic = isinstance(g_occ, (str, dict))
            if isinstance(g_occ, str) and g_occ != "occlusion_heuristic":
                raise ValueError("g_occ: expected a mask tensor, None, 'occlusion_heuristic' or a dict of its parameters")
            return self._vpp_rsgm_sampled(left, right, dict(sample), g_occ, heuristic, out, l_vpp, r_vpp, seed, vpp_kw, rsgm_kw, occ_out,
                                          inputs_ready, int(iscale), int(oscale), disp_small, gt, validgt, metrics_out, errormap)
        if hints is None:
            raise ValueError("hints: a float32 [B,H,W] tensor (or sample=dict(...) to sample them on the device)")
        heuristic = isinstance(g_occ, (str, dict))
        if isinstance(g_occ, str) and g_occ != "occlusion_heuristic":
            raise ValueError("g_occ: expected a mask tensor, None, 'occlusion_heuristic' or a dict of its parameters")
        if gt is not None or validgt is not None:
            return self._vpp_rsgm_eval(left, right, hints, g_occ, heuristic, out, l_vpp, r_vpp, seed, vpp_kw, rsgm_kw, occ_out,
                                       inputs_ready, validhints, int(iscale), int(oscale), disp_small, gt, validgt, metrics_out, errormap)
        if metrics_out is not None or errormap is not None:
            raise ValueError("metrics_out / errormap are outputs of the evaluating call: pass gt and validgt")
        if int(iscale) != 1 or int(oscale) != 1 or disp_small is not None:
            return self._vpp_rsgm_scaled(left, right, hints, g_occ, heuristic, out, l_vpp, r_vpp, seed, vpp_kw, rsgm_kw, occ_out,
                                         inputs_ready, validhints, int(iscale), int(oscale), disp_small)
        B, H, W, Cc, out = self._chk_call(left, right, ((hints, "hints"), (validhints, "validhints")), None, g_occ, heuristic, out,
                                          l_vpp, r_vpp, occ_out)
        vp, rp, op = self._call_params(seed, vpp_kw, rsgm_kw, g_occ, heuristic, inputs_ready)
        if validhints is not None:
            _lib.check(self.lib.vppx_occ_vpp_rsgm_guided_dev(self.ctx.handle, C.byref(op) if heuristic else None,
                                                             C.byref(vp), C.byref(rp), B, H, W, Cc, _ptr(left), _ptr(right),
                                                             _ptr(hints), None if heuristic else _ptr(g_occ),
                                                             _ptr(validhints), _ptr(occ_out), _ptr(l_vpp), _ptr(r_vpp),
                                                             _ptr(out)))
        elif heuristic:
            _lib.check(self.lib.vppx_occ_vpp_rsgm_dev(self.ctx.handle, C.byref(op), C.byref(vp), C.byref(rp), B, H, W, Cc,
                                                      _ptr(left), _ptr(right), _ptr(hints), _ptr(occ_out), _ptr(l_vpp),
                                                      _ptr(r_vpp), _ptr(out)))
        else:
            _lib.check(self.lib.vppx_vpp_rsgm_dev(self.ctx.handle, C.byref(vp), C.byref(rp), B, H, W, Cc, _ptr(left),
                                                  _ptr(right), _ptr(hints), _ptr(g_occ), _ptr(l_vpp), _ptr(r_vpp),
                                                  _ptr(out)))
        return out

    def _vpp_rsgm_scaled(self, left, right, hints, g_occ, heuristic, out, l_vpp, r_vpp, seed, vpp_kw, rsgm_kw, occ_out, inputs_ready,
                         validhints, iscale, oscale, disp_small):
        B, H, W, Cc, out = self._chk_call(left, right, ((hints, "hints"), (validhints, "validhints")), (iscale, oscale), g_occ, heuristic,
                                          out, l_vpp, r_vpp, occ_out, disp_small)
        sp = _lib.scale_params(iscale=iscale, oscale=oscale)
        vp, rp, op = self._call_params(seed, vpp_kw, rsgm_kw, g_occ, heuristic, inputs_ready)
        _lib.check(self.lib.vppx_occ_vpp_rsgm_scaled_dev(self.ctx.handle, C.byref(op) if heuristic else None, C.byref(vp), C.byref(rp),
                                                         C.byref(sp), B, H, W, Cc, _ptr(left), _ptr(right), _ptr(hints),
                                                         None if heuristic else _ptr(g_occ), _ptr(validhints), _ptr(occ_out),
                                                         _ptr(l_vpp), _ptr(r_vpp), _ptr(out), _ptr(disp_small)))
        return out

    def _metrics_tensor(self, B, metrics_out):
        torch = self.torch
        if metrics_out is None:
            return torch.empty((B, 8), dtype=torch.float64, device=self.device)
        self._chk(metrics_out, torch.float64, 2, "metrics_out", (B, 8))
        return metrics_out

    def guided_metrics(self, disp, gt, validgt, gt_scale=1, errormap=None, metrics_out=None):
        """losses.guided_metrics (losses.py:13-24) for a batch on the device, no synchronisation (vppx_guided_metrics_dev).
        disp: float32 [B,Ho,Wo]; gt, validgt: float32 [B,Hg,Wg] with (Hg // gt_scale, Wg // gt_scale) == (Ho, Wo): gt_scale is
        --oscale (test.py:150-152: every gt_scale-th row and column, gt / gt_scale).  Returns a float64 [B,8] tensor, one
        VppxMetrics record per frame: bad 1.0, 2.0, 3.0, 4.0, avgerr, rms, n_valid, reserved (`_lib.metrics_dict` names
        them); a frame's record does not depend on the batch it is in.  errormap: float32 [B,Ho,Wo] or None."""
        torch = self.torch
        if gt is None or validgt is None:
            raise ValueError("gt and validgt go together")
        self._chk(disp, torch.float32, 3, "disp")
        B, Ho, Wo = disp.shape
        self._chk(gt, torch.float32, 3, "gt")
        _, Hg, Wg = gt.shape
        self._chk(gt, torch.float32, 3, "gt", (B, Hg, Wg))
        self._chk(validgt, torch.float32, 3, "validgt", (B, Hg, Wg))
        _lib.check_gt_shape(Hg, Wg, gt_scale, Ho, Wo)
        if errormap is not None:
            self._chk(errormap, torch.float32, 3, "errormap", (B, Ho, Wo))
        m = self._metrics_tensor(B, metrics_out)
        self._bind_stream()
        ep = _lib.eval_params(gt_scale=int(gt_scale))
        _lib.check(self.lib.vppx_guided_metrics_dev(self.ctx.handle, C.byref(ep), B, Ho, Wo, _ptr(disp), Hg, Wg, _ptr(gt), _ptr(validgt),
                                                    _ptr(m), _ptr(errormap)))
        return m

    # ---- pictures (utils.py:17-79, test.py:318-343): viz_kernels.hip ----
    def _viz_out(self, shape, out):
        torch = self.torch
        if out is None:
            return torch.empty(shape, dtype=torch.uint8, device=self.device)
        self._chk(out, torch.uint8, len(shape), "out", shape)
        return out

    @staticmethod
    def _viz_dilation(dilation):
        d = int(dilation)
        if d < 0:
            raise ValueError(f"dilation {d} (>= 0)")
        if d > _lib.VIZ_MAX_DILATION:
            raise ValueError(f"dilation {d} is above this build's limit of {_lib.VIZ_MAX_DILATION}")
        return d

    def error_colors(self, errors, mask=None, scale=1, bgr=True, dilation=1, out=None):
        """utils.color_error_image_kitti (utils.py:17-36) for a batch on the device, no synchronisation (vppx_error_colors_dev).
        errors: float32 [B,H,W]; mask: float32 [B,H,W] or None (mask == 0 is black).  Returns uint8 [B,H,W,3]; the dilation
        (cv2.dilate with a d x d box, fused with the colouring) is 0 or 1 for none."""
        torch = self.torch
        self._chk(errors, torch.float32, 3, "errors")
        B, H, W = errors.shape
        if mask is not None:
            self._chk(mask, torch.float32, 3, "mask", (B, H, W))
        if not float(scale) > 0:
            raise ValueError(f"scale {scale} (> 0)")
        d = self._viz_dilation(dilation)
        out = self._viz_out((B, H, W, 3), out)
        self._bind_stream()
        _lib.check(self.lib.vppx_error_colors_dev(self.ctx.handle, B, H, W, _ptr(errors), _ptr(mask), float(scale), int(bool(bgr)), d,
                                                  _ptr(out)))
        return out

    def guided_visualize(self, disp, gt, valid, scale=1, dilation=7, which=None, out=None):
        """utils.guided_visualize (utils.py:39-79) for a batch on the device, no synchronisation (vppx_guided_visualize_dev).
        disp, gt, valid: float32 [B,H,W] (valid == 0 is black).  which: None (all six maps), one of the reference's keys, an
        iterable of keys or a VPPX_VIZ_* bit mask: only those maps are computed.  out: uint8 [6,B,H,W,3] to write into (the
        planes not selected are left alone).  Returns a dict keyed like the reference's, of uint8 [B,H,W,3] views of `out`."""
        torch = self.torch
        self._chk(disp, torch.float32, 3, "disp")
        B, H, W = disp.shape
        self._chk(gt, torch.float32, 3, "gt", (B, H, W))
        self._chk(valid, torch.float32, 3, "valid", (B, H, W))
        if not float(scale) > 0:
            raise ValueError(f"scale {scale} (> 0)")
        d = self._viz_dilation(dilation)
        w = _lib.viz_which(which)
        out = self._viz_out((6, B, H, W, 3), out)
        self._bind_stream()
        _lib.check(self.lib.vppx_guided_visualize_dev(self.ctx.handle, B, H, W, _ptr(disp), _ptr(gt), _ptr(valid), float(scale), d, w,
                                                      _ptr(out)))
        return {k: out[n] for n, k in enumerate(_lib.VIZ_KEYS) if w >> n & 1}

    def colorize(self, x, max_val, lut, dilation=0, out=None):
        """The colour-mapped map of test.py:325-326, :343 for a batch on the device, no synchronisation (vppx_colorize_dev):
        lut[uint8(clamp(x, 0, max_val) / max_val * 255)].  x: float32 [B,H,W]; max_val: float32 [B], one per frame
        (`finite_max`); lut: uint8 [256,3], the user colour map cv2.applyColorMap takes.  Returns uint8 [B,H,W,3]."""
        torch = self.torch
        self._chk(x, torch.float32, 3, "x")
        B, H, W = x.shape
        self._chk(max_val, torch.float32, 1, "max_val", (B,))
        self._chk(lut, torch.uint8, 2, "lut", (256, 3))
        d = self._viz_dilation(dilation)
        out = self._viz_out((B, H, W, 3), out)
        self._bind_stream()
        _lib.check(self.lib.vppx_colorize_dev(self.ctx.handle, B, H, W, _ptr(x), _ptr(max_val), _ptr(lut), d, _ptr(out)))
        return out

    def finite_max(self, x):
        """test.py:318 per frame: the maximum of x[f] with +-inf replaced by -inf (vppx_finite_max_dev).  x: float32 [B,H,W];
        returns float32 [B] on the device, no synchronisation."""
        torch = self.torch
        self._chk(x, torch.float32, 3, "x")
        B, H, W = x.shape
        out = torch.empty((B,), dtype=torch.float32, device=self.device)
        self._bind_stream()
        _lib.check(self.lib.vppx_finite_max_dev(self.ctx.handle, B, H, W, _ptr(x), _ptr(out)))
        return out

    def _vpp_rsgm_eval(self, left, right, hints, g_occ, heuristic, out, l_vpp, r_vpp, seed, vpp_kw, rsgm_kw, occ_out, inputs_ready,
                       validhints, iscale, oscale, disp_small, gt, validgt, metrics_out, errormap):
        if gt is None or validgt is None:
            raise ValueError("gt and validgt go together")
        planes = ((hints, "hints"), (gt, "gt"), (validgt, "validgt"), (validhints, "validhints"))
        B, H, W, Cc, out = self._chk_call(left, right, planes, (iscale, oscale), g_occ, heuristic, out, l_vpp, r_vpp, occ_out, disp_small,
                                          gt_scale=oscale, errormap=errormap)
        sp = _lib.scale_params(iscale=iscale, oscale=oscale)
        m = self._metrics_tensor(B, metrics_out)
        ep = _lib.eval_params(gt_scale=oscale)
        vp, rp, op = self._call_params(seed, vpp_kw, rsgm_kw, g_occ, heuristic, inputs_ready)
        _lib.check(self.lib.vppx_occ_vpp_rsgm_eval_dev(self.ctx.handle, C.byref(op) if heuristic else None, C.byref(vp), C.byref(rp),
                                                       C.byref(sp), C.byref(ep), B, H, W, Cc, _ptr(left), _ptr(right), _ptr(hints),
                                                       None if heuristic else _ptr(g_occ), _ptr(validhints), _ptr(gt), _ptr(validgt),
                                                       _ptr(occ_out), _ptr(l_vpp), _ptr(r_vpp), _ptr(out), _ptr(disp_small), _ptr(m),
                                                       _ptr(errormap)))
        return out, m

    SAMPLE_KEYS = ("probability", "seed", "src", "validsrc", "guided", "hints_out", "validhints_out")

    def sample_hints(self, src, validsrc, probability=0.05, seed=1, out=None, valid_out=None):
        """losses.sample_hints (losses.py:5-10) for a batch on the device, on torch's CPU random stream (vppx_sample_hints_dev):
        frame f equals ``torch.manual_seed(seed + f); sample_hints(src[f], validsrc[f] > 0, probability)`` on the CPU, bit for
        bit.  src, validsrc: float32 [B,H,W].  Returns (hints, validhints), float32 [B,H,W]; no synchronisation."""
        torch = self.torch
        self._chk(src, torch.float32, 3, "src")
        B, H, W = src.shape
        self._chk(validsrc, torch.float32, 3, "validsrc", (B, H, W))
        if out is None:
            out = torch.empty_like(src)
        if valid_out is None:
            valid_out = torch.empty_like(src)
        self._chk(out, torch.float32, 3, "out", (B, H, W))
        self._chk(valid_out, torch.float32, 3, "valid_out", (B, H, W))
        smp = _lib.sample_params(probability=float(probability), seed=int(seed) & 0xFFFFFFFF)
        self._bind_stream()
        _lib.check(self.lib.vppx_sample_hints_dev(self.ctx.handle, C.byref(smp), B, H, W, _ptr(src), _ptr(validsrc), _ptr(out), _ptr(valid_out)))
        return out, valid_out

    def _vpp_rsgm_sampled(self, left, right, sample, g_occ, heuristic, out, l_vpp, r_vpp, seed, vpp_kw, rsgm_kw, occ_out, inputs_ready,
                          iscale, oscale, disp_small, gt, validgt, metrics_out, errormap):
        unknown = set(sample) - set(self.SAMPLE_KEYS)
        if unknown:
            raise TypeError(f"sample: unknown keys {sorted(unknown)} (keys: {list(self.SAMPLE_KEYS)})")
        src, validsrc = sample.get("src"), sample.get("validsrc")
        if (src is None) != (validsrc is None):
            raise ValueError("sample: src and validsrc go together")
        evaluating = gt is not None or validgt is not None
        if evaluating and (gt is None or validgt is None):
            raise ValueError("gt and validgt go together")
        if src is None and not evaluating:
            raise ValueError("sample: without src / validsrc the hints are sampled from gt / validgt: pass them")
        if not evaluating and (metrics_out is not None or errormap is not None):
            raise ValueError("metrics_out / errormap are outputs of the evaluating call: pass gt and validgt")
        planes = ((src, "src"), (validsrc, "validsrc"), (gt, "gt"), (validgt, "validgt"), (sample.get("hints_out"), "hints_out"),
                  (sample.get("validhints_out"), "validhints_out"))
        B, H, W, Cc, out = self._chk_call(left, right, planes, (iscale, oscale), g_occ, heuristic, out, l_vpp, r_vpp, occ_out, disp_small,
                                          gt_scale=oscale if evaluating else None, errormap=errormap)
        sp = _lib.scale_params(iscale=iscale, oscale=oscale)
        m = self._metrics_tensor(B, metrics_out) if evaluating else None
        ep = _lib.eval_params(gt_scale=oscale) if evaluating else None
        smp = _lib.sample_params(probability=float(sample.get("probability", 0.05)), seed=int(sample.get("seed", 1)) & 0xFFFFFFFF)
        vp, rp, op = self._call_params(seed, vpp_kw, rsgm_kw, g_occ, heuristic, inputs_ready)
        _lib.check(self.lib.vppx_occ_vpp_rsgm_sampled_dev(
            self.ctx.handle, C.byref(op) if heuristic else None, C.byref(vp), C.byref(rp), C.byref(sp), C.byref(ep) if evaluating else None,
            C.byref(smp), B, H, W, Cc, _ptr(left), _ptr(right), _ptr(src), _ptr(validsrc), 1 if sample.get("guided") else 0,
            None if heuristic else _ptr(g_occ), _ptr(gt), _ptr(validgt), _ptr(occ_out), _ptr(l_vpp), _ptr(r_vpp), _ptr(out), _ptr(disp_small),
            _ptr(m), _ptr(errormap), _ptr(sample.get("hints_out")), _ptr(sample.get("validhints_out"))))
        return (out, m) if evaluating else out

    def occlusion_heuristic(self, hints, rx=9, ry=7, l=2, g=0.4375, th_conf=1, th_filter=0.1, out=None):
        torch = self.torch
        self._chk(hints, torch.float32, 3, "hints")
        B, H, W = hints.shape
        conf = torch.empty((B, H, W), dtype=torch.uint8, device=self.device) if out is None else out
        self._chk(conf, torch.uint8, 3, "out", (B, H, W))
        self._bind_stream()
        _lib.check(self.lib.vppx_occlusion_heuristic_dev(self.ctx.handle, B, H, W, _ptr(hints), int(rx), int(ry),
                                                         float(l), float(g), float(th_conf), float(th_filter),
                                                         _ptr(conf)))
        return conf

    def to_network_input(self, img_u8, dtype=None, pad_multiple=32):
        """Patterned uint8 [B,H,W,C] -> [B,C,Hq,Wq] float32/bfloat16 in [0,1], replicate-padded to
        multiples of 32: the tensors test.py:179-200 feeds to PSMNet / RAFT-Stereo."""
        torch = self.torch
        self._chk(img_u8, torch.uint8, 4, "img")
        dtype = dtype or torch.float32
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("dtype must be float32 or bfloat16")
        B, H, W, Cc = img_u8.shape
        ph = (((H // pad_multiple) + 1) * pad_multiple - H) % pad_multiple
        pw = (((W // pad_multiple) + 1) * pad_multiple - W) % pad_multiple
        out = torch.empty((B, Cc, H + ph, W + pw), dtype=dtype, device=self.device)
        self._bind_stream()
        _lib.check(self.lib.vppx_u8_to_nchw_dev(self.ctx.handle, B, H, W, Cc, int(pad_multiple), _ptr(img_u8), _ptr(out),
                                                int(dtype == torch.bfloat16)))
        return out

    # ---- hand-off rows ----
    def _handoff_dtype(self, t):
        """float32 or bfloat16 storage of a hand-off tensor -> (torch dtype, VppxDtype)."""
        torch = self.torch
        if getattr(t, "dtype", None) == torch.bfloat16:
            return torch.bfloat16, _lib.DT_BF16
        return torch.float32, _lib.DT_F32          # anything else fails _chk's float32 check with its usual message

    def psmnet_cost_volume(self, fea_l, fea_r, maxdisp, hints=None, validhints=None):
        """The tensor PSMNet.forward hands to dres0 (models/psmnet/psmnet.py:157-197): concat volume
        [B,2C,maxdisp//4,H4,W4] from the two feature maps [B,C,H4,W4], times the hint modulation when
        hints / validhints ([B,1,H,W] float32) are given.  The feature maps are float32 or bfloat16 (both the same) and
        the volume has their dtype; a bfloat16 cell is the float32 product rounded once (include/vppx.h)."""
        torch = self.torch
        dtype, dt = self._handoff_dtype(fea_l)
        if getattr(fea_r, "dtype", None) in (torch.float32, torch.bfloat16) and fea_r.dtype != dtype:
            raise ValueError("feature maps must have the same dtype (float32 or bfloat16)")
        self._chk(fea_l, dtype, 4, "fea_l")
        self._chk(fea_r, dtype, 4, "fea_r")
        if fea_r.shape != fea_l.shape:
            raise ValueError("feature maps must have the same shape")
        B, Cc, H4, W4 = fea_l.shape
        H = W = 0
        if hints is not None:
            self._chk_hint_pair(hints, validhints, B)
            H, W = hints.shape[2:]
        cost = torch.empty((B, 2 * Cc, int(maxdisp) // 4, H4, W4), dtype=dtype, device=self.device)
        self._bind_stream()
        _lib.check(self.lib.vppx_psmnet_cost_volume_dt_dev(self.ctx.handle, _ptr(fea_l), _ptr(fea_r),
                                                           _ptr(hints) if hints is not None else None,
                                                           _ptr(validhints) if hints is not None else None,
                                                           B, Cc, H4, W4, int(H), int(W), int(maxdisp), _ptr(cost), dt))
        return cost

    def _chk_hint_pair(self, hints, validhints, B):
        """Both [B,1,H,W] float32: the kernels index the two with one offset and read B frames of each."""
        torch = self.torch
        self._chk(hints, torch.float32, 4, "hints")
        self._chk(validhints, torch.float32, 4, "validhints")
        if hints.shape != validhints.shape or hints.shape[:2] != (B, 1):
            raise ValueError("hints / validhints must be [B,1,H,W]")

    def raft_corr(self, fmap2, fmap3, hints=None, validhints=None):
        """CorrBlock1D.corr (models/raft_stereo/corr.py:151-180): all-pairs correlation along the row
        (a library GEMM through torch) / sqrt(D), then the hint modulation in place on the device.  bfloat16 maps (both
        the same dtype) give a bfloat16 volume: torch does the GEMM and the division in bfloat16."""
        torch = self.torch
        dtype, dt = self._handoff_dtype(fmap2)
        if getattr(fmap3, "dtype", None) in (torch.float32, torch.bfloat16) and fmap3.dtype != dtype:
            raise ValueError("feature maps must have the same dtype (float32 or bfloat16)")
        self._chk(fmap2, dtype, 4, "fmap2")
        self._chk(fmap3, dtype, 4, "fmap3")
        B, Dc, H4, W2 = fmap2.shape
        if fmap3.shape[:3] != fmap2.shape[:3]:
            raise ValueError("fmap2 / fmap3 must be [B,D,H4,W2] / [B,D,H4,W3]")
        W3 = fmap3.shape[3]
        if hints is not None:
            self._chk_hint_pair(hints, validhints, B)
        corr = torch.einsum('aijk,aijh->ajkh', fmap2, fmap3).reshape(B, H4, W2, 1, W3).contiguous()
        corr = corr / torch.sqrt(torch.tensor(Dc).float())
        if corr.dtype != dtype:
            raise RuntimeError(f"raft_corr: torch returned {corr.dtype} for {dtype} maps")
        if hints is not None:
            self._bind_stream()
            _lib.check(self.lib.vppx_raft_corr_modulate_dt_dev(self.ctx.handle, _ptr(corr), _ptr(hints), _ptr(validhints), B, H4,
                                                               W2, W3, int(hints.shape[2]), int(hints.shape[3]), dt))
        return corr

    def raft_corr_modulate_(self, corr, hints, validhints):
        """In-place hint modulation of an existing correlation volume [B,H4,W2,1,W3], float32 or bfloat16
        (corr.py:160-178)."""
        dtype, dt = self._handoff_dtype(corr)
        self._chk(corr, dtype, 5, "corr")
        B, H4, W2, one, W3 = corr.shape
        if one != 1:
            raise ValueError("corr must be [B,H4,W2,1,W3]")
        self._chk_hint_pair(hints, validhints, B)
        self._bind_stream()
        _lib.check(self.lib.vppx_raft_corr_modulate_dt_dev(self.ctx.handle, _ptr(corr), _ptr(hints), _ptr(validhints), B, H4, W2,
                                                           W3, int(hints.shape[2]), int(hints.shape[3]), dt))
        return corr

    def _corr_offsets(self, N, W3, levels):
        """(cells of levels 1.., [first cell of level i]) from the library; its refusals raise."""
        off = (C.c_int64 * _lib.CORR_MAX_LEVELS)()
        cells = self.lib.vppx_raft_corr_pyramid_cells(N, W3, levels, off)
        if cells < 0:
            _lib.check(int(cells))
        return int(cells), list(off)[:levels]

    def raft_corr_pyramid(self, corr, hints=None, validhints=None, num_levels=4):
        """CorrBlock1D.__init__ after the GEMM (models/raft_stereo/corr.py:117-124): the hint modulation of `corr`
        [B,H4,W2,1,W3] (float32 or bfloat16) in place, when hints are given, and the avg_pool2d pyramid, in one pass over
        the volume.  -> list of `num_levels` tensors [N,1,1,W3 >> i], N = B*H4*W2: entry 0 is `corr` itself, the others
        are views into one buffer (include/vppx.h has the arithmetic)."""
        torch = self.torch
        dtype, dt = self._handoff_dtype(corr)
        self._chk(corr, dtype, 5, "corr")
        B, H4, W2, one, W3 = corr.shape
        if one != 1:
            raise ValueError("corr must be [B,H4,W2,1,W3]")
        H = W = 0
        if hints is not None:
            self._chk_hint_pair(hints, validhints, B)
            H, W = hints.shape[2:]
        levels, N = int(num_levels), B * H4 * W2
        cells, off = self._corr_offsets(N, W3, levels)
        pyr = torch.empty((cells,), dtype=dtype, device=self.device) if levels > 1 else None
        self._bind_stream()
        _lib.check(self.lib.vppx_raft_corr_pyramid_dt_dev(self.ctx.handle, _ptr(corr), _ptr(hints) if hints is not None else None,
                                                          _ptr(validhints) if hints is not None else None, B, H4, W2, W3,
                                                          int(H), int(W), levels, _ptr(pyr) if pyr is not None else None, dt))
        out = [corr.view(N, 1, 1, W3)]
        for i in range(1, levels):
            Wi = W3 >> i
            out.append(pyr[off[i]:off[i] + N * Wi].view(N, 1, 1, Wi))
        return out

    def raft_corr_fused(self, fmap2, fmap3, hints=None, validhints=None, num_levels=4):
        """CorrBlock1D's GEMM, / sqrt(D), hint modulation and pyramid (models/raft_stereo/corr.py:151-155, 116-124) in one
        launch on the matrix cores: the feature maps [B,D,H4,W2] / [B,D,H4,W3] (float32 or bfloat16, both the same) are
        read, the levels are written, the volume is never read back.  The division is one IEEE division and a bfloat16
        cell is the float32 result rounded once (include/vppx.h).  -> the list raft_corr_pyramid returns: entry 0 is
        [N,1,1,W3], N = B*H4*W2, the others are views into one buffer."""
        torch = self.torch
        dtype, dt = self._handoff_dtype(fmap2)
        if getattr(fmap3, "dtype", None) in (torch.float32, torch.bfloat16) and fmap3.dtype != dtype:
            raise ValueError("feature maps must have the same dtype (float32 or bfloat16)")
        self._chk(fmap2, dtype, 4, "fmap2")
        self._chk(fmap3, dtype, 4, "fmap3")
        B, Dc, H4, W2 = fmap2.shape
        if fmap3.shape[:3] != fmap2.shape[:3]:
            raise ValueError("fmap2 / fmap3 must be [B,D,H4,W2] / [B,D,H4,W3]")
        W3 = fmap3.shape[3]
        H = W = 0
        if hints is not None:
            self._chk_hint_pair(hints, validhints, B)
            H, W = hints.shape[2:]
        levels, N = int(num_levels), B * H4 * W2
        cells, off = self._corr_offsets(N, W3, levels)
        corr = torch.empty((N, 1, 1, W3), dtype=dtype, device=self.device)
        pyr = torch.empty((cells,), dtype=dtype, device=self.device) if levels > 1 else None
        self._bind_stream()
        _lib.check(self.lib.vppx_raft_corr_fused_dt_dev(self.ctx.handle, _ptr(fmap2), _ptr(fmap3),
                                                        _ptr(hints) if hints is not None else None,
                                                        _ptr(validhints) if hints is not None else None, B, Dc, H4, W2, W3,
                                                        int(H), int(W), levels, _ptr(corr), _ptr(pyr) if pyr is not None else None, dt))
        out = [corr]
        for i in range(1, levels):
            Wi = W3 >> i
            out.append(pyr[off[i]:off[i] + N * Wi].view(N, 1, 1, Wi))
        return out

    def raft_corr_lookup(self, pyramid, coords, radius=4, out=None):
        """CorrBlock1D.__call__ (corr.py:126-145) in one launch: `pyramid` is what raft_corr_pyramid returned, `coords`
        float32 [B,2,H4,W2] (channel 0 is read, as the reference does) or [B,H4,W2].  -> float32
        [B, levels*(2*radius+1), H4, W2]."""
        torch = self.torch
        _, dt, levels, N, W3, B, ch, H4, W2 = self._chk_pyramid(pyramid, coords)
        shape = (B, levels * (2 * int(radius) + 1), H4, W2)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        else:
            self._chk(out, torch.float32, 4, "out", shape)
        self._bind_stream()
        _lib.check(self.lib.vppx_raft_corr_lookup_dt_dev(self.ctx.handle, _ptr(pyramid[0]), _ptr(pyramid[1]) if levels > 1 else None,
                                                         _ptr(coords), ch * H4 * W2, B, H4, W2, W3, levels, int(radius), _ptr(out), dt))
        return out

    def _chk_pyramid(self, pyramid, coords):
        """What raft_corr_lookup checks of its pyramid and coordinates -> (dtype, dt, levels, N, W3, B, ch, H4, W2)."""
        torch = self.torch
        levels = len(pyramid)
        if levels < 1:
            raise ValueError("pyramid: no levels")
        dtype, dt = self._handoff_dtype(pyramid[0])
        self._chk(pyramid[0], dtype, 4, "pyramid[0]")
        N, W3 = pyramid[0].shape[0], pyramid[0].shape[3]
        if coords.dim() == 4:
            self._chk(coords, torch.float32, 4, "coords")
            B, ch, H4, W2 = coords.shape
            if ch != 2:
                raise ValueError("coords must be [B,2,H4,W2] or [B,H4,W2]")
        else:
            self._chk(coords, torch.float32, 3, "coords")
            (B, H4, W2), ch = coords.shape, 1
        if B * H4 * W2 != N:
            raise ValueError(f"coords are {tuple(coords.shape)}: the pyramid has {N} rows, not {B * H4 * W2}")
        _, off = self._corr_offsets(N, W3, levels)
        for i in range(1, levels):      # the library takes one pointer for levels 1..: they must lie where it expects them
            self._chk(pyramid[i], dtype, 4, f"pyramid[{i}]", (N, 1, 1, W3 >> i))
            if pyramid[i].data_ptr() != pyramid[1].data_ptr() + off[i] * pyramid[i].element_size():
                raise ValueError("pyramid: levels 1.. must be the views raft_corr_pyramid returned")
        return dtype, dt, levels, N, W3, B, ch, H4, W2

    def raft_motion_front(self, pyramid, coords, flow, convc1_weight, convc1_bias, convf1_weight, convf1_bias, radius=4, out_dtype=None,
                          out=None):
        """The front of BasicMotionEncoder.forward (models/raft_stereo/update.py:80,82) in one launch:
        cor1 = relu(convc1(lookup(pyramid, coords))) and flo1 = relu(convf1(flow)); the tensor of taps between the lookup
        and convc1 is never written.  `pyramid`, `coords` and `radius` are raft_corr_lookup's; `flow` is float32
        [B,2,H4,W2]; the weights are float32 [Cc, levels*(2*radius+1), 1, 1] and [Cf, 2, ks, ks], the biases float32 [Cc] /
        [Cf] or None.  `out_dtype`: torch.float32 (the default) or torch.bfloat16; `out`: a pair of tensors [B,Cc,H4,W2] and
        [B,Cf,H4,W2] to write, which may be channel slices of one buffer.  -> (cor1, flo1) (include/vppx.h has the
        arithmetic)."""
        torch = self.torch
        _, dt, levels, N, W3, B, ch, H4, W2 = self._chk_pyramid(pyramid, coords)
        self._chk(flow, torch.float32, 4, "flow", (B, 2, H4, W2))
        K = levels * (2 * int(radius) + 1)
        self._chk(convc1_weight, torch.float32, 4, "convc1_weight")
        Cc = convc1_weight.shape[0]
        if tuple(convc1_weight.shape[1:]) != (K, 1, 1):
            raise ValueError(f"convc1_weight: expected [Cc,{K},1,1] for {levels} levels of radius {int(radius)}, got {tuple(convc1_weight.shape)}")
        self._chk(convf1_weight, torch.float32, 4, "convf1_weight")
        Cf, cin, ks, kw = convf1_weight.shape
        if cin != 2 or ks != kw:
            raise ValueError(f"convf1_weight: expected [Cf,2,ks,ks], got {tuple(convf1_weight.shape)}")
        if convc1_bias is not None:
            self._chk(convc1_bias, torch.float32, 1, "convc1_bias", (Cc,))
        if convf1_bias is not None:
            self._chk(convf1_bias, torch.float32, 1, "convf1_bias", (Cf,))
        if out is None:
            odtype = torch.float32 if out_dtype is None else out_dtype
        else:
            if len(out) != 2:
                raise ValueError("out must be the pair (cor1, flo1)")
            odtype = out[0].dtype if out_dtype is None else out_dtype
        if odtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"out_dtype must be torch.float32 or torch.bfloat16, not {odtype}")
        if out is None:
            out_c = torch.empty((B, Cc, H4, W2), dtype=odtype, device=self.device)
            out_f = torch.empty((B, Cf, H4, W2), dtype=odtype, device=self.device)
        else:
            out_c, out_f = out
        sc = self._chk_frames(out_c, odtype, "out[0]", (B, Cc, H4, W2))
        sf = self._chk_frames(out_f, odtype, "out[1]", (B, Cf, H4, W2))
        self._bind_stream()
        _lib.check(self.lib.vppx_raft_motion_front_dt_dev(
            self.ctx.handle, _ptr(pyramid[0]), _ptr(pyramid[1]) if levels > 1 else None, _ptr(coords), ch * H4 * W2, _ptr(flow), 2 * H4 * W2,
            _ptr(convc1_weight), _ptr(convc1_bias), Cc, _ptr(convf1_weight), _ptr(convf1_bias), Cf, ks, B, H4, W2, W3, levels, int(radius),
            _ptr(out_c), sc, _ptr(out_f), sf, dt, _lib.DT_BF16 if odtype == torch.bfloat16 else _lib.DT_F32))
        return out_c, out_f

    # ---- the read-out: the networks' output back as a disparity map ----
    @staticmethod
    def _window(H, W, crop):
        """test.py's `_pad` list [left, right, top, bottom] (:194, :242-245) -> (top, left, Hout, Wout) of the H x W map."""
        if crop is None:
            return 0, 0, H, W
        if len(crop) != 4 or any(int(c) != c or c < 0 for c in crop):
            raise ValueError("crop must be [left, right, top, bottom], four integers >= 0")
        left, right, top, bottom = (int(c) for c in crop)
        if top + bottom >= H or left + right >= W:
            raise ValueError(f"crop {list(crop)} leaves nothing of a {H}x{W} map")
        return top, left, H - top - bottom, W - left - right

    def psmnet_disparity(self, cost, maxdisp, size, crop=None, out=None):
        """What PSMNet.forward does with cost3 (models/psmnet/psmnet.py:227-233, submodule.py:115-128) and test.py:242-245
        with the result, in one launch: trilinear upsampling to [maxdisp, H, W] = [maxdisp, *size], softmax over the
        disparities, the regression sum d * p_d, and the crop.  cost: [B,1,D4,H4,W4] or [B,D4,H4,W4], float32 or bfloat16;
        crop: test.py's `_pad` list [left, right, top, bottom] or None.  -> float32 [B,Hout,Wout], which `guided_metrics`,
        `error_colors` and `colorize` take as it is (include/vppx.h has the arithmetic)."""
        torch = self.torch
        dtype, dt = self._handoff_dtype(cost)
        if getattr(cost, "dim", lambda: 0)() == 5:
            self._chk(cost, dtype, 5, "cost")
            if cost.shape[1] != 1:
                raise ValueError("cost must be [B,1,D4,H4,W4] or [B,D4,H4,W4]")
            B, _, D4, H4, W4 = cost.shape
        else:
            self._chk(cost, dtype, 4, "cost")
            B, D4, H4, W4 = cost.shape
        if len(size) != 2:
            raise ValueError("size must be (H, W)")
        H, W = int(size[0]), int(size[1])
        if min(B, D4, H4, W4) < 1 or int(maxdisp) < 1 or H < 1 or W < 1:
            raise ValueError("cost, maxdisp and size must not be empty")
        top, left, Ho, Wo = self._window(H, W, crop)
        if out is None:
            out = torch.empty((B, Ho, Wo), dtype=torch.float32, device=self.device)
        else:
            self._chk(out, torch.float32, 3, "out", (B, Ho, Wo))
        self._bind_stream()
        _lib.check(self.lib.vppx_psmnet_readout_dt_dev(self.ctx.handle, _ptr(cost), B, D4, H4, W4, int(maxdisp), H, W, top, left, Ho,
                                                       Wo, _ptr(out), dt))
        return out

    def raft_upsample(self, flow, mask, n_downsample=2, negate=False, channels=None, crop=None, out=None):
        """RAFTStereo.upsample_flow (models/raft_stereo/raft_stereo.py:69-81) in one launch, with what follows it folded in:
        `channels=1` is the slice [:, :1] of :154 (the other channels are not read), `negate` the sign of test.py:238, `crop`
        test.py's `_pad` list [left, right, top, bottom] (:242-245).  flow [B,C,H4,W4] and mask [B,9*f*f,H4,W4], f =
        2**n_downsample, float32 or bfloat16 (both the same).  -> float32 [B,channels,Hout,Wout]; with the defaults
        [B,C,f*H4,f*W4], the reference's result."""
        torch = self.torch
        dtype, dt = self._handoff_dtype(flow)
        if getattr(mask, "dtype", None) in (torch.float32, torch.bfloat16) and mask.dtype != dtype:
            raise ValueError("flow and mask must have the same dtype (float32 or bfloat16)")
        self._chk(flow, dtype, 4, "flow")
        B, Cf, H4, W4 = flow.shape
        if int(n_downsample) not in (0, 1, 2, 3):
            raise ValueError("n_downsample must be 0, 1, 2 or 3")
        f = 2 ** int(n_downsample)
        self._chk(mask, dtype, 4, "mask", (B, 9 * f * f, H4, W4))
        Cc = Cf if channels is None else int(channels)
        if not 1 <= Cc <= Cf or min(B, H4, W4) < 1:
            raise ValueError(f"channels must be 1 .. {Cf} of a flow that is not empty")
        top, left, Ho, Wo = self._window(f * H4, f * W4, crop)
        if out is None:
            out = torch.empty((B, Cc, Ho, Wo), dtype=torch.float32, device=self.device)
        else:
            self._chk(out, torch.float32, 4, "out", (B, Cc, Ho, Wo))
        self._bind_stream()
        _lib.check(self.lib.vppx_raft_upsample_dt_dev(self.ctx.handle, _ptr(flow), Cf * H4 * W4, _ptr(mask), B, Cc, H4, W4, f, 9 * f * f,
                                                      -1 if negate else 1, top, left, Ho, Wo, _ptr(out), dt))
        return out

    # ---- the update block's glue: what BasicMultiUpdateBlock.forward runs between its convolutions ----
    def _chk_frames(self, t, dtype, name, shape=None):
        """A [B,C,H,W] tensor whose frames are contiguous and lie a frame stride apart (a channel slice of a wider
        tensor, as `.split(dim=1)` returns, or a contiguous tensor) -> the frame stride in cells."""
        if getattr(t, "device", None) != self.device or t.dtype != dtype or t.dim() != 4:
            raise ValueError(f"{name}: expected a {dtype} tensor with 4 dims on {self.device}")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
        B, Cc, H, W = t.shape
        if min(B, Cc, H, W) < 1:
            raise ValueError(f"{name}: empty tensor {tuple(t.shape)}")
        want = (Cc * H * W, H * W, W, 1)
        st = t.stride()
        if any(t.shape[d] > 1 and st[d] != want[d] for d in (1, 2, 3)) or (B > 1 and st[0] < want[0]):
            raise ValueError(f"{name}: every frame must be contiguous (strides {tuple(st)} of shape {tuple(t.shape)})")
        return int(st[0]) if B > 1 else want[0]

    def raft_gru_assemble(self, sources, out=None):
        """hx = torch.cat(sources, dim=1) for a ConvGRU (models/raft_stereo/update.py:24-25) in one launch.  `sources`:
        up to four (tensor, mode); mode "copy" takes the tensor [B,C,H,W] as it is, "pool2x" is update.py's pool2x
        (avg_pool2d(3, stride=2, padding=1)) and "interp" its interp (bilinear, align_corners=True) to the H x W of the
        result, which a copied source or `out` fixes.  float32 or bfloat16, all the same; every tensor may be a channel
        slice of a wider one.  -> contiguous [B, sum C_i, H, W]; with `out` nothing is allocated, and an `out` of more
        channels keeps the others (include/vppx.h has the arithmetic).  `out` may itself be a channel slice of a wider tensor
        whose frames are contiguous (vppx_raft_gru_assemble_strided_dt_dev): the cells of the wider tensor outside the
        sources' channels are not written."""
        torch = self.torch
        sources = list(sources)
        if not 1 <= len(sources) <= _lib.GRU_MAX_SOURCES:
            raise ValueError(f"sources: {len(sources)} given, 1 .. {_lib.GRU_MAX_SOURCES} are taken")
        dtype, dt = self._handoff_dtype(sources[0][0])
        arr = (_lib.VppxGruSource * len(sources))()
        size, total = None, 0
        for k, (t, mode) in enumerate(sources):
            if mode not in _lib.GRU_MODES:
                raise ValueError(f"sources[{k}]: unknown mode {mode!r} (one of {tuple(_lib.GRU_MODES)})")
            stride = self._chk_frames(t, dtype, f"sources[{k}]")
            if t.shape[0] != sources[0][0].shape[0]:
                raise ValueError(f"sources[{k}]: {t.shape[0]} frames, sources[0] has {sources[0][0].shape[0]}")
            arr[k] = _lib.VppxGruSource(t.data_ptr(), stride, t.shape[1], t.shape[2], t.shape[3], _lib.GRU_MODES[mode])
            total += t.shape[1]
            if mode == "copy" and size is None:
                size = tuple(t.shape[2:])
        B = sources[0][0].shape[0]
        if out is None:
            if size is None:
                raise ValueError("sources: no copied source fixes the size of hx; pass out=")
            out = torch.empty((B, total) + size, dtype=dtype, device=self.device)
        elif not out.is_contiguous():
            so = self._chk_frames(out, dtype, "out")
            if out.shape[0] != B or out.shape[1] < total:
                raise ValueError(f"out: expected [{B},>={total},H,W], got {tuple(out.shape)}")
            self._bind_stream()
            _lib.check(self.lib.vppx_raft_gru_assemble_strided_dt_dev(arr, len(sources), B, out.shape[2], out.shape[3], _ptr(out), so, dt,
                                                                      self.ctx.handle))
            return out
        else:
            self._chk(out, dtype, 4, "out")
            if out.shape[0] != B:
                raise ValueError(f"out: {out.shape[0]} frames, the sources have {B}")
        self._bind_stream()
        _lib.check(self.lib.vppx_raft_gru_assemble_dt_dev(self.ctx.handle, arr, len(sources), B, out.shape[2], out.shape[3], _ptr(out),
                                                          out.shape[1], dt))
        return out

    def raft_gru_reset(self, ar, cr, h, hx):
        """r = sigmoid(ar + cr), then r * h over the first C channels of `hx` [B,>=C,H,W], IN PLACE (ConvGRU.forward,
        update.py:28-29): `ar` is convr(hx), `cr` the context's share, `h` [B,C,H,W] the hidden state itself.  The z and
        r convolutions must have read hx by then (stream order); convq then reads the same buffer as cat([r*h, x]).
        -> hx."""
        dtype, dt = self._handoff_dtype(h)
        sh = self._chk_frames(h, dtype, "h")
        B, Cc, H, W = h.shape
        sa = self._chk_frames(ar, dtype, "ar", h.shape)
        sc = self._chk_frames(cr, dtype, "cr", h.shape)
        sx = self._chk_frames(hx, dtype, "hx")
        if hx.shape[0] != B or tuple(hx.shape[2:]) != (H, W):
            raise ValueError(f"hx: expected [{B},>={Cc},{H},{W}], got {tuple(hx.shape)}")
        self._bind_stream()
        _lib.check(self.lib.vppx_raft_gru_reset_dt_dev(self.ctx.handle, _ptr(ar), sa, _ptr(cr), sc, _ptr(h), sh, _ptr(hx), sx, B, Cc, H, W,
                                                       hx.shape[1], dt))
        return hx

    def raft_gru_update(self, az, cz, aq, cq, h, out=None):
        """z = sigmoid(az + cz), q = tanh(aq + cq), -> (1 - z) * h + z * q (ConvGRU.forward, update.py:27-31): `az`
        and `aq` are convz's and convq's outputs, `cz` and `cq` the context's shares.  `out` may be `h`."""
        dtype, dt = self._handoff_dtype(h)
        sh = self._chk_frames(h, dtype, "h")
        B, Cc, H, W = h.shape
        s = [self._chk_frames(t, dtype, n, h.shape) for t, n in ((az, "az"), (cz, "cz"), (aq, "aq"), (cq, "cq"))]
        if out is None:
            out = self.torch.empty(tuple(h.shape), dtype=dtype, device=self.device)
        so = self._chk_frames(out, dtype, "out", h.shape)
        self._bind_stream()
        _lib.check(self.lib.vppx_raft_gru_update_dt_dev(self.ctx.handle, _ptr(az), s[0], _ptr(cz), s[1], _ptr(aq), s[2], _ptr(cq), s[3],
                                                        _ptr(h), sh, _ptr(out), so, B, Cc, H, W, dt))
        return out

    # ---- the 3x3 convolution on the matrix cores, and ConvGRU's gates as its epilogues ----
    def raft_conv3x3_pack(self, weight, bias=None, dtype=None):
        """The weights [Cout,Cin,3,3] (and bias [Cout]) of an nn.Conv2d(Cin, Cout, 3, padding=1) in the layout the convolution
        kernel reads, for activations stored as `dtype` (torch.float32, the default, or torch.bfloat16: the weights are then
        rounded to bfloat16 once).  -> an opaque torch.uint8 device tensor; pack once per module, it serves any B, H, W."""
        return self._conv_pack(weight, bias, dtype, (3,), _OUT_16, self.lib.vppx_raft_conv3x3_pack_dev)

    def _conv_pack(self, weight, bias, dtype, ksizes, rule, pack_dev):
        """raft_conv3x3_pack and raft_conv_pack: the kernel sizes and the rule for the channels each takes, and its C entry."""
        torch = self.torch
        dtype = torch.float32 if dtype is None else dtype
        if dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"dtype is {dtype}; the kernels store float32 and bfloat16")
        dt = _lib.DT_BF16 if dtype == torch.bfloat16 else _lib.DT_F32
        if (getattr(weight, "device", None) != self.device or weight.dim() != 4 or weight.shape[2] != weight.shape[3]
                or weight.shape[2] not in ksizes):
            want = "[Cout,Cin,3,3] tensor" if ksizes == (3,) else "[Cout,Cin,k,k] tensor with k 1 or 3"
            raise ValueError(f"weight: expected a {want} on {self.device}")
        Cout, Cin, ksize = int(weight.shape[0]), int(weight.shape[1]), int(weight.shape[2])
        weight = weight.detach().to(torch.float32).contiguous()
        if bias is not None:
            bias = bias.detach().to(torch.float32).contiguous()
            self._chk(bias, torch.float32, 1, "bias", (Cout,))
        size = self._packed_bytes(rule, Cout, Cin, ksize, dt)
        if size == 0:
            raise ValueError(f"weight: {Cin} -> {Cout} channels: {_conv_built(rule)}")
        packed = torch.empty((size,), dtype=torch.uint8, device=self.device)
        self._bind_stream()
        shape = (Cout, Cin, ksize) if rule is _OUT_ANY else (Cout, Cin)
        _lib.check(pack_dev(_ptr(weight), _ptr(bias), *shape, dt, _ptr(packed), self.ctx.handle))
        return packed

    def _packed_bytes(self, rule, cout, cin, ksize, dt):
        """vppx_raft_conv3x3_packed_bytes (_OUT_16, ksize 3) or vppx_raft_conv_packed_bytes (_OUT_ANY), asked once per key: host
        arithmetic on constants."""
        key = (rule, cout, cin, ksize, dt)
        if key not in self._conv_sizes:
            self._conv_sizes[key] = int(self.lib.vppx_raft_conv_packed_bytes(cout, cin, ksize, dt) if rule is _OUT_ANY else
                                        self.lib.vppx_raft_conv3x3_packed_bytes(cout, cin, dt))
        return self._conv_sizes[key]

    def _chk_conv(self, rule, x0, x1, packed, cout, ksize=3):
        """The sources and the packed weights of a convolution call -> (dtype, dt, B, H, W, s0, C0, s1, C1).  _OUT_16: the 3x3
        calls that take multiples of 16 output channels; _OUT_ANY: raft_conv, ksize 1 or 3."""
        torch = self.torch
        dtype, dt = self._norm_dtype(x0, "x0")
        s0 = self._chk_frames(x0, dtype, "x0")
        B, C0, H, W = x0.shape
        s1, C1 = 0, 0
        if x1 is not None:
            s1 = self._chk_frames(x1, dtype, "x1")
            C1 = x1.shape[1]
            if (x1.shape[0], x1.shape[2], x1.shape[3]) != (B, H, W):
                raise ValueError(f"x1: expected [{B},C1,{H},{W}], got {tuple(x1.shape)}")
        if getattr(packed, "device", None) != self.device or packed.dtype != torch.uint8 or packed.dim() != 1 or not packed.is_contiguous():
            raise ValueError(f"packed: expected what raft_conv3x3_pack returns, a torch.uint8 vector on {self.device}")
        want = self._packed_bytes(rule, int(cout), C0 + C1, ksize, dt)
        if want == 0 or packed.numel() != want:
            built = ("kernel sizes 1 and 3, " if rule is _OUT_ANY else "") + _conv_built(rule)
            raise ValueError(f"packed: {packed.numel()} bytes; {C0 + C1} -> {cout} channels of {dtype} take {want or 'no'} bytes ({built})")
        return dtype, dt, B, H, W, s0, C0, s1, C1

    def raft_conv3x3(self, x0, packed, cout, x1=None, relu=False, out=None):
        """conv(cat([x0, x1], dim=1)) of an nn.Conv2d(C0 + C1, cout, 3, padding=1) whose weights `packed` holds
        (raft_conv3x3_pack, for the dtype of x0), with its bias and, with `relu`, torch's ReLU.  x0 [B,C0,H,W] and x1
        [B,C1,H,W] or None are float32 or bfloat16 and may be channel slices of wider tensors.  -> [B,cout,H,W]; with `out`
        nothing is allocated (include/vppx.h has the arithmetic)."""
        return self._conv_plain(_OUT_16, x0, x1, packed, cout, 3, 1, relu, 1.0, out)

    def _conv_plain(self, rule, x0, x1, packed, cout, ksize, stride, relu, scale, out):
        """raft_conv3x3 (_OUT_16: vppx_raft_conv3x3_dt_dev) and raft_conv (_OUT_ANY: vppx_raft_conv_dt_dev at stride 1,
        vppx_raft_conv_strided_dt_dev at stride 2)."""
        dtype, dt, B, H, W, s0, C0, s1, C1 = self._chk_conv(rule, x0, x1, packed, cout, ksize)
        cout, stride, relu = int(cout), int(stride), int(bool(relu))
        if stride not in (1, 2):
            raise ValueError(f"stride is {stride}; 1 and 2 are built")
        shape = (B, cout, (H - 1) // stride + 1, (W - 1) // stride + 1)
        if out is None:
            out = self.torch.empty(shape, dtype=dtype, device=self.device)
        so = self._chk_frames(out, dtype, "out", shape)
        self._bind_stream()
        lib, ctx, p0, p1, pw, po = self.lib, self.ctx.handle, _ptr(x0), _ptr(x1), _ptr(packed), _ptr(out)
        if rule is _OUT_16:
            rc = lib.vppx_raft_conv3x3_dt_dev(p0, s0, C0, p1, s1, C1, pw, cout, B, H, W, relu, po, so, dt, ctx)
        elif stride == 1:
            rc = lib.vppx_raft_conv_dt_dev(p0, s0, C0, p1, s1, C1, pw, cout, ksize, B, H, W, relu, float(scale), po, so, dt, ctx)
        else:
            rc = lib.vppx_raft_conv_strided_dt_dev(p0, s0, C0, p1, s1, C1, pw, cout, ksize, stride, B, H, W, relu, float(scale), po, so, dt, ctx)
        _lib.check(rc)
        return out

    def raft_conv_pack(self, weight, bias=None, dtype=None):
        """raft_conv3x3_pack for raft_conv: the weights [Cout,Cin,k,k], k 1 or 3, of an nn.Conv2d(Cin, Cout, k, padding=k // 2) with
        any Cout from 1 to CONV_MAX_COUT (Cin a multiple of 16).  -> an opaque torch.uint8 device tensor; for k = 3 and a Cout that is a
        multiple of 16, the bytes raft_conv3x3_pack makes."""
        return self._conv_pack(weight, bias, dtype, (1, 3), _OUT_ANY, self.lib.vppx_raft_conv_pack_dev)

    def raft_conv(self, x0, packed, cout, ksize, x1=None, relu=False, scale=1.0, out=None, stride=1):
        """conv(cat([x0, x1], dim=1)) of an nn.Conv2d(C0 + C1, cout, ksize, stride=stride, padding=ksize // 2), ksize 1 or 3, stride 1
        or 2, whose weights `packed` holds (raft_conv_pack, for the dtype of x0; the same buffer serves either stride): + bias, with
        `relu` torch's ReLU, then * scale (one float32 multiplication; 1.0 changes no bit).  cout is any count from 1 on; x0, x1 and
        `out` may be channel slices of wider tensors, and no cell of `out`'s buffer outside its cout channels is written.
        -> [B,cout,Ho,Wo] with Ho = (H - 1) // stride + 1, Wo likewise; with `out` nothing is allocated."""
        return self._conv_plain(_OUT_ANY, x0, x1, packed, cout, int(ksize), stride, relu, scale, out)

    def conv2d(self, x0, packed, cout, ksize, x1=None, stride=1, dilation=1, residual=None, relu=False, scale=1.0, out=None):
        """raft_conv with a dilation and a residual (vppx_conv2d_dt_dev; PSMNet's feature_extraction with its BatchNorm folded):
        nn.Conv2d(C0 + C1, cout, ksize, stride=stride, padding=dilation * (ksize // 2), dilation=dilation) on cat([x0, x1], dim=1),
        + bias, + `residual` [B,cout,Ho,Wo] where there is one, with `relu` torch's ReLU, then * scale.  Dilation 1 takes what
        raft_conv takes, dilation 2 goes with stride 1.  `packed` is raft_conv_pack's.  `out` may be `residual` itself; every
        tensor may be a channel slice of a wider one.  -> [B,cout,Ho,Wo]; with `out` nothing is allocated."""
        ksize, cout, stride, dilation, relu = int(ksize), int(cout), int(stride), int(dilation), int(bool(relu))
        dtype, dt, B, H, W, s0, C0, s1, C1 = self._chk_conv(_OUT_ANY, x0, x1, packed, cout, ksize)
        if stride not in (1, 2):
            raise ValueError(f"stride is {stride}; 1 and 2 are built")
        if dilation not in (1, 2) or (dilation == 2 and stride == 2):
            raise ValueError(f"dilation is {dilation} at stride {stride}; dilation 1, and dilation 2 at stride 1, are built")
        shape = (B, cout, (H - 1) // stride + 1, (W - 1) // stride + 1)
        sr = 0 if residual is None else self._chk_frames(residual, dtype, "residual", shape)
        if out is None:
            out = self.torch.empty(shape, dtype=dtype, device=self.device)
        so = self._chk_frames(out, dtype, "out", shape)
        self._bind_stream()
        _lib.check(self.lib.vppx_conv2d_dt_dev(_ptr(x0), s0, C0, _ptr(x1), s1, C1, _ptr(packed), cout, ksize, stride, dilation, B, H, W,
                                               _ptr(residual), sr, relu, float(scale), _ptr(out), so, dt, self.ctx.handle))
        return out

    # ---- the stride-1 3x3x3 convolution: the same kernel over 3 Cin pseudo-channels (include/vppx.h) ----
    def _conv3d_bytes(self, cout, cin, dt):
        key = ("3d", cout, cin, 3, dt)
        if key not in self._conv_sizes:
            self._conv_sizes[key] = int(self.lib.vppx_conv3d_packed_bytes(cout, cin, dt))
        return self._conv_sizes[key]

    @staticmethod
    def _conv3d_built():
        return (f"multiples of 16 up to {_lib.CONV_MAX_CIN // 48 * 16} in (3 x Cin up to {_lib.CONV_MAX_CIN}) and 1 to {_lib.CONV_MAX_COUT} "
                "out are built")

    def conv3d_pack(self, weight, bias=None, dtype=None):
        """The weights [Cout,Cin,3,3,3] (and bias [Cout]) of an nn.Conv3d(Cin, Cout, 3, stride=1, padding=1) in the layout the
        convolution kernel reads, for activations stored as `dtype` (torch.float32, the default, or torch.bfloat16: the weights are
        then rounded to bfloat16 once).  Cin is a multiple of 16 with 3 * Cin up to CONV_MAX_CIN, Cout any count from 1 to
        CONV_MAX_COUT.  -> an opaque torch.uint8 device tensor, the bytes raft_conv_pack makes for the [Cout,3*Cin,3,3] weight
        weight.permute(0, 2, 1, 3, 4).reshape(Cout, 3 * Cin, 3, 3); pack once per module, it serves any B, D, H, W."""
        torch = self.torch
        dtype = torch.float32 if dtype is None else dtype
        if dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"dtype is {dtype}; the kernels store float32 and bfloat16")
        dt = _lib.DT_BF16 if dtype == torch.bfloat16 else _lib.DT_F32
        if getattr(weight, "device", None) != self.device or weight.dim() != 5 or tuple(weight.shape[2:]) != (3, 3, 3):
            raise ValueError(f"weight: expected a [Cout,Cin,3,3,3] tensor on {self.device}")
        Cout, Cin = int(weight.shape[0]), int(weight.shape[1])
        weight = weight.detach().to(torch.float32).contiguous()
        if bias is not None:
            bias = bias.detach().to(torch.float32).contiguous()
            self._chk(bias, torch.float32, 1, "bias", (Cout,))
        size = self._conv3d_bytes(Cout, Cin, dt)
        if size == 0:
            raise ValueError(f"weight: {Cin} -> {Cout} channels: {self._conv3d_built()}")
        packed = torch.empty((size,), dtype=torch.uint8, device=self.device)
        self._bind_stream()
        _lib.check(self.lib.vppx_conv3d_pack_dev(_ptr(weight), _ptr(bias), Cout, Cin, dt, _ptr(packed), self.ctx.handle))
        return packed

    def _chk_volumes(self, t, dtype, name, shape=None):
        """_chk_frames for a [B,C,D,H,W] tensor: every frame contiguous, the frames a frame stride apart -> that stride in cells."""
        if getattr(t, "device", None) != self.device or t.dtype != dtype or t.dim() != 5:
            raise ValueError(f"{name}: expected a {dtype} tensor with 5 dims on {self.device}")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
        B, Cc, D, H, W = t.shape
        if min(B, Cc, D, H, W) < 1:
            raise ValueError(f"{name}: empty tensor {tuple(t.shape)}")
        want = (Cc * D * H * W, D * H * W, H * W, W, 1)
        st = t.stride()
        if any(t.shape[d] > 1 and st[d] != want[d] for d in (1, 2, 3, 4)) or (B > 1 and st[0] < want[0]):
            raise ValueError(f"{name}: every frame must be contiguous (strides {tuple(st)} of shape {tuple(t.shape)})")
        return int(st[0]) if B > 1 else want[0]

    def conv3d(self, x, packed, cout, residual=None, relu=False, scale=1.0, out=None):
        """nn.Conv3d(Cin, cout, 3, stride=1, padding=1) on x [B,Cin,D,H,W] (vppx_conv3d_dt_dev; PSMNet's stride-1 3-D convolutions
        with their BatchNorm3d folded): + bias, + `residual` [B,cout,D,H,W] where there is one, with `relu` torch's ReLU, then
        * scale.  `packed` is conv3d_pack's, for the dtype of x (float32 or bfloat16).  `out` may be `residual` itself; x, residual
        and out may be channel slices of wider tensors.  -> [B,cout,D,H,W]; with `out` nothing is allocated."""
        torch = self.torch
        cout, relu = int(cout), int(bool(relu))
        dtype, dt = self._norm_dtype(x, "x")
        sx = self._chk_volumes(x, dtype, "x")
        B, Cin, D, H, W = x.shape
        if getattr(packed, "device", None) != self.device or packed.dtype != torch.uint8 or packed.dim() != 1 or not packed.is_contiguous():
            raise ValueError(f"packed: expected what conv3d_pack returns, a torch.uint8 vector on {self.device}")
        want = self._conv3d_bytes(cout, Cin, dt)
        if want == 0 or packed.numel() != want:
            raise ValueError(f"packed: {packed.numel()} bytes; {Cin} -> {cout} channels of {dtype} take {want or 'no'} bytes ({self._conv3d_built()})")
        shape = (B, cout, D, H, W)
        sr = 0 if residual is None else self._chk_volumes(residual, dtype, "residual", shape)
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=self.device)
        so = self._chk_volumes(out, dtype, "out", shape)
        self._bind_stream()
        _lib.check(self.lib.vppx_conv3d_dt_dev(_ptr(x), sx, Cin, _ptr(packed), cout, B, D, H, W, _ptr(residual), sr, relu, float(scale),
                                               _ptr(out), so, dt, self.ctx.handle))
        return out

    def psm_spp_pool(self, x, ks=(8, 16, 32, 64)):
        """The average pools of PSMNet's pyramid pooling in one launch (vppx_psm_spp_pool_dt_dev): x [B,C,H,W], float32 or
        bfloat16, possibly a channel slice of a wider tensor, read once -> [nn.AvgPool2d((k, k), stride=(k, k))(x) for k in ks],
        each [B,C,H // k,W // k] contiguous (include/vppx.h has the arithmetic)."""
        dtype, dt = self._norm_dtype(x, "x")
        sx = self._chk_frames(x, dtype, "x")
        B, Cc, H, W = x.shape
        ks = [int(k) for k in ks]
        if not 1 <= len(ks) <= _lib.SPP_MAX_LEVELS:
            raise ValueError(f"ks: {len(ks)} levels, 1 .. {_lib.SPP_MAX_LEVELS} are taken")
        for k in ks:
            if not 1 <= k <= _lib.SPP_MAX_K or H // k == 0 or W // k == 0:
                raise ValueError(f"ks: a window of {k} over a {H}x{W} map: 1 .. {_lib.SPP_MAX_K} that leave a cell are taken")
        outs = [self.torch.empty((B, Cc, H // k, W // k), dtype=dtype, device=self.device) for k in ks]
        self._bind_stream()
        _lib.check(self.lib.vppx_psm_spp_pool_dt_dev(_ptr(x), sx, B, Cc, H, W, len(ks), (C.c_int * len(ks))(*ks),
                                                     (C.c_void_p * len(ks))(*[o.data_ptr() for o in outs]), dt, self.ctx.handle))
        return outs

    def raft_gru_zr(self, x0, packed_zr, cz, cr, h, x1=None, z=None, rh=None):
        """convz and convr of a ConvGRU (update.py:27-28) in one launch with their gates: `packed_zr` holds
        cat([convz.weight, convr.weight]) and the biases likewise; x0 (and x1) are hx = cat([h, *x]), usually the whole
        buffer raft_gru_assemble made.  -> (z, rh) = (sigmoid(convz(hx) + cz), sigmoid(convr(hx) + cr) * h), each [B,C,H,W].
        `rh` must be a buffer of its own, not the h part of hx."""
        Cc = h.shape[1]
        dtype, dt, B, H, W, s0, C0, s1, C1 = self._chk_conv(_OUT_16, x0, x1, packed_zr, 2 * Cc)
        shape = (B, Cc, H, W)
        sh = self._chk_frames(h, dtype, "h", shape)
        sz, sr = self._chk_frames(cz, dtype, "cz", shape), self._chk_frames(cr, dtype, "cr", shape)
        if z is None:
            z = self.torch.empty(shape, dtype=dtype, device=self.device)
        if rh is None:
            rh = self.torch.empty(shape, dtype=dtype, device=self.device)
        soz, sor = self._chk_frames(z, dtype, "z", shape), self._chk_frames(rh, dtype, "rh", shape)
        self._bind_stream()
        _lib.check(self.lib.vppx_raft_gru_zr_dt_dev(_ptr(x0), s0, C0, _ptr(x1), s1, C1, _ptr(packed_zr), _ptr(cz), sz, _ptr(cr), sr,
                                                    _ptr(h), sh, _ptr(z), soz, _ptr(rh), sor, B, Cc, H, W, dt, self.ctx.handle))
        return z, rh

    def raft_gru_q(self, x0, packed_q, cq, z, h, x1=None, out=None):
        """convq of a ConvGRU with the rest of its forward (update.py:29-31): x0 = rh of raft_gru_zr and x1 = the x part of
        hx (hx[:, C:]) are cat([r*h, x]); -> (1 - z) * h + z * tanh(convq(.) + cq).  `out` may be `h`."""
        Cc = h.shape[1]
        dtype, dt, B, H, W, s0, C0, s1, C1 = self._chk_conv(_OUT_16, x0, x1, packed_q, Cc)
        shape = (B, Cc, H, W)
        sh = self._chk_frames(h, dtype, "h", shape)
        sq, sz = self._chk_frames(cq, dtype, "cq", shape), self._chk_frames(z, dtype, "z", shape)
        if out is None:
            out = self.torch.empty(shape, dtype=dtype, device=self.device)
        so = self._chk_frames(out, dtype, "out", shape)
        self._bind_stream()
        _lib.check(self.lib.vppx_raft_gru_q_dt_dev(_ptr(x0), s0, C0, _ptr(x1), s1, C1, _ptr(packed_q), _ptr(cq), sq, _ptr(z), sz, _ptr(h),
                                                   sh, _ptr(out), so, B, Cc, H, W, dt, self.ctx.handle))
        return out

    # ---- the encoders' glue: what ResidualBlock.forward runs between its convolutions ----
    def _norm_dtype(self, t, name):
        if getattr(t, "dtype", None) not in (self.torch.float32, self.torch.bfloat16):
            raise TypeError(f"{name} is {getattr(t, 'dtype', type(t))}; the kernels store float32 and bfloat16")
        return self._handoff_dtype(t)

    def _chk_stats(self, t, name, B, Cc):
        """A statistics tensor: float32 [B,C,2], or [C,2] / [1,C,2] for one set that serves every frame -> its frame stride."""
        if getattr(t, "device", None) != self.device or t.dtype != self.torch.float32 or not t.is_contiguous():
            raise ValueError(f"{name}: expected a contiguous float32 tensor on {self.device}")
        if tuple(t.shape) == (B, Cc, 2) and B > 1:
            return 2 * Cc
        if tuple(t.shape) in ((Cc, 2), (1, Cc, 2)):
            return 0
        raise ValueError(f"{name}: expected shape {(B, Cc, 2)} or {(Cc, 2)}, got {tuple(t.shape)}")

    def _chk_channel_vec(self, t, name, Cc):
        if t is not None:
            self._chk(t, self.torch.float32, 1, name, (Cc,))

    def raft_norm_stats(self, x, eps=1e-5, out=None):
        """(mean, rstd) of every [H,W] plane of x [B,C,H,W] (float32 or bfloat16; a channel slice goes in as it is), as
        F.instance_norm takes them: biased variance, rstd = 1 / sqrt(var + eps), from float64 sums (include/vppx.h).
        -> float32 [B,C,2]; with `out` nothing is allocated."""
        dtype, dt = self._norm_dtype(x, "x")
        sx = self._chk_frames(x, dtype, "x")
        B, Cc, H, W = x.shape
        if out is None:
            out = self.torch.empty((B, Cc, 2), dtype=self.torch.float32, device=self.device)
        else:
            self._chk(out, self.torch.float32, 3, "out", (B, Cc, 2))
        self._bind_stream()
        _lib.check(self.lib.vppx_raft_norm_stats_dt_dev(_ptr(x), sx, B, Cc, H, W, float(eps), _ptr(out), dt, self.ctx.handle))
        return out

    def raft_norm_apply(self, x, stats, weight=None, bias=None, relu=True, residual=None, residual_stats=None, residual_weight=None,
                        residual_bias=None, out=None):
        """One launch of a ResidualBlock's norm / ReLU / sum lines (extractor.py:51-52, :54-60):
            v = (x - mean) * rstd [* weight + bias];  relu(v) if `relu`;  with `residual`: relu(u + v), where u is the
            residual, normalised with `residual_stats` (and `residual_weight`, `residual_bias`) when they are given.
        `stats` is raft_norm_stats' [B,C,2], or [C,2] for one set that serves every frame (a frozen BatchNorm:
        (running_mean, 1 / sqrt(running_var + eps))).  `out` may be x or the residual.  -> out [B,C,H,W]."""
        dtype, dt = self._norm_dtype(x, "x")
        sx = self._chk_frames(x, dtype, "x")
        B, Cc, H, W = x.shape
        sst = self._chk_stats(stats, "stats", B, Cc)
        self._chk_channel_vec(weight, "weight", Cc), self._chk_channel_vec(bias, "bias", Cc)
        self._chk_channel_vec(residual_weight, "residual_weight", Cc), self._chk_channel_vec(residual_bias, "residual_bias", Cc)
        sres = self._chk_frames(residual, dtype, "residual", x.shape) if residual is not None else 0
        srst = self._chk_stats(residual_stats, "residual_stats", B, Cc) if residual_stats is not None else 0
        if out is None:
            out = self.torch.empty(tuple(x.shape), dtype=dtype, device=self.device)
        so = self._chk_frames(out, dtype, "out", x.shape)
        self._bind_stream()
        _lib.check(self.lib.vppx_raft_norm_apply_dt_dev(_ptr(x), sx, _ptr(stats), sst, _ptr(weight), _ptr(bias), int(bool(relu)),
                                                        _ptr(residual), sres, _ptr(residual_stats), srst, _ptr(residual_weight),
                                                        _ptr(residual_bias), _ptr(out), so, B, Cc, H, W, dt, self.ctx.handle))
        return out

    def kitti_disp_decode(self, png_u16):
        """uint16 PNG samples (device tensor, int16/uint16 storage) -> (disp float32, valid uint8), same shape
        (frame_utils.readDispKITTI :66-69)."""
        torch = self.torch
        if png_u16.dtype not in (torch.int16, torch.uint16) or not png_u16.is_contiguous() or not png_u16.is_cuda:
            raise ValueError("png_u16 must be a contiguous 16-bit device tensor")
        disp = torch.empty(png_u16.shape, dtype=torch.float32, device=self.device)
        valid = torch.empty(png_u16.shape, dtype=torch.uint8, device=self.device)
        if png_u16.numel() == 0:            # an empty tensor has no storage: its NULL pointer is not the library's n = 0
            return disp, valid
        self._bind_stream()
        _lib.check(self.lib.vppx_kitti_disp_decode_dev(self.ctx.handle, _ptr(png_u16), png_u16.numel(), _ptr(disp), _ptr(valid)))
        return disp, valid

    def png_decode(self, files, height, width, channels=1, scale=1.0 / 256.0, want="disp"):
        """PNG FILES (a list of bytes objects, e.g. the KITTI disparity / LiDAR maps of frame_utils.readDispKITTI :66-69)
        decoded on the device: one upload of the compressed bytes, then chunk walk, inflate and unfiltering in a
        kernel (one workgroup per file).  want="disp": (disp float32 [n,H,W] = sample * scale, valid uint8);
        want="u8": uint8 [n,H,W,C] samples of 8-bit gray / RGB images.  Raises on a file the decoder rejects."""
        import numpy as np
        torch = self.torch
        n = len(files)
        offs = np.zeros(n + 1, np.int64)
        for i, b in enumerate(files):
            offs[i + 1] = offs[i] + len(b)
        blob = torch.frombuffer(bytearray(b"".join(files)), dtype=torch.uint8).to(self.device)
        status = torch.empty((n,), dtype=torch.int32, device=self.device)
        disp = valid = out = None
        if want == "disp":
            disp = torch.empty((n, height, width), dtype=torch.float32, device=self.device)
            valid = torch.empty((n, height, width), dtype=torch.uint8, device=self.device)
        else:
            out = torch.empty((n, height, width, channels), dtype=torch.uint8, device=self.device)
        self._bind_stream()
        _lib.check(self.lib.vppx_png_decode_dev(self.ctx.handle, n, _ptr(blob), offs.ctypes.data_as(C.POINTER(C.c_int64)),
                                                int(height), int(width), int(channels), float(scale), _ptr(disp), _ptr(valid),
                                                _ptr(out), _ptr(status)))
        st = status.cpu().numpy()
        if st.any():
            bad = int(np.flatnonzero(st)[0])
            raise ValueError(f"png_decode: file {bad} rejected with status {int(st[bad])} (see include/vppx.h)")
        return (disp, valid) if want == "disp" else out

    def pfm_decode(self, raw_u8, height, width, channels=1, little_endian=True):
        """PFM payload bytes (device uint8 tensor, header stripped) -> float32 [H,W] or [H,W,3], flipped
        upside-down like frame_utils.readPFM (:34-64)."""
        torch = self.torch
        self._chk(raw_u8, torch.uint8, 1, "raw")
        if raw_u8.numel() != height * width * channels * 4:
            raise ValueError("payload size does not match height*width*channels*4")
        out = torch.empty((height, width, 3) if channels == 3 else (height, width), dtype=torch.float32, device=self.device)
        self._bind_stream()
        _lib.check(self.lib.vppx_pfm_decode_dev(self.ctx.handle, _ptr(raw_u8), int(height), int(width), int(channels),
                                                int(bool(little_endian)), _ptr(out)))
        return out

    def synchronize(self):
        """Wait for torch's current stream (the stream the library launches on) and check the health of the asynchronous
        hot path: raises `VppxError` when a fused aggregation launch lost its lock step, i.e. when disparities returned
        since the last check are void (include/vppx.h, vppx_status).  Callers that synchronise through torch
        (`torch.cuda.synchronize()`, `.cpu()`, `.item()`) call `status()` afterwards instead."""
        self._bind_stream()
        self.ctx.synchronize()

    def status(self):
        """Non-blocking: raise `VppxError` if any fused aggregation launch finished so far lost its lock step."""
        self.ctx.status()

    def set_pipeline(self, enable=True):
        """Cross-call pipelining for streams of batches through `vpp_rsgm`: the front stage of a call (occlusion
        heuristic, VPP, pad + gray, census) runs on a second stream as soon as the previous call's aggregation is done,
        next to that call's sum / WTA and post kernels.  Safe by construction (include/vppx.h): outputs keep torch's
        stream order and are written on the current stream only (per-call allocated tensors are fine); the front stage
        waits for everything queued on the current stream before the call unless the caller passes `inputs_ready=`,
        the event after which this call's inputs exist -- only then is there anything to overlap.  Off by default."""
        _lib.check(self.lib.vppx_set_pipeline(self.ctx.handle, int(bool(enable))))

    def set_graph_mode(self, enable=True):
        """hipGraph replay of repeated identical vpp_rsgm calls (same tensors, parameters and stream; needs a
        non-default torch stream).  `graph_replays()` counts the calls served by a graph launch."""
        _lib.check(self.lib.vppx_set_graph_mode(self.ctx.handle, int(bool(enable))))

    def graph_replays(self):
        return int(self.lib.vppx_graph_replays(self.ctx.handle))

    def last_front_sets(self):
        """(scale set, sample set): which of the two sets of library-owned maps the last resizing / sampling call wrote
        (vppx_last_front_sets); -1 before the first such call."""
        a, b = C.c_int(-1), C.c_int(-1)
        _lib.check(self.lib.vppx_last_front_sets(self.ctx.handle, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def scale_table_builds(self):
        """Times the context built the index tables of a scaled call (vppx_scale_table_builds): a call of the previous scaled
        call's shape reuses them."""
        return int(self.lib.vppx_scale_table_builds(self.ctx.handle))

    # ---- measurement helpers (bench.py) ----
    def time_aggregate(self, iters=10):
        ms = C.c_float()
        _lib.check(self.lib.vppx_time_aggregate(self.ctx.handle, int(iters), C.byref(ms)))
        return float(ms.value)

    def agg_kernel_ms(self, last_n):
        """Average duration of the aggregation kernel over the last `last_n` pipeline launches (hipEvent pairs
        on the launch stream); `last_n <= 0` resets the counter.  Returns (ms, launches averaged)."""
        ms, n = C.c_float(0), C.c_int(0)
        _lib.check(self.lib.vppx_agg_kernel_ms(self.ctx.handle, int(last_n), C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def we_kernel_ms(self, last_n):
        """The same for the W/E launch of the fused layout (0 launches in the 8-path layout)."""
        ms, n = C.c_float(0), C.c_int(0)
        _lib.check(self.lib.vppx_we_kernel_ms(self.ctx.handle, int(last_n), C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def time_aggregate_frames(self):
        return int(self.lib.vppx_time_aggregate_frames(self.ctx.handle))

    def time_aggregate_part(self, part, iters=10):
        ms = C.c_float()
        _lib.check(self.lib.vppx_time_aggregate_part(self.ctx.handle, int(iters), int(part), C.byref(ms)))
        return float(ms.value)

    def timing_last_routes(self):
        """The kernel instantiations the last timing helper (`time_aggregate`, `time_aggregate_part`) launched, named as in
        `last_routes` (vppx_timing_last_routes); empty after a helper that refused."""
        return _lib._route_list(self.lib.vppx_timing_last_routes, self.ctx.handle)

    def uses_vert(self):
        """Aggregation layout of the last call: 0 = eight line-parallel paths, 1 = band marching (experiment),
        3 = W/E line-parallel + the fused three-path vertical kernel (default from 8 frames per launch on)."""
        return int(self.lib.vppx_uses_vert(self.ctx.handle))

    def last_call_parts(self):
        """Parts the last fused call ran as (a batch larger than one round of the lock-step kernel is split; 1 = unsplit)."""
        return int(self.lib.vppx_last_call_parts(self.ctx.handle))

    def we_last_pieces(self):
        """Pieces per line of the last layer of waves in the last W/E launch of the fused layout (1: no line was cut)."""
        return int(self.lib.vppx_we_last_pieces(self.ctx.handle))

    def wsum_last_pieces(self):
        """The same for the last launch of the W + sum + WTA kernel (route "wsum<12>")."""
        return int(self.lib.vppx_wsum_last_pieces(self.ctx.handle))

    def last_routes(self):
        """The kernel instantiations the last rSGM-bearing call launched, in launch order, each once (vppx_last_routes),
        e.g. ["paths<4,16,exact,census,u8,dirs=ff>", "sum_lr<4,u8,8,64,spare,sw4,fast,16,fullw>"]."""
        return _lib.last_routes(self.lib, self.ctx.handle)

    def last_front_routes(self):
        """The same for the front stage, a list of its own (vppx_last_front_routes): the occlusion heuristic, VPP and bilateral
        filling kernels the last call launched, e.g. ["occ_warp4", "occ_test<2,4>", "compact<plain>", "rowscan", "rand",
        "vpp_order<late,side>", "l_bits<3,1>", "r_rows<u16,mode=3,seg=1>", "l_heavy<3>"]."""
        return _lib.last_front_routes(self.lib, self.ctx.handle)

    def fused_pixels_per_wave(self):
        """16 / 8: which fused vertical kernel the last call used (sgm_vert4_kernel / sgm_vert3_kernel); 0: none."""
        return int(self.lib.vppx_fused_pixels_per_wave(self.ctx.handle))

    def batch_quantum(self, h, w, dmax=192):
        """Frames per full round of the fused layout's lock-step kernel for h x w frames (a scheduling hint: batches that are
        a multiple of it leave no part-filled last round; 0 when the fused layout does not apply)."""
        return int(self.lib.vppx_batch_quantum(self.ctx.handle, int(h), int(w), int(dmax)))

    def enable_stage_timing(self, on=True):
        _lib.check(self.lib.vppx_enable_stage_timing(self.ctx.handle, int(bool(on))))

    def stage_marks(self):
        """Marks the last call recorded while stage timing was on, over all its parts (vppx_stage_marks)."""
        return int(self.lib.vppx_stage_marks(self.ctx.handle))

    def stage_ms(self):
        arr = (C.c_float * 32)()
        n = _lib.check(self.lib.vppx_get_stage_ms(self.ctx.handle, arr, 32))
        return {self.lib.vppx_stage_name(i).decode(): float(arr[i]) for i in range(n)}
