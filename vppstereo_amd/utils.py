"""Drop-in for the reference's ``utils.py``: ``color_error_image_kitti`` (utils.py:17-36) and ``guided_visualize``
(utils.py:39-79), numpy in and numpy out through the ``_host`` calls of libvppx.so (include/vppx.h "pictures").

The inputs are taken as float32, which is what test.py:327-328 passes; a boolean ``mask`` / ``valid`` becomes 0.0 / 1.0.
The dilation is the library's restatement of ``cv2.dilate(img, np.ones((d, d)))``; ``dilation`` 0
and 1 leave the picture as it is.  As everywhere in this package there is no CPU fallback."""
import numpy as np

from . import _lib


def _frame(a, name, shape=None):
    a = np.ascontiguousarray(a, np.float32)
    if a.ndim != 2 or a.size == 0:
        raise ValueError(f"{name} must be HxW")
    if shape is not None and a.shape != shape:
        raise ValueError(f"{name}: expected shape {shape}, got {a.shape}")
    return a


def color_error_image_kitti(errors, scale=1, mask=None, BGR=True, dilation=1):
    errors = _frame(errors, "errors")
    h, w = errors.shape
    if mask is not None:
        mask = _frame(mask, "mask", (h, w))
    out = np.empty((h, w, 3), np.uint8)
    _lib.check(_lib.load().vppx_error_colors_host(_lib.default_context().handle, 1, h, w, _lib.np_ptr(errors), _lib.np_ptr(mask),
                                                  float(scale), int(bool(BGR)), int(dilation), _lib.np_ptr(out)))
    return out


def guided_visualize(disp, gt, valid, scale=1, dilation=7):
    disp = _frame(disp, "disp")
    h, w = disp.shape
    gt = _frame(gt, "gt", (h, w))
    valid = _frame(valid, "valid", (h, w))
    out = np.empty((6, h, w, 3), np.uint8)
    _lib.check(_lib.load().vppx_guided_visualize_host(_lib.default_context().handle, 1, h, w, _lib.np_ptr(disp), _lib.np_ptr(gt),
                                                      _lib.np_ptr(valid), float(scale), int(dilation), _lib.VIZ_ALL, _lib.np_ptr(out)))
    return {k: out[n] for n, k in enumerate(_lib.VIZ_KEYS)}
