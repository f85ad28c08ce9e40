#!/usr/bin/env python3
"""tests/pin_resize.py -- one command that pins the resize of --iscale (DESIGN section 5 rule 1)
for whoever HAS OpenCV.

OpenCV is not a dependency of this project and is absent where it was built, so `tests/_scale_ref.py` restates
`cv2.resize(u8, (w, h))` (INTER_LINEAR) from our reading of OpenCV 4.x, and the device resize is tested against that
restatement.  Given a real `cv2`, this script compares it with the restatement -- and, with --gpu on a gfx950 box, with the
library (the patterned pair of a scaled call without hints is the resized pair) -- on odd and even shapes, C = 1 and 3 and
s = 2, 3, 4:

    python tests/pin_resize.py [--cv2-module cv2] [--gpu] [--seed N]

Without cv2 it says so and exits 0.  Exit status: 0 = every case agrees (or nothing to compare with), 1 = a case differs;
the first differing case is named with the number of differing bytes.  `tests/test_pin_resize.py` drives it with stand-in
modules.
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _scale_ref as ref  # noqa: E402

SHAPES = [(48, 160), (49, 163), (61, 177), (375, 1242), (540, 960)]
SCALES = [2, 3, 4]
CHANNELS = [1, 3]


def _cases(seed):
    rng = np.random.default_rng(seed)
    for H, W in SHAPES:
        for C in CHANNELS:
            img = rng.integers(0, 256, (H, W, C) if C == 3 else (H, W), dtype=np.uint8)
            for s in SCALES:
                yield H, W, C, s, img


def _gpu_resize(imgs, s):
    """The library's resize of a [B, H, W, C] batch: the patterned left image of a scaled call with all-zero hints."""
    import torch
    from vppstereo_amd.engine import Engine
    eng = Engine()
    a = np.ascontiguousarray(imgs if imgs.ndim == 4 else imgs[..., None])
    B, H, W, C = a.shape
    t = torch.from_numpy(a).to(eng.device)
    lv = torch.empty((B, H // s, W // s, C), dtype=torch.uint8, device=eng.device)
    eng.vpp_rsgm(t, t, torch.zeros((B, H, W), dtype=torch.float32, device=eng.device), l_vpp=lv, iscale=s, rsgm_kw=dict(dmax=64))
    torch.cuda.synchronize()
    out = lv.cpu().numpy()
    return out[..., 0] if imgs.ndim == 3 else out


def run(cv2mod, gpu=False, seed=0, log=print):
    """Returns (cases run, first failing case description or None)."""
    ran, first = 0, None
    for H, W, C, s, img in _cases(seed):
        w, h = W // s, H // s
        want = np.asarray(cv2mod.resize(img, (w, h))).reshape(ref.resize_u8(img, w, h).shape)
        sides = {"restatement": ref.resize_u8(img, w, h)}
        if gpu:
            sides["library"] = _gpu_resize(img[None], s)[0]
        for name, got in sides.items():
            ran += 1
            bad = int(np.count_nonzero(got != want))
            tag = f"{H}x{W}x{C} s={s} {name}"
            log(f"{'PASS' if bad == 0 else 'FAIL'} {tag}" + (f": {bad} bytes differ from cv2.resize" if bad else ""))
            if bad and first is None:
                first = tag
    if first:
        log(f"first differing case: {first} (DESIGN section 5 rule 1; INTEGRATION section 6 row 17)")
    return ran, first


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cv2-module", default="cv2")
    ap.add_argument("--gpu", action="store_true", help="also compare the library's resize (needs a gfx950 GPU)")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    try:
        cv2mod = importlib.import_module(a.cv2_module)
    except Exception as e:  # noqa: BLE001
        print(f"skipped: no {a.cv2_module} ({type(e).__name__}: {e}); nothing to compare the restatement with")
        return 0
    _, first = run(cv2mod, gpu=a.gpu, seed=a.seed)
    return 1 if first else 0


if __name__ == "__main__":
    sys.exit(main())
