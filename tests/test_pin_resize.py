"""CPU: tests/pin_resize.py (the pin of the --iscale resize for whoever has OpenCV) -- it must skip cleanly without cv2, pass
against a stand-in module with cv2's name that resizes like the restatement, and name the first case a different rounding
breaks."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _scale_ref as ref  # noqa: E402
import pin_resize  # noqa: E402


def test_skips_cleanly_without_cv2():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pin_resize.py"), "--cv2-module", "no_such_cv2_module"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "skipped: no no_such_cv2_module" in r.stdout


def test_a_stand_in_resizing_like_the_restatement_passes_every_case():
    fake = types.SimpleNamespace(resize=lambda img, size: ref.resize_u8(img, size[0], size[1]))
    lines = []
    ran, first = pin_resize.run(fake, log=lines.append)
    assert first is None and ran == len(pin_resize.SHAPES) * len(pin_resize.SCALES) * len(pin_resize.CHANNELS)
    assert all(l.startswith("PASS") for l in lines)


def test_the_first_differing_case_is_named():
    """A stand-in with the scalar tail's rounding, (t0 * b0 + t1 * b1 + 2^21) >> 22, where the restatement has OpenCV's vector
    formula: some byte of some odd shape differs, and the report names the case."""
    def resize(img, size):
        w, h = size
        a = np.asarray(img)
        a3 = a[..., None] if a.ndim == 2 else a
        H, W = a3.shape[:2]
        sy0, sy1, b0, b1 = ref.axis_table(H, h)
        sx0, sx1, a0, a1 = ref.axis_table(W, w)
        s = a3.astype(np.int64)
        t0 = s[sy0][:, sx0] * a0[None, :, None] + s[sy0][:, sx1] * a1[None, :, None]
        t1 = s[sy1][:, sx0] * a0[None, :, None] + s[sy1][:, sx1] * a1[None, :, None]
        out = ((t0 * b0[:, None, None] + t1 * b1[:, None, None] + (1 << 21)) >> 22).astype(np.uint8)
        return out[..., 0] if a.ndim == 2 else out
    lines = []
    ran, first = pin_resize.run(types.SimpleNamespace(resize=resize), log=lines.append)
    assert first is not None and any(l.startswith("FAIL") for l in lines)
    assert any("first differing case" in l for l in lines)


@pytest.mark.gpu
def test_library_side_agrees_with_a_stand_in_resizing_like_the_restatement():
    fake = types.SimpleNamespace(resize=lambda img, size: ref.resize_u8(img, size[0], size[1]))
    lines = []
    ran, first = pin_resize.run(fake, gpu=True, log=lines.append)
    assert first is None, "\n".join(l for l in lines if l.startswith("FAIL"))
