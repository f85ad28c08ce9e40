"""How a VppxMetrics record and an error map are held to the CPU oracle (oracle.guided_metrics, pinned to the reference by
tests/test_oracle_glue.py) and to the reference's two numpy statements: shared by tests/test_gpu_metrics.py and the sequence
tests, so that the bound is stated once.

Bound on the two sums.  The oracle adds the same non-negative float32 terms in index order in float64, the kernels add them in a
fixed tree order; each order is within (n - 1) * 2^-53 relative of the exact sum, so the two differ by at most 2 (n - 1) * 2^-53;
the division and the square root add one rounding each on either side: |ours - oracle| <= (2 * n_valid + 4) * 2^-53 * oracle.
Counts (bad 1.0 ... 4.0, n_valid) are integers divided once in float64 on both sides: bit-equal."""
import numpy as np

import oracle

KEYS = ('bad 1.0', 'bad 2.0', 'bad 3.0', 'bad 4.0', 'avgerr', 'rms')


def check_record(rec, disp, gt, valid, tag=""):
    """rec: the 8 doubles of one VppxMetrics; disp, gt, valid: what the oracle gets (gt already decimated and divided)."""
    m = oracle.guided_metrics(disp, gt, valid)
    n = int((np.asarray(valid) > 0).sum())
    assert rec[6] == n and rec[7] == 0.0, (tag, rec[6], n)
    if n == 0:
        assert np.isnan(rec[:6]).all(), (tag, rec)
        assert all(np.isnan(m[k]) for k in KEYS)
        return
    for k in range(4):
        assert np.float64(rec[k]).tobytes() == np.float64(m[KEYS[k]]).tobytes(), (tag, KEYS[k], rec[k], m[KEYS[k]])
    bound = (2 * n + 4) * 2.0 ** -53
    for k in (4, 5):
        o = m[KEYS[k]]
        if np.isnan(o):
            assert np.isnan(rec[k]), (tag, KEYS[k], rec[k])
            continue
        print(f"{tag} {KEYS[k]}: ours {rec[k]!r} oracle {o!r} |diff| {abs(rec[k] - o):.3e} bound {bound * o:.3e}")
        assert abs(rec[k] - o) <= bound * o, (tag, KEYS[k], rec[k], o, abs(rec[k] - o), bound * o)


def numpy_errormap(disp, gt, valid):
    """losses.py:14-15, :24"""
    with np.errstate(invalid="ignore"):
        error = np.abs(disp - gt)
        error[valid == 0] = 0
        return error * (valid > 0)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def decimated_gt(gt, valid, s, Ho, Wo):
    """test.py:150-152: every s-th row and column of gt and validgt, gt / s in float32, cut to the map's shape."""
    gts = (gt[..., ::s, ::s][..., :Ho, :Wo] / np.float32(s)).astype(np.float32)
    return np.ascontiguousarray(gts), np.ascontiguousarray(valid[..., ::s, ::s][..., :Ho, :Wo])
