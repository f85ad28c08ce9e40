"""The referee of the fused correlation call (tests/_corr_fused_ref.py) against the arrays the reference's own CorrBlock1D
produced, and every premise tests/test_gpu_corr_fused.py relies on, asserted on the very arrays that file uploads.  No
GPU is needed."""
import numpy as np
import pytest

import _corr_fused_ref as FR
import _corr_ref as CR
import _handoff_bf16_ref as BR
import _handoff_ref as R

F32, F64 = np.float32, np.float64


@pytest.mark.parametrize("t", FR.GOLDEN_TAGS)
def test_referee_equals_the_recorded_level0_bit_for_bit(t):
    c = FR.golden_case(t)
    want = c.g("plain_level0")
    got = FR.exact_level0(c.f2, c.f3)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not (np.signbit(want) & (want == 0)).any(), "a negative zero: the sum's start at +0 would matter"
    # what the GPU file pools and looks up is the recording's too
    pyr = CR.pyramid(got, 4)
    for i in range(4):
        assert np.array_equal(pyr[i].view(np.uint32), c.g(f"plain_level{i}").view(np.uint32))
    out = CR.channels_first(CR.lookup(pyr, c.coords[:, 0], 4), c.B, c.H4, c.W2)
    assert CR.same_bits(out, c.g("plain_lookup")) == 0


def test_the_division_is_not_a_reciprocal_multiply_where_sqrt_d_is_no_power_of_two():
    """Why the bit-for-bit tests can tell the two apart: on cases a, c and d some cell differs."""
    for t, differs in (("a", True), ("b", False), ("c", True), ("d", True)):
        c = FR.golden_case(t)
        dot = np.einsum("aijk,aijh->ajkh", c.f2.astype(F64), c.f3.astype(F64)).astype(F32).reshape(c.N, c.W3)
        recip = dot * (F32(1) / np.sqrt(F32(c.D)))
        assert (recip.view(np.uint32) != c.g("plain_level0").view(np.uint32)).any() == differs, t


@pytest.mark.parametrize("shape", FR.DIRECTED_SHAPES + [FR.LEVELS_SHAPE, FR.ONE_HOT_SHAPE], ids=FR.tag)
def test_exactness_holds_on_every_directed_shape(shape):
    kind = "one_hot" if shape == FR.ONE_HOT_SHAPE else "grid"
    c = FR.case(shape, kind)
    assert c.f2.shape == (c.B, c.D, c.H4, c.W2) and c.f3.shape == (c.B, c.D, c.H4, c.W3)
    level0 = FR.exact_level0(c.f2, c.f3)                         # asserts the grid, the 24 bits and the exact conversion
    assert level0.shape == (c.N, c.W3) and np.isfinite(level0).all()
    # bfloat16 holds the same features
    assert np.array_equal(BR.bf16_rne_f32(c.f2), c.f2) and np.array_equal(BR.bf16_rne_f32(c.f3), c.f3)
    # a transposed or swapped operand gives another volume
    if c.W2 == c.W3:
        swapped = FR.exact_level0(c.f3, c.f2)
        assert not np.array_equal(swapped, level0)
    # hints: the first rows run through V_ORDER, so rows with v = 0 and -0 sit next to modulated ones
    v = c.v4.reshape(-1)
    k = min(c.N, len(CR.V_ORDER))
    assert np.array_equal(v[:k].view(np.uint32), CR.V_ORDER[:k].view(np.uint32))
    assert (v == 0).any() and (v != 0).any()
    assert (c.H // 4, c.W // 4) == (c.H4, c.W2)
    _, vs = R.subsample(c.hints, c.valid, raft=True)
    assert np.array_equal(vs.view(np.uint32), c.v4.view(np.uint32))
    if kind == "one_hot":                                        # row x2 of level 0 is the chosen plane of fmap3 / sqrt(D)
        plane = np.take_along_axis(c.f3[:, :, :, None, :], c.khot[:, None, :, :, None], axis=1)[:, 0]
        want = (F32(0) + plane) / np.sqrt(F32(c.D))
        assert np.array_equal(level0.view(np.uint32), np.ascontiguousarray(want.reshape(c.N, c.W3)).view(np.uint32))
        assert len(np.unique(c.khot)) > 1


def test_the_shapes_reach_what_the_table_says():
    TM, TN, KS = 128, 64, 32                                     # the kernel's tile and slab
    B, D, H4, W2, W3 = FR.DIRECTED_SHAPES[0]
    assert B > 1 and H4 > 1 and D % KS == 0 and D // KS > 1 and W2 % 16 and W3 % 16 and W3 % 2 and W2 != W3
    _, D, _, W2, W3 = FR.DIRECTED_SHAPES[1]
    assert D > KS and D % KS and D % 4 == 0 and W2 % 16
    _, D, _, W2, W3 = FR.DIRECTED_SHAPES[2]
    assert W2 > TN and W3 > TM and W2 % 16 == 0 and W3 % 16 == 0  # more than one workgroup along both, whole 16x16 tiles
    _, D, _, W2, W3 = FR.MISALIGNED_SHAPE
    assert D % 4 and W2 % 8 == 0 and W3 % 8 == 0                  # the rows allow vectors: only the pointer forbids them
    _, D, _, W2, W3 = FR.LEVELS_SHAPE
    assert W3 > TM and W3 % 2 and (W3 >> 1) % 2 == 0


@pytest.mark.parametrize("with_hints", [False, True])
def test_the_reference_arithmetic_stays_inside_the_bound_on_the_random_case(with_hints):
    c = FR.case(FR.RANDOM_SHAPE, "random")
    assert np.array_equal(BR.bf16_rne_f32(c.f2), c.f2) and np.array_equal(BR.bf16_rne_f32(c.f3), c.f3)
    dot = np.einsum("aijk,aijh->ajkh", c.f2.astype(F64), c.f3.astype(F64))
    assert (dot.astype(F32).astype(F64) != dot).mean() > 0.9, "the sums are exact: the case does not test the bound"
    own = FR.einsum_level0(c.f2, c.f3)
    if with_hints:
        own = R.raft_modulate(own.reshape(c.B, c.H4, c.W2, 1, c.W3), c.hints, c.valid, rule="library").out.reshape(c.N, c.W3)
    for bf16 in (False, True):
        c64, lim = FR.bound(c.f2, c.f3, c.hints if with_hints else None, c.valid if with_hints else None, bf16)
        got = BR.bf16_rne_f32(own) if bf16 else own
        dist = np.abs(got.astype(F64) - c64)
        ok = (dist <= lim) | (got == 0)
        worst = float(np.max(np.where(lim > 0, dist / np.where(lim > 0, lim, 1.0), 0.0)))
        print(f"einsum / sqrt, hints={with_hints}, bf16={bf16}: worst distance / bound {worst:.3f}")
        assert ok.all()
        assert worst > 1e-3, "the bound is loose beyond use"
        if bf16:    # the plain product 2^-9 * |value| is not a bound of one correct rounding: these very cells pass it by
            plain = FR.bound(c.f2, c.f3, c.hints if with_hints else None, c.valid if with_hints else None, False)[1] + 2.0 ** -9 * np.abs(c64)
            beyond = int((~(dist <= plain) & (got != 0)).sum())
            print(f"    cells beyond corr_whole + 2^-9 * |value|: {beyond} of {got.size}")
            assert beyond > 0


def test_half_a_bfloat16_ulp():
    assert FR.bf16_half_ulp(1.0) == 2.0 ** -8 and FR.bf16_half_ulp(1.99) == 2.0 ** -8 and FR.bf16_half_ulp(2.0) == 2.0 ** -7
    assert FR.bf16_half_ulp(0.0) == 2.0 ** -134
    x = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8], F32)                  # ties: to 1 and to 1 + 2^-6
    r = BR.bf16_rne_f32(x)
    assert np.array_equal(r, np.array([1.0, 1 + 2.0 ** -6], F32))
    assert (np.abs(r.astype(F64) - x) == FR.bf16_half_ulp(np.abs(x.astype(F64)))).all()
    assert (np.abs(r.astype(F64) - x) > 2.0 ** -9 * np.abs(x)).all()


def test_the_nonfinite_case_marks_rows_and_columns():
    f2, f3, bad = FR.nonfinite_case()
    c = FR.case(FR.RANDOM_SHAPE)
    with np.errstate(invalid="ignore"):
        dot = np.einsum("aijk,aijh->ajkh", f2.astype(F64), f3.astype(F64)).reshape(c.N, c.W3)
    assert np.array_equal(~np.isfinite(dot), bad)
    assert 0 < bad.sum() < bad.size / 4
    marks = FR.pooled_any(bad, 4)
    assert [m.shape[1] for m in marks] == [c.W3 >> i for i in range(4)] and all(m.any() and not m.all() for m in marks)
