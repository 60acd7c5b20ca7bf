"""The conversion the pair form of the fine LK kernel applies to a window sum (wide_halves_to_f32 in velocity_amd/csrc/vh_lk_shared.hpp), restated in NumPy
and compared with the conversion it replaces.

The one-wavefront k_lk3 kernels reduce a window sum as two 16-bit halves and, since the pair form, convert it in the lane the reduction leaves it in:
    (float)((double)hi * 65536.0 + (double)lo)
where the other kernels recombine the halves on the scalar unit and convert the int64 (i64_to_f32):
    (float)(int64)(hi * 65536 + lo)
The two are the same float when the float64 expression is exact, because both then round the same integer once, to nearest even.

Bounds (wave_sum2_i32_wide in velocity_amd/csrc/vh_lk.hip): a lane's int32 partial v is split into v & 0xffff, in [0, 2^16 - 1], and v >> 16 (arithmetic), in
[-2^15, 2^15 - 1]; each half is summed over the 64 lanes of a wavefront.  So 0 <= lo <= 64 * (2^16 - 1) < 2^22 and -2^21 <= hi <= 2^21 - 64.  hi * 65536 is
then a multiple of 2^16 below 2^37 in magnitude and the sum stays below 2^37 + 2^22 < 2^53: every step of the float64 expression is exact.  No GPU."""
import numpy as np

LO_MAX = 64 * (2 ** 16 - 1)
HI_MIN, HI_MAX = -(2 ** 21), 2 ** 21 - 64


def _pair_form(hi, lo):
    return (np.asarray(hi, np.int64).astype(np.float64) * np.float64(65536.0) + np.asarray(lo, np.int64).astype(np.float64)).astype(np.float32)


def _int64_form(hi, lo):
    return (np.asarray(hi, np.int64) * np.int64(65536) + np.asarray(lo, np.int64)).astype(np.float32)


def _assert_same(hi, lo):
    hi, lo = np.asarray(hi, np.int64), np.asarray(lo, np.int64)
    a, b = _pair_form(hi, lo), _int64_form(hi, lo)
    bad = np.flatnonzero(a.view(np.uint32) != b.view(np.uint32))
    assert not len(bad), (hi[bad[:8]], lo[bad[:8]], a[bad[:8]], b[bad[:8]])


def _split(v):
    """(hi, lo) with hi * 65536 + lo == v and 0 <= lo < 65536: the halves of a value as one lane would hold them."""
    v = np.asarray(v, np.int64)
    return v >> 16, v & 0xFFFF


def test_the_float64_expression_is_exact_inside_the_bounds():
    """The argument itself: at the corners of the bounds the float64 value equals the integer."""
    for hi in (HI_MIN, HI_MAX, -1, 0, 1):
        for lo in (0, 1, LO_MAX - 1, LO_MAX):
            d = np.float64(hi) * np.float64(65536.0) + np.float64(lo)
            assert int(d) == hi * 65536 + lo and abs(hi * 65536 + lo) < 2 ** 53


def test_both_extremes_of_either_half():
    hi = np.array([HI_MIN, HI_MIN, HI_MAX, HI_MAX, 0, 0, -1, -1, 1, 1, HI_MIN + 1, HI_MAX - 1])
    lo = np.array([0, LO_MAX, 0, LO_MAX, 0, LO_MAX, 0, LO_MAX, 0, LO_MAX, LO_MAX - 1, 1])
    _assert_same(hi, lo)


def test_round_to_even_ties_and_their_neighbours():
    """An integer in [2^k, 2^(k+1)), k >= 24, lies between float32 neighbours 2^(k-23) apart: the odd multiples of 2^(k-24) are ties, and the float must be the
    even neighbour.  Both signs, the first and the last ties of every binade and ones in the middle, each with the integers one below and one above it.
    Through k = 36 the halves are inside the kernel's bounds (|hi| <= 2^21); 37 ... 40 are beyond what 64 lanes can sum and are here because the identity
    does not depend on the bounds (it needs |hi * 65536 + lo| < 2^53 only)."""
    vals = []
    for k in range(24, 41):
        half = 1 << (k - 24)
        n = 1 << 24  # odd multiples m * half with m in [2^24, 2^25)
        for m in (n + 1, n + 3, n + 5, n + (n >> 1) + 1, n + (n >> 1) - 1, 2 * n - 3, 2 * n - 1):
            for d in (-1, 0, 1):
                vals += [m * half + d, -(m * half + d)]
    v = np.array(vals, np.int64)
    hi, lo = _split(v)
    inside = (hi >= HI_MIN) & (hi <= HI_MAX)
    assert inside.any() and (~inside).any()
    assert (np.abs(v[inside]).max() >= 2 ** 36) and (np.abs(v).max() >= 2 ** 40)
    _assert_same(hi, lo)
    # the ties really are ties: the int64 conversion lands on an even significand
    ties = v[2::6]  # (the positive one of every triple)
    gap = ties & -ties  # the lowest set bit of an odd multiple of 2^(k-24) is 2^(k-24): half the float32 spacing
    f = _pair_form(hi, lo)[2::6].astype(np.float64)
    assert (np.abs(f - ties.astype(np.float64)) == gap.astype(np.float64)).all()
    assert ((f / (2.0 * gap.astype(np.float64))) % 2.0 == 0.0).all()
    # lo spread over the whole of its range as well: the same values with part of hi moved into lo
    move = np.minimum(np.maximum(hi - HI_MIN, 0), 63)
    _assert_same(hi - move, lo + move * 65536)


def test_seeded_random_pairs_over_the_whole_range():
    rng = np.random.default_rng(5116)
    hi = rng.integers(HI_MIN, HI_MAX + 1, 100_000)
    lo = rng.integers(0, 2 ** 22, 100_000)
    _assert_same(hi, lo)
    # and small magnitudes, where most real sums of the Newton iterations lie (hi near 0, either sign)
    hi = rng.integers(-300, 301, 100_000)
    lo = rng.integers(0, 2 ** 22, 100_000)
    _assert_same(hi, lo)
