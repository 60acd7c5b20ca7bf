"""CPU only: oracle/klt_oracle.c::ko_corner_subpix held to the exact NumPy model of tests/subpix_ref.py bit for bit -- every window 1 .. 7, every stop
setting, patches that leave the image, a strided view -- on the scenes of tests/subpix_scenes.py; the census of the loop's exits on those scenes; the
proof that the scenes see each of ten deliberate defects of the model; and the model (with the oracle) held to truth that no implementation supplied:
the corner of a point-symmetric X-junction.  Every comparison is exact equality of bit patterns except the derived bound of the truth test."""
import collections

import numpy as np
import pytest

import subpix_ref as SR
import subpix_scenes as S
from oracle import klt_oracle as KO

F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same(got, want, ctx):
    bad = np.flatnonzero((bits(got) != bits(want)).any(1))
    assert got.shape == want.shape and not len(bad), (ctx, len(bad), bad[:8], got[bad[:8]], want[bad[:8]])


# ---------------------------------------------------------------------------------------------------------------------
# a. oracle == model
# ---------------------------------------------------------------------------------------------------------------------
def test_mask_table_layout():
    """The seven masks back to back are 679 floats, each symmetric with a centre of exactly 1, and no two windows share an offset but 0 and 1
    (window 1 starts the table)."""
    t = SR.mask_table()
    assert len(t) == 679 == SR.mask_offset(SR.MAXWIN + 1)
    assert [SR.mask_offset(w) for w in S.WINS] == [0, 9, 34, 83, 164, 285, 454]
    for win in S.WINS:
        m = SR.mask(win)
        assert m.dtype == F32 and m.shape == (2 * win + 1, 2 * win + 1) and np.array_equal(m, m.T) and m[win, win] == 1 and m[0, 0] == m.min() > 0


@pytest.mark.parametrize("win", S.WINS)
def test_oracle_equals_the_model_on_the_texture(win):
    """96 points at every stop setting: image corners, edges, the flat band, patches that leave the image on every side."""
    img, pts = S.texture()
    for k, (max_iter, eps) in enumerate(S.STOPS):
        _same(KO.corner_subpix(img, pts, win, max_iter, eps), S.texture_model(win, k)[0], (win, max_iter, eps))


@pytest.mark.parametrize("name", sorted(S.TINY))
def test_oracle_equals_the_model_where_the_patch_is_larger_than_the_image(name):
    img, pts = S.tiny(name)
    w, h, win = S.TINY[name]
    assert img.shape == (h, w) and 2 * win + 3 > max(w, h)
    for k, (max_iter, eps) in enumerate(S.STOPS):
        want, exits, reverted, _ = S.tiny_model(name, k)
        _same(KO.corner_subpix(img, pts, win, max_iter, eps), want, (name, max_iter, eps))
    assert not np.array_equal(S.tiny_model(name, 0)[0], pts)  # a condition on the scene: something moves


def test_oracle_equals_the_model_on_a_strided_view_and_on_the_exact_step():
    """img[3:, 5:] of a larger array has the texture's pixels behind a row pitch that is not its width; and the step scene, whose one point lands ON
    x = w having moved exactly win in x and in y (subpix_scenes.step)."""
    img, pts = S.texture()
    big = np.full((S.TH + 3, S.TW + 11), 255, np.uint8)
    big[3:, 5:5 + S.TW] = img
    view = big[3:, 5:5 + S.TW]
    assert view.strides == (S.TW + 11, 1) and not view.flags.c_contiguous
    for win in (1, 5, 7):
        _same(KO.corner_subpix(view, pts, win, 100, 0.001), S.texture_model(win, 0)[0], ("view", win))
        _same(SR.corner_subpix(view, pts, win, 100, 0.001), S.texture_model(win, 0)[0], ("model on the view", win))
    simg, spts = S.step()
    want, exits, reverted, iters = SR.corner_subpix(simg, spts, S.STEP_WIN, 100, 0.001, trace=True)
    assert want.tolist() == [list(S.STEP_END)] and S.STEP_END[0] == simg.shape[1] and exits[0] == "left" and not reverted[0] and iters[0] == 0
    assert (want[0] - spts[0] == S.STEP_WIN).all()
    _same(KO.corner_subpix(simg, spts, S.STEP_WIN, 100, 0.001), want, "step")


# ---------------------------------------------------------------------------------------------------------------------
# b. what the scenes exercise, asserted on the model alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win", S.WINS)
def test_every_exit_of_the_loop_occurs(win):
    """At (100, 0.001) every (exit, reverted) combination of subpix_scenes.CENSUS[win] occurs: for windows 1 and 2 all seven that exist (`det` never
    comes with a revert: see CENSUS), for every window `eps` with and without the revert and `det`."""
    _, exits, reverted, iters = S.texture_model(win, 0)
    seen = collections.Counter(zip(exits.tolist(), reverted.tolist()))
    print(win, sorted(seen.items()))
    assert set(exits.tolist()) <= set(SR.EXITS)
    for combo in S.CENSUS[win]:
        assert seen[combo] >= 1, (win, combo, sorted(seen.items()))
    assert (iters[exits == "iter"] == 100).all() and (iters[exits == "det"] < 100).all()


def test_stop_settings_do_what_they_say():
    """(0, -1.0) is (1, 0.0) and (1000, 0.0) is (100, 0.0): the clamps.  With eps = 0 nothing but the cap stops a corner that still moves: an `eps`
    exit there is a point that did not move at all in its last step (err = 0), and there are corners that the cap of 2 and the cap of 100 stop.
    (1, .) takes exactly one step; the loose eps of (1000, 0.5) stops corners that (100, 0.001) lets run on."""
    img, pts = S.texture()
    stop = {s: k for k, s in enumerate(S.STOPS)}
    for win in S.WINS:
        for a, b in (((0, -1.0), (1, 0.0)), ((1000, 0.0), (100, 0.0)), ((1000, 0.5), (100, 0.5))):
            ra = S.texture_model(win, stop[a]) if a in stop else SR.corner_subpix(img, pts, win, *a, trace=True)
            rb = S.texture_model(win, stop[b]) if b in stop else SR.corner_subpix(img, pts, win, *b, trace=True)
            assert np.array_equal(bits(ra[0]), bits(rb[0])) and np.array_equal(ra[3], rb[3]), (win, a, b)
        one = S.texture_model(win, stop[(1, 0.001)])
        assert one[3].max() <= 1 and set(one[1].tolist()) <= {"iter", "det", "left"}
        for cap in (2, 100):
            p, exits, reverted, iters = S.texture_model(win, stop[(cap, 0.0)])
            assert ((exits == "iter") & (iters == cap)).sum() >= 5, (win, cap)
            still = np.flatnonzero((exits == "eps") & ~reverted)
            again = SR.corner_subpix(img, p[still], win, 1, 0.0)
            assert np.array_equal(bits(again), bits(p[still])), (win, cap)  # a fixed point, bit for bit
        loose, tight = S.texture_model(win, stop[(1000, 0.5)]), S.texture_model(win, stop[(100, 0.001)])
        assert (loose[3] < tight[3]).sum() >= 10, win


# ---------------------------------------------------------------------------------------------------------------------
# c. sensitivity: the scenes see each defect
# ---------------------------------------------------------------------------------------------------------------------
# The one mutant that the scenes cannot show in the output (the issue grants two).  pairwise_sum (np.sum for the sequential accumulation) changes the
# five float64 sums by a few units of 2^-53 relative, and a coordinate is rounded to float32 (2^-24) at every step: an output bit changes only if the
# step carries the difference across a float32 rounding boundary (a chance of about 2^-29 per coordinate and step), or where a nearly singular system
# amplifies it by 10^8 -- and such a step leaves the image or the window and is turned back to the start.  Where the terms are exact (whole-pixel
# starts: 9-bit differences, 24-bit masks) the order does not matter at all.  On these scenes no bit changes; what is asserted instead is that the
# mutant's sums do differ from the sequential ones.
INVISIBLE = ("pairwise_sum",)


def _scene_runs():
    """(image, points, window, stop) of everything the oracle and the device are compared on."""
    img, pts = S.texture()
    for win in S.WINS:
        for stop in S.STOPS:
            yield img, pts, win, stop
    for name in sorted(S.TINY):
        yield S.tiny(name) + (S.TINY[name][2], S.STOPS[0])
    yield S.step() + (S.STEP_WIN, S.STOPS[0])


@pytest.mark.parametrize("mutant", SR.MUTANTS)
def test_the_scenes_see_each_defect(mutant):
    """Each deliberate defect of subpix_ref.MUTANTS changes at least one output bit somewhere on the scenes, and -- so that a wrong mask offset cannot
    hide at the one window the rest of the suite uses -- the mask, border and bb1 / bb2 defects do so at EVERY window.  The one of INVISIBLE is
    held to what is said there."""
    changed = collections.Counter()
    traced = 0
    for img, pts, win, stop in _scene_runs():
        want = SR.corner_subpix(img, pts, win, *stop, trace=True)
        got = SR.corner_subpix(img, pts, win, *stop, trace=True, mutate=mutant)
        changed[win] += int((bits(got[0]) != bits(want[0])).any(1).sum())
        traced += int((got[1] != want[1]).sum() + (got[3] != want[3]).sum())
    print(mutant, sorted(changed.items()), traced)
    if mutant == "pairwise_sum":
        t = (SR.rect_subpix(*S.texture(), 17)[:, 1:-1, 2:] - SR.rect_subpix(*S.texture(), 17)[:, 1:-1, :-2]).astype(np.float64).reshape(96, -1) ** 2 * SR.mask(7).ravel()
        differ = int((t.sum(1) != np.cumsum(t, axis=1)[:, -1]).sum())
        print("sums that differ:", differ, "of 96")
        assert not sum(changed.values()) and differ >= 10, (mutant, changed, differ)
        return
    assert sum(changed.values()) >= 1, mutant
    if mutant in ("mask_neighbour", "mask_shifted", "mask_npexp", "reflect101", "bb_swapped"):
        assert all(changed[win] >= 1 for win in S.WINS), (mutant, sorted(changed.items()))


def test_at_most_two_defects_are_invisible():
    assert len(INVISIBLE) <= 2 and set(INVISIBLE) <= set(SR.MUTANTS) and len(SR.MUTANTS) == 10


# ---------------------------------------------------------------------------------------------------------------------
# d. truth
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["axis", "sheared"])
def test_junction_truth(kind):
    """The image is exactly point-symmetric about (23.5, 19.5), so the corner equation's exact fixed point is that corner.  From 16 starts up to
    win - 1 away, at eps = 0 and 100 iterations, windows 2 .. 7: max |p - corner| <= JUNCTION_BOUND = 4 x the worst error of the float64 form of the
    model (the same iteration with no float32 rounding, measured here and written down in subpix_scenes.JUNCTION_F64_ERR: 0 on the axis-aligned
    junction, at most 3.6e-15 on the sheared one) + one float32 ulp of 23.5 for the final rounding of a coordinate = 1.9e-6 px.  Window 1 is left out:
    with its 3 x 3 support the float64 form itself does not get there (4.2e-5 after 100 iterations on the axis-aligned junction, 0.9 px on the sheared
    one, whose slanted edge a 3 x 3 window cannot tell from a step).
    With bb1 and bb2 exchanged the bound must break on the sheared junction.  (On the axis-aligned one the exchange is invisible for a start on the
    diagonal, by the symmetry x <-> y; these starts are off it, so it breaks there too, which is printed and not asserted.)"""
    img = S.junction(kind)
    for k, win in enumerate(S.JUNCTION_WINS):
        starts = S.junction_starts(win)
        assert np.abs(starts - F32(S.JUNCTION_TRUTH)).max() <= win - 1 and (np.abs(starts - F32(S.JUNCTION_TRUTH)).min(1) > 0).all()
        e64 = S.junction_error(SR.corner_subpix_f64(img, starts, win, *S.JUNCTION_STOP))
        print(f"{kind} win {win}: float64 form {e64:.3e} (recorded {S.JUNCTION_F64_ERR[kind][k]:.3e})")
        assert e64 <= S.JUNCTION_BOUND - 2.0 ** -19, (kind, win, e64)  # the recorded errors still stand: within the 4 x that the bound grants them
        for name, p in (("model", S.junction_model(kind, win)), ("oracle", KO.corner_subpix(img, starts, win, *S.JUNCTION_STOP))):
            e = S.junction_error(p)
            print(f"{kind} win {win} {name}: max |p - corner| = {e:.3e}, bound {S.JUNCTION_BOUND:.3e}")
            assert e <= S.JUNCTION_BOUND, (kind, win, name, e)
        e = S.junction_error(S.junction_model(kind, win, "bb_swapped"))
        print(f"{kind} win {win}, bb1 and bb2 exchanged: {e:.3e}")
        assert kind != "sheared" or e > S.JUNCTION_BOUND, (win, e)
        _same(KO.corner_subpix(img, starts, win, *S.JUNCTION_STOP), S.junction_model(kind, win), (kind, win))
