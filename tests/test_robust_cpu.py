"""The model of bundle adjustment with Huber weights (tests/robust_ref.py): against tests/anchor_ref.py without a threshold, against the dense
weighted solve, what the weights do to a speed when a few measurements are wrong (the experiment behind profiles/ba_robust/truth.json), and the
drivers' argument checks and printed line.  No GPU."""
import numpy as np
import pytest

import anchor_ref as AR
import robust_ref as RB
from oracle import nls_oracle as O
from velocity_amd import synth

SHAPES = [(24, 4, 700), (50, 6, 400), (24, 22, 701)]  # tests/test_anchor_cpu.py's


def _packed(nt, nf, seed, moved=0):
    K = synth.K_1080P.astype(float)
    P, pw, cw = synth.ba_scene(nt, nf, seed=seed)
    if moved:
        P = RB.move_measurements(P, count=moved, seed=seed + 1)[0]
    z, bad, x0, nt, nc = O.ba_pack(K, P, pw, cw)
    return K, z, bad, x0, nt, nc


@pytest.mark.parametrize("nt,nf,seed", SHAPES)
def test_without_a_threshold_the_model_is_anchor_ref_bit_for_bit(nt, nf, seed):
    K, z, bad, x0, nt, nc = _packed(nt, nf, seed, moved=3)
    some = np.arange(nt) < 4
    for fixed in (None, some):
        ed, ef = AR.anchored_step(x0, z, K, nc, nt, fixed=fixed, bad=bad)
        for delta in (None, 0.0):
            d, f, n = RB.robust_step(x0, z, K, nc, nt, fixed=fixed, bad=bad, delta=delta)
            assert d.tobytes() == ed.tobytes() and f == ef and n == 0
        ex, etr = AR.solve_anchored(K, z, bad, x0, nt, nt, nc, fixed=fixed)
        x, tr, nout = RB.solve_robust(K, z, bad, x0, nt, nt, nc, fixed=fixed)
        assert x.tobytes() == ex.tobytes() and tr.tobytes() == etr.tobytes() and len(nout) == len(tr) and not nout.any()
    # a threshold no residual reaches changes nothing either, and counts nothing
    d, f, n = RB.robust_step(x0, z, K, nc, nt, fixed=some, bad=bad, delta=1e6)
    ed, ef = AR.anchored_step(x0, z, K, nc, nt, fixed=some, bad=bad)
    assert d.tobytes() == ed.tobytes() and f == ef and n == 0


@pytest.mark.parametrize("nt,nf,seed", SHAPES)
def test_robust_step_is_the_dense_weighted_solve(nt, nf, seed):
    """inv(J^T W J + I) J^T W r at the agreement tests/test_anchor_cpu.py asks of the anchored forms (atol 1e-8), with and without anchors, on a start where
    the weights are at work; the returned rms residual is the unweighted one."""
    K, z, bad, x0, nt, nc = _packed(nt, nf, seed, moved=3)
    assert not bad.any()
    some = np.arange(nt) < 4
    for fixed in (np.zeros(nt, bool), some):
        d, f, n = RB.robust_step(x0, z, K, nc, nt, fixed=fixed, delta=1.0)
        dense = RB.dense_robust_step(x0, z, K, nc, nt, fixed, 1.0)
        plain, fp = AR.anchored_step(x0, z, K, nc, nt, fixed=fixed)
        print(f"({nt}, {nf}, {seed}), {int(fixed.sum())} anchors: {n} down-weighted, max |schur - dense| = {np.abs(d - dense).max():.3g}, "
              f"max |step| = {np.abs(d).max():.3g}, max |robust - plain| = {np.abs(d - plain).max():.3g}")
        np.testing.assert_allclose(d, dense, rtol=0, atol=1e-8)
        assert 3 <= n <= nt * (nc + 1) and f == fp and np.abs(d - plain).max() > 1e-3
        assert np.all(d[: 3 * int(fixed.sum())] == 0.0)


def test_the_weights_of_a_pair():
    r = np.array([[[3.0, 4.0], [0.3, 0.4], [0.6, 0.8], [0.0, 0.0]]])
    sw, down = RB.huber_sqrt_weights(r, 1.0)
    assert down.tolist() == [[True, False, False, False]]  # |r| = 1 exactly is not down-weighted
    assert sw[0, 0] == np.sqrt(1.0 / 5.0) and (sw[0, 1:] == 1.0).all()


SEEDS = range(8)
_TRUTH = {}


def _truth():
    """The (40, 6) scenes with 3 % of their measurements moved, seeds 0..7, solved plain and with 1 pixel: once for the tests below."""
    if not _TRUTH:
        for s in SEEDS:
            K, z, x0, nt, nc, moved = RB.outlier_problem(40, 6, s, 0.03)
            bad = np.zeros(z.size, bool)
            xp, _, _ = RB.solve_robust(K, z, bad, x0, nt, nt, nc)
            xr, tr, nout = RB.solve_robust(K, z, bad, x0, nt, nt, nc, delta=1.0)
            _TRUTH[s] = (moved, RB.step_error(xp, nt, nc), RB.step_error(xr, nt, nc), nout)
    return _TRUTH


def test_huber_weights_keep_the_speed_where_plain_least_squares_loses_it():
    """Every one of the eight seeds: Huber 1 px is within 2 % of the true camera step, plain least squares off by more than 5 %.
    Measured: plain 0.067 .. 1.36 (median 0.136), Huber 0.0008 .. 0.0099 (median 0.0054), 1 .. 9 of the 200 measurements moved."""
    for s, (moved, plain, robust, _) in _truth().items():
        print(f"seed {s}: {moved} moved, plain {plain:.4f}, huber {robust:.4f}")
    for s, (moved, plain, robust, _) in _truth().items():
        assert 1 <= moved <= 10, s
        assert robust < 0.02, s
        assert plain > 0.05, s


def test_the_last_count_is_the_number_moved():
    for s, (moved, _, _, nout) in _truth().items():
        assert abs(int(nout[-1]) - moved) <= 2 and nout[0] >= moved, (s, moved, nout.tolist())


def test_clean_data_is_left_alone():
    K, z, x0, nt, nc, moved = RB.outlier_problem(40, 6, 0, 0.0)
    bad = np.zeros(z.size, bool)
    xp, _, _ = RB.solve_robust(K, z, bad, x0, nt, nt, nc)
    xr, _, nout = RB.solve_robust(K, z, bad, x0, nt, nt, nc, delta=1.0)
    assert moved == 0 and nout[-1] == 0 and abs(RB.step_error(xp, nt, nc) - RB.step_error(xr, nt, nc)) < 1e-4


def test_refine_robust_is_checked_before_anything_runs():
    from velocity_amd.driver import _check_robust, run_queue, run_sequence, run_sequences

    assert _check_robust("ba", None) is None and _check_robust(None, None) is None and _check_robust("ba", 0) is None
    assert _check_robust("ba", 1) == 1.0 and _check_robust("ba", "0.5") == 0.5
    for call in (lambda: run_sequence([None, None], None, None, fps=25.0, refine_robust=1.0), lambda: run_sequences([], None, refine_robust=1.0),
                 lambda: run_queue([], None, 2, refine_robust=1.0)):
        with pytest.raises(ValueError, match="refine_robust needs refine='ba'"):
            call()
    for bad in (-1.0, float("nan"), float("inf")):
        for call in (lambda: run_sequence([None, None], None, None, fps=25.0, refine="ba", refine_robust=bad),
                     lambda: run_sequences([], None, refine="ba", refine_robust=bad), lambda: run_queue([], None, 2, refine="ba", refine_robust=bad)):
            with pytest.raises(ValueError, match="refine_robust = .*finite number of pixels"):
                call()


def test_merge_and_lines_carry_the_counts():
    from velocity_amd.driver import _merged_ba, _tag_anchor, ba_line

    nan = np.nan
    wins = [dict(first=0, speed=np.array([nan, 10.0, 12.0]), nt=30, nfix=4, iterations=10, converged=0, f_last=0.5, robust=1.0, nout_first=9, nout_last=3),
            dict(first=2, speed=np.array([nan, 20.0, 22.0]), nt=25, nfix=0, iterations=7, converged=1, f_last=0.75, robust=1.0, nout_first=5, nout_last=0)]
    ba = _merged_ba(5, wins, 3, 2)
    assert ba["robust"] == 1.0 and ba["nout_first"].tolist() == [9, 5] and ba["nout_last"].tolist() == [3, 0]
    assert ba_line(ba) == "BA speed = 16.00 +/- 5.10 km/h (2 windows of 3 frames, 25-30 tracks, huber 1 px: 3 of 165 measurements down-weighted, f = 0.750 pixels)"
    assert ba_line(_tag_anchor(ba, "plate")) == ("BA speed = 16.00 +/- 5.10 km/h (2 windows of 3 frames, 25-30 tracks, 0-4 anchors, "
                                                 "huber 1 px: 3 of 165 measurements down-weighted, f = 0.750 pixels)")
    plain = _merged_ba(5, [{k: v for k, v in w.items() if k not in ("robust", "nout_first", "nout_last")} for w in wins], 3, 2)
    assert "robust" not in plain and "nout_last" not in plain
    assert ba_line(plain) == "BA speed = 16.00 +/- 5.10 km/h (2 windows of 3 frames, 25-30 tracks, f = 0.750 pixels)"  # not asked for: the line it was
    whole = dict(nt=20, nfix=4, speed=np.full(8, 40.0), speed_mean=40.456, speed_std=1.0049, f_last=0.08449, iterations=10, converged=0)
    assert ba_line(whole) == "BA speed = 40.46 +/- 1.00 km/h (20 tracks, f = 0.084 pixels)"
    assert ba_line(dict(whole, robust=0.5, nout_first=12, nout_last=7)) == \
        "BA speed = 40.46 +/- 1.00 km/h (20 tracks, huber 0.5 px: 7 of 160 measurements down-weighted, f = 0.084 pixels)"


def test_the_robust_entry_points_are_declared_and_bound():
    from velocity_amd import _lib as L

    declared = L.declared_symbols()
    for s in ("vh_nls_batch_windows_robust", "vh_session_set_refine_robust"):
        assert s in declared and s in L._SIGS and hasattr(L.load(), s), s
    assert len(L._SIGS["vh_nls_batch_windows_robust"][1]) == len(L._SIGS["vh_nls_batch_windows_fixed"][1]) + 2
    # no struct of offsets changed: the tail of a robust record sits at what `bytes` was
    assert [n for n, _ in L.RefineRecord._fields_][-4:] == ["n0", "nhist", "max_iter", "nfix"]
    assert [n for n, _ in L.RefineWindowRecord._fields_][-6:] == ["pw", "nfix", "n0", "nf", "max_iter", "with_points"]
