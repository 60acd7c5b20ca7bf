"""Refinement of frame windows of a clip, the parts that need no GPU: the NumPy model of a window (tests/refine_window_ref.py) against the whole-clip
model, the window schedule (refine_window_starts), the merge of the windows' speeds (merge_window_speeds), the binding and the drivers' argument
refusals."""
import numpy as np
import pytest

import refine_ref as RR
import refine_window_ref as RW
from velocity_amd import synth


def _clip(nt=24, nf=9, seed=71):
    """A small clip as the session keeps it: history P [5, nt, nf] (float32), points p3 and records B [nf, 14] (float32) with the camera positions in
    columns 3:6 (row 0 zero) and the time in column 12."""
    K = synth.K_1080P.astype(np.float64)
    P, pw0, cw0 = synth.ba_scene(nt, nf, seed=seed, K=K)
    B = np.zeros((nf, 14), np.float32)
    B[:, 3:6] = cw0
    B[0, 3:6] = 0
    B[:, 12] = np.float32(3.0) + np.arange(nf, dtype=np.float32) / np.float32(25.0)
    return K, P.astype(np.float32), pw0, B


def test_window_zero_of_the_whole_clip_is_the_whole_clip_model_exactly():
    K, P, p3, B = _clip()
    n = P.shape[2]
    a, b = RW.refine_window_ref(K, P, p3, B, 0, n), RR.refine_ref(K, P, p3, B, n)
    assert a.pop("first") == 0 and a.pop("f_first") == b["trace"][0, 0] and a.pop("f_last") == b["trace"][-1, 0] and a.keys() == b.keys()
    assert a["nt"] == b["nt"] > 0 and a["iterations"] == b["iterations"] > 0 and a["converged"] == b["converged"]
    for key in ("ids", "cw", "pw", "trace", "dr", "speed"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    assert a["speed_mean"] == b["speed_mean"] and a["speed_std"] == b["speed_std"]


def test_a_mid_clip_window_keeps_a_track_that_is_dead_at_the_end_of_the_clip():
    K, P, p3, B = _clip()
    P[:, 5, 7:] = np.nan    # track 5 dies at frame 7, track 9 at frame 4, track 11 is born dead
    P[:, 9, 4:] = np.nan
    P[:, 11, :] = np.nan
    whole = RR.refine_ref(K, P, p3, B, 9)
    assert not {5, 9, 11} & set(whole["ids"])
    mid = RW.refine_window_ref(K, P, p3, B, 2, 4)  # frames 2..5
    assert 5 in mid["ids"] and 9 not in mid["ids"] and 11 not in mid["ids"]
    assert np.array_equal(mid["ids"], RW.window_ids(P, 2, 4)) and np.all(np.diff(mid["ids"]) > 0)
    assert mid["nt"] == whole["nt"] + 1 and set(whole["ids"]) < set(mid["ids"])
    early = RW.refine_window_ref(K, P, p3, B, 0, 4)
    assert {5, 9} <= set(early["ids"])
    # the window's coordinates: camera 0 at the origin, the others relative to B[first, 3:6], the points shifted the other way
    Pw, pw0, Bw = RW.window_inputs(P, p3, B, 2, 4)
    assert Pw.shape == (5, 24, 4) and np.all(Bw[0, 3:6] == 0) and Bw.dtype == np.float64
    assert np.array_equal(Bw[:, 3:6], B[2:6, 3:6].astype(np.float64) - B[2, 3:6].astype(np.float64))
    assert np.array_equal(pw0, p3 + B[2, 3:6].astype(np.float64))
    assert np.array_equal(Bw[:, 12].astype(np.float32), B[2:6, 12])
    assert mid["cw"].shape == (4, 3) and np.all(mid["cw"][0] == 0) and np.isnan(mid["speed"][0]) and np.all(np.isfinite(mid["speed"][1:]))


@pytest.mark.parametrize("n,window,stride", [(12, 4, None), (12, 4, 1), (12, 4, 2), (260, 16, None), (9, 4, 3), (31, 8, 5), (2, 2, None), (7, 2, 1)])
def test_window_starts_cover_every_frame_and_every_step(n, window, stride):
    from velocity_amd.driver import refine_window_starts

    starts = refine_window_starts(n, window) if stride is None else refine_window_starts(n, window, stride)
    st = window - 1 if stride is None else stride
    assert starts[0] == 0 and starts[-1] == n - window and all(b > a for a, b in zip(starts, starts[1:]))
    assert starts[:-1] == list(range(0, n - window + 1, st))[: len(starts) - 1] and all(b - a <= st for a, b in zip(starts, starts[1:]))
    frames, steps = np.zeros(n, int), np.zeros(n, int)
    for f in starts:
        frames[f:f + window] += 1
        steps[f + 1:f + window] += 1
    assert frames.min() >= 1 and steps[1:].min() >= 1
    if stride is None and (n - 1) % (window - 1) == 0:
        assert steps[1:].max() == 1  # the default stride covers each step exactly once when the windows tile the clip


def test_window_starts_edge_cases_and_refusals():
    from velocity_amd.driver import refine_window_starts

    assert refine_window_starts(8, 8) == [0]              # n == W: the whole clip
    assert refine_window_starts(9, 8) == [0, 1]           # n == W + 1: the end-aligned window overlaps all but one frame
    assert refine_window_starts(12, 4) == [0, 3, 6, 8]
    assert refine_window_starts(10, 4) == [0, 3, 6]
    assert refine_window_starts(12, 4, 2) == [0, 2, 4, 6, 8]
    for args, word in (((3, 4), "shorter"), ((8, 1), "two frames"), ((8, 4, 0), "stride"), ((8, 4, 4), "stride"), ((8, 4, -1), "stride")):
        with pytest.raises(ValueError, match=word):
            refine_window_starts(*args)


def test_merge_window_speeds_means_and_cover():
    from velocity_amd.driver import merge_window_speeds

    nan = np.nan
    wins = [dict(first=0, speed=np.array([nan, 10.0, 12.0, 14.0]), nt=30, iterations=4, converged=1, f_last=0.5),
            dict(first=2, speed=np.array([nan, 20.0, 22.0, 24.0]), nt=25, iterations=5, converged=1, f_last=0.7),
            dict(first=3, speed=np.array([nan, 40.0, 43.0, 46.0]), nt=7, iterations=10, converged=0, f_last=0.9)]
    m = merge_window_speeds(7, wins)
    assert np.array_equal(m["cover"], [0, 1, 1, 2, 2, 2, 1])
    assert np.isnan(m["speed"][0])
    np.testing.assert_allclose(m["speed"][1:], [10.0, 12.0, (14.0 + 20.0) / 2, (22.0 + 40.0) / 2, (24.0 + 43.0) / 2, 46.0], rtol=1e-15)
    assert m["speed_mean"] == m["speed"][1:].mean() and m["speed_std"] == m["speed"][1:].std()
    assert np.array_equal(m["first"], [0, 2, 3]) and np.array_equal(m["nt"], [30, 25, 7]) and np.array_equal(m["iterations"], [4, 5, 10])
    assert np.array_equal(m["converged"], [1, 1, 0]) and np.array_equal(m["f_last"], [0.5, 0.7, 0.9])
    # a step nobody covers is NaN and is counted as uncovered
    gap = merge_window_speeds(6, [wins[0], dict(wins[1], first=3, speed=np.array([nan, 20.0, 22.0]))])
    assert np.array_equal(gap["cover"], [0, 1, 1, 1, 1, 1])
    hole = merge_window_speeds(8, [wins[0], dict(wins[1], first=4)])
    assert hole["cover"][4] == 0 and np.isnan(hole["speed"][4]) and np.isnan(hole["speed_mean"])
    # one window that is the whole clip: its own speeds
    one = merge_window_speeds(4, wins[:1])
    assert np.array_equal(one["speed"][1:], [10.0, 12.0, 14.0]) and np.array_equal(one["cover"], [0, 1, 1, 1])


def test_ba_line_of_a_clip_refined_in_windows():
    from velocity_amd.driver import _merged_ba, ba_line

    nan = np.nan
    wins = [dict(first=0, speed=np.array([nan, 10.0, 12.0]), nt=30, iterations=4, converged=1, f_last=0.5),
            dict(first=2, speed=np.array([nan, 20.0, 22.0]), nt=25, iterations=5, converged=1, f_last=0.75)]
    ba = _merged_ba(5, wins, 3, 2)
    assert ba["window"] == 3 and ba["stride"] == 2
    assert ba_line(ba) == "BA speed = 16.00 +/- 5.10 km/h (2 windows of 3 frames, 25-30 tracks, f = 0.750 pixels)"


def test_the_new_entry_points_are_declared_and_bound():
    import ctypes as C

    from velocity_amd import _lib as L

    declared = L.declared_symbols()
    lib = L.load()
    for s in ("vh_session_refine_windows_size", "vh_session_refine_windows_workspace", "vh_session_refine_windows"):
        assert s in declared and s in L._SIGS and hasattr(lib, s), s
    assert L._SIGS["vh_session_refine_windows"][1][1] == C.POINTER(L.RefineWindow) and C.sizeof(L.RefineWindow) == 8
    names = [k for k, _ in L.RefineWindowRecord._fields_]
    assert names[:6] == ["bytes", "slot", "first", "nt", "iterations", "converged"] and names[-4:] == ["n0", "nf", "max_iter", "with_points"]
    # the bad-argument paths of the two size queries need no device
    assert lib.vh_session_refine_windows_size(None, 4, 10, 0, None) == 0 and b"vh_session_refine_windows_size" in lib.vh_last_error()
    assert lib.vh_session_refine_windows_workspace(None, 1, 4) == 0 and b"vh_session_refine_windows_workspace" in lib.vh_last_error()


@pytest.mark.parametrize("kw,words", [(dict(refine_window=4), "refine_window needs refine"),
                                      (dict(refine="ba", refine_window=1), "refine_window = 1"),
                                      (dict(refine="ba", refine_window=257), "refine_window = 257"),
                                      (dict(refine="ba", refine_window=4, refine_stride=0), "refine_stride = 0"),
                                      (dict(refine="ba", refine_window=4, refine_stride=4), "refine_stride = 4"),
                                      (dict(refine="ba", refine_stride=2), "refine_stride needs refine_window")])
def test_the_drivers_refuse_bad_window_arguments_before_anything_is_queued(kw, words):
    """The refusal comes first in every driver: nothing of the clip is looked at (the frames here are not even images) and no device is needed."""
    from velocity_amd.driver import run_queue, run_sequence, run_sequences

    K = synth.K_1080P
    with pytest.raises(ValueError, match=words):
        run_sequence([None, None], None, K, fps=25.0, out=None, **kw)
    with pytest.raises(ValueError, match=words):
        run_sequences([dict(frames=[None, None], q=None, times=[0, 1])], K, **kw)
    with pytest.raises(ValueError, match=words):
        run_queue([dict(frames=[None, None], q=None, times=[0, 1])], K, streams=1, **kw)


def test_the_accepted_window_arguments():
    from velocity_amd.driver import _check_refine

    assert _check_refine(None) == (False, None, None) and _check_refine("ba") == (True, None, None)
    assert _check_refine("ba", 8) == (True, 8, 7) and _check_refine("ba", 8, 3) == (True, 8, 3) and _check_refine("ba", 256) == (True, 256, 255)
    assert _check_refine("ba", 2) == (True, 2, 1)
