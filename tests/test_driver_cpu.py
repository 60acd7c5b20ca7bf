"""The host-side pieces the three clip drivers of velocity_amd.driver share (no GPU): clip_result, which turns a stream's state into the result dict and its
printed lines, and Frame0Settings, the frame-0 configuration they hand down."""
import numpy as np
import pytest

from velocity_amd.driver import TABLE_HEADER, Admitted, Frame0Settings, clip_result, summary_lines, table_row

NHIST, N0, K_TRACKS, N = 6, 8, 5, 4


def _state():
    """A stream of a session sized for 6 frames and 8 tracks after a 4-frame clip whose frame 0 found 5 tracks: NaN history beyond the clip, dead rows beyond
    the tracks."""
    rng = np.random.default_rng(7)
    P = np.full((5, N0, NHIST), np.nan, np.float32)
    P[:, :K_TRACKS, :N] = rng.normal(size=(5, K_TRACKS, N))
    B = np.zeros((NHIST, 14), np.float32)
    B[:N] = rng.normal(size=(N, 14))
    S = np.zeros((NHIST, 9), np.float32)
    S[:N] = rng.uniform(1, 50, size=(N, 9))
    S[:N, 0] = np.arange(N)
    S[0, 2], S[0, 4], S[0, 8] = K_TRACKS, np.nan, np.nan
    vg = np.zeros(N0, bool)
    vg[[0, 2, 3]] = True
    vp = vg.copy()
    vp[3] = False
    return dict(vg=vg, vp=vp, p=rng.normal(size=(3, 2)).astype(np.float32), ids=np.array([0, 2, 3], np.int32), P=P, B=B, S=S, p3=rng.normal(size=(N0, 3)),
                t=B[N - 1, 3:6].copy(), res=1.5, n_cur=3, n_pose=2, frame_i=N - 1, klt_flags=0, pose_info=np.zeros(2, np.int32))


def test_clip_result_cuts_the_state_to_the_clip_and_prints_its_table():
    st = _state()
    before = {k: np.copy(v) for k, v in st.items()}
    clip = dict(n=N, name="hand made", frame_numbers=[100, 101, 102, 103])
    f0 = Admitted((1, 2, 3, 4), (5, 6, 7, 8), np.arange(9.0), 0.25)
    recoveries = np.array([1, 1], np.int32)
    res = clip_result(st, clip, f0, seconds=2.0, step_seconds=0.5, sessions=2, recoveries=recoveries)
    assert res["P"].shape == (5, K_TRACKS, N) and res["B"].shape == (N, 14) and res["S"].shape == (N, 9)
    assert res["vg"].shape == res["vp"].shape == (K_TRACKS,) and res["p3"].shape == (K_TRACKS, 3)
    assert res["n_tracks0"] == K_TRACKS and res["sessions"] == 2 and res["klt_flags"] == 0 and np.array_equal(res["recoveries"], [1, 1])
    assert np.array_equal(res["P"], before["P"][:, :K_TRACKS, :N]) and np.array_equal(res["B"], before["B"][:N])
    assert np.array_equal(res["vg"], before["vg"][:K_TRACKS]) and np.array_equal(res["vp"], before["vp"][:K_TRACKS])
    assert np.array_equal(res["p3"], before["p3"][:K_TRACKS]) and np.array_equal(res["p"], before["p"]) and np.array_equal(res["ids"], before["ids"])
    assert np.array_equal(res["t0"], res["B"][0, :3]) and res["t0"].dtype == np.float32
    assert np.array_equal(res["R0"], np.arange(9.0).reshape(3, 3)) and res["res0"] == 0.25 and res["boxa"] == (1, 2, 3, 4) and res["boxb"] == (5, 6, 7, 8)
    # every column of S but procTime is the state's; procTime: 0 at frame 0, the mean time of a step after it
    assert np.array_equal(res["S"][:, [0, 2, 3, 4, 5, 6, 7, 8]], before["S"][:N, [0, 2, 3, 4, 5, 6, 7, 8]], equal_nan=True)
    assert np.array_equal(res["S"][:, 1], np.float32([0, 0.5, 0.5, 0.5]))
    assert res["seconds"] == 2.0 and res["ms_per_frame"] == 500.0
    lines = res["lines"]
    assert lines[0:2] == ["Starting image processing on hand made ...", TABLE_HEADER]
    assert lines[2:-2] == [table_row(res["S"][i]) for i in range(N)] and len(lines) == N + 4
    assert lines[-2:] == summary_lines(res["S"], N, [100, 101, 102, 103], 2.0)
    # a live table gives the column frame by frame
    live = clip_result(st, clip, f0, 2.0, 0.5, 1, recoveries, proc=np.array([0.3, 0.1, 0.2, 0.4]))
    assert np.array_equal(live["S"][:, 1], np.float32([0.3, 0.1, 0.2, 0.4])) and live["ms_per_frame"] == 500.0
    assert live["lines"][2:-2] == [table_row(live["S"][i]) for i in range(N)]
    # the inputs were not touched, and nothing of the result is a view of them
    for k, v in before.items():
        assert np.array_equal(st[k], v, equal_nan=True), k
    want = {k: np.copy(res[k]) for k in ("P", "B", "S", "vg", "vp", "p", "p3", "ids", "t0", "R0", "recoveries")}
    for k in ("P", "B", "S", "p", "p3"):
        st[k] += 1
    st["vg"][:], st["vp"][:], st["ids"][:] = ~st["vg"], ~st["vp"], -1
    f0.R0[:] = -1
    for k, v in want.items():
        assert np.array_equal(res[k], v, equal_nan=True), k


def test_frame0_settings_derive_capacity_plate_and_detector():
    from velocity_amd.common import worldPointsLicensePlate

    s = Frame0Settings()
    assert (s.plate, s.roi_border, s.max_corners, s.quality, s.block, s.harris_k, s.subpix, s.use_harris, s.min_distance) == \
        ("Chile", (700, 500), 1000, 0.01, 5, 0.04, (5, 100, 0.001), True, 0.0)  # vidExample.py:105-127
    assert s.cap == 1004 and Frame0Settings(max_corners=37).cap == 41
    w = s.plate_w
    assert w.dtype == np.float64 and w.shape == (12,) and w.flags["C_CONTIGUOUS"] and w is s.plate_w
    assert np.array_equal(w, np.asarray(worldPointsLicensePlate("Chile"), np.float64).reshape(12))
    assert s.reference_detector and Frame0Settings(use_harris=1, min_distance=0).reference_detector
    assert not Frame0Settings(use_harris=False).reference_detector and not Frame0Settings(min_distance=10).reference_detector
    with pytest.raises(Exception):
        s.max_corners = 5  # frozen
    for md in (float("inf"), -float("inf"), float("nan")):
        with pytest.raises(ValueError, match="min_distance must be finite"):
            Frame0Settings(min_distance=md)
