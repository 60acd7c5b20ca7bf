"""velocity_amd.driver.run_queue on the real stills: a queue of clips of different lengths on a few resident streams.  Every clip must come out as
run_sequence gives it alone -- the assertions of test_gpu_stills.py::test_run_sequences_batches_clips_like_single_runs -- whatever slot it lands in,
whoever its neighbours are and however the slots are split over sessions."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from scenes import stills  # noqa: E402, F401 (a fixture)

BORDER = (180, 140)


def _clips(stills):
    """Seven clips of lengths 12, 4, 7, 9, 2, 12, 3 from sequence B; four of them pass the MSV frame 5.  The fixture holds SEVEN frames of sequence B
    (IMG_4127..4133), so the twelve-frame clip is the sequence there and back again -- frames 0..6, then 5..1, on a clock that keeps running with the
    same intervals -- and the shorter clips are its prefixes (up to seven frames: the stills as they are)."""
    back = [0, 1, 2, 3, 4, 5, 6, 5, 4, 3, 2, 1]
    t7 = stills["b_times"]
    frames, q = np.ascontiguousarray(stills["b_frames"][back]), stills["b_q"]
    times = np.concatenate([t7, t7[6] + np.cumsum(np.diff(t7)[::-1])[:5]])
    W = frames.shape[2]
    qm = q.copy()
    qm[:, 0] = (W - 1) - qm[:, 0]
    qm = qm[[1, 0, 3, 2]]
    mirrored = np.ascontiguousarray(frames[:, :, ::-1])
    n = len(frames)
    return [dict(frames=frames, q=q, times=times, name="b"),
            dict(frames=frames[:4], q=q, times=times[:4], name="b[:4]"),
            dict(frames=mirrored[:7], q=qm, times=times[:7], name="b mirrored[:7]"),
            dict(frames=frames[:9], q=q, times=(times * np.float32(1.5) + np.float32(2.0))[:9], frame_numbers=list(range(100, 109)), name="b slow[:9]"),
            dict(frames=frames[:2], q=q, times=times[:2], name="b[:2]"),
            dict(frames=mirrored, q=qm, times=times, name="b mirrored"),
            dict(frames=frames[:3], q=q, times=times[:3], name="b[:3]")], n


_SINGLE = {}


def _single(c, K, border, fallback=False):
    """run_sequence on the clip alone, computed once per clip and configuration."""
    from velocity_amd.driver import run_sequence

    key = (c["name"], border, fallback)
    if key not in _SINGLE:
        _SINGLE[key] = run_sequence(c["frames"], c["q"], K, times=c["times"], frame_numbers=c.get("frame_numbers"), roi_border=border, out=None, live=False,
                                    name=c["name"], fallback=fallback)
    return _SINGLE[key]


def _same_as_single(g, one, where):
    assert g["n_tracks0"] == one["n_tracks0"] > 100 and g["boxb"] == one["boxb"], where
    assert np.array_equal(g["vg"], one["vg"]) and np.array_equal(g["vp"], one["vp"]) and np.array_equal(g["p"], one["p"]) and np.array_equal(g["ids"], one["ids"]), where
    assert g["P"].shape == one["P"].shape and g["B"].shape == one["B"].shape and g["S"].shape == one["S"].shape, where
    for r in (0, 1, 4):
        assert np.array_equal(g["P"][r], one["P"][r], equal_nan=True), (where, r)
    np.testing.assert_allclose(g["B"], one["B"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(g["S"][:, [0, 2, 3, 4, 5, 6, 7, 8]], one["S"][:, [0, 2, 3, 4, 5, 6, 7, 8]], rtol=1e-6, equal_nan=True)
    assert g["lines"][0] == one["lines"][0] and g["lines"][1] == one["lines"][1], where
    assert len(g["lines"]) == len(one["lines"])
    for a_, b_ in zip(g["lines"][2:-2], one["lines"][2:-2]):
        assert a_[:13] == b_[:13] and a_[26:] == b_[26:], (a_, b_)  # every column but procTime
    assert g["lines"][-2] == one["lines"][-2], where  # Speed / Res summary


def test_run_queue_gives_every_clip_what_run_sequence_gives_it_alone(stills, monkeypatch):
    from velocity_amd import _lib as L
    from velocity_amd.driver import run_queue

    clips, n = _clips(stills)
    assert n == 12
    K = stills["b_K"]
    lib = L.load()
    calls, batch_fn = [], lib.vh_frame0_init_batch
    monkeypatch.setattr(lib, "vh_frame0_init_batch", lambda *a: (calls.append(a[1]), batch_fn(*a))[1])
    runs = {}
    for ns in (1, 2):
        del calls[:]
        got = run_queue(clips, K, streams=3, sessions=ns, roi_border=BORDER)
        assert len(got) == len(clips) and got[0]["sessions"] == ns and run_queue.last_stats["steps"] == 18
        # all admissions of a session at one step are ONE frame-0 batch call: steps 0, 3, 6, 7, 11 of the plan (two sessions: slots 0-1 and slot 2)
        assert calls == ([3, 1, 1, 1, 1] if ns == 1 else [2, 1, 1, 1, 1, 1]), calls
        runs[ns] = got
    for k, (c, g) in enumerate(zip(clips, runs[1])):
        _same_as_single(g, _single(c, K, BORDER), c["name"])
        assert g["P"].shape[2] == len(c["frames"])
    msv = [bool(np.array_equal(g["vp"], g["vg"])) and len(c["frames"]) > 5 for c, g in zip(clips, runs[1])]
    assert msv == [True, False, True, True, False, True, False]  # the clips that passed their frame 5 re-triangulated: every live track is a pose track
    # the split over sessions changes nothing, bit for bit
    for g, h in zip(runs[1], runs[2]):
        for key in ("vg", "vp", "p", "ids", "B", "p3", "t0", "R0", "res0", "n_tracks0", "boxa", "boxb", "klt_flags"):
            assert np.array_equal(g[key], h[key]), key
        assert np.array_equal(g["P"], h["P"], equal_nan=True) and np.array_equal(g["S"][:, [0, 2, 3, 4, 5, 6, 7, 8]], h["S"][:, [0, 2, 3, 4, 5, 6, 7, 8]], equal_nan=True)
        assert g["lines"][-2] == h["lines"][-2]


def test_run_queue_pulls_clips_only_when_a_slot_is_free(stills):
    """The same clips from a generator that counts what it has handed out.  The generator stands in for a decoder that is slower than the tracker -- it
    hands a clip out only once the device has caught up -- so what has landed by then is the same in every run: when the first finished clip (the
    4-frame one) is reported, the three first clips and the one that took its slot have been pulled, and nothing else."""
    import torch

    from velocity_amd.driver import run_queue

    clips, n = _clips(stills)
    K = stills["b_K"]
    pulled, seen = [0], []

    def source():
        for c in clips:
            torch.cuda.synchronize()
            pulled[0] += 1
            yield c

    def on_result(index, res):
        seen.append((index, pulled[0]))
        assert res["n_tracks0"] > 100

    with pytest.raises(ValueError, match="max_frames"):
        run_queue(source(), K, streams=3, roi_border=BORDER)
    pulled[0] = 0
    got = run_queue(source(), K, streams=3, max_frames=n, sessions=1, on_result=on_result, roi_border=BORDER)
    assert seen[0][0] == 1 and seen[0][1] <= 3 + 1, seen
    assert sorted(i for i, _ in seen) == list(range(len(clips))), seen  # every result exactly once
    for c, g in zip(clips, got):
        _same_as_single(g, _single(c, K, BORDER), c["name"])
    with pytest.raises(ValueError, match="more than max_frames"):
        run_queue(iter(clips), K, streams=3, max_frames=8, roi_border=BORDER)


def test_run_queue_with_fewer_clips_than_slots(stills):
    from velocity_amd.driver import run_queue

    clips, _ = _clips(stills)
    K = stills["b_K"]
    got = run_queue([clips[2]], K, streams=3, sessions=1, roi_border=BORDER)
    assert len(got) == 1 and run_queue.last_stats["mean_idle_slots"] == 2.0
    _same_as_single(got[0], _single(clips[2], K, BORDER), "alone")


def test_run_queue_recovers_a_failed_stream_like_run_sequence(stills):
    """fallback=True under sequence A's camera and border (the configuration of test_gpu_session_fallback.py::
    test_run_sequences_gives_each_clip_what_run_sequence_gives_it_alone): A fails at its frame 1 and is recovered, in a slot another clip has just left
    (streams = 2: B[:4] and A first, then B[:3] and A[:2]); the B clips beside it never count a recovery."""
    from velocity_amd.driver import run_queue

    K, border = stills["a_K"], (233, 167)
    a = dict(frames=stills["a_frames"], q=stills["a_q"], times=stills["a_times"], name="a")
    clips = [dict(frames=stills["b_frames"][:4], q=stills["b_q"], times=stills["b_times"][:4], name="b[:4] cam a"), a,
             dict(frames=stills["b_frames"][:3], q=stills["b_q"], times=stills["b_times"][:3], name="b[:3] cam a"),
             dict(frames=stills["a_frames"][:2], q=stills["a_q"], times=stills["a_times"][:2], name="a[:2]")]
    got = run_queue(clips, K, streams=2, sessions=1, roi_border=border, fallback=True)
    for c, g in zip(clips, got):
        one = _single(c, K, border, fallback=True)
        _same_as_single(g, one, c["name"])
        assert tuple(g["recoveries"]) == tuple(one["recoveries"]), c["name"]
    assert tuple(got[1]["recoveries"]) == (1, 1) and tuple(got[0]["recoveries"]) == tuple(got[2]["recoveries"]) == (0, 0)
    assert got[1]["S"][1:, 2].min() >= 90
