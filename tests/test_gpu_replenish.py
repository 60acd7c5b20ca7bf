"""Replacing lost tracks with new corners on the device (TrackerSession(replenish=...), vh_session_set_replenish) against its NumPy model
tests/replenish_ref.py::ReplenishOracle, on the scenes of tests/replenish_scenes.py -- 640 x 360 frames, at most 128 frame-0 tracks and 64 spare rows,
nhist 16, MSV frame 3, a birth every 2 frames, baseline 3.  tests/test_replenish_cpu.py asserts on the same scenes that no newborn's gate and no prefix
cut is a near-tie, so every comparison here runs without exclusions: masks, ids, points, born, tri and n_rows exactly, p3, B and S with the tolerances
of session_support.equals_oracle."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import refine_ref as RR  # noqa: E402
import refine_window_ref as RW  # noqa: E402
import replenish_scenes as RS  # noqa: E402
from replenish_ref import ReplenishOracle  # noqa: E402
from session_support import same_dict  # noqa: E402


def _session(scenes, replenish=RS.REP, spare=RS.SPARE, n0=None, W=RS.W, H=RS.H, first_slot=0, **kw):
    """A session of len(scenes) slots (None: never initialised), every stream on its own clock (time0 = 10 b; first_slot: the b of slot 0)."""
    from velocity_amd.driver import TrackerSession

    first = next(s for s in scenes if s is not None)
    ses = TrackerSession(first["K"], W, H, len(first["p"]) if n0 is None else n0, nhist=RS.NHIST, batch=len(scenes), msv_frame=RS.MSV_FRAME,
                         replenish=replenish, spare=spare, replenish_settings=RS.DET, **kw)
    for b, sc in enumerate(scenes):
        if sc is not None:
            ses.init_stream(b, sc["frames"][0], sc["p"], sc["p3"], sc["vp"], RS.T0, time0=10.0 * (b + first_slot), K=sc["K"])
    return ses


def _oracle(sc, b=0, replenish=RS.REP, spare=RS.SPARE):
    return ReplenishOracle(sc["K"], sc["frames"][0], sc["p"], sc["p3"], sc["vp"], RS.T0, replenish, RS.DET, spare=spare, time0=10.0 * b, nhist=RS.NHIST,
                           msv_frame=RS.MSV_FRAME)


def _clock(b, k):
    return np.float32(10.0 * b + k / (25.0 + b))


def _step(ses, scenes, ks):
    """One global step: stream b gets frame ks[b] of its clip (None: it sits the step out)."""
    import torch

    frames = [None if k is None else torch.from_numpy(scenes[b]["frames"][k]).cuda() for b, k in enumerate(ks)]
    ses.step(frames, time_s=[np.float32(0) if k is None else _clock(b, k) for b, k in enumerate(ks)], frame_no=[0 if k is None else k for k in ks])


def _equals_model(st, orc, where):
    assert st["frame_i"] == orc.i, where
    for key, want in (("vg", orc.vg), ("vp", orc.vp), ("ids", np.nonzero(orc.vg)[0]), ("p", orc.p), ("born", orc.born), ("tri", orc.tri)):
        assert np.array_equal(st[key], want), (where, key)
    assert st["n_rows"] == orc.n_rows and st["n_cur"] == len(orc.p), where
    assert np.array_equal(st["P"][[0, 1, 4]], orc.P[[0, 1, 4]], equal_nan=True), (where, "history rows 0, 1, 4")
    np.testing.assert_allclose(st["p3"], orc.p3, rtol=1e-4, atol=1e-5, err_msg=str(where))
    n = orc.i + 1
    np.testing.assert_allclose(st["B"][:n, 12:14], orc.B[:n, 12:14], rtol=0, atol=0)
    np.testing.assert_allclose(st["S"][1:n, [0, 2, 4, 5]], orc.S[1:n, [0, 2, 4, 5]], rtol=0, atol=0)
    np.testing.assert_allclose(st["S"][1:n, [3, 6, 7, 8]], orc.S[1:n, [3, 6, 7, 8]], rtol=1e-4)


def test_device_equals_the_model_after_every_step():
    sc = RS.scene()
    ses, orc = _session([sc]), _oracle(sc)
    _equals_model(ses.state(0), orc, 0)
    for k in range(1, RS.NHIST):
        _step(ses, [sc], [k])
        orc.step(sc["frames"][k], _clock(0, k), k)
        _equals_model(ses.state(0), orc, k)
    born, tri, counts = ses.replenish_state(0)
    assert counts.tolist() == [orc.n_rows, int(orc.counts["born"].sum()), int(orc.counts["promoted"].sum()), int(orc.counts["rejected"].sum())]
    assert counts[1] > 0 and counts[2] > 0 and orc.n_rows > len(sc["p"])  # the clip did replace tracks, and some of them joined the pose


def test_a_strict_gate_rejects_and_the_rejected_stay_tracked():
    """max_reproj between the newborns' errors of the scene (test_replenish_cpu.py holds the threshold away from every one of them): both outcomes of
    the gate on the device."""
    sc = RS.scene()
    ses, orc = _session([sc], replenish=RS.REP_STRICT), _oracle(sc, replenish=RS.REP_STRICT)
    for k in range(1, 11):
        _step(ses, [sc], [k])
        orc.step(sc["frames"][k], _clock(0, k), k)
    st = ses.state(0)
    _equals_model(st, orc, 10)
    _, _, counts = ses.replenish_state(0)
    assert counts[2] == orc.counts["promoted"].sum() > 0 and counts[3] == orc.counts["rejected"].sum() > 0
    rejected = (st["born"] > 0) & (st["born"] + RS.REP.baseline <= 10) & (st["tri"] == 0) & st["vg"]
    assert rejected.any() and not st["vp"][rejected].any()


# own frame of (stream 0, stream 1, stream 2) at every global step.  Stream 1 starts two steps late; stream 2 (the smaller camera) reaches its birth frame
# 5 at step 5 and sits steps 6 and 7 out, parked there, while streams 0 and 1 pass their birth and promotion frames.
BATCH_TABLE = [(1, None, 1), (2, None, 2), (3, 1, 3), (4, 2, 4), (5, 3, 5), (6, 4, None), (7, 5, None), (8, 6, 6), (9, 7, 7), (10, 8, 8), (11, 9, 9)]


def test_a_batch_of_three_slots_equals_each_stream_alone():
    import torch

    scenes = [RS.scene(), RS.scene(seed=1234), RS.scene(seed=4321, w=480, h=270, n0=96)]
    ses = _session([scenes[0], None, scenes[2]], n0=128)
    solo = [_session([scenes[0]], n0=128), None, _session([scenes[2]], n0=128, W=480, H=270, first_slot=2)]
    for g, ks in enumerate(BATCH_TABLE, 1):
        if g == 3:  # stream 1 starts later
            sc = scenes[1]
            ses.init_stream(1, sc["frames"][0], sc["p"], sc["p3"], sc["vp"], RS.T0, time0=10.0, K=sc["K"])
            solo[1] = _session([sc], n0=128, first_slot=1)
        idle = {b: ses.state(b) for b, k in enumerate(ks) if k is None}  # (slot 1 before its start: a slot never initialised is a legal idle stream)
        _step(ses, scenes, ks)
        for b, k in enumerate(ks):
            if k is None:
                same_dict(ses.state(b), idle[b], (g, b, "idle"))
                continue
            solo[b].step([torch.from_numpy(scenes[b]["frames"][k]).cuda()], time_s=[_clock(b, k)], frame_no=[k])
            same_dict(ses.state(b), solo[b].state(0), (g, b))
    rows = [ses.state(b)["n_rows"] for b in range(3)]
    assert rows[0] > 128 and rows[1] > 128 and rows[2] > 96, rows  # every stream had births
    assert ses.state(2)["frame_i"] == 9 and ses.state(1)["frame_i"] == 9


def test_option_off_on_a_session_with_spare_rows_is_a_plain_session():
    sc = RS.scene()
    n = len(sc["p"])
    off, plain, small = _session([sc], replenish=None), _session([sc], replenish=None, spare=0, n0=n + RS.SPARE), _session([sc], replenish=None, spare=0)
    for k in range(1, 8):
        for s in (off, plain, small):
            _step(s, [sc], [k])
    a, b, c = off.state(0), plain.state(0), small.state(0)
    assert "born" not in a and "tri" not in a and "n_rows" not in a
    same_dict(a, b, "spare rows against a plain session of as many rows")
    for key in c:  # ... and against the plain session of n rows, on the rows that one has
        x = a[key]
        if key in ("vg", "vp", "p3"):
            x = x[:n]
        elif key == "P":
            x = x[:, :n]
        assert np.array_equal(np.asarray(x), np.asarray(c[key]), equal_nan=np.asarray(c[key]).dtype.kind == "f"), key
    assert not a["vg"][n:].any() and np.isnan(a["P"][:, n:]).all()


def test_births_stop_when_the_rows_are_exhausted():
    """10 spare rows: the first birth fills them; slot 1, whose arrays follow slot 0's on the device, is initialised and never stepped -- nothing of it
    may change."""
    sc, other = RS.scene(), RS.scene(seed=1234)
    ses, orc = _session([sc, other], spare=10, n0=128), _oracle(sc, spare=10)
    beside = ses.state(1)
    for k in range(1, 10):
        _step(ses, [sc, other], [k, None])
        orc.step(sc["frames"][k], _clock(0, k), k)
        _equals_model(ses.state(0), orc, k)
    st = ses.state(0)
    assert st["n_rows"] == ses.n0 == len(sc["p"]) + 10 and orc.counts["born"].sum() == 10
    assert [b["entered"] for b in orc.births] == [10] and st["n_cur"] < len(sc["p"])  # later births were due and had nowhere to go
    same_dict(ses.state(1), beside, "the slot beside")


def test_a_stream_without_tracks_has_no_birth():
    sc = RS.scene()
    p = np.full_like(sc["p"], -40.0)  # every window far outside the frame: no track survives the first step
    ses = _session([dict(sc, p=p)])
    for k in range(1, 7):
        _step(ses, [sc], [k])
    st = ses.state(0)
    assert st["n_cur"] == 0 and st["n_rows"] == len(p) and not st["vg"].any() and (st["born"][len(p):] == -1).all()
    assert ses.replenish_state(0)[2].tolist() == [len(p), 0, 0, 0]


def _ba_equals(got, ref, nf, where):
    assert got["nt"] == ref["nt"] > 0 and np.array_equal(got["ids"], ref["ids"]), where
    assert got["iterations"] == ref["iterations"] and got["converged"] == ref["converged"], where
    for key in ("cw", "pw", "dr", "speed", "speed_mean", "speed_std"):
        np.testing.assert_allclose(got[key], ref[key], rtol=1e-6, atol=1e-8, equal_nan=True, err_msg=f"{where}: {key}")
    np.testing.assert_allclose(got["trace"][:, 0], ref["trace"][:, 0], rtol=1e-6, err_msg=where)


def test_refinement_of_a_replenished_slot():
    """Whole clip: the tracks alive from frame 0 (refine_ref's own selection: newborns have no frame 0).  A late window: alive through it AND
    triangulated -- more tracks than the same clip has there without the option."""
    sc = RS.scene()
    AT, FIRST, NF = 10, 7, 4
    ses, plain = _session([sc]), _session([sc], replenish=None)
    for k in range(1, AT + 1):
        _step(ses, [sc], [k])
        _step(plain, [sc], [k])
    st = ses.state(0)
    whole = ses.refine([0]).result()[0]
    ref = RR.refine_ref(sc["K"], st["P"], st["p3"], st["B"], AT + 1)
    _ba_equals(whole, ref, AT + 1, "whole clip")
    assert (st["born"][whole["ids"]] == 0).all() and whole["nt"] < st["n_cur"]
    win = ses.refine_windows([(0, FIRST)], NF, with_points=True).result()[0]
    P = st["P"].copy()
    P[4, st["tri"] == 0] = np.nan  # the model's selection: a row that is not triangulated has no world point
    ref = RW.refine_window_ref(sc["K"], P, st["p3"], st["B"], FIRST, NF)
    _ba_equals(win, ref, NF, "late window")
    newborn = st["born"][win["ids"]] > 0
    assert newborn.any() and (st["tri"][win["ids"]] == 1).all()
    assert win["nt"] > plain.refine_windows([(0, FIRST)], NF).result()[0]["nt"]
    # the last two frames: the rows born at frame 9 are tracked through them and not yet triangulated -- they are left out
    last = ses.refine_windows([(0, AT - 1)], 2, with_points=True).result()[0]
    _ba_equals(last, RW.refine_window_ref(sc["K"], P, st["p3"], st["B"], AT - 1, 2), 2, "last two frames")
    alive_untri = np.isfinite(st["P"][4, :, AT - 1:AT + 1]).all(1) & (st["tri"] == 0)
    assert alive_untri.any() and not np.isin(np.nonzero(alive_untri)[0], last["ids"]).any() and (st["tri"][last["ids"]] == 1).all()


def test_run_sequence_with_replenish_equals_stepping_by_hand():
    from velocity_amd.driver import Frame0Settings, TrackerSession, run_sequence

    clip = RS.plate_clip()
    n = len(clip["frames"])
    kw = dict(max_corners=100, min_distance=10.0, roi_border=(300, 200))
    res = run_sequence(clip["frames"], clip["q"], clip["K"], times=clip["times"], msv_frame=RS.MSV_FRAME, live=False, out=None, replenish=RS.REP, spare=RS.SPARE, **kw)
    settings = Frame0Settings(**kw)
    import torch

    ses = TrackerSession(clip["K"], RS.W, RS.H, settings.cap, nhist=n, msv_frame=RS.MSV_FRAME, replenish=RS.REP, spare=RS.SPARE, replenish_settings=settings)
    dev = [torch.from_numpy(f).cuda() for f in clip["frames"]]
    ses.admit([(0, dev[0], clip["q"], clip["times"][0], 0)], settings)
    for i in range(1, n):
        ses.step([dev[i]], time_s=float(clip["times"][i]), frame_no=float(i))
    st = ses.state(0)
    k = st["n_rows"]
    assert k > int(st["S"][0, 2]) and res["P"].shape == (5, k, n)  # the result keeps the rows the births used
    for key in ("vg", "vp", "p3"):
        assert np.array_equal(res[key], st[key][:k]), key
    assert np.array_equal(res["P"], st["P"][:, :k, :n], equal_nan=True) and np.array_equal(res["S"][:, [0, 2, 3]], st["S"][:n, [0, 2, 3]])
    assert np.array_equal(res["ids"], st["ids"]) and np.array_equal(res["p"], st["p"])
    rp = res["replenish"]
    assert np.array_equal(rp["born_frame"], st["born"][:k]) and np.array_equal(rp["tri"], st["tri"][:k])
    born, _, counts = ses.replenish_state(0)
    assert rp["born"].sum() == counts[1] > 0 and rp["promoted"].sum() == counts[2] > 0 and rp["rejected"].sum() == counts[3]
    assert rp["rows_left"] == ses.n0 - k and any("replenish" in ln.lower() for ln in res["lines"])
    assert np.array_equal(np.bincount(born[born > 0], minlength=n), rp["born"])


def test_the_batch_drivers_equal_run_sequence():
    """run_sequences and run_queue with the option on: every clip's result equals run_sequence's on the clip alone (the queue reads born / tri right
    behind the export of a finished clip)."""
    from velocity_amd.driver import run_queue, run_sequence, run_sequences

    clips = [RS.plate_clip(), RS.plate_clip(seed=2025)]
    kw = dict(max_corners=100, min_distance=10.0, roi_border=(300, 200), msv_frame=RS.MSV_FRAME, replenish=RS.REP, spare=RS.SPARE)
    alone = [run_sequence(c["frames"], c["q"], c["K"], times=c["times"], live=False, out=None, **kw) for c in clips]
    for name, got in (("run_sequences", run_sequences(clips, clips[0]["K"], **kw)), ("run_queue", run_queue(clips, clips[0]["K"], 2, **kw))):
        for b, (g, a) in enumerate(zip(got, alone)):
            assert g["replenish"]["born"].sum() > 0, (name, b)
            for key in ("P", "vg", "vp", "p3", "ids", "p"):
                assert np.array_equal(g[key], a[key], equal_nan=g[key].dtype.kind == "f"), (name, b, key)
            assert np.array_equal(g["S"][:, [0, 2, 3, 6, 7, 8]], a["S"][:, [0, 2, 3, 6, 7, 8]], equal_nan=True), (name, b)
            for key in ("born", "promoted", "rejected", "born_frame", "tri"):
                assert np.array_equal(g["replenish"][key], a["replenish"][key]), (name, b, key)
            assert g["replenish"]["rows_left"] == a["replenish"]["rows_left"] and g["lines"][-1] == a["lines"][-1] and "Replenish" in g["lines"][-1]


def test_a_set_call_inside_a_capture_is_refused():
    import torch

    from velocity_amd import _lib as L

    sc = RS.scene()
    ses = _session([sc], replenish=None)
    rp = L.replenish_params(RS.REP, RS.DET)
    x = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        x += 1  # (the capture holds something whatever the call does)
        rc = ses.lib.vh_session_set_replenish(ses.handle, C.byref(rp), L.stream_ptr())
        msg = ses.lib.vh_last_error()
    assert rc == -6 and b"capture" in msg and b"vh_session_set_replenish before capturing" in msg, (rc, msg)
    torch.cuda.synchronize()
    # ... and left the option off and the session usable
    _step(ses, [sc], [1])
    assert ses.state(0)["frame_i"] == 1
    L.check(ses.lib.vh_session_set_replenish(ses.handle, C.byref(rp), L.stream_ptr()), "vh_session_set_replenish")
