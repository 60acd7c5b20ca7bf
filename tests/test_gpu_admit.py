"""TrackerSession.admit, the one admission of the clip drivers (velocity_amd.driver): frame 0 of several clips as ONE frame-0 batch call whose device
outputs initialise the slots, and the session's own record of what each slot must keep alive.  On frames 0 and 1 of sequence B of the stills fixture
(1024 x 768) and their mirror image, in a session of three slots of which slot 1 is never initialised."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BORDER = (180, 140)
ARRAYS = ("vg", "vp", "p", "ids", "P", "B", "S", "t", "pose_info")
SCALARS = ("res", "n_cur", "n_pose", "frame_i", "klt_flags")


def _same_state(a, b, where):
    """Two streams of sessions of one capacity hold the same state.  The world points are compared up to the tracks frame 0 found (S[0, 2]): the rows of p3
    beyond them are never written or read (k_sess_init copies the counted rows only), so there a re-admitted slot keeps what its last clip left."""
    k = int(a["S"][0, 2])
    assert k == int(b["S"][0, 2]) > 100, where
    for key in ARRAYS:
        assert np.array_equal(a[key], b[key], equal_nan=True), (where, key)
    assert np.array_equal(a["p3"][:k], b["p3"][:k]), where
    assert all(a[key] == b[key] for key in SCALARS), (where, [(a[key], b[key]) for key in SCALARS])


def test_admit_is_one_batch_call_and_the_session_keeps_what_each_slot_needs(monkeypatch):
    import torch

    from velocity_amd import _lib as L
    from velocity_amd.driver import Frame0Settings, TrackerSession, frame0_batch

    stills = np.load(os.path.join(ROOT, "tests", "golden", "stills_gray.npz"))
    K, q = stills["b_K"], stills["b_q"]
    frames = stills["b_frames"][:2]
    H, W = frames[0].shape
    assert (W, H) == (1024, 768)
    qm = q.copy()  # the mirrored clip and its corners: tests/test_gpu_queue.py::_clips
    qm[:, 0] = (W - 1) - qm[:, 0]
    qm = qm[[1, 0, 3, 2]]
    f = [torch.from_numpy(x).cuda() for x in frames]
    m = [torch.from_numpy(np.ascontiguousarray(x[:, ::-1])).cuda() for x in frames]
    settings = Frame0Settings(roi_border=BORDER)
    clip, mirror = (f[0], q, 0.5, 0.0), (m[0], qm, 7.25, 100.0)  # (frame 0, corners, time0, frame_no0)
    t1, t2 = np.float32([0.75, 0.0, 7.5]), np.float32([1.0, 0.0, 7.75])  # the clocks of the two steps (slot 1 idle)
    n1, n2 = np.float32([1, 0, 101]), np.float32([2, 0, 102])

    def session():
        return TrackerSession(K, W, H, settings.cap, nhist=4, batch=3)

    lib = L.load()
    calls, batch_fn = [], lib.vh_frame0_init_batch
    monkeypatch.setattr(lib, "vh_frame0_init_batch", lambda *a: (calls.append(a[1]), batch_fn(*a))[1])

    # 1. slots 0 and 2 in ONE call; slot 1 is never initialised
    ses = session()
    adm = ses.admit([(0,) + clip, (2,) + mirror], settings)
    assert calls == [2], calls
    got = [ses.state(0), None, ses.state(2)]
    # the long way: frame0_batch read back to the host, then init_stream with those arrays.  init_stream takes exactly its session's capacity of tracks
    # (it has no count to pass), so each clip gets a session of capacity k = the tracks found, and the admitted slot is compared on its first k track rows
    # (the point lists p / ids and the records B / S whole); its rows beyond k must be dead: masks off, history NaN.  pose_info is left out here: no
    # step has written it yet.  res: init_stream passes it as a float32.
    long_way = frame0_batch([f[0], m[0]], [q, qm], K, roi_border=BORDER)
    assert calls == [2, 2]
    for slot, a, f0, (frame0, _, time0, frame_no0) in ((0, adm[0], long_way[0], clip), (2, adm[1], long_way[1], mirror)):
        k = len(f0["p"])
        assert k == int(got[slot]["S"][0, 2]) > 100
        one = TrackerSession(K, W, H, k, nhist=4, batch=1)
        one.init_stream(0, frame0, f0["p"], f0["p3"], f0["vp"], f0["t"], time0=time0, frame_no=frame_no0, res0=f0["res"])
        want, st = one.state(0), got[slot]
        for key in ("p", "ids", "B", "S", "t"):
            assert np.array_equal(st[key], want[key], equal_nan=True), (slot, key)
        for key in ("vg", "vp", "p3"):
            assert np.array_equal(st[key][:k], want[key]), (slot, key)
        assert np.array_equal(st["P"][:, :k], want["P"], equal_nan=True), slot
        assert not st["vg"][k:].any() and not st["vp"][k:].any() and np.isnan(st["P"][:, k:]).all(), slot
        assert (st["n_cur"], st["n_pose"], st["frame_i"], st["klt_flags"]) == (want["n_cur"], want["n_pose"], want["frame_i"], want["klt_flags"]) == (k, 0, 0, 0)
        assert np.float32(st["res"]) == np.float32(want["res"]) == st["S"][0, 3]
        # what admit hands back: the ROIs and the plate pose the state does not hold
        assert a.boxa == f0["boxa"] and a.boxb == f0["boxb"]
        assert np.array_equal(a.R0.cpu().numpy().reshape(3, 3), f0["R"]) and float(a.res0.item()) == f0["res"]
    assert not np.array_equal(got[0]["B"][0], got[2]["B"][0])  # (the two clips are two clips)

    # 2. one step for all three, slot 1 idle; then slot 0 is admitted AGAIN, with the mirrored clip, while slot 2 carries on
    ses.step([f[1], None, m[1]], time_s=t1, frame_no=n1)
    ses.admit([(0,) + mirror], settings)
    ses.step([m[1], None, m[0]], time_s=np.float32([t1[2], 0, t2[2]]), frame_no=np.float32([n1[2], 0, n2[2]]))
    assert calls == [2, 2, 1]
    # ... against a session in which slot 0 was never admitted again (its first clip carries on),
    ref = session()
    ref.admit([(0,) + clip, (2,) + mirror], settings)
    ref.step([f[1], None, m[1]], time_s=t1, frame_no=n1)
    ref.step([f[0], None, m[0]], time_s=t2, frame_no=n2)
    _same_state(ses.state(2), ref.state(2), "slot 2 beside a re-admitted slot")
    # ... and against a fresh admission of the mirrored clip: the first admission's tensors are released, the neighbour's are not
    fresh = session()
    fresh.admit([(0,) + mirror], settings)
    fresh.step([m[1], None, None], time_s=np.float32([t1[2], 0, 0]), frame_no=np.float32([n1[2], 0, 0]))
    _same_state(ses.state(0), fresh.state(0), "slot 0 admitted again")
    assert ses.state(0)["frame_i"] == 1 and ses.state(2)["frame_i"] == 2
    assert ses._init_keep[1] is None and ses._keep[1] is None  # the idle slot holds nothing
    assert ses._init_keep[0][0].data_ptr() != ses._init_keep[2][0].data_ptr() and ses._keep[0] is m[1] and ses._keep[2] is m[0]
