"""The recovery by feature matching on the product route: vh_match_affine_batch against the single-pair entry and the NumPy model (tests/match_ref.py) bit
for bit, then TrackerSession / run_sequence / run_sequences with fallback=True against the oracles whose klt_main is wrapped with match_ref.recover (the way
tests/test_gpu_match.py checks the drop-in loop).  The model of a frame pair costs seconds of CPU, so every pair is computed once and shared."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import match_ref as MR  # noqa: E402
from oracle import driver_oracle as DO  # noqa: E402 (checker only)
from oracle import klt_oracle as KO  # noqa: E402 (checker only)
from oracle.session_oracle import SessionOracle  # noqa: E402 (checker only)
from scenes import load_stills as stills  # noqa: E402
from velocity_amd import synth  # noqa: E402

W, H, N0, NH = 480, 270, 100, 8
T0 = np.float32([0.0, 0.0, 3.6])
SHIFTS = {"jump": ((0, 100, 103, 106), 0xC0FFEE), "calm": ((0, 3, 6, 9), 0xC0FFEE + 1)}

_REAL_MATCH = MR.match_affine
_MODELS = {}


def _model(im1, im2, p1, **params):
    """match_ref.match_affine, each distinct frame pair computed once per run."""
    key = (np.ascontiguousarray(im1).tobytes(), np.ascontiguousarray(im2).tobytes(), np.asarray(p1, np.float32).tobytes(), tuple(sorted(params.items())))
    if key not in _MODELS:
        _MODELS[key] = _REAL_MATCH(im1, im2, p1, **params)
    return _MODELS[key]


@pytest.fixture(autouse=True)
def _shared_models(monkeypatch):
    monkeypatch.setattr(MR, "match_affine", _model)  # match_ref.recover calls it through the module


@functools.lru_cache(maxsize=None)
def scene():
    K = synth.K_1080P.copy() * (W / 1920.0)
    K[2, 2] = 1.0
    K[2, 0], K[2, 1] = 240.5, 135.5
    p = synth.grid_tracks(N0, W, H, frac=0.5)
    return K, p, synth.plane_pose_scene(p, K), np.ones(N0, bool)


@functools.lru_cache(maxsize=None)
def clip(name):
    c, seed = SHIFTS[name]
    m = [synth.AffineMotion(W, H, tx=ck, ty=0) for ck in c]
    return [synth.render_frame(W, H, mk, 1, seed).numpy() for mk in m]


class Recovering:
    """oracle.klt_oracle.klt_main wrapped with the recovery (match_ref.recover), as test_gpu_match.py wraps it; `ran`: the point count of every recovery."""

    def __init__(self, monkeypatch):
        self.real, self.ran, self.found = KO.klt_main, [], []
        monkeypatch.setattr(KO, "klt_main", self)

    def __call__(self, im, im0, im0_small, p0, lk_coarse=None, lk_fine=None, stages=False, L=None):
        p, v, small, S = self.real(im, im0, im0_small, p0, lk_coarse=lk_coarse, lk_fine=lk_fine, stages=True, L=L)
        if S["flags"] & 1 and len(p0):
            self.ran.append(len(p0))
            rec = MR.recover(im0, im, p0)
            self.found.append(rec is not None)
            if rec is not None:
                p_all, v = rec[0], rec[1]
                p = p_all[v]
        return (p, v, small, S) if stages else (p, v, small)


def launches():
    from velocity_amd import _lib as L

    return L.load().vh_match_launch_count()


def new_session(batch, fallback, clips):
    from velocity_amd.driver import TrackerSession

    K, p, p3, vp = scene()
    ses = TrackerSession(K, W, H, N0, nhist=NH, batch=batch, msv_frame=0, fallback=fallback)
    for b, fr in enumerate(clips):
        ses.init_stream(b, fr[0], p, p3, vp, T0)
    return ses


def new_oracle(frames):
    K, p, p3, vp = scene()
    return SessionOracle(K, frames[0], p, p3, vp, T0, nhist=NH, msv_frame=0)


def step(ses, frames, i):
    import torch

    ses.step([torch.from_numpy(f).cuda() for f in frames], time_s=np.float32(i / 30.0), frame_no=i)


def same_state(st, orc, where):
    assert np.array_equal(st["vg"], orc.vg), (where, "vg")
    assert np.array_equal(st["vp"], orc.vp), (where, "vp")
    assert np.array_equal(st["ids"], np.nonzero(orc.vg)[0]), (where, "ids")
    assert np.array_equal(st["p"], orc.p), (where, "p")


def same_records(st, orc):
    """the tolerances of test_session_matches_reference_loop"""
    for r in (0, 1, 4):
        assert np.array_equal(st["P"][r], orc.P[r], equal_nan=True)
    np.testing.assert_allclose(st["B"], orc.B, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(st["S"][1:, [0, 2, 4, 5]], orc.S[1:, [0, 2, 4, 5]], rtol=0, atol=0)
    np.testing.assert_allclose(st["S"][1:, [3, 6, 7, 8]], orc.S[1:, [3, 6, 7, 8]], rtol=1e-4)


def test_the_batch_equals_the_singles_and_the_model():
    from velocity_amd import KLT

    _, p, _, _ = scene()
    jump = clip("jump")
    m = synth.AffineMotion(W, H, s=0.75, theta_deg=2, tx=60, ty=-20)
    warp = [synth.render_frame(W, H, m, k).numpy() for k in (0, 1)]
    flat = np.full((H, W), 117, np.uint8)
    pairs_in = [(jump[0], jump[1], p), (jump[0], jump[1], p[:37]), (warp[0], warp[1], p), (flat, flat, p)]
    before = launches()
    M, inl, pairs, info = (x.cpu().numpy() for x in KLT._match_call_batch([a for a, _, _ in pairs_in], [b for _, b, _ in pairs_in], [q for _, _, q in pairs_in],
                                                                        {}))
    assert launches() == before + 6, "one launch per matcher kernel whatever the number of pairs"
    print("info", info.tolist())
    assert tuple(info[3]) == (0, 0, 0, 0) and not M[3].any() and not inl[3].any() and not pairs[3].any()
    for k, (a, b, q) in enumerate(pairs_in[:3]):
        ref = MR.match_affine(a, b, q)
        ng = int(ref["info"][1])
        assert ref["M"] is not None and ref["info"][0] == 1 and ng == (2035, 1903, 1449)[k], (k, ref["info"])  # (what the model finds: every pair has one)
        assert np.array_equal(info[k], ref["info"]), (k, info[k], ref["info"])
        assert np.array_equal(M[k].reshape(2, 3), ref["M"]), k
        assert np.array_equal(inl[k, :ng], ref["inl"]) and not inl[k, ng:].any(), k
        assert np.array_equal(pairs[k, :ng], ref["pairs"]) and not pairs[k, ng:].any(), k
    for k, (a, b, q) in enumerate(pairs_in):
        one = [x.cpu().numpy() for x in KLT._match_call(a, b, q, {})]
        for got, single, what in zip((M[k], inl[k], pairs[k], info[k]), one, ("M", "inl", "pairs", "info")):
            assert np.array_equal(got, single), (k, what)


def test_the_batch_entry_refuses_bad_arguments_before_queuing():
    import ctypes as C

    import torch

    from velocity_amd import _lib as L

    _, p, _, _ = scene()
    ws = L.workspace(W, H, 2500)
    im = torch.from_numpy(clip("calm")[0]).cuda()
    pt = torch.from_numpy(p).cuda()
    M, inl, info = torch.zeros(12, dtype=torch.float64, device="cuda"), torch.zeros(5000, dtype=torch.uint8, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda")
    before = launches()

    def call(nb, ims, pts, ns, mp=None):
        tab = lambda v: C.cast((C.c_void_p * len(v))(*v), C.c_void_p)  # noqa: E731
        return ws.lib.vh_match_affine_batch(ws.handle, nb, tab(ims), tab(ims), W, H, W, W, tab(pts), (C.c_int * len(ns))(*ns), C.byref(mp) if mp else None,
                                            L.dptr(M), L.dptr(inl), None, L.dptr(info), L.stream_ptr())

    a, q = im.data_ptr(), pt.data_ptr()
    assert call(0, [a], [q], [N0]) == -1
    assert call(2, [a, None], [q, q], [N0, N0]) == -1
    assert call(2, [a, a], [q, None], [N0, N0]) == -1
    assert call(2, [a, a], [q, q], [N0, 0]) == -1
    assert call(2, [a, a], [q, q], [N0, N0], L.match_params(dict(levels=9))) == -1
    assert launches() == before
    assert ws.lib.vh_match_reserve_batch(ws.handle, 0, W, H, None, L.stream_ptr()) == -1
    assert ws.lib.vh_match_reserve_batch(ws.handle, 2, W, H, None, L.stream_ptr()) == 0


def test_a_failed_stream_recovers_and_its_neighbour_is_untouched(monkeypatch):
    rec = Recovering(monkeypatch)
    clips = [clip("jump"), clip("calm")]
    orcs = [new_oracle(c) for c in clips]
    ses = new_session(2, True, clips)
    for i in (1, 2, 3):
        before = launches()
        step(ses, [c[i] for c in clips], i)
        st = [ses.state(b) for b in (0, 1)]
        assert launches() - before == (6 if i == 1 else 0), i
        for b in (0, 1):
            orcs[b].step(clips[b][i], np.float32(i / 30.0), i)
            same_state(st[b], orcs[b], (i, b))
        assert st[0]["klt_flags"] & 7 == (7 if i == 1 else 0) and st[1]["klt_flags"] & 7 == 0, (i, st[0]["klt_flags"], st[1]["klt_flags"])
    for b in (0, 1):
        same_records(ses.state(b), orcs[b])
    S = ses.state(0)["S"]
    print("tracks alive, jump clip:", S[:4, 2], "calm clip:", ses.state(1)["S"][:4, 2])
    assert tuple(S[1:4, 2]) == (99, 95, 94)
    assert tuple(ses.state(1)["S"][1:4, 2]) == (100, 100, 100)
    assert ses.recoveries().tolist() == [[1, 1], [0, 0]]
    assert rec.ran == [100] and rec.found == [True], "the oracle's recovery ran exactly once, on slot 0's 100 points"


def test_off_changes_nothing(monkeypatch):
    jump, calm = clip("jump"), clip("calm")
    before = launches()
    orc = new_oracle(jump)  # the plain oracle
    ses = new_session(1, False, [jump])
    for i in (1, 2):
        step(ses, [jump[i]], i)
        orc.step(jump[i], np.float32(i / 30.0), i)
        same_state(ses.state(0), orc, i)
        if i == 1:
            st = ses.state(0)
            assert st["n_cur"] == 1 and st["S"][1, 2] == 1 and st["klt_flags"] & 7 == 1
    assert ses.recoveries().tolist() == [[0, 0]]
    states = []
    for fb in (True, False):
        s2 = new_session(2, fb, [calm, calm])
        for i in (1, 2, 3):
            step(s2, [calm[i], calm[i]], i)
        states.append([s2.state(b) for b in (0, 1)])
        assert s2.recoveries().tolist() == [[0, 0], [0, 0]]
    for b in (0, 1):
        for key, val in states[0][b].items():
            a, c = np.asarray(val), np.asarray(states[1][b][key])
            assert a.dtype == c.dtype and a.tobytes() == c.tobytes(), (b, key)
    assert states[0][0]["n_cur"] == 100
    assert launches() == before, "no matcher kernel: the option is off, or no stream failed"


def test_without_a_model_the_blind_fine_stage_stands():
    import torch

    jump = clip("jump")
    gray = np.full((H, W), 128, np.uint8)
    _, p, _, _ = scene()
    assert MR.recover(jump[0], gray, p) is None and MR.match_affine(jump[0], gray, p)["info"][0] == 0
    got = {}
    for fb in (False, True):
        ses = new_session(1, fb, [jump])
        before = launches()
        step(ses, [gray], 1)
        got[fb] = ses.state(0)
        assert launches() - before == (6 if fb else 0)
        if fb:
            assert ses.recoveries().tolist() == [[1, 0]]
            before = launches()
            step(ses, [gray], 2)  # the stream is empty now: left alone
            assert launches() == before and ses.recoveries().tolist() == [[1, 0]]
            assert ses.state(0)["n_cur"] == 0
    assert got[False]["n_cur"] == 0 and got[False]["klt_flags"] & 7 == 1 and got[True]["klt_flags"] & 7 == 3
    for key, val in got[False].items():
        if key != "klt_flags":
            a, c = np.asarray(val), np.asarray(got[True][key])
            assert a.tobytes() == c.tobytes(), key
    del torch


def test_a_step_with_the_option_on_cannot_be_captured():
    import torch

    from velocity_amd import _lib as L

    calm = clip("calm")
    ses = new_session(1, True, [calm])
    frame = torch.from_numpy(calm[1]).cuda()
    ses.set_frames([frame])
    x = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    before = launches()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        x += 1  # (the capture holds something whatever the step does)
        rc = ses.lib.vh_session_step(ses.handle, L.dptr(ses._frames), 0.0, 1.0, L.stream_ptr())
        msg = ses.lib.vh_last_error()
    assert rc == -6 and b"capture" in msg, (rc, msg)
    assert launches() == before and ses.state(0)["frame_i"] == 0


def test_stills_a_through_the_product_measures_the_labelled_speed(monkeypatch):
    from _helpers import same_table
    from velocity_amd.driver import run_sequence

    st = stills()
    frames, times, q, K = st["a_frames"], st["a_times"], st["a_q"], st["a_K"]
    rec = Recovering(monkeypatch)
    with np.errstate(all="ignore"):
        ref = DO.run_sequence(frames, q, K, times, roi_border=(233, 167))
    monkeypatch.setattr(KO, "klt_main", rec.real)
    got = run_sequence(frames, q, K, times=times, roi_border=(233, 167), fallback=True, live=True, clock=lambda: 0.0, out=None)
    print("\n".join(got["lines"]))
    print("the oracle's recovery ran", len(rec.ran), "time(s); tracks alive per frame:", got["S"][:, 2])
    assert len(rec.ran) == 1 and tuple(got["recoveries"]) == (1, 1), "the fallback runs once; frames 2 and 3 track normally"
    assert np.array_equal(got["S"][:, 2], ref["S"][:, 2]) and got["S"][1:, 2].min() >= 90
    assert np.array_equal(got["vg"], ref["vg"]) and np.array_equal(got["vp"], ref["vp"]) and np.array_equal(got["p"], ref["p"])
    for r in (0, 1, 4):
        assert np.array_equal(got["P"][r], ref["P"][r], equal_nan=True)
    np.testing.assert_allclose(got["B"], ref["B"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(got["S"][1:, [0, 2, 4, 5]], ref["S"][1:, [0, 2, 4, 5]], rtol=0, atol=0)
    np.testing.assert_allclose(got["S"][1:, [3, 6, 7, 8]], ref["S"][1:, [3, 6, 7, 8]], rtol=1e-4)
    same_table(got["lines"][2:-1], ref["lines"][2:])
    speed = got["S"][1:, 8]
    assert np.all((speed > 33) & (speed < 46)), speed
    off = run_sequence(frames, q, K, times=times, roi_border=(233, 167), fallback=False, live=True, clock=lambda: 0.0, out=None)
    assert off["S"][1, 2] == 0 and tuple(off["recoveries"]) == (0, 0)


def test_run_sequences_gives_each_clip_what_run_sequence_gives_it_alone():
    from velocity_amd.driver import run_sequence, run_sequences

    st = stills()
    # one call serves one frame size, clip length, camera and ROI border: sequence A, and the first four frames of B under A's camera and border
    K = st["a_K"]
    clips = [dict(frames=st["a_frames"], q=st["a_q"], times=st["a_times"], name="a"),
             dict(frames=st["b_frames"][:4], q=st["b_q"], times=st["b_times"][:4], name="b")]
    many = run_sequences(clips, K, roi_border=(233, 167), fallback=True)
    for c, got in zip(clips, many):
        one = run_sequence(c["frames"], c["q"], K, times=c["times"], roi_border=(233, 167), fallback=True, live=False, out=None, name=c["name"])
        assert got["n_tracks0"] == one["n_tracks0"] > 100 and got["boxb"] == one["boxb"]
        for key in ("vg", "vp", "p", "ids"):
            assert np.array_equal(got[key], one[key]), (c["name"], key)
        for r in (0, 1, 4):
            assert np.array_equal(got["P"][r], one["P"][r], equal_nan=True), (c["name"], r)
        # (records: the tolerances of test_run_sequences_batches_clips_like_single_runs)
        np.testing.assert_allclose(got["B"], one["B"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(got["S"][:, [0, 2, 3, 4, 5, 6, 7, 8]], one["S"][:, [0, 2, 3, 4, 5, 6, 7, 8]], rtol=1e-6, equal_nan=True)
        assert tuple(got["recoveries"]) == tuple(one["recoveries"]), c["name"]
    print("recoveries:", [tuple(m["recoveries"]) for m in many], "tracks alive:", [m["S"][:, 2] for m in many])
    assert tuple(many[0]["recoveries"]) == (1, 1) and many[0]["S"][1:, 2].min() >= 90
