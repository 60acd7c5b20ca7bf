"""Bundle adjustment of frame windows of a clip on the device (vh_session_refine_windows, TrackerSession.refine_windows, the drivers'
refine_window=W) against the NumPy model tests/refine_window_ref.py and against the whole-clip entry (vh_session_refine).

Tolerances: a window against the model is held to what tests/test_gpu_refine.py holds the whole-clip refinement to (and tests/test_gpu_nls.py the
windows call): nt and ids exact, iterations and converged equal, the rest within rtol 1e-6 / atol 1e-8.  Two device solves of the same window are
bit-identical except for the trace, whose sums of squares are accumulated with atomics (rtol 1e-12)."""
import ctypes as C

import numpy as np
import pytest

import refine_window_ref as RW
import scenes as S
from scenes import T0
from session_support import raw_export, same_dict, session_at, step_to
from velocity_amd import synth

pytestmark = pytest.mark.gpu

N0, NHIST, AT, W4 = 150, 12, 8, 4
# (x0, y0, x1, y1) of stream 2 is noise from frame 4 on: the tracks inside fail the forward-backward gate THERE -- tracks that die in the middle of the
# clip (found with oracle/session_oracle.py: 128 tracks live through frames 0..3, 95 of them through 5..8)
PATCH = (0, 0, 120, 240)
_SES = {}


def _patched3():
    """scenes.scenes3 with the patch in its third stream."""
    return S.scenes3(N0, NHIST, patch=PATCH)


def _ses8():
    """THE session of the tests that only read it: at frame AT = 8, with its three host states."""
    if not _SES:
        ses = session_at(_patched3(), AT)
        _SES.update(ses=ses, st=[ses.state(b) for b in range(3)])
    return _SES["ses"], _SES["st"]


def _window_equals_model(got, K, st, first, nf, where):
    """A refined window (unpack_refine_window's dict, with points) against refine_window_ref on the same state."""
    ref = RW.refine_window_ref(K, st["P"], st["p3"], st["B"], first, nf)
    print(f"{where}: nt {got['nt']} / {ref['nt']}, iterations {got['iterations']} / {ref['iterations']}, converged {got['converged']} / {ref['converged']}, "
          f"speed {got['speed_mean']:.4f} +/- {got['speed_std']:.4f} (model {ref['speed_mean']:.4f} +/- {ref['speed_std']:.4f}), f_last {got['f_last']:.4f}, "
          f"max |dcw| {np.abs(got['cw'] - ref['cw']).max():.3g}" + (f", max |dpw| {np.abs(got['pw'] - ref['pw']).max():.3g}" if ref["nt"] else ""))
    assert got["first"] == first and got["nt"] == ref["nt"] and np.array_equal(got["ids"], ref["ids"]), where
    assert got["iterations"] == ref["iterations"] and got["converged"] == ref["converged"], where
    for key in ("cw", "pw", "dr", "speed", "speed_mean", "speed_std"):
        np.testing.assert_allclose(got[key], ref[key], rtol=1e-6, atol=1e-8, equal_nan=True, err_msg=f"{where}: {key}")
    np.testing.assert_allclose(got["trace"][:, 0], ref["trace"][:, 0], rtol=1e-6, err_msg=where)
    if ref["nt"]:
        assert got["f_first"] == got["trace"][0, 0] and got["f_last"] == got["trace"][-1, 0], where
    assert got["cw"].shape == (nf, 3) and np.all(got["cw"][0] == 0) and np.isnan(got["dr"][0]) and np.isnan(got["speed"][0]), where
    return ref


def test_window_zero_of_a_finished_clip_is_the_whole_clip_entry():
    ses, _ = _ses8()
    NF = AT + 1
    new = ses.refine_windows([(b, 0) for b in range(3)], NF, with_points=True).result()
    old = ses.refine([0, 1, 2]).result()
    assert len(new) == len(old) == 3
    for b, (a, o) in enumerate(zip(new, old)):
        assert (a["slot"], a["first"]) == (b, 0)
        assert a["nt"] == o["nt"] > 0 and a["iterations"] == o["iterations"] > 0 and a["converged"] == o["converged"], b
        assert np.array_equal(a["ids"], o["ids"]) and np.array_equal(a["cw"], o["cw"][:NF]) and np.array_equal(a["pw"], o["pw"]), b
        assert np.array_equal(a["dr"], o["dr"], equal_nan=True) and np.array_equal(a["speed"], o["speed"], equal_nan=True), b
        np.testing.assert_allclose(a["trace"], o["trace"], rtol=1e-12)  # (sums of squares accumulated with atomics)
    assert len({a["nt"] for a in new}) == 3  # three track counts, two cameras, one launch sequence


def test_windows_that_are_not_the_whole_clip_equal_the_model():
    ses, st = _ses8()
    scenes = _patched3()
    wins = [(0, 0), (0, 3), (1, 0), (1, 4), (2, 2)]
    assert all(st[b]["frame_i"] == AT and f + W4 - 1 < AT for b, f in wins)  # none of them ends at the current frame
    h = ses.refine_windows(wins, W4, with_points=True)
    got = h.result()
    assert h.done() and len(got) == len(wins)
    for (b, f), g in zip(wins, got):
        assert g["slot"] == b
        _window_equals_model(g, scenes[b][4], st[b], f, W4, f"window ({b}, {f})")
    # without points: the same numbers, no ids / pw in the record
    lean = ses.refine_windows(wins, W4).result()
    for g, l in zip(got, lean):
        assert "ids" not in l and "pw" not in l and l["nt"] == g["nt"] and np.array_equal(l["cw"], g["cw"]) and np.array_equal(l["speed"], g["speed"], equal_nan=True)
    assert ses.refine_window_layout(W4).bytes < ses.refine_window_layout(W4, with_points=True).bytes < ses.refine_layout().bytes


def test_tracks_that_die_mid_clip_belong_to_the_early_window_only():
    ses, st = _ses8()
    K = _patched3()[2][4]
    early, late = ses.refine_windows([(2, 0), (2, 5)], W4, with_points=True).result()
    a, b, cur = set(early["ids"]), set(late["ids"]), set(st[2]["ids"])
    print(f"stream 2: {len(a)} tracks in frames 0..3, {len(b)} in 5..8, {len(a - b)} of the early ones gone, {len(cur)} alive now")
    assert len(a - b) >= 0.1 * len(a), "the scene lost too few tracks in the middle"
    assert len(b) >= 20
    assert cur < a  # a strict superset: the early window holds tracks the slot no longer has
    _window_equals_model(early, K, st[2], 0, W4, "stream 2, frames 0..3")
    _window_equals_model(late, K, st[2], 5, W4, "stream 2, frames 5..8")


def test_the_session_is_only_read():
    ses, twin = session_at(_patched3(), 6), session_at(_patched3(), 6)
    wins = [(0, 1), (1, 2), (2, 3), (2, 0)]  # (2, 3) ends at the current frame, the others before it
    before = [raw_export(ses, b) for b in range(3)]
    mid = ses.refine_windows(wins, W4, with_points=True).result()
    assert [raw_export(ses, b) for b in range(3)] == before
    step_to(ses, _patched3(), 7, 8)
    step_to(twin, _patched3(), 7, 8)
    for b in range(3):
        same_dict(ses.state(b), twin.state(b), f"stream {b} two frames later")
    after = ses.refine_windows(wins, W4, with_points=True).result()  # the same windows once the clip has run on
    for m, a in zip(mid, after):
        assert m["nt"] == a["nt"] > 0 and np.array_equal(m["ids"], a["ids"])
        for key in ("cw", "pw", "speed"):
            assert np.array_equal(m[key], a[key], equal_nan=True), key


def test_refusals_queue_nothing():
    import torch

    from velocity_amd import _lib as L

    ses, _ = _ses8()
    good = [(0, 1), (1, 0), (0, 4), (2, 5)]
    first = ses.refine_windows(good, W4, with_points=True).result()
    lib = ses.lib
    lay = ses.refine_window_layout(W4, 10, True)
    need = int(lib.vh_session_refine_windows_workspace(ses.handle, 3, W4))
    assert need > 0 and lay.bytes % 8 == 0 and need > int(lib.vh_session_refine_windows_workspace(ses.handle, 2, W4))
    recs = torch.zeros(3 * lay.bytes + 8, dtype=torch.uint8, device="cuda")
    work = torch.zeros(need + 256, dtype=torch.uint8, device="cuda")

    def call(wins, nf=W4, max_iter=10, nwin=None, nbytes=need, rec_off=0, work_off=0):
        tab = (L.RefineWindow * max(len(wins), 1))(*[L.RefineWindow(b, f) for b, f in wins])
        rc = lib.vh_session_refine_windows(ses.handle, tab, len(wins) if nwin is None else nwin, nf, max_iter, 1, C.c_void_p(recs.data_ptr() + rec_off),
                                           C.c_void_p(work.data_ptr() + work_off), nbytes, L.stream_ptr())
        return rc, lib.vh_last_error().decode()

    ok = [(0, 1), (1, 1), (2, 1)]
    for kw, words in ((dict(wins=[(0, 1), (3, 0)]), ("slot 3", "3 slots")),                       # a slot outside the session
                      (dict(wins=[(0, 1), (1, -1)]), ("slot 1", "first = -1", "negative")),       # first < 0
                      (dict(wins=[(0, 1), (1, 6)]), ("slot 1, first 6", "frame 9", "frame 8")),   # past the slot's frame counter
                      (dict(wins=[(0, 1), (1, 1), (0, 1)]), ("slot 0, first 1", "twice")),        # the same window twice
                      (dict(wins=ok, nf=1), ("nf = 1", "two frames")),
                      (dict(wins=ok, nf=257), ("nf = 257", "255")),
                      (dict(wins=ok, nf=NHIST + 1), (f"nf = {NHIST + 1}", f"{NHIST} frames")),
                      (dict(wins=ok, max_iter=0), ("max_iter = 0",)),
                      (dict(wins=ok, nwin=0), ("nwin = 0",)),
                      (dict(wins=ok, rec_off=4), ("misaligned", "8-byte")),
                      (dict(wins=ok, work_off=8), ("misaligned", "256-byte")),
                      (dict(wins=ok, nbytes=need - 1), ("workspace", str(need)))):
        rc, msg = call(**kw)
        assert rc == -1 and all(w in msg for w in words), (kw, msg)
    with pytest.raises(RuntimeError, match="twice"):
        ses.refine_windows([(1, 1), (1, 1)], W4)
    with pytest.raises(ValueError, match="no window"):
        ses.refine_windows([], W4)
    torch.cuda.synchronize()
    assert not recs.any().item() and not work.any().item()  # nothing was queued: neither buffer was written
    rc, msg = call(ok)
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert recs[: 3 * lay.bytes].any().item()
    again = ses.refine_windows(good, W4, with_points=True).result()
    for a, b in zip(first, again):
        assert (a["slot"], a["first"], a["nt"], a["iterations"], a["converged"]) == (b["slot"], b["first"], b["nt"], b["iterations"], b["converged"])
        for key in ("ids", "cw", "pw", "dr", "speed"):
            assert np.array_equal(a[key], b[key], equal_nan=True), key
        np.testing.assert_allclose(a["trace"], b["trace"], rtol=1e-12)
    # a request cut into chunks by a small scratch budget gathers the same records in the same order
    one = int(lib.vh_session_refine_windows_workspace(ses.handle, 1, W4))
    with pytest.raises(ValueError, match=r"window \(slot 0, first 6\)"):  # a chunked request refuses a bad window before its first chunk is queued
        ses.refine_windows(good + [(0, 6)], W4, workspace_budget=2 * one)
    h = ses.refine_windows(good, W4, with_points=True, workspace_budget=2 * one)
    assert h.chunk == 2
    for a, b in zip(first, h.result()):
        assert (a["slot"], a["first"], a["nt"]) == (b["slot"], b["first"], b["nt"]) and np.array_equal(a["cw"], b["cw"]) and np.array_equal(a["pw"], b["pw"])


def test_a_request_past_the_launch_chunk_of_one_call():
    """The library launches pack and unpack 256 windows at a time (their table travels in the kernel arguments).  30 slots -- the three scenes, ten times
    -- at their last frame hold 30 x 9 = 270 distinct windows of W4 frames: ONE vh_session_refine_windows call of two launches, the second of 14 windows
    behind 242 padding entries.  The windows are given start-major, so entries 255 and 256 sit in two slots of two cameras."""
    from velocity_amd.driver import TrackerSession

    scenes = _patched3()
    B, last = 30, NHIST - 1
    ses = TrackerSession(scenes[0][4], 320, 240, N0, nhist=NHIST, batch=B, msv_frame=5)
    for b in range(B):
        frames, p, p3, vp, Kb = scenes[b % 3]
        ses.init_stream(b, frames[0], p, p3, vp, T0, time0=10.0 * b, K=Kb)
    dev = [[S.to_cuda(f) for f in sc[0]] for sc in scenes]
    for k in range(1, last + 1):
        ses.step([dev[b % 3][k] for b in range(B)], time_s=[np.float32(10.0 * b + k / (25.0 + b % 3)) for b in range(B)], frame_no=[k] * B)
    wins = [(b, f) for f in range(last - W4 + 2) for b in range(B)]
    assert len(wins) == len(set(wins)) == 270 and wins[255] == (15, 8) and wins[256] == (16, 8)
    one = int(ses.lib.vh_session_refine_windows_workspace(ses.handle, 1, W4))
    h = ses.refine_windows(wins, W4, with_points=True, workspace_budget=2 * len(wins) * one)
    assert h.chunk == len(wins) >= 257  # Python did not split the request
    got = h.result()
    probe = [0, 254, 255, 256, 257, len(wins) - 1]
    for k in probe:
        assert (got[k]["slot"], got[k]["first"]) == wins[k], k
    assert all((g["slot"], g["first"]) == w for g, w in zip(got, wins))
    small = ses.refine_windows([wins[k] for k in probe], W4, with_points=True)
    assert small.chunk == len(probe) < 256
    for k, s in zip(probe, small.result()):
        g = got[k]
        for key in ("slot", "first", "nt", "nfix", "iterations", "converged"):
            assert g[key] == s[key], (k, key)
        assert g["nt"] > 0 and g["iterations"] > 0, k
        for key in ("ids", "cw", "pw", "speed"):
            assert np.array_equal(g[key], s[key], equal_nan=True), (k, key)
        np.testing.assert_allclose(g["trace"], s["trace"], rtol=1e-12)  # (sums of squares accumulated with atomics)
    for k in (255, 256):
        b, f = wins[k]
        _window_equals_model(got[k], scenes[b % 3][4], ses.state(b), f, W4, f"entry {k}: window ({b}, {f})")


# ---- the drivers ---------------------------------------------------------------------------------------------------------------------------------
def _merged_equals(got, want, where, exact_ints=True):
    """Two merged dicts (merge_window_speeds'): the per-window integers exact, the floats within the window tolerances."""
    for key in ("first", "nt", "iterations", "converged", "cover"):
        assert np.array_equal(got[key], want[key]), (where, key, got[key], want[key])
    for key in ("speed", "speed_mean", "speed_std", "f_last"):
        np.testing.assert_allclose(got[key], want[key], rtol=1e-6, atol=1e-8, equal_nan=True, err_msg=f"{where}: {key}")


_LONG_TRAJ = synth.oscillating_traj(period=65.0)


def _long_clip():
    """260 frames of 160 x 120, rendered once: a bounded, periodic camera path (a straight one would leave the scene)."""
    return S.plate_clip(160, 120, 350.0, 260, 907, "260 frames", traj=_LONG_TRAJ)


def test_a_clip_longer_than_the_whole_clip_refinement_takes(monkeypatch):
    from velocity_amd import driver as D

    c = _long_clip()
    n, W = len(c["frames"]), 16
    seen = []
    plain = D.TrackerSession.refine_windows

    def spy(self, *a, **kw):
        seen.append(self)
        return plain(self, *a, **kw)

    monkeypatch.setattr(D.TrackerSession, "refine_windows", spy)
    res = D.run_sequence(c["frames"], c["q"], c["K"], times=c["times"], out=None, live=False, name=c["name"], roi_border=(60, 40), max_corners=56,
                         refine="ba", refine_window=W)
    assert len(seen) == 1 and seen[0].nhist == n == 260
    with pytest.raises(RuntimeError, match="nf = 260: at most 255 free cameras"):
        seen[0].refine([0])
    ba = res["ba"]
    starts = D.refine_window_starts(n, W)
    assert ba["window"] == W and ba["stride"] == W - 1 and list(ba["first"]) == starts and len(starts) == 18
    assert np.all(ba["cover"][1:] >= 1) and ba["cover"][0] == 0 and ba["cover"].max() == 2
    model = D.merge_window_speeds(n, [RW.refine_window_ref(c["K"], res["P"], res["p3"], res["B"], f, W) for f in starts])
    print(f"{n} frames in {len(starts)} windows of {W}: tracks {ba['nt'].min()}-{ba['nt'].max()} of {res['n_tracks0']}, {len(res['ids'])} alive at the end; "
          f"iterations {ba['iterations'].tolist()} / {model['iterations'].tolist()}; speed {ba['speed_mean']:.4f} +/- {ba['speed_std']:.4f} "
          f"(model {model['speed_mean']:.4f} +/- {model['speed_std']:.4f}); max |dspeed| {np.nanmax(np.abs(ba['speed'] - model['speed'])):.3g}")
    assert ba["nt"].min() > 0
    _merged_equals(ba, model, c["name"])
    assert res["lines"][-1] == D.ba_line(ba) and f"({len(starts)} windows of {W} frames, " in res["lines"][-1]


KW = dict(roi_border=(60, 40), max_corners=150)
LENGTHS = (6, 9, 12, 9, 3)  # at two streams clips 2 (12 frames) and 3 (9 frames) end at the same step; the 3-frame clip is shorter than the window


def test_the_drivers_refine_in_windows(monkeypatch):
    from velocity_amd import driver as D

    cams = ((320, 240, 700.0), (256, 192, 560.0))
    clips = [S.plate_clip(*cams[k % 2], n, 700 + k, f"clip {k}") for k, n in enumerate(LENGTHS)]
    K0 = S.camera(320, 240, 650.0)
    alone = [D.run_sequence(c["frames"], c["q"], c["K"], times=c["times"], out=None, live=False, name=c["name"], refine="ba", refine_window=W4, **KW) for c in clips]
    for c, one in zip(clips, alone):
        n = len(c["frames"])
        if n < W4:  # refined whole, with today's record
            assert "window" not in one["ba"] and one["ba"]["cw"].shape == (n, 3) and len(one["ba"]["ids"]) == one["ba"]["nt"] > 0
            continue
        ba, starts = one["ba"], D.refine_window_starts(n, W4)
        assert ba["window"] == W4 and ba["stride"] == W4 - 1 and list(ba["first"]) == starts and np.all(ba["cover"][1:] >= 1) and ba["nt"].min() > 0
        _merged_equals(ba, D.merge_window_speeds(n, [RW.refine_window_ref(c["K"], one["P"], one["p3"], one["B"], f, W4) for f in starts]), c["name"])
        assert one["lines"][-1] == D.ba_line(ba)
    calls = []
    plain = D.TrackerSession.refine_windows

    def spy(self, windows, *a, **kw):
        calls.append(list(windows))
        return plain(self, windows, *a, **kw)

    monkeypatch.setattr(D.TrackerSession, "refine_windows", spy)
    # run_sequences: one call per length; the two 9-frame clips (two cameras) of one session in ONE request
    for idx in ([0], [2], [1, 3]):
        del calls[:]
        got = D.run_sequences([clips[k] for k in idx], K0, sessions=1, refine="ba", refine_window=W4, **KW)
        assert len(calls) == 1 and len(calls[0]) == len(idx) * len(D.refine_window_starts(LENGTHS[idx[0]], W4))
        for k, g in zip(idx, got):
            _merged_equals(g["ba"], alone[k]["ba"], f"run_sequences, clip {k}")
            assert g["lines"][-1] == alone[k]["lines"][-1]
    # run_queue: all five in one queue; one request per step at which windowed clips finished, not one per length
    del calls[:]
    got = D.run_queue(clips, K0, streams=2, sessions=1, max_size=(240, 320), refine="ba", refine_window=W4, **KW)
    plan = D.queue_plan(LENGTHS, 2, 1)
    ends = [[LENGTHS[k] for _, _, k in s["done"] if LENGTHS[k] >= W4] for s in plan]
    assert any(len(set(e)) == 2 for e in ends), "the plan no longer ends two windowed clips of different lengths at one step"
    assert len(calls) == sum(1 for e in ends if e) == 3 < sum(len(set(e)) for e in ends)
    assert sorted(len(c) for c in calls) == sorted(sum(len(D.refine_window_starts(n, W4)) for n in e) for e in ends if e)
    for k, (g, one) in enumerate(zip(got, alone)):
        if LENGTHS[k] >= W4:
            _merged_equals(g["ba"], one["ba"], f"run_queue, clip {k}")
            assert g["lines"][-1].startswith("BA speed = ") and " windows of 4 frames, " in g["lines"][-1]
        else:  # the clip shorter than the window: refined whole, today's record shape
            assert "window" not in g["ba"] and g["ba"]["cw"].shape == (3, 3) and g["ba"]["nt"] == one["ba"]["nt"] and np.array_equal(g["ba"]["ids"], one["ba"]["ids"])
            np.testing.assert_allclose(g["ba"]["speed"], one["ba"]["speed"], rtol=1e-6, atol=1e-8, equal_nan=True)
    # whole-clip mode is untouched by the new keywords' defaults
    assert "window" not in D.run_queue(clips[:1], K0, streams=1, sessions=1, refine="ba", **KW)[0]["ba"]
