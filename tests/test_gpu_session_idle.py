"""A stream may sit a step out (vh_session_step_some; TrackerSession.step with None entries) and a stream's results leave the device as one record
(vh_session_export).  Every stream is held against its own SessionOracle, which sees only that stream's ACTIVE steps, with the comparisons and tolerances
of test_gpu_session.py::test_streams_started_at_different_times_keep_their_own_clock_and_msv_frame; an idle stream's state() must be what it was before
the step, field for field."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle.session_oracle import SessionOracle  # noqa: E402 (checker only)
from scenes import T0, plane_scene, to_cuda  # noqa: E402
from session_support import equals_oracle, same_dict  # noqa: E402
from velocity_amd import synth  # noqa: E402


class _Streams:
    """A session of `len(scenes)` streams (None: a slot that is never initialised) and one oracle per initialised stream, stepped by an activity row."""

    def __init__(self, scenes, W, H, n0, nhist, msv_frame, oracles=None, **kw):
        from velocity_amd.driver import TrackerSession

        self.scenes = scenes
        K = next(s for s in scenes if s is not None)[4]
        self.ses = TrackerSession(K, W, H, n0, nhist=nhist, batch=len(scenes), msv_frame=msv_frame, **kw)
        self.orc, self.k = {}, [0] * len(scenes)
        for b, sc in enumerate(scenes):
            if sc is None:
                continue
            frames, p, p3, vp, Kb = sc
            self.ses.init_stream(b, frames[0], p, p3, vp, T0, time0=10.0 * b)
            if oracles is None or b in oracles:
                self.orc[b] = SessionOracle(Kb, frames[0], p, p3, vp, T0, time0=10.0 * b, nhist=nhist, msv_frame=msv_frame)

    def step(self, active, bgr=None):
        """active: one flag per stream.  Each active stream gets the next frame of its own clip on its own clock."""
        frames, ts, fn = [], [], []
        for b, a in enumerate(active):
            if not a:
                frames.append(None)
                ts.append(np.float32(0))
                fn.append(0)
                continue
            self.k[b] += 1
            k = self.k[b]
            t = np.float32(10.0 * b + k / (25.0 + b))
            frames.append(to_cuda(self.scenes[b][0][k] if bgr is None else bgr[b][k]))
            ts.append(t)
            fn.append(k)
            if b in self.orc:
                self.orc[b].step(self.scenes[b][0][k], t, k)
        if bgr is None:
            self.ses.step(frames, time_s=ts, frame_no=fn)
            return None
        return self.ses.step_bgr(frames, time_s=ts, frame_no=fn)


# global step -> who is active.  Stream 1 is out at steps 2-3; step 2 has a single active stream, step 6 none.  With msv_frame = 3 stream 2 re-triangulates
# at step 3 and is then PARKED at its frame 3 during step 5, in which streams 0 and 1 reach their frame 3 and the MSV kernels are launched for everybody.
TABLE = [(0, 1, 1), (0, 0, 1), (1, 0, 1), (1, 1, 0), (1, 1, 0), (0, 0, 0), (1, 1, 1)]


def _table_run(steps, check):
    W, H, n0 = 480, 270, 220
    run = _Streams([plane_scene(W, H, n0, 6, 555 + 222 * b) for b in range(3)], W, H, n0, nhist=8, msv_frame=3)
    prev = [run.ses.state(b) for b in range(3)]
    for g, active in enumerate(TABLE[:steps], 1):
        run.step(active)
        if not check:
            continue
        cur = [run.ses.state(b) for b in range(3)]
        for b, a in enumerate(active):
            if a:
                equals_oracle(cur[b], run.orc[b], (g, b))
            else:
                same_dict(cur[b], prev[b], (g, b))
        prev = cur
    return run


def test_streams_sit_steps_out_and_keep_their_own_clock_state_and_msv_frame():
    run = _table_run(len(TABLE), True)
    assert [run.orc[b].i for b in range(3)] == [4, 4, 4]  # every stream passed ITS frame 3: each re-triangulated exactly once (p3 is compared at every step)
    assert run.ses.state(2)["vp"].sum() == run.ses.state(2)["vg"].sum()  # vp = vg after the re-triangulation (vidExample.py:160)


def test_a_slot_that_was_never_initialised_is_a_legal_idle_stream():
    W, H, n0 = 480, 270, 220
    run = _Streams([plane_scene(W, H, n0, 5, 1000), None, plane_scene(W, H, n0, 5, 1077)], W, H, n0, nhist=5, msv_frame=0)
    empty = run.ses.state(1)
    for g in range(1, 5):
        run.step((1, 0, 1))
        for b in (0, 2):
            equals_oracle(run.ses.state(b), run.orc[b], (g, b))
        same_dict(run.ses.state(1), empty, g)


def test_idle_streams_inside_the_lk_stream_sets():
    """20 streams x 170 tracks (the first shape of test_session_batches_with_partial_stream_sets: a full fine set of 16 + a tail of 4, one coarse set):
    every third stream sits the odd steps out.  Stream 7 (always active, half of its tracks die in the first step), stream 3 (idle on odd steps, inside
    the full set) and stream 18 (idle on odd steps, in the tail) against their oracles; every idle stream unchanged."""
    W, H, n0, B = 320, 240, 170, 20
    scenes = []
    for b in range(B):
        frames, p, p3, vp, K = plane_scene(W, H, n0, 5, 4000 + 31 * b)
        if b % 3 == 1:
            p = p.copy()
            p[n0 // 2:] = np.float32([-60.0, -60.0])
        scenes.append((frames, p, p3, vp, K))
    run = _Streams(scenes, W, H, n0, nhist=5, msv_frame=0, oracles=(3, 7, 18))
    for g in range(1, 5):
        active = [0 if (b % 3 == 0 and g % 2 == 1) else 1 for b in range(B)]
        before = {b: run.ses.state(b) for b in range(B) if not active[b]}
        run.step(active)
        for b, st in before.items():
            same_dict(run.ses.state(b), st, (g, b))
        for b in (3, 7, 18):
            if active[b]:
                equals_oracle(run.ses.state(b), run.orc[b], (g, b))
    assert [run.orc[b].i for b in (3, 7, 18)] == [2, 4, 2]


def test_an_idle_stream_on_the_unfused_bookkeeping_path():
    """N0 = 4500 > 4096: bookkeeping, the 1024-thread pose kernel and the records are three launches, each of which must pass an idle stream by."""
    W, H, n0 = 960, 540, 4500
    run = _Streams([plane_scene(W, H, n0, 4, 31337), plane_scene(W, H, n0, 3, 31338)], W, H, n0, nhist=4, msv_frame=0)
    for g, active in enumerate([(1, 1), (1, 0), (1, 1)], 1):
        before = run.ses.state(1)
        run.step(active)
        for b in (0, 1):
            if active[b]:
                equals_oracle(run.ses.state(b), run.orc[b], (g, b))
                np.testing.assert_allclose(run.ses.state(b)["t"], run.orc[b].t, rtol=1e-5)
            else:
                same_dict(run.ses.state(b), before, (g, b))


def test_step_bgr_with_an_idle_stream_equals_the_gray_path():
    """step_bgr with None entries == step on the converted gray frames with the same None entries (a stream's two gray buffers alternate on ITS active
    steps: stream 1 is out for two steps in a row, then stream 0 for one)."""
    from oracle import klt_oracle as KO

    W, H, n0, B = 482, 270, 180, 2
    rng = np.random.default_rng(5)
    scenes = [plane_scene(W, H, n0, 6, 321 + 11 * b) for b in range(B)]
    bgr = [[np.clip(np.stack([sc[0][i].astype(int) + rng.integers(-20, 21, (H, W)) * (c - 1) for c in range(3)], -1), 0, 255).astype(np.uint8)
            for i in range(6)] for sc in scenes]
    gray = [([KO.bgr2gray(f) for f in bgr[b]],) + scenes[b][1:] for b in range(B)]
    table = [(1, 1), (1, 0), (1, 0), (0, 1), (1, 1)]
    states = []
    for mode in ("gray", "bgr"):
        run = _Streams(gray, W, H, n0, nhist=6, msv_frame=0, oracles=() if mode == "bgr" else None)
        for g, active in enumerate(table, 1):
            out = run.step(active, bgr=bgr if mode == "bgr" else None)
            if mode == "bgr":
                for b in range(B):
                    assert (out[b] is None) == (not active[b])
                    if active[b]:
                        assert np.array_equal(out[b].cpu().numpy(), gray[b][0][run.k[b]]), (g, b)
        states.append([run.ses.state(b) for b in range(B)])
        if mode == "gray":
            for b in range(B):
                equals_oracle(states[0][b], run.orc[b], b)
    for b in range(B):
        same_dict(states[0][b], states[1][b], b)
    assert [s["frame_i"] for s in states[1]] == [4, 3]


def test_export_is_one_record_equal_to_state():
    """TrackerSession.export(slot).result() == state(slot) for every key, mid-clip (after step 4 of the activity table: stream 2 has re-triangulated, the
    others have not; every history has frames to come, i.e. NaN columns), with the history already in the reference's [5, N0, nhist] order."""
    run = _table_run(4, False)
    ses = run.ses
    lay = ses.record_layout()
    assert lay.n0 == 220 and lay.nhist == 8 and lay.bytes >= lay.P + 4 * 5 * 220 * 8
    handles = [ses.export(b) for b in range(3)]  # three packs and copies in flight before anybody waits
    for b, h in enumerate(handles):
        st, ex = ses.state(b), h.result()
        same_dict(ex, st, b)
        assert ex["P"].shape == (5, 220, 8) and ex["P"].flags["C_CONTIGUOUS"]
        assert tuple(h.recoveries) == (0, 0) and h.done()
    assert np.isnan(handles[0].result()["P"][0, :, 3:]).all() and not np.isnan(handles[2].result()["P"][4, :, 0]).any()


def test_an_idle_stream_with_a_stale_failure_flag_is_not_recovered_again():
    """With the recovery on, the host reads every stream's klt_flags in every step.  A stream that failed (and was recovered) in its last active step still
    carries bit 0 while it is idle: it must report no failure -- its counters stand still, its state is untouched and the step does not look for its
    (missing) frame."""
    W, H, n0 = 480, 270, 100
    K = synth.K_1080P.copy() * (W / 1920.0)
    K[2, 2] = 1.0
    K[2, 0], K[2, 1] = 240.5, 135.5
    p = synth.grid_tracks(n0, W, H, frac=0.5)
    p3, vp = synth.plane_pose_scene(p, K), np.ones(n0, bool)
    clips = [[synth.render_frame(W, H, synth.AffineMotion(W, H, tx=c, ty=0), 1, seed).numpy() for c in shifts]
             for shifts, seed in (((0, 100, 103), 0xC0FFEE), ((0, 3, 6, 9), 0xC0FFEE + 1))]  # a 100-pixel jump (the coarse stage fails), a calm clip
    run = _Streams([(c, p, p3, vp, K) for c in clips], W, H, n0, nhist=8, msv_frame=0, oracles=(), fallback=True)
    run.step((1, 1))
    st = run.ses.state(0)
    assert st["klt_flags"] & 1 and st["n_cur"] > 0 and tuple(run.ses.recoveries()[0]) == (1, 1) and tuple(run.ses.recoveries()[1]) == (0, 0)
    for g in (2, 3):
        run.step((0, 1))
        same_dict(run.ses.state(0), st, g)
        assert run.ses.recoveries().tolist() == [[1, 1], [0, 0]]
    run.step((1, 0))
    assert run.ses.state(0)["frame_i"] == 2 and run.ses.recoveries().tolist() == [[1, 1], [0, 0]]
