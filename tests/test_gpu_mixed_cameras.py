"""Streams of different cameras in one session: a stream's frame size and intrinsics are its own (vh_session_set_camera, vh_frame0_init_batch3,
TrackerSession.init_stream(K=...) / admit, run_sequences, run_queue(max_size=...)); the session's width x height is the largest frame a slot can hold.

Two yardsticks wherever both can serve: the stream's own SessionOracle (it is per stream and takes its own K and frames), with the comparisons and
tolerances of test_gpu_session_idle.py, and the same stream ALONE in a session of exactly its size and K, whose state() must be equal field for field,
bit for bit (every LK route is bit-identical and the pose / MSV solves are per stream).  Scenes and comparisons are those of tests/scenes.py and
tests/session_support.py; _Streams is this module's own (that file's has no per-stream camera and no solo twin)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import scenes as S  # noqa: E402
from _helpers import frame0_host  # noqa: E402
from oracle.session_oracle import SessionOracle  # noqa: E402 (checker only)
from scenes import T0  # noqa: E402
from session_support import equals_oracle, same_dict  # noqa: E402
from velocity_amd import synth  # noqa: E402


class _Streams:
    """A session of max_w x max_h whose slot b runs scene b (its own size and K), beside one oracle per stream and -- solo=True -- the same stream alone in a
    session of exactly its size and K; stepped by an activity row, every stream on its own clock."""

    def __init__(self, scenes, max_w, max_h, n0, nhist, msv_frame, oracles=True, solo=True, t0=T0, **kw):
        from velocity_amd.driver import TrackerSession

        self.scenes = scenes
        self.ses = TrackerSession(scenes[0][4], max_w, max_h, n0, nhist=nhist, batch=len(scenes), msv_frame=msv_frame, **kw)
        self.orc, self.solo, self.k = {}, {}, [0] * len(scenes)
        for b, (frames, p, p3, vp, Kb) in enumerate(scenes):
            H, W = frames[0].shape
            self.ses.init_stream(b, frames[0], p, p3, vp, t0, time0=10.0 * b, K=Kb)
            assert self.ses.slot_size(b) == (H, W)
            if oracles:
                self.orc[b] = SessionOracle(Kb, frames[0], p, p3, vp, t0, time0=10.0 * b, nhist=nhist, msv_frame=msv_frame)
            if solo:
                self.solo[b] = TrackerSession(Kb, W, H, n0, nhist=nhist, batch=1, msv_frame=msv_frame, **kw)
                self.solo[b].init_stream(0, frames[0], p, p3, vp, t0, time0=10.0 * b)

    def step(self, active, bgr=None):
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
            frames.append(S.to_cuda(self.scenes[b][0][k] if bgr is None else bgr[b][k]))
            ts.append(t)
            fn.append(k)
            if b in self.orc:
                self.orc[b].step(self.scenes[b][0][k], t, k)
            if b in self.solo:
                self.solo[b].step([S.to_cuda(self.scenes[b][0][k])], time_s=[t], frame_no=[k])
        if bgr is None:
            self.ses.step(frames, time_s=ts, frame_no=fn)
            return None
        return self.ses.step_bgr(frames, time_s=ts, frame_no=fn)

    def check(self, b, where):
        st = self.ses.state(b)
        if b in self.orc:
            equals_oracle(st, self.orc[b], where)
        if b in self.solo:
            same_dict(st, self.solo[b].state(0), where)
        return st


# the idle table of test_gpu_session_idle.py: stream 1 is out at steps 2-3; step 2 has a single active stream, step 6 none.  With msv_frame = 3 stream 2
# re-triangulates at step 3 and is parked at its frame 3 during step 5, in which streams 0 and 1 reach theirs
TABLE = [(0, 1, 1), (0, 0, 1), (1, 0, 1), (1, 1, 0), (1, 1, 0), (0, 0, 0), (1, 1, 1)]
# slot 0: landscape; slot 1: portrait, principal point off centre; slot 2: a width of 2 mod 4 (rn(414 / 4) sits on a half, rows are not dword aligned) and
# an odd height
CAMERAS = [(480, 270, 700.0, None), (270, 480, 520.0, (150.5, 222.0)), (414, 233, 610.0, None)]


def test_three_cameras_in_one_session():
    n0 = 220
    scenes = [S.plane_scene(W, H, n0, 6, 555 + 222 * b, f, c) for b, (W, H, f, c) in enumerate(CAMERAS)]
    run = _Streams(scenes, 480, 480, n0, nhist=8, msv_frame=3)
    prev = [run.ses.state(b) for b in range(3)]
    for g, active in enumerate(TABLE, 1):
        run.step(active)
        cur = []
        for b, a in enumerate(active):
            cur.append(run.check(b, (g, b)) if a else run.ses.state(b))
            if not a:
                same_dict(cur[b], prev[b], (g, b))  # a slot sits the step out while neighbours of other sizes run
        prev = cur
    assert [run.orc[b].i for b in range(3)] == [4, 4, 4]
    assert all(st["n_cur"] > n0 // 4 for st in prev), [st["n_cur"] for st in prev]  # (every camera kept tracking: the comparison is not of empty streams)


def test_both_level_layouts_side_by_side():
    """Slot 0: 640 x 480 with tracks over 80 % of the frame under a sideways motion (a receding camera would shrink the track cloud below the boundary by
    the third step), so its ROI is (all but) the whole frame and level 1 of the ROI pyramid has more than 65 536 pixels: dense.  Slot 1: 480 x 270, whose level 1 has at most 32 400: it carries the border ring.  The same level index of the same launch is so ringed
    for one stream and dense for its neighbour."""
    from velocity_amd import _lib as L

    n0 = 220
    scenes = [S.plane_scene(640, 480, n0, 4, 901, 760.0, traj=lambda k: np.array([0.02 * k, 0.005 * k, 0.0])), S.plane_scene(480, 270, n0, 4, 902, 700.0)]
    run = _Streams(scenes, 640, 480, n0, nhist=6, msv_frame=0)
    for g in range(1, 4):
        run.step((1, 1))
        rois = np.zeros((2, 4), np.int32)
        L.check(run.ses.lib.vh_klt_rois(run.ses.ws.handle, rois.ctypes.data_as(L.i32p)), "vh_klt_rois")
        lv1 = [((int(x1 - x0) + 1) // 2) * ((int(y1 - y0) + 1) // 2) for x0, x1, y0, y1 in rois]
        assert lv1[0] > 65536 >= lv1[1] > 0, (g, rois.tolist(), lv1)  # the case covers the boundary between the two layouts
        assert rois[1, 1] <= 480 and rois[1, 3] <= 270, rois.tolist()
        for b in range(2):
            run.check(b, (g, b))


# ---- frame 0 ------------------------------------------------------------------------------------------------------------------------------------------
F0_BORDER, F0_CORNERS = (60, 40), 150


def _f0_outputs(torch, nb, cap):
    dev = "cuda"
    return (torch.full((nb, cap, 2), -7.0, dtype=torch.float32, device=dev), torch.full((nb, cap, 3), -7.0, dtype=torch.float64, device=dev),
            torch.full((nb, cap), 77, dtype=torch.uint8, device=dev), torch.full((nb, 3), -7.0, dtype=torch.float32, device=dev),
            torch.full((nb, 9), -7.0, dtype=torch.float64, device=dev), torch.full((nb,), -7.0, dtype=torch.float64, device=dev),
            torch.full((nb,), -5, dtype=torch.int32, device=dev))


def _batch3(ws, frames, cams, qs, use_harris, min_distance, outs=None):
    """vh_frame0_init_batch3 through ctypes on the current stream -> (rc, outputs, rois); frames: CUDA tensors, cams: ClipCamera per clip."""
    from velocity_amd import _lib as L

    torch = L.torch_cuda()
    nb, cap = len(frames), 4 + F0_CORNERS
    outs = _f0_outputs(torch, nb, cap) if outs is None else outs
    q = np.ascontiguousarray(np.stack([np.asarray(x, np.float32).reshape(4, 2) for x in qs]))
    ptrs = (C.c_void_p * nb)(*[f.data_ptr() for f in frames])
    rois = (C.c_int * (8 * nb))(*([-5] * 8 * nb))
    rc = ws.lib.vh_frame0_init_batch3(ws.handle, nb, C.cast(ptrs, C.c_void_p), (L.ClipCamera * nb)(*cams), q.ctypes.data_as(L.f32p), S.plate_world().ctypes.data_as(L.f64p),
                                      F0_BORDER[0], F0_BORDER[1], F0_CORNERS, 0.01, 5, 0.04, use_harris, min_distance, 5, 100, 0.001,
                                      *[L.dptr(x) for x in outs], rois, L.stream_ptr())
    return rc, outs, rois


def _f0_single(frame, q, K, use_harris, min_distance):
    """The clip alone on a context of its own size: vh_frame0_init for the reference's detector; vh_frame0_init has no detector argument, so for any
    other detector the one-clip call is vh_frame0_init_batch2 with nb = 1."""
    from velocity_amd import _lib as L

    torch = L.torch_cuda()
    H, W = frame.shape
    ws = L.Workspace(1, W, H, 64)
    outs = _f0_outputs(torch, 1, 4 + F0_CORNERS)
    rois = (C.c_int * 8)()
    f = torch.from_numpy(np.ascontiguousarray(frame)).cuda()
    q = np.ascontiguousarray(np.asarray(q, np.float32).reshape(4, 2))
    common = (q.ctypes.data_as(L.f32p), L.host_K(K).ctypes.data_as(L.f64p), S.plate_world().ctypes.data_as(L.f64p), F0_BORDER[0], F0_BORDER[1], F0_CORNERS, 0.01, 5, 0.04)
    tail = (5, 100, 0.001, *[L.dptr(x) for x in outs], rois, L.stream_ptr())
    if use_harris and min_distance == 0:
        L.check(ws.lib.vh_frame0_init(ws.handle, L.dptr(f), W, H, W, *common, *tail), "vh_frame0_init")
    else:
        ptrs = (C.c_void_p * 1)(f.data_ptr())
        L.check(ws.lib.vh_frame0_init_batch2(ws.handle, 1, C.cast(ptrs, C.c_void_p), W, H, W, *common, use_harris, float(min_distance), *tail), "vh_frame0_init_batch2")
    return frame0_host(outs, rois, 1)


def _f0_clips():
    """Three clips of three sizes and three K: (frame, q, K)."""
    out = []
    for b, ((W, H, f, c), (X, Y)) in enumerate(zip(CAMERAS, ((0.1, -0.05), (-0.15, 0.4), (0.3, 0.1)))):
        K = S.camera(W, H, f, c)
        frame = synth.render_frame(W, H, synth.AffineMotion(W, H), 0, seed=0x5EED + b).numpy()
        out.append((frame, S.plate_quad(K, X, Y, 3.6), K))
    return out


@pytest.mark.parametrize("use_harris,min_distance", [(1, 0.0), (0, 5.0)], ids=["harris", "shi_tomasi_md5"])
def test_frame0_of_three_cameras_in_one_call(use_harris, min_distance):
    from velocity_amd import _lib as L

    torch = L.torch_cuda()
    clips = _f0_clips()
    ws = L.Workspace(1, 480, 480, 64)
    L.check(ws.lib.vh_init_reserve_batch(ws.handle, 2, 480, 480, L.stream_ptr()), "vh_init_reserve_batch")  # chunks of 2: the three clips span two
    dev = [torch.from_numpy(f).cuda() for f, _, _ in clips]
    cams = [L.clip_camera(f.shape[1], f.shape[0], K) for f, _, K in clips]
    rc, outs, rois = _batch3(ws, dev, cams, [q for _, q, _ in clips], use_harris, min_distance)
    L.check(rc, "vh_frame0_init_batch3")
    got = frame0_host(outs, rois, 3)
    for b, (frame, q, K) in enumerate(clips):
        one = _f0_single(frame, q, K, use_harris, min_distance)
        n = int(got["n"][b])
        assert n == int(one["n"][0]) and n > 20, (b, n, one["n"])
        assert np.array_equal(got["p"][b, :n], one["p"][0, :n]), b
        for key in ("p3", "vp", "t", "R", "res", "rois"):
            assert np.array_equal(got[key][b], one[key][0]), (b, key)
        assert got["rois"][b, 5] <= frame.shape[1] and got["rois"][b, 7] <= frame.shape[0]  # boxb inside the clip's own frame


# ---- the drivers ------------------------------------------------------------------------------------------------------------------------------------------
def _same_as_single(g, one, where):
    """test_gpu_queue.py's comparison of a batched result with run_sequence's on the clip alone (the procTime column and the wall-clock line are held out)."""
    assert g["n_tracks0"] == one["n_tracks0"] > 20 and g["boxa"] == one["boxa"] and g["boxb"] == one["boxb"], where
    assert np.array_equal(g["vg"], one["vg"]) and np.array_equal(g["vp"], one["vp"]) and np.array_equal(g["p"], one["p"]) and np.array_equal(g["ids"], one["ids"]), where
    assert g["P"].shape == one["P"].shape and g["B"].shape == one["B"].shape and g["S"].shape == one["S"].shape, where
    for r in (0, 1, 4):
        assert np.array_equal(g["P"][r], one["P"][r], equal_nan=True), (where, r)
    np.testing.assert_allclose(g["B"], one["B"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(g["S"][:, [0, 2, 3, 4, 5, 6, 7, 8]], one["S"][:, [0, 2, 3, 4, 5, 6, 7, 8]], rtol=1e-6, equal_nan=True)
    for key in ("p3", "t0", "R0", "res0", "klt_flags"):
        assert np.array_equal(g[key], one[key]), (where, key)
    assert g["lines"][0] == one["lines"][0] and g["lines"][1] == one["lines"][1], where
    assert len(g["lines"]) == len(one["lines"])
    for a_, b_ in zip(g["lines"][2:-2], one["lines"][2:-2]):
        assert a_[:13] == b_[:13] and a_[26:] == b_[26:], (a_, b_)  # every column but procTime
    assert g["lines"][-2] == one["lines"][-2], where  # Speed / Res summary


def _alone(c, K, **kw):
    from velocity_amd.driver import run_sequence

    return run_sequence(c["frames"], c["q"], c.get("K", K), times=c["times"], out=None, live=False, name=c["name"], **kw)


def test_run_sequences_on_clips_of_two_cameras():
    """The reference's stills B (1024 x 768, their own intrinsics and plate corners) beside a synthetic 960 x 540 clip of the same length with its own K."""
    from velocity_amd.driver import run_sequences

    stills = S.load_stills()
    a = dict(frames=stills["b_frames"], q=stills["b_q"], times=stills["b_times"], name="stills b")
    b = S.plate_clip(960, 540, 1100.0, len(a["frames"]), 77, "synthetic 960 x 540")
    kw = dict(roi_border=(180, 140), max_corners=400)
    lines = []
    got = run_sequences([a, b], stills["b_K"], sessions=1, out=lines.append, **kw)
    assert len(got) == 2
    for c, g in zip((a, b), got):
        _same_as_single(g, _alone(c, stills["b_K"], **kw), c["name"])
    assert lines == got[0]["lines"] + got[1]["lines"]
    assert got[0]["P"].shape[2] == got[1]["P"].shape[2] == len(a["frames"])


def test_run_queue_on_clips_of_two_cameras():
    from velocity_amd.driver import run_queue

    cams = ((480, 270, 700.0), (414, 233, 610.0))
    clips = [S.plate_clip(*cams[k % 2], n, 300 + k, f"clip {k} {cams[k % 2][0]} x {cams[k % 2][1]}") for k, n in enumerate((3, 6, 4, 5, 6, 3))]
    K0 = S.camera(480, 270, 650.0)  # the default camera: no clip uses it (each brings its own K)
    kw = dict(roi_border=(60, 40), max_corners=150, msv_frame=3)
    alone = [_alone(c, K0, **kw) for c in clips]
    for ns in (1, 2):
        got = run_queue(clips, K0, streams=2, sessions=ns, max_size=(270, 480), **kw)
        assert len(got) == 6 and got[0]["sessions"] == ns
        for c, g, one in zip(clips, got, alone):
            _same_as_single(g, one, (ns, c["name"]))
            assert g["P"].shape[2] == len(c["frames"])
    big = S.plate_clip(640, 480, 800.0, 3, 999, "too large")
    seen = []
    with pytest.raises(ValueError, match=r"clip 6 .*640 x 480.*480 x 270"):
        run_queue(clips + [big], K0, streams=2, sessions=1, max_size=(270, 480), on_result=lambda i, r: seen.append(i), **kw)
    assert sorted(seen) == list(range(6)), seen  # the six clips before it ran to their end and were delivered


def test_step_bgr_with_two_frame_sizes_equals_the_gray_path():
    from oracle import klt_oracle as KO

    n0 = 180
    rng = np.random.default_rng(5)
    scenes = [S.plane_scene(480, 270, n0, 5, 321, 700.0), S.plane_scene(414, 233, n0, 5, 332, 610.0)]
    bgr = [[np.clip(np.stack([f.astype(int) + rng.integers(-20, 21, f.shape) * (c - 1) for c in range(3)], -1), 0, 255).astype(np.uint8) for f in sc[0]]
           for sc in scenes]
    gray = [([KO.bgr2gray(f) for f in bgr[b]],) + scenes[b][1:] for b in range(2)]
    table = [(1, 1), (1, 0), (1, 1), (0, 1)]
    states = []
    for mode in ("gray", "bgr"):
        run = _Streams(gray, 480, 270, n0, nhist=6, msv_frame=0, oracles=mode == "gray", solo=False)
        for g, active in enumerate(table, 1):
            out = run.step(active, bgr=bgr if mode == "bgr" else None)
            if mode == "bgr":
                for b in range(2):
                    assert (out[b] is None) == (not active[b])
                    if active[b]:
                        assert np.array_equal(out[b].cpu().numpy(), gray[b][0][run.k[b]]), (g, b)
        states.append([run.ses.state(b) for b in range(2)])
        if mode == "gray":
            for b in range(2):
                equals_oracle(states[0][b], run.orc[b], b)
    for b in range(2):
        same_dict(states[0][b], states[1][b], b)
    assert [s["frame_i"] for s in states[1]] == [3, 3]


# ---- recovery ------------------------------------------------------------------------------------------------------------------------------------------
def _jump_scene(W, H, seed, n0=100):
    """The scene of test_gpu_session_fallback.py at another size: frame 1 is shifted by 100 px, then 3 px per frame.  The CPU oracle (oracle.klt_oracle.
    klt_main, flags & 1) loses the tracker on that 100-px shift at 640 x 360 and at 480 x 270 alike, so the shift needed no enlarging."""
    K = synth.K_1080P.copy() * (W / 1920.0)
    K[2, 2] = 1.0
    K[2, 0], K[2, 1] = W / 2 + 0.5, H / 2 + 0.5
    p = synth.grid_tracks(n0, W, H, frac=0.5)
    frames = [synth.render_frame(W, H, synth.AffineMotion(W, H, tx=c, ty=0), 1, seed).numpy() for c in (0, 100, 103, 106)]
    return frames, p, synth.plane_pose_scene(p, K), np.ones(n0, bool), K


def test_recovery_of_two_failed_streams_of_different_sizes():
    # (both with the seed of that scene: on another texture -- 0xC0FFEE + 7 at 480 x 270 -- the oracle keeps every track through the same shift)
    scenes = [_jump_scene(640, 360, 0xC0FFEE), _jump_scene(480, 270, 0xC0FFEE)]
    run = _Streams(scenes, 640, 360, 100, nhist=8, msv_frame=0, oracles=False, t0=np.float32([0.0, 0.0, 3.6]), fallback=True)
    for g in range(1, 4):
        run.step((1, 1))
        for b in range(2):
            st = run.check(b, (g, b))
            assert st["klt_flags"] == run.solo[b].state(0)["klt_flags"]
            assert run.ses.recoveries()[b].tolist() == run.solo[b].recoveries()[0].tolist(), (g, b)
        if g == 1:  # both streams failed in the same step: two sizes, so two matcher calls
            assert [run.ses.state(b)["klt_flags"] & 3 for b in range(2)] == [3, 3] and run.ses.recoveries()[:, 0].tolist() == [1, 1]
    assert run.ses.recoveries()[:, 1].min() >= 1 and all(run.ses.state(b)["n_cur"] > 50 for b in range(2))  # a model was found and the tracks live on


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_queue_nothing_and_change_nothing():
    from velocity_amd import _lib as L

    torch = L.torch_cuda()
    n0 = 120
    scenes = [S.plane_scene(480, 270, n0, 4, 71, 700.0), S.plane_scene(414, 233, n0, 4, 72, 610.0)]
    run = _Streams(scenes, 480, 270, n0, nhist=5, msv_frame=0, solo=False)
    run.step((1, 1))
    before = [run.ses.state(b) for b in range(2)]
    ses, lib = run.ses, run.ses.lib
    K64 = L.host_K(scenes[0][4])

    def unchanged(what):
        assert ses.slot_size(1) == (233, 414), what
        for b in range(2):
            same_dict(ses.state(b), before[b], (what, b))

    assert lib.vh_session_set_camera(ses.handle, 1, 481, 270, K64.ctypes.data_as(L.f64p), 0, L.stream_ptr()) == -1
    msg = lib.vh_last_error()
    assert b"slot 1" in msg and b"481 x 270" in msg and b"480 x 270" in msg, msg
    unchanged("w above the session's")
    assert lib.vh_session_set_camera(ses.handle, 1, 270, 480, K64.ctypes.data_as(L.f64p), 0, L.stream_ptr()) == -1  # a portrait frame in a landscape session
    unchanged("portrait")
    assert lib.vh_session_set_camera(ses.handle, 1, 3, 270, K64.ctypes.data_as(L.f64p), 0, L.stream_ptr()) == -1
    assert lib.vh_session_set_camera(ses.handle, 2, 414, 233, K64.ctypes.data_as(L.f64p), 0, L.stream_ptr()) == -1 and b"slot 2" in lib.vh_last_error()
    assert lib.vh_session_set_camera(ses.handle, 1, 414, 233, None, 0, L.stream_ptr()) == -1 and b"K_host" in lib.vh_last_error()
    unchanged("a null K")
    frames, p, p3, vp, K = S.plane_scene(640, 480, n0, 1, 73)
    with pytest.raises(ValueError, match="slot 1.*640 x 480.*480 x 270"):
        ses.init_stream(1, frames[0], p, p3, vp, T0, K=K)
    unchanged("a frame larger than the session")
    # frame 0: the second clip's row stride is below its width
    clips = _f0_clips()
    ws = L.Workspace(1, 480, 480, 64)
    dev = [torch.from_numpy(f).cuda() for f, _, _ in clips]
    cams = [L.clip_camera(f.shape[1], f.shape[0], K) for f, _, K in clips]
    cams[1].stride = cams[1].w - 1
    rc, outs, rois = _batch3(ws, dev, cams, [q for _, q, _ in clips], 1, 0.0)
    assert rc == -1 and b"clip 1" in lib.vh_last_error() and b"vh_frame0_init_batch3" in lib.vh_last_error(), lib.vh_last_error()
    torch.cuda.synchronize()
    assert all(bool((x == s).all()) for x, s in zip(outs, (-7.0, -7.0, 77, -7.0, -7.0, -7.0, -5))) and list(rois) == [-5] * 24  # nothing written
    unchanged("a refused frame-0 call")
    run.step((1, 1))  # and both streams go on as if nothing had been asked
    for b in range(2):
        equals_oracle(ses.state(b), run.orc[b], ("after", b))
