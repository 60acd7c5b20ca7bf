"""The device blocks behind a context and a session (velocity_amd/csrc/vh_arena.hpp): every layout is one function of a carver and every scratch that grows
is one owner-held block.  These tests look for what a wrong layout or a wrong growth leaves behind -- a misaligned, overlapping, stale or shifted pointer --
at the smallest shapes at which each block is laid out anew: a call after a growth must return the bytes the same call returns on a fresh context."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from velocity_amd import synth  # noqa: E402

# vh_session_export_size(s, NULL), vh_session_refine_workspace(s, 2, 3) and vh_session_refine_windows_workspace(s, 3, 2) of the session of
# test_session_layout, as the library returned them BEFORE the layouts went through the carver: read with tools/exp/arena_parity.py under the parent
# commit's library (profiles/arena/parity.json, "sizes"; equal under both libraries).
PARENT_EXPORT_SIZE = 832
PARENT_REFINE_WORKSPACE = 21760
PARENT_REFINE_WINDOWS_WORKSPACE = 22016


def frame(w, h, k=0, tx=3.0):
    return synth.render_frame(w, h, synth.AffineMotion(w, h, s=1.0, theta_deg=0.0, tx=tx, ty=0.0), k).numpy()


def test_session_layout():
    from velocity_amd.driver import TrackerSession

    n0, nh = 5, 3
    ses = TrackerSession(synth.K_1080P, 16, 12, n0, nhist=nh, batch=2)
    arrays = dict(vg=n0, vp=n0, p=8 * n0, ids=4 * n0, p3=24 * n0, P=4 * 5 * n0 * nh, B=4 * 14 * nh, S=4 * 9 * nh, sel_pw=4 * n0, p_proj=16 * n0)  # bytes
    scalars = dict(n_cur=4, n_pose=4, t=12, res=8, frame_i=4, klt_flags=4, pose_info=8)  # fields of the stream's own record, not carved buffers
    spans, views = [], [ses.view(b) for b in (0, 1)]
    for b, v in enumerate(views):
        for name, size in arrays.items():
            a = getattr(v, name)
            assert a and a % 256 == 0, (b, name, a)
            spans.append((a, a + size, b, name))
        for name, size in scalars.items():
            a = getattr(v, name)
            assert a and a % 4 == 0, (b, name)
            spans.append((a, a + size, b, name))
    # the scalars live in the stream records, [batch] of them at the head of the block: one stride for every field, the first record on a 256-byte boundary
    strides = {getattr(views[1], n) - getattr(views[0], n) for n in scalars}
    assert len(strides) == 1 and 0 < min(strides) < 65536
    # ... and they fit one record, with every carved array behind both records (the start of record 0 itself is no pointer the view hands out)
    lo, hi = min(getattr(views[0], n) for n in scalars), max(getattr(views[0], n) + size for n, size in scalars.items())
    assert hi - lo <= min(strides) and hi + min(strides) <= min(getattr(v, n) for v in views for n in arrays), (lo, hi, strides)
    spans.sort()
    for (a0, a1, *who0), (b0, b1, *who1) in zip(spans, spans[1:]):
        assert a1 <= b0, (who0, who1)
    lib = ses.lib
    got = (lib.vh_session_export_size(ses.handle, None), lib.vh_session_refine_workspace(ses.handle, 2, 3), lib.vh_session_refine_windows_workspace(ses.handle, 3, 2))
    print("sizes", got)
    assert got == (PARENT_EXPORT_SIZE, PARENT_REFINE_WORKSPACE, PARENT_REFINE_WINDOWS_WORKSPACE)


MATCH = dict(levels=2, query_per_level=64, train_per_level=64, border_x=4, border_y=4, min_good=3)


@functools.lru_cache(maxsize=None)
def match_pair(w, h):
    return frame(w, h, 0), frame(w, h, 1), synth.grid_tracks(20, w, h, frac=0.5)


def match_call(ws, w, h):
    """vh_match_affine on the w x h pair through context ws -> the bytes of (M, inliers, pairs, info)."""
    import torch

    from velocity_amd import _lib as L

    a, b, p = match_pair(w, h)
    im1, im2, pt = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(p).cuda()
    cap = MATCH["levels"] * MATCH["query_per_level"]
    M, inl = torch.zeros(6, dtype=torch.float64, device="cuda"), torch.zeros(cap, dtype=torch.uint8, device="cuda")
    pairs, info = torch.zeros((cap, 4), dtype=torch.float32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    mp = L.match_params(MATCH)
    L.check(ws.lib.vh_match_affine(ws.handle, L.dptr(im1), L.dptr(im2), w, h, w, w, L.dptr(pt), len(p), C.byref(mp), L.dptr(M), L.dptr(inl), L.dptr(pairs),
                                   L.dptr(info), L.stream_ptr()), "vh_match_affine")
    return tuple(x.cpu().numpy().tobytes() for x in (M, inl, pairs, info)), info.cpu().numpy()


def test_match_scratch_growth():
    from velocity_amd import _lib as L

    new = lambda: L.Workspace(1, 96, 80, 256)  # noqa: E731
    ws = new()
    first, info_small = match_call(ws, 64, 48)
    second, info_large = match_call(ws, 96, 80)  # more pixels per level: the block grows and is laid out anew
    third, _ = match_call(ws, 64, 48)
    print("info", info_small.tolist(), info_large.tolist())
    assert info_small[3] > 0 and info_large[3] > info_small[3], "the pairs have keypoints to lay out"
    assert first == third
    assert second == match_call(new(), 96, 80)[0]
    assert first == match_call(new(), 64, 48)[0]


SEL_MAX = 2048  # F0B_SEL_MAX (vh_init.hip): budgets above it select through the sort block


def corners_call(ws, w, h, max_corners):
    """vh_good_features2 (Shi-Tomasi, no spacing, no mask) on the w x h frame through context ws -> the bytes of (corners, count)."""
    import torch

    from velocity_amd import _lib as L

    im = torch.from_numpy(frame(w, h)).cuda()
    out, cnt = torch.zeros((max_corners, 2), dtype=torch.float32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    L.check(ws.lib.vh_good_features2(ws.handle, L.dptr(im), w, h, w, None, 0, max_corners, 0.001, 0.0, 3, 0, 0.04, L.dptr(out), L.dptr(cnt), L.stream_ptr()),
            "vh_good_features2")
    return (out.cpu().numpy().tobytes(), cnt.cpu().numpy().tobytes()), int(cnt.item())


def test_frame0_scratch_growth():
    from velocity_amd import _lib as L

    new = lambda: L.Workspace(1, 96, 80, 64)  # noqa: E731
    ws = new()
    calls = [(32, 32, 50), (96, 80, 50), (96, 80, SEL_MAX + 2), (32, 32, 50)]  # first block, its growth, the sort block, and the small image on the grown blocks
    counts = []
    for w, h, mc in calls:
        got, n = corners_call(ws, w, h, mc)
        counts.append(n)
        assert got == corners_call(new(), w, h, mc)[0], (w, h, mc)
    print("corners", counts)
    assert counts[0] == counts[3] and 0 < counts[0] and 0 < counts[1] <= counts[2], counts


def test_fallback_scratch_growth():
    import torch

    from velocity_amd import _lib as L
    from test_gpu_session_fallback import N0, NH, H, T0, W, clip, scene
    from velocity_amd.driver import TrackerSession

    clips = [clip("jump"), clip("calm")]
    K, p, p3, vp = scene()
    half = dict(query_per_level=L.MATCH_DEFAULTS["query_per_level"] // 2)
    states = []
    for grown in (True, False):
        ses = TrackerSession(K, W, H, N0, nhist=NH, batch=2, msv_frame=0, fallback=True, fallback_params=half if grown else None)
        if grown:  # on again with the query budget doubled: qcap grows, and with it the device block
            mp = L.match_params(None)
            L.check(ses.lib.vh_session_set_fallback(ses.handle, 1, C.byref(mp)), "vh_session_set_fallback")
        for b, fr in enumerate(clips):
            ses.init_stream(b, fr[0], p, p3, vp, T0)
        ses.step([torch.from_numpy(c[1]).cuda() for c in clips], time_s=np.float32(1 / 30.0), frame_no=1)
        states.append(([ses.state(b) for b in (0, 1)], ses.recoveries().tolist()))
    (grown, rec_grown), (plain, rec_plain) = states
    assert rec_grown == rec_plain == [[1, 1], [0, 0]]
    assert grown[0]["klt_flags"] & 7 == 7 and grown[1]["klt_flags"] & 7 == 0
    # the recovered model M stays inside the library; what it produces does not: the fine stage that ran with it wrote p, v and the records
    for b in (0, 1):
        for key, val in grown[b].items():
            a, c = np.asarray(val), np.asarray(plain[b][key])
            assert a.dtype == c.dtype and a.tobytes() == c.tobytes(), (b, key)
