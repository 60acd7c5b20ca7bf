"""Frame 0 of many clips in one launch sequence (vh_frame0_init_batch, torch.ops.velocity_hip.frame0_init, driver.frame0_batch, run_sequences) and of one
clip (vh_frame0_init, the batch of one).

Against the oracle's frame0 the corners / masks / ROIs are exact and the pose holds the tolerances of test_gpu_stills._run_both: that comparison carries
the arithmetic.  Every clip of a batch must also be bit-identical to vh_frame0_init on that clip alone (Harris corners, cornerSubPix, plate pose, world
points, masks, ROIs), whatever the chunking, the stream, a graph capture or a second context running beside it: both run the same kernels, so this
guards the one-clip wrapper's output layout and the independence of a clip from its neighbours."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from _helpers import frame0_host  # noqa: E402
from oracle import driver_oracle as DO  # noqa: E402 (checker only)
from scenes import plate_quad, plate_world, stills  # noqa: E402, F401 (stills: a fixture)

BORDER = (180, 140)
SENT_F, SENT_I = -7.0, -5
MIRRORED = 1  # index of the mirrored stills in _mixed_clips


def _mixed_clips(stills):
    """The five clips of one 1024 x 768 batch: stills b, b mirrored, stills a, a synthetic scene with its plate near the top-left corner (boxb clipped),
    a uniform grey frame (no candidate at all)."""
    from velocity_amd import synth

    fb, qb, K = stills["b_frames"][0], stills["b_q"], stills["b_K"]
    H, W = fb.shape
    qm = qb.copy()
    qm[:, 0] = (W - 1) - qm[:, 0]
    syn = synth.render_frame(W, H, synth.AffineMotion(W, H), 0, seed=0x5EED).numpy()
    return K, [(fb, qb), (np.ascontiguousarray(fb[:, ::-1]), qm[[1, 0, 3, 2]]), (stills["a_frames"][0], stills["a_q"]), (syn, plate_quad(K, 0.5, -0.97, 6.0)),
               (np.full((H, W), 128, np.uint8), qb)]


def _outputs(torch, nb, cap):
    """Sentinel-filled device outputs: p, p3, vp, t, R, res, n."""
    dev = "cuda"
    return (torch.full((nb, cap, 2), SENT_F, dtype=torch.float32, device=dev), torch.full((nb, cap, 3), SENT_F, dtype=torch.float64, device=dev),
            torch.full((nb, cap), 77, dtype=torch.uint8, device=dev), torch.full((nb, 3), SENT_F, dtype=torch.float32, device=dev),
            torch.full((nb, 9), SENT_F, dtype=torch.float64, device=dev), torch.full((nb,), SENT_F, dtype=torch.float64, device=dev),
            torch.full((nb,), SENT_I, dtype=torch.int32, device=dev))


def _batch(ws, frames, qs, K, border=BORDER, max_corners=1000, outs=None, rois=None, nb=None):
    """vh_frame0_init_batch through ctypes on the current stream.  -> (rc, outputs, rois); frames: CUDA [H, W] tensors (nb: the count passed, default all)."""
    from velocity_amd import _lib as L

    torch = L.torch_cuda()
    nb, cap = len(frames) if nb is None else nb, 4 + max_corners
    H, W = frames[0].shape
    outs = _outputs(torch, max(nb, 1), cap) if outs is None else outs
    q = np.ascontiguousarray(np.stack([np.asarray(x, np.float32).reshape(4, 2) for x in qs]))
    ptrs = (C.c_void_p * len(frames))(*[f.data_ptr() for f in frames])
    rois = (C.c_int * (8 * max(nb, 1)))(*([SENT_I] * 8 * max(nb, 1))) if rois is None else rois
    K64 = L.host_K(K)
    p, p3, vp, t, R, res, n = outs
    rc = ws.lib.vh_frame0_init_batch(ws.handle, nb, C.cast(ptrs, C.c_void_p), W, H, W, q.ctypes.data_as(L.f32p), K64.ctypes.data_as(L.f64p),
                                     plate_world().ctypes.data_as(L.f64p), border[0], border[1], max_corners, 0.01, 5, 0.04, 5, 100, 0.001, L.dptr(p), L.dptr(p3),
                                     L.dptr(vp), L.dptr(t), L.dptr(R), L.dptr(res), L.dptr(n), rois, L.stream_ptr())
    return rc, outs, rois


def _single(frame, q, K, border=BORDER, max_corners=1000):
    """vh_frame0_init on one clip, own context."""
    from velocity_amd import _lib as L

    torch = L.torch_cuda()
    H, W = frame.shape
    ws = L.Workspace(1, W, H, 64)
    cap = 4 + max_corners
    p, p3, vp, t, R, res, n = (x[0] for x in _outputs(torch, 1, cap))
    rois = (C.c_int * 8)()
    f = torch.from_numpy(np.ascontiguousarray(frame)).cuda()
    q = np.ascontiguousarray(np.asarray(q, np.float32).reshape(4, 2))
    L.check(ws.lib.vh_frame0_init(ws.handle, L.dptr(f), W, H, W, q.ctypes.data_as(L.f32p), L.host_K(K).ctypes.data_as(L.f64p), plate_world().ctypes.data_as(L.f64p),
                                  border[0], border[1], max_corners, 0.01, 5, 0.04, 5, 100, 0.001, L.dptr(p), L.dptr(p3), L.dptr(vp), L.dptr(t), L.dptr(R),
                                  L.dptr(res), L.dptr(n), rois, L.stream_ptr()), "vh_frame0_init")
    return dict(p=p.cpu().numpy(), p3=p3.cpu().numpy(), vp=vp.cpu().numpy(), t=t.cpu().numpy(), R=R.cpu().numpy(), res=res.cpu().numpy(),
                n=int(n.item()), rois=np.array(list(rois)))


def _same_as_single(got, b, one):
    """Row b of a batch result equals the single call bit for bit (p up to n; p3 / vp on every row: zero beyond n in both)."""
    n = int(got["n"][b])
    assert n == one["n"], (b, n, one["n"])
    assert np.array_equal(got["p"][b, :n], one["p"][:n]), b
    assert np.array_equal(got["p3"][b], one["p3"]) and np.array_equal(got["vp"][b], one["vp"]), b
    assert np.array_equal(got["t"][b], one["t"]) and np.array_equal(got["R"][b], one["R"]) and np.array_equal(got["res"][b], one["res"]), b
    assert np.array_equal(got["rois"][b], one["rois"]), b


def _same_as_oracle(got, b, ref, pose=True):
    """pose=False: the plate fit has no pose to agree on (the mirrored stills: a reflected plate that no rotation reproduces; the 4-point fit stops at a
    ~30 px residual, where its end point is no parity quantity -- vh_frame0_init alone differs from the oracle there too); corners, masks, ROIs still exact."""
    n = int(got["n"][b])
    assert n == len(ref["p"]), (b, n, len(ref["p"]))
    assert np.array_equal(got["p"][b, :n], ref["p"]), b
    assert np.array_equal(got["vp"][b, :n].astype(bool), ref["vp"]), b
    assert tuple(got["rois"][b, 0:4]) == ref["boxa"] and tuple(got["rois"][b, 4:8]) == ref["boxb"], b
    if not pose:
        return
    np.testing.assert_allclose(got["t"][b], ref["t"], rtol=1e-5)
    np.testing.assert_allclose(got["R"][b].reshape(3, 3), ref["R"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(got["res"][b], ref["res"], rtol=1e-4, atol=1e-4)  # atol: an exactly projected plate leaves ~1e-5 px of float32 rounding


def _oracle(frame, q, K, border=BORDER, max_corners=1000):
    with np.errstate(all="ignore"):
        return DO.frame0(np.ascontiguousarray(frame), q, K, roi_border=border, max_corners=max_corners)


def _dev(frames):
    import torch

    return [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in frames]


def test_one_call_of_mixed_clips_equals_single_calls_and_the_oracle(stills):
    from velocity_amd import _lib as L

    K, clips = _mixed_clips(stills)
    H, W = clips[0][0].shape
    ws = L.Workspace(1, W, H, 64)
    rc, outs, rois = _batch(ws, _dev([f for f, _ in clips]), [q for _, q in clips], K)
    L.check(rc, "vh_frame0_init_batch")
    got = frame0_host(outs, rois, len(clips))
    for b, (f, q) in enumerate(clips):
        _same_as_single(got, b, _single(f, q, K))
        _same_as_oracle(got, b, _oracle(f, q, K), pose=b != MIRRORED)
    assert got["n"][0] > 100 and got["n"][2] > 100 and got["n"][4] == 4, got["n"]
    rw = got["rois"][:, 5] - got["rois"][:, 4]
    assert got["rois"][3, 4] == 1 and got["rois"][3, 6] == 1 and rw[3] != rw[0], got["rois"]  # the corner clip's ROI is clipped to another size
    assert not np.array_equal(got["p"][0, :20], got["p"][1, :20])


def test_chunked_call_equals_one_chunk(stills):
    """A context reserved for 2 clips runs 5 clips as chunks of 2, 2, 1: the same results as a context reserved for all 5."""
    from velocity_amd import _lib as L

    K, clips = _mixed_clips(stills)
    H, W = clips[0][0].shape
    frames, qs = _dev([f for f, _ in clips]), [q for _, q in clips]
    res = []
    for nres in (2, 5):
        ws = L.Workspace(1, W, H, 64)
        L.check(ws.lib.vh_init_reserve_batch(ws.handle, nres, W, H, L.stream_ptr()), "vh_init_reserve_batch")
        rc, outs, rois = _batch(ws, frames, qs, K)
        L.check(rc, "vh_frame0_init_batch")
        res.append(frame0_host(outs, rois, len(clips)))
    for key in res[0]:
        assert np.array_equal(res[0][key], res[1][key]), key


def test_many_candidates_select_and_large_max_corners(stills):
    """A textured frame with ~23 k candidates in a full-frame ROI: max_corners 1000 (radix select, LDS sort) and 3000 (above the in-LDS bound: the segmented
    sort route) both equal the oracle and the single call, for both clips."""
    from velocity_amd import _lib as L
    from velocity_amd import synth

    W, H = 1024, 768
    K = stills["b_K"]
    f = synth.render_frame(W, H, synth.AffineMotion(W, H), 0).numpy()
    f2 = synth.render_frame(W, H, synth.AffineMotion(W, H), 0, seed=99).numpy()
    q = stills["b_q"]
    border = (2000, 2000)
    for mc in (1000, 3000):
        ws = L.Workspace(1, W, H, 64)
        rc, outs, rois = _batch(ws, _dev([f, f2]), [q, q], K, border=border, max_corners=mc)
        L.check(rc, "vh_frame0_init_batch")
        got = frame0_host(outs, rois, 2)
        assert got["n"][0] == 4 + mc and got["n"][1] == 4 + mc, got["n"]
        for b, frame in enumerate((f, f2)):
            _same_as_single(got, b, _single(frame, q, K, border=border, max_corners=mc))
            _same_as_oracle(got, b, _oracle(frame, q, K, border=border, max_corners=mc))


def test_single_call_on_a_tiny_frame_equals_the_oracle():
    """vh_frame0_init at the ABI on a 96 x 64 frame whose border-clipped plate ROI (30 x 15) is smaller than one 64 x 16 detector tile, and on the same
    frame as uniform grey (no corner: exactly the 4 plate corners)."""
    from velocity_amd import synth

    W, H, border = 96, 64, (8, 5)
    K = np.array([[100.0, 0, 0], [0, 100.0, 0], [48.0, 32.0, 1.0]])
    q = plate_quad(K, -0.05, -0.02, 3.0)
    textured = synth.render_frame(W, H, synth.AffineMotion(W, H), 0, seed=0x5EED).numpy()
    for frame, corners in ((textured, True), (np.full((H, W), 128, np.uint8), False)):
        ref = _oracle(frame, q, K, border=border)
        x0, x1, y0, y1 = ref["boxb"]
        assert 3 <= x1 - x0 < 64 and 3 <= y1 - y0 < 16, ref["boxb"]
        assert (len(ref["p"]) > 8) if corners else (len(ref["p"]) == 4), len(ref["p"])
        one = _single(frame, q, K, border=border)
        got = {key: np.asarray(val)[None] for key, val in one.items()}
        _same_as_oracle(got, 0, ref)
        assert np.all(one["p3"][one["n"]:] == 0) and np.all(one["vp"][one["n"]:] == 0)  # rows beyond n: zero


def test_single_call_refuses_what_it_always_refused():
    """vh_frame0_init's rejections as the batch of one: a null argument, bad arguments and an empty plate ROI return -1, name the entry, queue nothing."""
    from velocity_amd import _lib as L

    torch = L.torch_cuda()
    W, H = 96, 64
    ws = L.Workspace(1, W, H, 64)
    f = torch.full((H, W), 128, dtype=torch.uint8, device="cuda")
    K64, plate = L.host_K(np.array([[100.0, 0, 0], [0, 100.0, 0], [48.0, 32.0, 1.0]])), plate_world()
    inside = np.float32([[40, 29], [53, 29], [53, 34], [40, 34]])
    outs = _outputs(torch, 1, 54)

    def call(q, w=W, block=5, null=None):
        p, p3, vp, t, R, res, n = (None if k == null else L.dptr(x) for k, x in enumerate(outs))
        rois = (C.c_int * 8)()
        q = np.ascontiguousarray(q, np.float32)
        return ws.lib.vh_frame0_init(ws.handle, L.dptr(f), w, H, W, q.ctypes.data_as(L.f32p), K64.ctypes.data_as(L.f64p), plate.ctypes.data_as(L.f64p), 8, 5, 50,
                                     0.01, block, 0.04, 5, 100, 0.001, p, p3, vp, t, R, res, n, rois, L.stream_ptr())

    for kwargs, word in ((dict(q=inside, null=4), b"null argument"), (dict(q=inside, w=2), b"bad arguments"), (dict(q=inside, block=16), b"bad arguments"),
                         (dict(q=inside + np.float32([5000, 0])), b"empty")):
        assert call(**kwargs) == -1
        msg = ws.lib.vh_last_error()
        assert msg.startswith(b"vh_frame0_init:") and word in msg, msg
    torch.cuda.synchronize()
    assert bool((outs[0] == SENT_F).all()) and int(outs[6].item()) == SENT_I
    assert call(inside) == 0


def test_graph_capture_replays_the_eager_result(stills):
    import torch

    from velocity_amd import _lib as L

    K, clips = _mixed_clips(stills)
    H, W = clips[0][0].shape
    frames, qs = _dev([f for f, _ in clips]), [q for _, q in clips]
    ws = L.Workspace(1, W, H, 64)
    L.check(ws.lib.vh_init_reserve_batch(ws.handle, len(clips), W, H, L.stream_ptr()), "vh_init_reserve_batch")
    rc, outs, rois = _batch(ws, frames, qs, K)
    L.check(rc, "vh_frame0_init_batch")
    eager = frame0_host(outs, rois, len(clips))
    cap_outs = _outputs(torch, len(clips), 1004)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc, _, _ = _batch(ws, frames, qs, K, outs=cap_outs)
    assert rc == 0, ws.lib.vh_last_error()
    torch.cuda.synchronize()
    assert int((cap_outs[6] != SENT_I).sum()) == 0 and bool((cap_outs[0] == SENT_F).all()), "work ran during the capture"
    for _ in range(2):
        for x in cap_outs:
            x.fill_(3)
        g.replay()
        torch.cuda.synchronize()
        got = frame0_host(cap_outs, rois, len(clips))
        for key in ("n", "t", "R", "res", "p3", "vp"):
            assert np.array_equal(got[key], eager[key]), key
        for b in range(len(clips)):
            n = int(eager["n"][b])
            assert np.array_equal(got["p"][b, :n], eager["p"][b, :n]), b


def test_two_contexts_on_two_streams_interleaved(stills):
    """Two contexts on two HIP streams, each with its own batch of another frame size, 10 rounds without synchronising: every round equals the oracle."""
    import torch

    from velocity_amd import _lib as L
    from velocity_amd import synth

    K, clips = _mixed_clips(stills)
    A = clips[:3]
    Ws, Hs = 640, 480
    B = [(synth.render_frame(Ws, Hs, synth.AffineMotion(Ws, Hs), 0, seed=s).numpy(), plate_quad(K, x, y, 7.0)) for s, x, y in ((3, 0.91, -0.79), (4, 1.01, -0.87))]
    refs = [[_oracle(f, q, K) for f, q in A], [_oracle(f, q, K) for f, q in B]]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    jobs = []
    for clipset, st in zip((A, B), streams):
        h, w = clipset[0][0].shape
        with torch.cuda.stream(st):
            jobs.append((L.Workspace(1, w, h, 64), _dev([f for f, _ in clipset]), [q for _, q in clipset]))
    torch.cuda.synchronize()
    results = [[], []]
    for _ in range(10):
        for j in range(2):
            ws, frames, qs = jobs[j]
            with torch.cuda.stream(streams[j]):
                rc, outs, rois = _batch(ws, frames, qs, K)
                assert rc == 0, ws.lib.vh_last_error()
                results[j].append((outs, rois))
    torch.cuda.synchronize()
    for j in range(2):
        for outs, rois in results[j]:
            got = frame0_host(outs, rois, len(refs[j]))
            for b, ref in enumerate(refs[j]):
                _same_as_oracle(got, b, ref, pose=not (j == 0 and b == MIRRORED))


def test_bad_arguments_queue_nothing(stills):
    from velocity_amd import _lib as L

    K, clips = _mixed_clips(stills)
    H, W = clips[0][0].shape
    frames, qs = _dev([f for f, _ in clips]), [q for _, q in clips]
    ws = L.Workspace(1, W, H, 64)
    lib = ws.lib

    def untouched(outs, rois, nb):
        got = frame0_host(outs, rois, nb)
        assert np.all(got["p"] == SENT_F) and np.all(got["p3"] == SENT_F) and np.all(got["vp"] == 77) and np.all(got["t"] == SENT_F)
        assert np.all(got["R"] == SENT_F) and np.all(got["res"] == SENT_F) and np.all(got["n"] == SENT_I) and np.all(got["rois"] == SENT_I)

    rc, outs, rois = _batch(ws, frames[:1], qs[:1], K, nb=0)
    assert rc == -1
    untouched(outs, rois, 1)
    import torch

    outs = _outputs(torch, len(clips), 1004)
    nulled = outs[:4] + (torch.empty(0, dtype=torch.float64, device="cuda"),) + outs[5:]  # R_out = NULL (an empty tensor's data_ptr is 0)
    assert nulled[4].data_ptr() == 0
    rc, _, rois = _batch(ws, frames, qs, K, outs=nulled)
    assert rc == -1 and b"null" in lib.vh_last_error()
    untouched(outs, rois, len(clips))
    bad = list(qs)
    bad[2] = np.full((4, 2), 5000.0, np.float32)  # far right of the frame: boxb empty
    rc, outs, rois = _batch(ws, frames, bad, K)
    assert rc == -1 and b"clip 2" in lib.vh_last_error(), lib.vh_last_error()
    torch.cuda.synchronize()
    untouched(outs, rois, len(clips))


def test_torch_op_equals_the_ctypes_call(stills):
    import torch

    import velocity_amd.torch_ops  # noqa: F401
    from velocity_amd import _lib as L

    K, clips = _mixed_clips(stills)
    H, W = clips[0][0].shape
    frames = torch.from_numpy(np.stack([f for f, _ in clips])).cuda()
    qs = np.stack([q for _, q in clips]).astype(np.float32)
    p, p3, vp, t, R, res, n, rois = torch.ops.velocity_hip.frame0_init(frames, torch.from_numpy(qs), torch.from_numpy(np.asarray(K, np.float64)),
                                                                        torch.from_numpy(plate_world().reshape(4, 3)), BORDER[0], BORDER[1])
    assert p.shape == (5, 1004, 2) and p3.shape == (5, 1004, 3) and R.shape == (5, 3, 3) and rois.shape == (5, 8) and not rois.is_cuda
    ws = L.Workspace(1, W, H, 64)
    rc, outs, crois = _batch(ws, [frames[b] for b in range(5)], list(qs), K)
    L.check(rc, "vh_frame0_init_batch")
    want = frame0_host(outs, crois, 5)
    assert np.array_equal(n.cpu().numpy(), want["n"]) and np.array_equal(rois.numpy(), want["rois"])
    for b in range(5):
        k = int(want["n"][b])
        assert np.array_equal(p[b, :k].cpu().numpy(), want["p"][b, :k]) and np.all(p[b, k:].cpu().numpy() == 0)
    assert np.array_equal(p3.cpu().numpy(), want["p3"]) and np.array_equal(vp.cpu().numpy(), want["vp"])
    assert np.array_equal(t.cpu().numpy(), want["t"]) and np.array_equal(R.cpu().numpy().reshape(5, 9), want["R"]) and np.array_equal(res.cpu().numpy(), want["res"])


def test_frame0_batch_driver_matches_the_oracle(stills):
    from velocity_amd.driver import frame0_batch

    K, clips = _mixed_clips(stills)
    got = frame0_batch([f for f, _ in clips], [q for _, q in clips], K, roi_border=BORDER)
    assert len(got) == len(clips)
    for b, ((f, q), g) in enumerate(zip(clips, got)):
        ref = _oracle(f, q, K)
        assert set(g) == set(ref)
        assert np.array_equal(g["p"], ref["p"]) and np.array_equal(g["vp"], ref["vp"]) and g["boxa"] == ref["boxa"] and g["boxb"] == ref["boxb"]
        if b == MIRRORED:
            continue
        np.testing.assert_allclose(g["p3"], ref["p3"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(g["t"], ref["t"], rtol=1e-5)


def test_run_sequences_initialises_each_session_with_one_batch_call(stills, monkeypatch):
    from velocity_amd import _lib as L
    from velocity_amd.driver import run_sequence, run_sequences

    frames, times, q, K = stills["b_frames"], stills["b_times"], stills["b_q"], stills["b_K"]
    W = frames.shape[2]
    qm = q.copy()
    qm[:, 0] = (W - 1) - qm[:, 0]
    clips = [dict(frames=frames, q=q, times=times, name="b"),
             dict(frames=frames, q=q, times=times * np.float32(1.5) + np.float32(2.0), frame_numbers=list(range(100, 100 + len(frames))), name="b slow"),
             dict(frames=np.ascontiguousarray(frames[:, :, ::-1]), q=qm[[1, 0, 3, 2]], times=times, name="b mirrored")]
    singles = [run_sequence(c["frames"], c["q"], K, times=c["times"], frame_numbers=c.get("frame_numbers"), roi_border=BORDER, out=None, live=False, name=c["name"])
               for c in clips]
    lib = L.load()
    calls = []
    batch_fn = lib.vh_frame0_init_batch

    def counted(*a):
        calls.append(a[1])
        return batch_fn(*a)

    def refuse(*a):
        raise AssertionError("run_sequences called vh_frame0_init")

    monkeypatch.setattr(lib, "vh_frame0_init", refuse)
    monkeypatch.setattr(lib, "vh_frame0_init_batch", counted)
    got = run_sequences(clips, K, roi_border=BORDER, sessions=2)
    assert calls == [2, 1], calls
    for g, one in zip(got, singles):
        assert g["n_tracks0"] == one["n_tracks0"] > 100 and g["boxb"] == one["boxb"]
        assert np.array_equal(g["vg"], one["vg"]) and np.array_equal(g["vp"], one["vp"]) and np.array_equal(g["p"], one["p"]) and np.array_equal(g["ids"], one["ids"])
        for r in (0, 1, 4):
            assert np.array_equal(g["P"][r], one["P"][r], equal_nan=True)
        np.testing.assert_allclose(g["B"], one["B"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(g["S"][:, [0, 2, 3, 4, 5, 6, 7, 8]], one["S"][:, [0, 2, 3, 4, 5, 6, 7, 8]], rtol=1e-6, equal_nan=True)
        for a_, b_ in zip(g["lines"][2:-2], one["lines"][2:-2]):
            assert a_[:13] == b_[:13] and a_[26:] == b_[26:], (a_, b_)
        assert g["lines"][-2] == one["lines"][-2]
