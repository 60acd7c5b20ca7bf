"""goodFeaturesToTrack on the device: the Harris and Shi-Tomasi detectors, minDistance and a mask (vh_good_features, vh_good_features2, vh_frame0_init_batch2, the
goodFeaturesToTrack shim, torch.ops.velocity_hip.good_features, driver.run_sequences).  Every comparison is bit-exact: coordinates, order and count
against tests/gftt_ref.py, which tests/test_gftt_cpu.py pins to the oracle (Harris, minDistance 0) and to OpenCV's spacing grid."""
import ctypes as C

import numpy as np
import pytest

import gftt_ref as G
from _helpers import frame0_host
from scenes import plate_world, stills  # noqa: F401 (stills: a fixture)
from test_gpu_frame0_batch import BORDER, _dev, _mixed_clips, _outputs

pytestmark = pytest.mark.gpu

from oracle import klt_oracle as KO  # noqa: E402 (checker only)

MDS = (0, 1, 2.5, 10, 30)
MCS = (1, 50, 1000, 3000)


@pytest.fixture(scope="module")
def images(stills):
    from velocity_amd import synth

    syn = synth.render_frame(640, 480, synth.AffineMotion(640, 480), 0, seed=0x5EED).numpy()
    return dict(synthetic=syn, stills=np.ascontiguousarray(stills["b_frames"][0]))


def _ref_all(img, block, use_harris, mask=None, quality=0.01):
    """{md: corners for max_corners = max(MCS)}; the greedy result for fewer corners is a prefix of it."""
    img = np.ascontiguousarray(img)
    w = img.shape[1]
    xy = G.keys_xy(G.candidate_keys(G.response(img, block, use_harris), quality, mask), w)
    out = {}
    for md in MDS:
        sel = G.spread_greedy(xy, md, max(MCS)) if md >= 1 else np.arange(min(len(xy), max(MCS)))
        out[md] = xy[sel].astype(np.float32)
    return out


def _gf2(img_t, mc, md, block, use_harris, mask_t=None, quality=0.01, k=0.04):
    """vh_good_features2 through ctypes -> (rc, corners [n, 2] numpy)."""
    import torch

    from velocity_amd import _lib as L

    h, w = img_t.shape
    ws = L.workspace()
    out = torch.full((mc, 2), -7.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((1,), -5, dtype=torch.int32, device="cuda")
    rc = ws.lib.vh_good_features2(ws.handle, L.dptr(img_t), w, h, img_t.stride(0), L.dptr(mask_t), w if mask_t is not None else 0, mc, quality, float(md),
                                  block, 1 if use_harris else 0, k, L.dptr(out), L.dptr(cnt), L.stream_ptr())
    if rc:
        return rc, None
    n = int(cnt.item())
    return 0, out[:n].cpu().numpy()


@pytest.mark.parametrize("use_harris", [False, True])
@pytest.mark.parametrize("block", [3, 5, 7])
def test_single_image_grid_equals_the_reference(images, use_harris, block):
    import torch

    from velocity_amd.images import goodFeaturesToTrack

    for name, img in images.items():
        ref = _ref_all(img, block, use_harris)
        t = torch.from_numpy(img).cuda()
        for md in MDS:
            for mc in MCS:
                want = ref[md][:mc]
                rc, got = _gf2(t, mc, md, block, use_harris)
                assert rc == 0
                assert np.array_equal(got, want), (name, md, mc, len(got), len(want))
            got = goodFeaturesToTrack(img, 1000, 0.01, md, blockSize=block, useHarrisDetector=use_harris).reshape(-1, 2)
            assert np.array_equal(got, ref[md][:1000]), (name, md)
        assert len(ref[10]) > 50 and len(ref[30]) < len(ref[10]) < len(ref[0]), name


def test_strided_roi_view(images):
    import torch

    from velocity_amd.images import goodFeaturesToTrack

    full = torch.from_numpy(images["stills"]).cuda()
    view = full[100:600, 150:900]
    assert view.stride(0) != view.shape[1]
    roi = images["stills"][100:600, 150:900]
    for use_harris in (False, True):
        ref = _ref_all(roi, 5, use_harris)
        for md in MDS:
            rc, got = _gf2(view, 1000, md, 5, use_harris)
            assert rc == 0 and np.array_equal(got, ref[md][:1000]), md
            assert np.array_equal(goodFeaturesToTrack(view, 1000, 0.01, md, blockSize=5, useHarrisDetector=use_harris).reshape(-1, 2), ref[md][:1000])


def test_masks(images):
    import torch

    from velocity_amd.images import goodFeaturesToTrack

    img = images["stills"]
    h, w = img.shape
    rng = np.random.default_rng(3)
    rand = (rng.random((h, w)) < 0.7).astype(np.uint8) * rng.integers(1, 256, (h, w)).astype(np.uint8)
    t = torch.from_numpy(img).cuda()
    for use_harris in (False, True):
        ref = _ref_all(img, 3, use_harris, rand)
        for md in (0, 10):
            rc, got = _gf2(t, 1000, md, 3, use_harris, torch.from_numpy(rand).cuda())
            assert rc == 0 and np.array_equal(got, ref[md][:1000]), (use_harris, md)
            shim = goodFeaturesToTrack(img, 1000, 0.01, md, blockSize=3, useHarrisDetector=use_harris, mask=rand).reshape(-1, 2)
            assert np.array_equal(shim, ref[md][:1000])
    zero = np.zeros((h, w), np.uint8)
    rc, got = _gf2(t, 1000, 10, 3, False, torch.from_numpy(zero).cuda())
    assert rc == 0 and len(got) == 0


@pytest.mark.parametrize("use_harris", [False, True])
def test_mask_hiding_the_maximum_sets_the_threshold(images, use_harris):
    """The mask hides the detector's global maximum: the threshold must come from the maximum over the kept pixels.  quality 0.05 and 3000 corners
    keep every candidate, so a threshold taken from the global maximum (checked here on the reference) would give other corners, with md 0 and 10."""
    import torch

    img = images["stills"]
    h, w = img.shape
    resp = G.response(img, 3, use_harris)
    y, x = np.unravel_index(np.argmax(resp), resp.shape)
    hide = np.ones((h, w), np.uint8)
    hide[max(y - 30, 0):y + 31, max(x - 30, 0):x + 31] = 0
    ref = _ref_all(img, 3, use_harris, hide, quality=0.05)
    kg = G.candidate_keys(resp, 0.05)  # threshold from the global maximum, then the mask
    xg = G.keys_xy(kg, w)
    xg = xg[hide[xg[:, 1], xg[:, 0]] != 0]
    t, m = torch.from_numpy(img).cuda(), torch.from_numpy(hide).cuda()
    for md in (0, 10):
        wrong = (xg[G.spread_greedy(xg, md, 3000)] if md else xg[:3000]).astype(np.float32)
        assert not np.array_equal(wrong, ref[md]), md
        rc, got = _gf2(t, 3000, md, 3, use_harris, m, quality=0.05)
        assert rc == 0 and np.array_equal(got, ref[md]), md


def test_old_parameters_through_the_new_entry(images):
    import torch

    from velocity_amd import _lib as L

    for img in images.values():
        t = torch.from_numpy(img).cuda()
        h, w = img.shape
        for block, mc in ((3, 50), (5, 1000), (7, 3000)):
            ws = L.workspace()
            out = torch.zeros((mc, 2), dtype=torch.float32, device="cuda")
            cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
            L.check(ws.lib.vh_good_features(ws.handle, L.dptr(t), w, h, w, mc, 0.01, block, 0.04, L.dptr(out), L.dptr(cnt), L.stream_ptr()), "vh_good_features")
            old = out[:int(cnt.item())].cpu().numpy()
            rc, new = _gf2(t, mc, 0.0, block, True)
            assert rc == 0 and np.array_equal(new, old), (block, mc)
            assert np.array_equal(new, KO.good_features(img, max_corners=mc, quality=0.01, block=block, k=0.04))


def _gf1(img_t, mc, block, quality=0.01, k=0.04):
    """vh_good_features through ctypes -> corners [n, 2] numpy."""
    import torch

    from velocity_amd import _lib as L

    h, w = img_t.shape
    ws = L.workspace()
    out = torch.full((mc, 2), -7.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((1,), -5, dtype=torch.int32, device="cuda")
    L.check(ws.lib.vh_good_features(ws.handle, L.dptr(img_t), w, h, img_t.stride(0), mc, quality, block, k, L.dptr(out), L.dptr(cnt), L.stream_ptr()),
            "vh_good_features")
    return out[:int(cnt.item())].cpu().numpy()


SMALL_SIZES = ((3, 3), (4, 3), (5, 5), (7, 40), (63, 15), (64, 16), (65, 17), (129, 33), (200, 9))  # (w, h) around the detector's 64 x 16 tile
SMALL_BLOCKS = (1, 2, 4, 5, 15)
SMALL_BUDGETS = (1, 50, 3000)  # a one-key select, the in-LDS sort, the segmented sort
STRIDED = (65, 17)  # this size runs as a view of a larger tensor


def _small_images():
    rng = np.random.default_rng(7)
    return {wh: rng.integers(0, 256, (wh[1], wh[0]), dtype=np.uint8) for wh in SMALL_SIZES}


def _small_refs(img):
    """{(block, max_corners): (Harris corners of the C oracle, Shi-Tomasi corners of gftt_ref)}, with the counts the test relies on asserted."""
    w, h = img.shape[1], img.shape[0]
    refs = {}
    for block in SMALL_BLOCKS:
        for mc in SMALL_BUDGETS:
            refs[block, mc] = (KO.good_features(img, mc, 0.01, block, 0.04), G.good_features(img, mc, 0.01, 0.0, block=block, use_harris=False))
        n = len(refs[block, 3000][0])
        if block == 1:
            assert n == 0, (w, h, n)  # a rank-one structure tensor has no positive Harris response
        elif w >= 7 and h >= 7:
            assert n >= 1, (w, h, block)  # the case compares corners, not two empty lists
    if (w, h) == (5, 5):  # 25 pixels, 9 of them interior: some blocks leave no candidate, not all
        assert any(len(refs[block, 3000][0]) for block in SMALL_BLOCKS[1:])
    return refs


@pytest.mark.parametrize("size", SMALL_SIZES, ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_small_and_awkward_shapes_through_both_entries(size):
    """The only detector on images below, at and just past its 64 x 16 tile, with even blocks and a halo wider than the image (block 15: REFLECT_101
    folds more than once), at budgets that take the one-key select, the in-LDS sort and the segmented sort: vh_good_features and vh_good_features2
    equal the C oracle bit for bit (Harris), vh_good_features2 equals gftt_ref (Shi-Tomasi)."""
    import torch

    img = _small_images()[size]
    w, h = size
    refs = _small_refs(img)
    if size == STRIDED:
        big = torch.full((h + 9, w + 30), 255, dtype=torch.uint8, device="cuda")
        big[4:4 + h, 11:11 + w] = torch.from_numpy(img).cuda()
        t = big[4:4 + h, 11:11 + w]
        assert t.stride(0) != w
    else:
        t = torch.from_numpy(img).cuda()
    for (block, mc), (harris, shi) in refs.items():
        assert np.array_equal(_gf1(t, mc, block), harris), ("vh_good_features", block, mc)
        rc, got = _gf2(t, mc, 0.0, block, True)
        assert rc == 0 and np.array_equal(got, harris), ("vh_good_features2 harris", block, mc)
        rc, got = _gf2(t, mc, 0.0, block, False)
        assert rc == 0 and np.array_equal(got, shi), ("vh_good_features2 shi-tomasi", block, mc)


def test_equal_responses_keep_the_larger_pixel_index_first():
    """A periodic 80 x 32 image whose candidates share a few exactly equal responses: the order among equals (larger pixel index first) must hold through
    the select threshold (10 corners: the threshold falls inside a run of equal responses) and the full list (3000)."""
    import torch

    img = np.tile(np.array([[0, 255, 0, 0], [255, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]], np.uint8), (8, 20))
    assert img.shape == (32, 80)
    t = torch.from_numpy(img).cuda()
    full = KO.good_features(img, 3000, 0.01, 3, 0.04)
    resp = G.response(img, 3, True)
    vals = resp[full[:, 1].astype(int), full[:, 0].astype(int)]
    assert len(full) > 100 and len(np.unique(vals)) < len(full) // 4 and vals[9] == vals[10], "the image must give many equal responses, across the cut at 10"
    ten = KO.good_features(img, 10, 0.01, 3, 0.04)
    assert np.array_equal(ten, full[:10])
    for mc, want in ((10, ten), (3000, full)):
        assert np.array_equal(_gf1(t, mc, 3), want), mc
        rc, got = _gf2(t, mc, 0.0, 3, True)
        assert rc == 0 and np.array_equal(got, want), mc


def test_torch_op_equals_the_shim(images):
    import torch

    import velocity_amd.torch_ops  # noqa: F401

    img = images["stills"]
    mask = np.ones(img.shape, np.uint8)
    mask[:, :300] = 0
    corners, count = torch.ops.velocity_hip.good_features(torch.from_numpy(img).cuda(), 500, 0.01, 10.0, torch.from_numpy(mask).cuda(), 5, False)
    n = int(count.item())
    assert corners.shape == (500, 2) and corners.is_cuda
    ref = _ref_all(img, 5, False, mask)[10][:500]
    assert np.array_equal(corners[:n].cpu().numpy(), ref)


def _batch2(ws, frames, qs, K, use_harris, md, max_corners=1000, outs=None, border=BORDER):
    from velocity_amd import _lib as L

    torch = L.torch_cuda()
    nb, cap = len(frames), 4 + max_corners
    H, W = frames[0].shape
    outs = _outputs(torch, nb, cap) if outs is None else outs
    q = np.ascontiguousarray(np.stack([np.asarray(x, np.float32).reshape(4, 2) for x in qs]))
    ptrs = (C.c_void_p * nb)(*[f.data_ptr() for f in frames])
    rois = (C.c_int * (8 * nb))()
    p, p3, vp, t, R, res, n = outs
    rc = ws.lib.vh_frame0_init_batch2(ws.handle, nb, C.cast(ptrs, C.c_void_p), W, H, W, q.ctypes.data_as(L.f32p), L.host_K(K).ctypes.data_as(L.f64p),
                                      plate_world().ctypes.data_as(L.f64p), border[0], border[1], max_corners, 0.01, 5, 0.04, 1 if use_harris else 0, float(md), 5,
                                      100, 0.001, L.dptr(p), L.dptr(p3), L.dptr(vp), L.dptr(t), L.dptr(R), L.dptr(res), L.dptr(n), rois, L.stream_ptr())
    return rc, outs, rois


def _batch1(ws, frames, qs, K, max_corners=1000):
    from velocity_amd import _lib as L

    torch = L.torch_cuda()
    nb, cap = len(frames), 4 + max_corners
    H, W = frames[0].shape
    outs = _outputs(torch, nb, cap)
    q = np.ascontiguousarray(np.stack([np.asarray(x, np.float32).reshape(4, 2) for x in qs]))
    ptrs = (C.c_void_p * nb)(*[f.data_ptr() for f in frames])
    rois = (C.c_int * (8 * nb))()
    p, p3, vp, t, R, res, n = outs
    L.check(ws.lib.vh_frame0_init_batch(ws.handle, nb, C.cast(ptrs, C.c_void_p), W, H, W, q.ctypes.data_as(L.f32p), L.host_K(K).ctypes.data_as(L.f64p),
                                        plate_world().ctypes.data_as(L.f64p), BORDER[0], BORDER[1], max_corners, 0.01, 5, 0.04, 5, 100, 0.001, L.dptr(p), L.dptr(p3),
                                        L.dptr(vp), L.dptr(t), L.dptr(R), L.dptr(res), L.dptr(n), rois, L.stream_ptr()), "vh_frame0_init_batch")
    return outs, rois


def _same(a, b, nb):
    for key in ("n", "t", "R", "res", "p3", "vp", "rois"):
        assert np.array_equal(a[key], b[key]), key
    for i in range(nb):
        n = int(a["n"][i])
        assert np.array_equal(a["p"][i, :n], b["p"][i, :n]), i


def test_batch2_shi_tomasi_spaced_equals_reference_and_single_clips(stills):
    from velocity_amd import _lib as L

    K, clips = _mixed_clips(stills)
    H, W = clips[0][0].shape
    frames, qs = _dev([f for f, _ in clips]), [q for _, q in clips]
    ws = L.Workspace(1, W, H, 64)
    rc, outs, rois = _batch2(ws, frames, qs, K, False, 10)
    L.check(rc, "vh_frame0_init_batch2")
    got = frame0_host(outs, rois, len(clips))
    assert got["n"][0] > 50 and got["n"][4] == 4, got["n"]
    for b, (f, q) in enumerate(clips):
        x0, x1, y0, y1 = got["rois"][b, 4:8]
        ref = G.good_features(f[y0:y1, x0:x1], 1000, 0.01, 10, block=5, use_harris=False) + np.float32([x0, y0])
        ref = KO.corner_subpix(f, ref, 5, 100, 0.001)
        n = int(got["n"][b])
        assert n == 4 + len(ref), (b, n, len(ref))
        assert np.array_equal(got["p"][b, 4:n], ref), b
        assert np.array_equal(got["p"][b, :4], np.asarray(q, np.float32).reshape(4, 2)), b
        ws1 = L.Workspace(1, W, H, 64)
        rc, o1, r1 = _batch2(ws1, frames[b:b + 1], qs[b:b + 1], K, False, 10)
        L.check(rc, "vh_frame0_init_batch2")
        one = frame0_host(o1, r1, 1)
        for key in ("n", "t", "R", "res", "p3", "vp", "rois"):
            assert np.array_equal(got[key][b:b + 1], one[key]), (b, key)
        assert np.array_equal(got["p"][b, :n], one["p"][0, :n]), b


def test_batch2_defaults_equal_batch(stills):
    from velocity_amd import _lib as L

    K, clips = _mixed_clips(stills)
    H, W = clips[0][0].shape
    frames, qs = _dev([f for f, _ in clips]), [q for _, q in clips]
    ws = L.Workspace(1, W, H, 64)
    rc, outs, rois = _batch2(ws, frames, qs, K, True, 0.0)
    L.check(rc, "vh_frame0_init_batch2")
    outs1, rois1 = _batch1(L.Workspace(1, W, H, 64), frames, qs, K)
    _same(frame0_host(outs, rois, len(clips)), frame0_host(outs1, rois1, len(clips)), len(clips))


def test_batch2_chunked_equals_one_chunk_and_large_max_corners(stills):
    from velocity_amd import _lib as L

    K, clips = _mixed_clips(stills)
    H, W = clips[0][0].shape
    frames, qs = _dev([f for f, _ in clips]), [q for _, q in clips]
    for mc in (1000, 3000):
        res = []
        for nres in (2, 5):
            ws = L.Workspace(1, W, H, 64)
            L.check(ws.lib.vh_init_reserve_batch(ws.handle, nres, W, H, L.stream_ptr()), "vh_init_reserve_batch")
            rc, outs, rois = _batch2(ws, frames, qs, K, False, 10, max_corners=mc)
            L.check(rc, "vh_frame0_init_batch2")
            res.append(frame0_host(outs, rois, len(clips)))
        _same(res[0], res[1], len(clips))
    # a textured frame with a full-frame ROI: more than one window of candidates walked, more than 2048 corners kept
    from velocity_amd import synth

    f = synth.render_frame(W, H, synth.AffineMotion(W, H), 0).numpy()
    rc, outs, rois = _batch2(L.Workspace(1, W, H, 64), _dev([f]), qs[:1], K, False, 2.5, max_corners=3000, border=(2000, 2000))
    L.check(rc, "vh_frame0_init_batch2")
    got = frame0_host(outs, rois, 1)
    x0, x1, y0, y1 = got["rois"][0, 4:8]
    ref = G.good_features(f[y0:y1, x0:x1], 3000, 0.01, 2.5, block=5, use_harris=False) + np.float32([x0, y0])
    assert len(ref) > 2048 and int(got["n"][0]) == 4 + len(ref)
    assert np.array_equal(got["p"][0, 4:4 + len(ref)], KO.corner_subpix(f, ref, 5, 100, 0.001))


def test_batch2_graph_capture_replays_the_eager_result(stills):
    import torch

    from velocity_amd import _lib as L

    K, clips = _mixed_clips(stills)
    H, W = clips[0][0].shape
    frames, qs = _dev([f for f, _ in clips]), [q for _, q in clips]
    ws = L.Workspace(1, W, H, 64)
    L.check(ws.lib.vh_init_reserve_batch(ws.handle, len(clips), W, H, L.stream_ptr()), "vh_init_reserve_batch")
    rc, outs, rois = _batch2(ws, frames, qs, K, False, 10)
    L.check(rc, "vh_frame0_init_batch2")
    eager = frame0_host(outs, rois, len(clips))
    cap_outs = _outputs(torch, len(clips), 1004)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc, _, _ = _batch2(ws, frames, qs, K, False, 10, outs=cap_outs)
    assert rc == 0, ws.lib.vh_last_error()
    for x in cap_outs:
        x.fill_(3)
    g.replay()
    torch.cuda.synchronize()
    _same(frame0_host(cap_outs, rois, len(clips)), eager, len(clips))


def test_run_sequences_spaced_shi_tomasi_equals_run_sequence(stills):
    from velocity_amd.driver import run_sequence, run_sequences

    frames, times, q, K = stills["b_frames"], stills["b_times"], stills["b_q"], stills["b_K"]
    clips = [dict(frames=frames, q=q, times=times, name="b"),
             dict(frames=np.ascontiguousarray(frames[::-1]), q=q, times=times, name="b reversed")]
    got = run_sequences(clips, K, roi_border=BORDER, use_harris=False, min_distance=10)
    for g, c in zip(got, clips):
        one = run_sequence(c["frames"], c["q"], K, times=c["times"], roi_border=BORDER, out=None, live=False, use_harris=False, min_distance=10)
        assert g["n_tracks0"] == one["n_tracks0"] > 20 and g["boxb"] == one["boxb"]
        assert np.array_equal(g["vg"], one["vg"]) and np.array_equal(g["vp"], one["vp"])
        for r in (0, 1, 4):
            assert np.array_equal(g["P"][r], one["P"][r], equal_nan=True)
        np.testing.assert_allclose(g["B"], one["B"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(g["S"][:, [0, 2, 3, 4, 5, 6, 7, 8]], one["S"][:, [0, 2, 3, 4, 5, 6, 7, 8]], rtol=1e-6, equal_nan=True)
        f0 = c["frames"][0]
        x0, x1, y0, y1 = g["boxb"]
        ref = G.good_features(f0[y0:y1, x0:x1], 1000, 0.01, 10, block=5, use_harris=False) + np.float32([x0, y0])
        assert np.array_equal(g["P"][0:2, 4:g["n_tracks0"], 0].T, KO.corner_subpix(f0, ref, 5, 100, 0.001)), "frame-0 corners"


def test_bad_arguments(images):
    import torch

    from velocity_amd import _lib as L
    from velocity_amd.images import goodFeaturesToTrack

    t = torch.from_numpy(images["synthetic"]).cuda()
    for md in (float("nan"), float("inf"), -float("inf")):
        rc, _ = _gf2(t, 100, md, 3, False)
        assert rc == -1 and b"min_distance" in L.load().vh_last_error()
    rc, _ = _gf2(t, 0, 10, 3, False)
    assert rc == -1
    with pytest.raises(ValueError):
        goodFeaturesToTrack(images["synthetic"], 100, 0.01, 10, useHarrisDetector=False, mask=np.ones((10, 10), np.uint8))
    with pytest.raises(ValueError):
        goodFeaturesToTrack(images["synthetic"], 100, 0.01, 10, useHarrisDetector=False, mask=np.ones(images["synthetic"].shape, np.float32))
