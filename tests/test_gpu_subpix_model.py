"""GPU: cornerSubPix on the device -- k_init_subpix through vh_corner_subpix and the drop-in shim, k_f0b_subpix through vh_frame0_init_batch2 / 3 -- held
directly to the exact NumPy model of tests/subpix_ref.py on the scenes of tests/subpix_scenes.py (tests/test_subpix_model_cpu.py holds the C oracle to
the same model on the same scenes, and proves there which defects the scenes see).  No expected value here comes from the oracle.  Every comparison is
exact equality of bit patterns except the derived bound of the truth test."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import subpix_ref as SR  # noqa: E402
import subpix_scenes as S  # noqa: E402
from _helpers import frame0_host  # noqa: E402
from lk_support import strided_view  # noqa: E402
from scenes import plate_world  # noqa: E402
from scenes import to_cuda as to_dev  # noqa: E402 (copies first: the scenes are read-only)

F32 = np.float32
SENT = -7.0


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same(got, want, ctx):
    bad = np.flatnonzero((bits(got) != bits(want)).any(1))
    assert got.shape == want.shape and not len(bad), (ctx, len(bad), bad[:8], got[bad[:8]], want[bad[:8]])


def _subpix(img_t, pts, win, max_iter, eps, n=None):
    """vh_corner_subpix through the C ABI on the first n points of a sentinel-padded buffer -> (rc, the whole buffer [len(pts) + 2, 2])."""
    import torch

    from velocity_amd import _lib as L

    n = len(pts) if n is None else n
    h, w = img_t.shape
    ws = L.workspace()
    buf = torch.full((len(pts) + 2, 2), SENT, dtype=torch.float32, device="cuda")
    buf[:n] = torch.from_numpy(np.array(pts[:n], F32)).cuda()
    rc = ws.lib.vh_corner_subpix(ws.handle, L.dptr(img_t), w, h, img_t.stride(0), L.dptr(buf), n, win, max_iter, eps, L.stream_ptr())
    return rc, buf.cpu().numpy()


def _refined(img_t, pts, win, max_iter, eps):
    rc, buf = _subpix(img_t, pts, win, max_iter, eps)
    assert rc == 0 and (buf[len(pts):] == SENT).all()
    return buf[:len(pts)]


# ---------------------------------------------------------------------------------------------------------------------
# vh_corner_subpix (k_init_subpix)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win", S.WINS)
def test_corner_subpix_equals_the_model_at_every_window(win):
    """The texture's 96 points (image corners, edges, the flat band, every exit of the loop: asserted on the model by the CPU suite and again here) at
    the reference's stop setting, and every other stop setting at windows 1, 5 and 7: each window reads its own mask of the context's table."""
    img, pts = S.texture()
    t = to_dev(img)
    want, exits, reverted, _ = S.texture_model(win, 0)
    seen = set(zip(exits.tolist(), reverted.tolist()))
    assert set(S.CENSUS[win]) <= seen, (win, sorted(seen))
    _same(_refined(t, pts, win, *S.STOPS[0]), want, (win, S.STOPS[0]))
    if win in (1, 5, 7):
        for k, stop in enumerate(S.STOPS[1:], 1):
            _same(_refined(t, pts, win, *stop), S.texture_model(win, k)[0], (win, stop))


def test_corner_subpix_on_tiny_images_and_the_exact_step():
    """Patches larger than the image (8 x 6 at window 7: every tap clamped; 3 x 3 at window 1), at every stop setting; and the point whose first step
    lands ON x = w having moved exactly win (subpix_scenes.step), where `>= w` ends the loop and `> win` keeps the point."""
    for name in sorted(S.TINY):
        img, pts = S.tiny(name)
        t = to_dev(img)
        for k, stop in enumerate(S.STOPS):
            _same(_refined(t, pts, S.TINY[name][2], *stop), S.tiny_model(name, k)[0], (name, stop))
    img, pts = S.step()
    got = _refined(to_dev(img), pts, S.STEP_WIN, 100, 0.001)
    assert got.tolist() == [list(S.STEP_END)], got
    _same(got, SR.corner_subpix(img, pts, S.STEP_WIN, 100, 0.001), "step")


@pytest.mark.parametrize("win", [1, 5, 7])
def test_corner_counts_around_the_block_and_none(win):
    """Prefixes of 1, 63, 64, 65 and 96 points: the prefix is refined, every row behind it keeps its sentinel.  n = 0 returns 0 and writes nothing."""
    img, pts = S.texture()
    t = to_dev(img)
    want = S.texture_model(win, 0)[0]
    for n in (0,) + S.COUNTS:
        rc, buf = _subpix(t, pts, win, 100, 0.001, n=n)
        assert rc == 0, n
        assert (buf[n:] == SENT).all(), n
        _same(buf[:n], want[:n], (win, n))


def test_corner_subpix_on_pitched_views_at_every_base_alignment():
    """The texture as a view with a row pitch of 64 bytes and its base address at each residue modulo 4."""
    img, pts = S.texture()
    for phase in range(4):
        v = strided_view(np.array(img), 64, phase)
        for win in (2, 7):
            _same(_refined(v, pts, win, 100, 0.001), S.texture_model(win, 0)[0], (phase, win))


def test_windows_outside_1_to_7_are_refused():
    """win = 0 and win = 8 return -1 and leave the points untouched."""
    img, pts = S.texture()
    t = to_dev(img)
    for win in (0, 8, -1):
        rc, buf = _subpix(t, pts, win, 100, 0.001)
        assert rc == -1, win
        assert np.array_equal(bits(buf[:len(pts)]), bits(pts)) and (buf[len(pts):] == SENT).all(), win


# ---------------------------------------------------------------------------------------------------------------------
# truth
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["axis", "sheared"])
def test_junction_truth(kind):
    """The device's own output on the point-symmetric junctions: max |p - corner| <= subpix_scenes.JUNCTION_BOUND (derived at
    tests/test_subpix_model_cpu.py::test_junction_truth) from 16 starts up to win - 1 away, windows 2 .. 7, eps = 0."""
    t = to_dev(S.junction(kind))
    for win in S.JUNCTION_WINS:
        got = _refined(t, S.junction_starts(win), win, *S.JUNCTION_STOP)
        e = S.junction_error(got)
        print(f"{kind} win {win}: max |p - corner| = {e:.3e}, bound {S.JUNCTION_BOUND:.3e}")
        assert e <= S.JUNCTION_BOUND, (kind, win, e)
        _same(got, S.junction_model(kind, win), (kind, win))


# ---------------------------------------------------------------------------------------------------------------------
# k_f0b_subpix
# ---------------------------------------------------------------------------------------------------------------------
def _outputs(torch, nb, cap):
    dev = "cuda"
    return (torch.full((nb, cap, 2), SENT, dtype=torch.float32, device=dev), torch.full((nb, cap, 3), SENT, dtype=torch.float64, device=dev),
            torch.full((nb, cap), 77, dtype=torch.uint8, device=dev), torch.full((nb, 3), SENT, dtype=torch.float32, device=dev),
            torch.full((nb, 9), SENT, dtype=torch.float64, device=dev), torch.full((nb,), SENT, dtype=torch.float64, device=dev),
            torch.full((nb,), -5, dtype=torch.int32, device=dev))


def _check_clip(got, b, k, win, use_harris, min_distance):
    frame, q, K, roi = S.frame0_scene(k)
    corners, want = S.frame0_model(k, win, use_harris, min_distance)
    n = int(got["n"][b])
    assert tuple(got["rois"][b, 4:8]) == roi, (b, got["rois"][b])
    assert n == 4 + len(corners) and len(corners) > 64, (b, n, len(corners))
    assert np.array_equal(got["p"][b, :4], q), b
    assert (want != corners).any(1).sum() >= 5, (b, win)  # a condition on the scene: the refinement moves corners
    _same(got["p"][b, 4:n], want, (b, k, win))


@pytest.mark.parametrize("win", S.WINS)
def test_frame0_batch2_refines_with_each_window(win):
    """vh_frame0_init_batch2 on the 96 x 64 frame whose plate ROI the border clips at the frame: rows 4 .. n of p_out are the model applied on the FULL
    frame to the detector's model (gftt_ref.good_features of the ROI + the ROI's origin), 90 corners in two blocks, for subpix_win 1 .. 7."""
    import torch

    from velocity_amd import _lib as L

    frame, q, K, roi = S.frame0_scene(0)
    h, w = frame.shape
    ws = L.Workspace(1, w, h, 64)
    f = to_dev(frame)
    outs = _outputs(torch, 1, 4 + S.F0_CORNERS)
    rois = (C.c_int * 8)()
    ptrs = (C.c_void_p * 1)(f.data_ptr())
    qh = np.ascontiguousarray(q, F32).reshape(1, 4, 2)
    L.check(ws.lib.vh_frame0_init_batch2(ws.handle, 1, C.cast(ptrs, C.c_void_p), w, h, w, qh.ctypes.data_as(L.f32p), L.host_K(K).ctypes.data_as(L.f64p),
                                         plate_world().ctypes.data_as(L.f64p), S.F0_BORDER[0], S.F0_BORDER[1], S.F0_CORNERS, 0.01, 5, 0.04, 1, 0.0, win, 100, 0.001,
                                         *[L.dptr(x) for x in outs], rois, L.stream_ptr()), "vh_frame0_init_batch2")
    _check_clip(frame0_host(outs, rois, 1), 0, 0, win, True, 0.0)


def test_frame0_batch3_clamps_each_clip_to_its_own_frame():
    """One vh_frame0_init_batch3 call with two clips of different frame sizes and row pitches (96 x 64 dense; 80 x 56 in rows of 128 bytes): each clip's
    patches are clamped with its own w, h and stride.  Window 7, whose patches leave both frames; the Shi-Tomasi detector spaced by 3 px."""
    import torch

    from velocity_amd import _lib as L

    win, use_harris, md = 7, False, 3.0
    scenes = [S.frame0_scene(0), S.frame0_scene(1)]
    views = [to_dev(scenes[0][0]), strided_view(np.array(scenes[1][0]), 128, 1)]
    cams = [L.clip_camera(v.shape[1], v.shape[0], sc[2], stride=v.stride(0)) for v, sc in zip(views, scenes)]
    assert (cams[0].w, cams[0].h, cams[0].stride) == (96, 64, 96) and (cams[1].w, cams[1].h, cams[1].stride) == (80, 56, 128)
    ws = L.Workspace(1, 96, 64, 64)
    outs = _outputs(torch, 2, 4 + S.F0_CORNERS)
    rois = (C.c_int * 16)()
    ptrs = (C.c_void_p * 2)(*[v.data_ptr() for v in views])
    qh = np.ascontiguousarray(np.stack([sc[1] for sc in scenes]), F32)
    L.check(ws.lib.vh_frame0_init_batch3(ws.handle, 2, C.cast(ptrs, C.c_void_p), (L.ClipCamera * 2)(*cams), qh.ctypes.data_as(L.f32p),
                                         plate_world().ctypes.data_as(L.f64p), S.F0_BORDER[0], S.F0_BORDER[1], S.F0_CORNERS, 0.01, 5, 0.04, 0, md, win, 100, 0.001,
                                         *[L.dptr(x) for x in outs], rois, L.stream_ptr()), "vh_frame0_init_batch3")
    got = frame0_host(outs, rois, 2)
    for b in range(2):
        _check_clip(got, b, b, win, use_harris, md)


# ---------------------------------------------------------------------------------------------------------------------
# the drop-in shim
# ---------------------------------------------------------------------------------------------------------------------
def test_shim_criteria_types():
    """velocity_amd.images.cornerSubPix: criteria type 1 (count only) is eps = 0, type 2 (eps only) is the cap of 100, type 3 both; in the shape given."""
    from velocity_amd.images import cornerSubPix

    img, pts = S.texture()
    for win in (3, 5):
        for typ, cnt, eps, model in ((1, 2, 0.5, (2, 0.0)), (2, 3, 0.001, (100, 0.001)), (3, 1, 0.001, (1, 0.001)), (3, 100, 0.001, (100, 0.001))):
            want = S.texture_model(win, S.STOPS.index(model))[0]
            got = cornerSubPix(np.array(img), np.array(pts).reshape(-1, 1, 2), (win, win), (-1, -1), (typ, cnt, eps))
            assert got.shape == (len(pts), 1, 2) and got.dtype == F32
            _same(got.reshape(-1, 2), want, (win, typ, cnt, eps))
