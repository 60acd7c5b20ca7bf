"""GPU: the HIP KLT kernels held directly to the exact NumPy models of tests/image_ref.py and tests/lk_ref.py, on the scenes of
tests/klt_model_scenes.py (tests/test_klt_model_cpu.py holds the C oracle to the same models on the same scenes).  No expected value here comes from
the oracle.  Every comparison is exact equality except the two derived bounds of the truth tests."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import image_ref as IM  # noqa: E402
import klt_model_scenes as S  # noqa: E402
import lk_ref as R  # noqa: E402
from lk_support import forced_route  # noqa: E402

F32 = np.float32
ROUTES = {15: (0, 1, 2, 3, 4, 8), 51: (0, 1, 2, 5, 6, 7)}  # 0: the launcher's own choice; the forced routes that exist for the window (tests/test_gpu_klt.py)


def _lib():
    import torch

    from velocity_amd import _lib as L

    return L, torch


def _pyr_lk(f0, f1, pts, lk, fbt):
    """vh_pyr_lk through the C ABI with the err and fbe outputs -> (p2, v, err, fbe)."""
    L, torch = _lib()
    h, w = f0.shape
    n = len(pts)
    ws = L.workspace(w, h, n)
    a, b = torch.from_numpy(np.array(f0)).cuda(), torch.from_numpy(np.array(f1)).cuda()  # (copies: the scenes are read-only)
    p = torch.from_numpy(np.array(pts, F32)).cuda()
    p2 = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    v = torch.zeros(n, dtype=torch.uint8, device="cuda")
    err = torch.zeros(n, dtype=torch.float32, device="cuda")
    fbe = torch.zeros(n, dtype=torch.float32, device="cuda")
    prm = L.lk_params(lk)
    L.check(ws.lib.vh_pyr_lk(ws.handle, L.dptr(a), L.dptr(b), w, h, w, w, L.dptr(p), n, C.byref(prm), C.c_float(-1.0 if fbt is None else fbt), L.dptr(p2), L.dptr(v),
                             L.dptr(err), L.dptr(fbe), L.stream_ptr()), "vh_pyr_lk")
    return p2.cpu().numpy(), v.cpu().numpy().astype(bool), err.cpu().numpy(), fbe.cpu().numpy()


def _same_lk(got, want, ctx, with_fbe):
    p2, v, err, fbe = got
    mp, mv, merr, mfbe = want
    assert np.array_equal(v, mv), (ctx, np.flatnonzero(v != mv))
    assert np.array_equal(p2, mp, equal_nan=True), ctx
    assert np.array_equal(err, merr), ctx
    if with_fbe:
        assert np.array_equal(fbe, mfbe, equal_nan=True), ctx


@pytest.mark.parametrize("fbt", [None, 0.3])
@pytest.mark.parametrize("case", [0, 1])
def test_pyr_lk_equals_the_model_on_every_route(case, fbt):
    """Position, status, err and fbe of the coarse-window scene (3 levels) and the fine-window scene (2 levels), live and dead tracks in each (asserted
    on the model by the CPU suite and again here), under the default route and every forced one."""
    L, _ = _lib()
    f0, f1, pts = S.lk_scene(case)
    lk = S.lk_params(case)
    want = S.lk_model(case, fbt)
    assert want[1].sum() >= 20 and (~want[1]).sum() >= 20
    for route in ROUTES[lk["win"]]:
        with forced_route(route):
            got = _pyr_lk(f0, f1, pts, lk, fbt)
        _same_lk(got, want, (case, fbt, route), fbt is not None)


def test_pyr_lk_keeps_the_status_to_level_0_and_the_gate_strict():
    """The checkerboard whose upper level fails the min-eigenvalue test for every track while level 0 passes it, and identical frames at fbt = 0, where
    every fbe is exactly 0 and `<` keeps no track."""
    case = len(S.LK_CASES) - 1
    f0, f1, pts = S.lk_scene(case)
    for fbt in (None, 1.0):
        want = S.lk_model(case, fbt)
        assert want[1].sum() >= 20 and (~want[1]).sum() >= 20
        _same_lk(_pyr_lk(f0, f1, pts, S.lk_params(case), fbt), want, ("checkerboard", fbt), fbt is not None)
    f0, _, pts = S.lk_scene(0)
    pts = np.rint(pts)
    want = R.lk_fb(f0, f0, pts, 0.0, **S.lk_params(0))
    alive = R.lk_fb(f0, f0, pts, None, **S.lk_params(0))[1]
    assert alive.sum() >= 20 and not want[3][alive].any() and not want[1].any()
    _same_lk(_pyr_lk(f0, f0, pts, S.lk_params(0), 0.0), want, "fbt = 0", True)


def _klt_regional(im0, im, p0, T, lk, fbt, translate):
    """vh_klt_regional through the C ABI -> (p, v, roi)."""
    L, torch = _lib()
    h, w = im0.shape
    n = len(p0)
    ws = L.workspace(w, h, n)
    a, b = torch.from_numpy(np.array(im0)).cuda(), torch.from_numpy(np.array(im)).cuda()
    p = torch.from_numpy(np.array(p0, F32)).cuda()
    Tf = np.ascontiguousarray(T, F32).reshape(6)
    pout = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    v = torch.zeros(n, dtype=torch.uint8, device="cuda")
    roi = torch.zeros(4, dtype=torch.int32, device="cuda")
    prm = L.lk_params(lk)
    L.check(ws.lib.vh_klt_regional(ws.handle, L.dptr(a), L.dptr(b), w, h, w, w, L.dptr(p), n, Tf.ctypes.data_as(L.f32p), C.byref(prm), C.c_float(float(fbt)),
                                   int(bool(translate)), L.dptr(pout), L.dptr(v), L.dptr(roi), L.stream_ptr()), "vh_klt_regional")
    return pout.cpu().numpy(), v.cpu().numpy().astype(bool), tuple(int(x) for x in roi.cpu().numpy())


@pytest.mark.parametrize("cfg", sorted(S.REGIONAL_CONFIGS))
def test_klt_regional_equals_the_model_at_every_roi_alignment(cfg):
    """The translate path (integer shift truncated towards zero), the fine affine path and a pyramidal affine one, with the ROI's left edge at every
    residue modulo 4 (asserted on the model's ROIs): p, v and roi_out."""
    f0, f1, T_af, T_tr = S.regional_scene()
    lk, fbt, translate = S.REGIONAL_CONFIGS[cfg]
    assert sorted(S.regional_model(shift, cfg)[2][0] % 4 for shift in range(4)) == [0, 1, 2, 3]
    for shift in range(4):
        p, v, roi, _ = S.regional_model(shift, cfg)
        gp, gv, groi = _klt_regional(f0, f1, S.regional_points(shift), T_tr if translate else T_af, lk, fbt, translate)
        assert groi == roi, (shift, groi, roi)
        assert np.array_equal(gv, v), (shift, np.flatnonzero(gv != v))
        assert np.array_equal(gp, p, equal_nan=True), shift


def _remap(img, T, roi):
    L, torch = _lib()
    h, w = img.shape
    ws = L.workspace(w, h, 1)
    t = torch.from_numpy(np.array(img)).cuda()
    Tf = np.ascontiguousarray(T, F32).reshape(6)
    out = torch.zeros((roi[3] - roi[2], roi[1] - roi[0]), dtype=torch.uint8, device="cuda")
    L.check(ws.lib.vh_remap_affine(ws.handle, L.dptr(t), w, h, w, Tf.ctypes.data_as(L.f32p), *roi, L.dptr(out), L.stream_ptr()), "vh_remap_affine")
    return out.cpu().numpy()


def test_remap_equals_the_model_and_maps_a_plane_to_the_plane():
    """Ten of the seeded maps of a 70 x 90 image (rotations, zooms, footprints that leave the frame, translations on the rint ties) bit for bit, and the
    plane of tests/test_klt_model_cpu.py under the same derived bound, which the map with T[1] and T[2] exchanged must break."""
    img, cases = S.remap_cases()
    for k in range(0, 20, 2):  # (four tie translations, six rotations)
        T, roi = cases[k]
        assert np.array_equal(_remap(img, T, roi), IM.remap_affine(img, T, roi)), (k, T, roi)
    plane, ramp, T = S.ramp()
    assert S.footprint_inside(T, S.RAMP_ROI, ramp.shape) and S.footprint_inside(S.swapped(T), S.RAMP_ROI, ramp.shape)
    truth = IM.remap_truth(plane, T, S.RAMP_ROI)
    e = np.abs(_remap(ramp, T, S.RAMP_ROI).astype(np.float64) - truth).max()
    print(f"max |remap - plane| = {e:.4f}, bound {S.RAMP_BOUND:.4f}")
    assert e <= S.RAMP_BOUND, e
    assert np.abs(_remap(ramp, S.swapped(T), S.RAMP_ROI).astype(np.float64) - truth).max() > S.RAMP_BOUND


@pytest.mark.parametrize("shape", [(21, 30), (33, 1), (1, 9), (2, 2), (5, 7), (64, 63)])
def test_pyr_down_chain_equals_the_model(shape):
    """Level after level down to a single pixel, each level of the model computed from the DEVICE's previous level."""
    L, torch = _lib()
    img = np.random.default_rng(shape[0] * 100 + shape[1]).integers(0, 256, shape, dtype=np.uint8)
    ws = L.workspace(max(shape[1], 4), max(shape[0], 4), 1)
    t = torch.from_numpy(img).cuda()
    while True:
        h, w = t.shape
        out = torch.zeros(((h + 1) // 2, (w + 1) // 2), dtype=torch.uint8, device="cuda")
        L.check(ws.lib.vh_pyr_down(ws.handle, L.dptr(t), w, h, w, L.dptr(out), L.stream_ptr()), "vh_pyr_down")
        assert np.array_equal(out.cpu().numpy(), IM.pyr_down(t.cpu().numpy())), (shape, (h, w))
        if out.numel() == 1:
            break
        t = out


@pytest.mark.parametrize("cfg", sorted(S.PAIR_CONFIGS))
def test_klt_regional_returns_the_map_of_a_pair_built_from_it(cfg):
    """im0's ROI is the model's warp of im under T, so the device's warp must equal the template, no track may move, every track is valid and
    |p - p0 T| <= 8 * 2^-15 px (derived at tests/test_klt_model_cpu.py); with T[1] and T[2] exchanged the call must lose tracks or leave the bound."""
    im0, im, p0, T, truth, roi = S.pair_scene()
    lk, fbt = S.PAIR_CONFIGS[cfg]
    p, v, groi = _klt_regional(im0, im, p0, T, lk, fbt, False)
    assert groi == roi
    e = np.abs(p.astype(np.float64) - truth).max()
    print(f"{cfg}: {int(v.sum())} of {len(v)} valid, max |p - p0 T| = {e:.3g}, bound {S.PAIR_BOUND:.3g}")
    assert v.all() and e <= S.PAIR_BOUND, (int(v.sum()), e)
    p, v, _ = _klt_regional(im0, im, p0, S.swapped(T), lk, fbt, False)
    assert not v.all() or np.abs(p.astype(np.float64) - truth).max() > S.PAIR_BOUND


def test_klt_main_stages_equal_the_model():
    """Every modelled stage of KLTmain, the model fed from the device's own upstream stage output (RANSAC's selection is taken from the device)."""
    from velocity_amd import KLT

    f0, f1, p0 = S.main_scene()
    p, v, small, p_all, flags = KLT.KLTmain(f1.copy(), f0.copy(), None, p0.copy(), return_all=True)  # (copies: the scene is read-only)
    G = KLT.klt_stages(len(p0))
    assert flags == 0 and G["flags"] == 0 and v.sum() >= 20 and (~v).sum() >= 4
    assert np.array_equal(small, IM.resize_nearest(f1, 0.25))
    assert np.array_equal(p, p_all[v])
    for name, ok in S.main_stage_checks(f0, f1, p0, dict(G, p_fine=p_all, v=v)):
        assert ok, name
