"""RANSAC affine on the device (vh_ransac.hip) against the oracle and against plain float64 / NumPy references.

Every case calls the C entry vh_ransac_affine directly (with and without a `valid` mask) on each launch path -- 0: the launcher's choice, 1: the
three-kernel path (compaction, scoring spread over the chip, selection + refit), 2: the fused one-workgroup kernel whenever n <= RANSAC_FUSED_MAX
(3072) -- and asserts status, M (float64, bit for bit) and the inlier mask equal the oracle.  The sizes straddle the fused kernel's 512-pair chunks,
its 3072-pair limit and the rounds of eight hypotheses; the inlier ratios reach both the first-round stop and the 2000-hypothesis cap."""
import contextlib

import numpy as np
import pytest

from oracle import klt_oracle as KO
from ransac_ref import affine_scene, check_refit, refit_scenes, threshold_scene
from velocity_amd import synth

pytestmark = pytest.mark.gpu

FULL_HD = (0, 1920, 0, 1080)
SIZES = (0, 1, 2, 3, 4, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2559, 2560, 2561, 3071, 3072)


@contextlib.contextmanager
def ransac_path(path):
    from velocity_amd import _lib as L

    L.load().vh_debug_ransac_path(path)
    try:
        yield
    finally:
        L.load().vh_debug_ransac_path(0)


def run(src, dst, valid=None, path=0):
    """vh_ransac_affine on the device -> (status, M 2x3 float64, inl bool[n]).  The outputs start as garbage, so every entry is checked as written."""
    from velocity_amd import _lib as L

    torch = L.torch_cuda()
    n = len(src)
    s = L.to_dev(np.ascontiguousarray(src, np.float32).reshape(-1, 2), torch.float32)
    d = L.to_dev(np.ascontiguousarray(dst, np.float32).reshape(-1, 2), torch.float32)
    v = None if valid is None else L.to_dev(np.ascontiguousarray(valid, np.uint8), torch.uint8)
    ws = L.workspace(0, 0, max(n, 1))
    M = torch.full((6,), float("nan"), dtype=torch.float64, device="cuda")
    inl = torch.full((max(n, 1),), 0xA5, dtype=torch.uint8, device="cuda")
    st = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    with ransac_path(path):
        L.check(ws.lib.vh_ransac_affine(ws.handle, L.dptr(s), L.dptr(d), None if v is None else L.dptr(v), n, L.dptr(M), L.dptr(inl), L.dptr(st),
                                        L.stream_ptr()), "vh_ransac_affine")
        torch.cuda.synchronize()
    inl = inl[:n].cpu().numpy()
    assert np.isin(inl, (0, 1)).all()
    return int(st.item()), M.cpu().numpy().reshape(2, 3), inl.astype(bool)


def expect(src, dst, valid=None):
    """The oracle on the valid pairs, scattered back -> (status, M | None, inl bool[n], hypotheses replayed)."""
    n = len(src)
    idx = np.arange(n) if valid is None else np.nonzero(valid)[0]
    inl = np.zeros(n, bool)
    try:
        M, einl, it = KO.ransac_affine(np.asarray(src, np.float32).reshape(-1, 2)[idx], np.asarray(dst, np.float32).reshape(-1, 2)[idx])
    except ValueError:
        return -1, None, inl, None
    inl[idx] = einl
    return (1 if M is not None else 0), M, inl, it


def same(src, dst, valid=None, paths=(0, 1, 2), what=""):
    """Every path equals the oracle: status, inliers, M bit for bit.  Returns the oracle's result."""
    est, eM, einl, it = expect(src, dst, valid)
    for path in paths:
        st, M, inl = run(src, dst, valid, path)
        assert st == est, (what, path, st, est)
        assert np.array_equal(inl, einl), (what, path, int(inl.sum()), int(einl.sum()))
        if est == 1:
            assert np.array_equal(M, eM), (what, path, M, eM)
    return est, eM, einl, it


def test_sizes_and_paths_match_the_oracle():
    """m around the 512-pair chunks and the 3072-pair limit of the fused kernel, and around the rounds of eight: all three paths.  Past 3072 the
    launcher always takes the three-kernel path."""
    rng = np.random.default_rng(31)
    for m in SIZES:
        src, dst = affine_scene(rng, m, 0.7, FULL_HD)
        same(src, dst, what=m)
    for m in (3073, 5000, 20000):
        src, dst = affine_scene(rng, m, 0.7, FULL_HD)
        same(src, dst, paths=(0,), what=m)


@pytest.mark.parametrize("frame", [(1920, 1080), (3840, 2160)], ids=["1080p", "4k"])
def test_inlier_ratios_from_the_first_round_stop_to_the_hypothesis_cap(frame):
    W, H = frame
    rng = np.random.default_rng(7)
    # exact model: integer pairs under identity + integer translation -- hypothesis 0 is exact, scores every pair and ends the search
    src = np.c_[rng.integers(0, W, 1500), rng.integers(0, H, 1500)].astype(np.float32)
    st, M, inl, it = same(src, src + np.float32([7, -4]), paths=(1, 2), what="exact")
    assert st == 1 and inl.all() and it <= 8
    for ratio in (0.9, 0.5, 0.2, 0.08, 0.03):
        src, dst = affine_scene(rng, 1500, ratio, (0, W, 0, H), noise=0.3)
        st, M, inl, it = same(src, dst, paths=(1, 2), what=ratio)
        assert st == 1
        if ratio <= 0.08:
            assert it == 2000, (ratio, it)  # (1 - 0.08^3 -> 8990 hypotheses wanted: the cap)


def test_degenerate_inputs_match_the_oracle_including_failure():
    k = np.arange(50)
    line = np.c_[20 * k, 12 * k + 20].astype(np.float32)  # (integer points: exactly collinear in float32)
    tri = np.float32([[10, 10], [400, 30], [120, 300]])
    two_off = np.r_[line, np.float32([[300, 10], [700, 900]])]  # from: 2 pairs off the line; to: all on one line -> every sample collinear
    cases = {
        "identical": (np.full((100, 2), 321.5, np.float32), np.full((100, 2), 300.25, np.float32), 0),
        "collinear": (line, line + np.float32([3, 1]), 0),
        "m=3 collinear": (line[:3], line[:3], 0),
        "m=2": (tri[:2], tri[:2] + 1, 0),
        "at most 2 consistent pairs": (two_off, np.r_[line, line[[5, 40]]] + np.float32([1, 1]), 0),
        "duplicates exhaust the draws": (np.float32([[5, 5], [5, 5], [90, 7], [90, 7]]), np.float32([[6, 5], [6, 5], [91, 7], [91, 7]]), 0),
        "three non-collinear": (tri, tri @ np.float32([[1.01, 0.02], [-0.03, 0.98]]) + np.float32([4, -2]), 1),
        "four, two coincident": (np.r_[tri, tri[:1]], np.r_[tri, tri[:1]] + np.float32([2, 2]), 1),
    }
    for name, (src, dst, want) in cases.items():
        st, M, inl, it = same(src, dst, paths=(0, 1, 2), what=name)
        assert st == want, (name, st)
        if want == 0:
            assert M is None and not inl.any()
    st, M, inl, it = same(tri, tri * 2 + 1, paths=(1, 2), what="exact triangle")
    np.testing.assert_allclose(M, [[2, 0, 1], [0, 2, 1]], rtol=0, atol=1e-6)  # (the refit's moments are rounded to 2^-21)


def _masks(n, rng):
    yield "all zero", np.zeros(n, np.uint8)
    yield "first chunk", (np.arange(n) < 512).astype(np.uint8)
    yield "last chunk", (np.arange(n) >= (n - 1) // 512 * 512).astype(np.uint8)
    yield "alternating", (np.arange(n) % 2).astype(np.uint8)
    holes = np.ones(n, np.uint8)
    holes[500:530] = 0
    holes[3060:3090] = 0
    yield "holes at 511/512 and 3071/3072", holes
    yield "random 60 %", (rng.random(n) < 0.6).astype(np.uint8)


def test_valid_masks_compact_like_the_oracle():
    """The `valid` argument (the product passes LK status here): invalid pairs are skipped by the compaction and get inl == 0; the result is the
    oracle's on src[valid], scattered back."""
    rng = np.random.default_rng(5)
    for n in (3072, 5000):
        src, dst = affine_scene(rng, n, 0.75, FULL_HD)
        for name, valid in _masks(n, rng):
            same(src, dst, valid, what=(n, name))
    src, dst = affine_scene(rng, 4000, 0.75, FULL_HD)
    for count in (2, 3, 4, 511, 512, 513, 3071, 3072, 3073):  # valid counts across 3, 512 and 3072 while n > 3072
        valid = np.zeros(4000, np.uint8)
        valid[np.sort(rng.choice(4000, count, replace=False))] = 1
        same(src, dst, valid, what=count)


def test_inlier_threshold_is_float32_of_the_float64_squared_residual():
    """Against plain NumPy, not the oracle: float32(ex^2 + ey^2) <= 9 on pairs at exactly 3 px and on both float32 neighbours of 9 (ransac_ref.
    threshold_scene), on both paths and in the oracle."""
    src, dst, exp = threshold_scene()
    for path in (1, 2):
        st, M, inl = run(src, dst, path=path)
        assert st == 1 and np.array_equal(inl, exp), path
    same(src, dst, paths=(1, 2))


@pytest.mark.parametrize("scene", refit_scenes(), ids=lambda s: s[0])
def test_refit_matches_float64_least_squares(scene):
    """The device's refit on the inliers it returned against np.linalg.lstsq (bound: ransac_ref.refit_tol, from the float64 problem), on every path
    that serves the size.  Before the split mean sums the 1000-px box at 1e6 was off by 1.18 px (m = 3072) and 1.13 px (m = 20000), on the oracle and
    the device alike (bit-exact with each other); measured now <= 2.5e-10 px on frames up to 8K and at the offsets, <= 2.7e-6 px on 1-4 px clusters."""
    name, src, dst = scene
    paths = (1, 2) if len(src) <= 3072 else (0,)
    same(src, dst, paths=paths, what=name)
    for path in paths:
        st, M, inl = run(src, dst, path=path)
        check_refit(name, src, dst, M, inl)


def test_refit_out_of_range_fails_loudly():
    """A coordinate of 2^31 or more has no representable refit: status -1, no inliers, and the shim raises -- never a wrong M."""
    from velocity_amd.KLT import estimateAffine2D

    rng = np.random.default_rng(4)
    src, dst = affine_scene(rng, 200, 1.0, (3e9, 3e9 + 1e4, 0, 1e4), noise=0.0, A=np.array([[1.0, 0, 0], [0, 1.0, 0]]))
    for path in (1, 2):
        st, M, inl = run(src, dst, path=path)
        assert st == -1 and not inl.any(), path
    with pytest.raises(ValueError, match="representable"):
        estimateAffine2D(src, dst)
    src, dst = affine_scene(rng, 4000, 1.0, (0, 1e6, 0, 1e6), noise=0.0, A=np.array([[1.0, 0, 0], [0, 1.0, 0]]))
    same(src, dst, paths=(0,))
    assert run(src, dst)[0] == -1


def _klt_scenes():
    W, H = 960, 540
    m = synth.AffineMotion(W, H, tx=5.5, ty=-1.25)
    yield "seq", synth.render_frame(W, H, m, 1).numpy(), synth.render_frame(W, H, m, 0).numpy(), synth.grid_tracks(600, W, H)
    f0, f1, p0 = synth.gate_scene()
    yield "gate", f1, f0, p0
    K = synth.K_1080P.copy()
    K[:2, :2] *= 0.5
    K[2, 0], K[2, 1] = W / 2 + 0.5, H / 2 + 0.5
    hs = synth.HardScene(K, W, H, ring=12)
    yield "hard", hs.frame(1).numpy(), hs.frame(0).numpy(), synth.grid_tracks(500, W, H, seed=5)


@pytest.mark.parametrize("path", [1, 2])
def test_klt_main_all_stages_with_the_ransac_path_forced(path):
    """KLTmain with both RANSACs on the three-kernel path + the separate glue launch (1) or the fused kernel with the glue as its epilogue (2): every
    stage bit-exact with the oracle on the plain, the gate and the hard scene."""
    from velocity_amd import KLT

    for name, f1, f0, p0 in _klt_scenes():
        with ransac_path(path):
            p, v, small, p_all, flags = KLT.KLTmain(f1, f0, None, p0, lk_coarse=dict(max_level=2), return_all=True)
            G = KLT.klt_stages(len(p0))
        ep, ev, esmall, S = KO.klt_main(f1, f0, None, p0, lk_coarse=dict(max_level=2), stages=True)
        assert np.array_equal(small, esmall), name
        for k in ("p_small", "v_small", "T_trans", "roi", "p_coarse", "v_coarse", "T23", "warped"):
            assert np.array_equal(G[k], S[k]), (name, k)
        assert flags == S["flags"], name
        assert np.array_equal(v, ev) and np.array_equal(p_all, S["p_all"]) and np.array_equal(p, ep), name
