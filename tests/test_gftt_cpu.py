"""goodFeaturesToTrack beyond the reference's call, without a GPU: tests/gftt_ref.py is pinned to the oracle on the half they share (Harris, minDistance 0),
its greedy spacing to OpenCV's cell grid, its minimum eigenvalue to a float64 eigen solve; the new C ABI symbols and the torch op exist."""
import os

import numpy as np
import pytest
import torch

import gftt_ref as G
from oracle import klt_oracle as KO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _synthetic(w=320, h=240, seed=7):
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w), np.float64)
    for _ in range(60):  # random rectangles of random grey: many corners, some response ties
        x0, y0 = rng.integers(0, w - 8), rng.integers(0, h - 8)
        img[y0:y0 + rng.integers(4, 40), x0:x0 + rng.integers(4, 40)] = rng.integers(0, 256)
    img += rng.normal(0, 3, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def stills_roi():
    d = np.load(os.path.join(ROOT, "tests", "golden", "stills_gray.npz"))
    return d["b_frames"][0][200:520, 300:700]


@pytest.mark.parametrize("block", [3, 5, 7])
def test_harris_response_equals_the_oracle_bit_for_bit(block, stills_roi):
    for img in (_synthetic(), stills_roi):
        ref = G.harris_response(img, block, 0.04)
        assert np.array_equal(ref.view(np.uint32), KO.harris_response(img, block=block, k=0.04).view(np.uint32))


@pytest.mark.parametrize("block,mc", [(3, 300), (5, 1000), (7, 50)])
def test_harris_corners_without_spacing_equal_the_oracle(block, mc, stills_roi):
    for img in (_synthetic(), stills_roi):
        got = G.good_features(img, mc, 0.01, 0.0, block=block, use_harris=True)
        assert len(got) > 0
        assert np.array_equal(got, KO.good_features(img, max_corners=mc, quality=0.01, block=block, k=0.04))


@pytest.mark.parametrize("md", [1, 1.5, 2.4, 2.5, 3.7, 10, 33.3])
def test_greedy_spacing_equals_opencv_grid(md):
    rng = np.random.default_rng(int(md * 10))
    w, h = 211, 157
    for trial in range(6):
        n = int(rng.integers(50, 3000))
        idx = rng.choice(w * h, size=n, replace=False)
        xy = np.stack([idx % w, idx // w], 1)
        mc = int(rng.choice([5, 100, 10**6]))
        g = G.spread_greedy(xy, md, mc)
        assert np.array_equal(g, G.spread_grid(xy, w, h, md, mc)), (md, trial)
        assert len(g) <= mc
        kx = xy[g]
        d2 = ((kx[:, None, :] - kx[None, :, :]) ** 2).sum(-1)
        np.fill_diagonal(d2, 1 << 40)
        assert (d2 >= md * md).all()


def test_spacing_on_real_candidates_equals_opencv_grid(stills_roi):
    keys = G.candidate_keys(G.min_eig_response(stills_roi, 3), 0.01)
    xy = G.keys_xy(keys, stills_roi.shape[1])
    for md in (1, 2.5, 10, 30):
        assert np.array_equal(G.spread_greedy(xy, md, 1000), G.spread_grid(xy, stills_roi.shape[1], stills_roi.shape[0], md, 1000)), md


@pytest.mark.parametrize("block", [3, 5, 7])
def test_min_eigenvalue_agrees_with_a_float64_solve(block, stills_roi):
    for img in (_synthetic(), stills_roi):
        r = G.min_eig_response(img, block).astype(np.float64)
        sxx, sxy, syy = G.structure_sums(img, block)
        s2 = float(G._s2(block))
        A = np.stack([np.stack([sxx, sxy], -1), np.stack([sxy, syy], -1)], -2).astype(np.float64) * s2
        ev = np.linalg.eigvalsh(A)
        lo, hi = ev[..., 0], ev[..., 1]
        ok = lo > 0.1 * hi  # little cancellation in (a + c) - sqrt(...): float32 rounding stays within a few ulp of the result
        assert ok.sum() > 100
        np.testing.assert_allclose(r[ok], lo[ok], rtol=1e-5)


def test_mask_sets_the_maximum_and_filters_candidates(stills_roi):
    resp = G.min_eig_response(stills_roi, 3)
    h, w = resp.shape
    y, x = np.unravel_index(np.argmax(resp), resp.shape)
    mask = np.ones((h, w), np.uint8)
    mask[max(y - 20, 0):y + 21, max(x - 20, 0):x + 21] = 0
    keys = G.candidate_keys(resp, 0.05, mask)
    xy = G.keys_xy(keys, w)
    assert len(xy) > len(G.candidate_keys(resp, 0.05)) and (mask[xy[:, 1], xy[:, 0]] != 0).all()
    assert len(G.candidate_keys(resp, 0.05, np.zeros((h, w), np.uint8))) == 0


def test_new_symbols_are_declared_and_exported():
    from velocity_amd import _lib

    L = _lib.load()
    assert L.vh_version() >= 107
    for s in ("vh_good_features2", "vh_frame0_init_batch2"):
        assert s in _lib.declared_symbols() and s in _lib._SIGS and hasattr(L, s)


def test_good_features_op_is_registered_and_refuses_cpu_tensors():
    import velocity_amd.torch_ops  # noqa: F401

    op = torch.ops.velocity_hip.good_features
    sch = str(op.default._schema)
    assert "min_distance" in sch and "mask" in sch and "use_harris" in sch
    assert "min_distance" in str(torch.ops.velocity_hip.frame0_init.default._schema)
    with pytest.raises((RuntimeError, NotImplementedError)):
        op(torch.zeros((64, 64), dtype=torch.uint8), 10, 0.01, 5.0)


def test_shim_signature_takes_a_mask():
    import inspect

    from velocity_amd import images

    ps = inspect.signature(images.goodFeaturesToTrack).parameters
    assert list(ps)[:7] == ["image", "maxCorners", "qualityLevel", "minDistance", "blockSize", "useHarrisDetector", "k"]
    assert ps["mask"].kind is inspect.Parameter.KEYWORD_ONLY and ps["useHarrisDetector"].default is True
