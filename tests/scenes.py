"""The synthetic cameras, scenes and clips of the GPU tests, each defined once: a test module that needs one imports it from here, it keeps no copy.

Several of these scenes carry results of CPU studies (145 survivors of 150 in the refine streams, seed 439 of the anchor tests' free slot, the tracks
that die in the patch of the refine-windows stream), so a scene must not drift between the modules that share it.  The builders are cached: a scene
is rendered once per process.  Every variation is a parameter -- and so part of the cache key -- and the cached arrays are read-only: a test that
wants another scene asks for it or copies, it never writes into a shared one.  Frames go to the device through to_cuda(), which copies first."""
import functools
import os

import numpy as np
import pytest

from _helpers import frozen
from velocity_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T0 = frozen(np.float32([1.5, 0.45, 3.6]))[0]  # the start of the frame-0 pose fit


def to_cuda(a):
    """A (read-only) host array as a device tensor of the same values."""
    import torch

    return torch.from_numpy(np.array(a)).cuda()


def camera(W, H, f, c=None):
    """synth.K_1080P (row-vector layout) with focal length f and principal point c (default: the middle of a W x H frame)."""
    K = synth.K_1080P.copy()
    K[0, 0] = K[1, 1] = f
    K[2, 0], K[2, 1] = c if c is not None else (W / 2 + 0.5, H / 2 + 0.5)
    return K


def plate_quad(K, X, Y, Z):
    """worldPointsLicensePlate("Chile") at camera-frame offset (X, Y, Z) metres, projected through K (row-vector layout)."""
    from velocity_amd.common import worldPointsLicensePlate

    P = worldPointsLicensePlate("Chile").astype(np.float64) + np.array([X, Y, Z])
    uvw = P @ np.asarray(K, np.float64)
    return (uvw[:, :2] / uvw[:, 2:]).astype(np.float32)


def plate_world():
    """worldPointsLicensePlate("Chile") as the 12 float64 the frame-0 entry points take."""
    from velocity_amd.common import worldPointsLicensePlate

    return np.ascontiguousarray(np.asarray(worldPointsLicensePlate("Chile"), np.float64).reshape(12))


@functools.lru_cache(maxsize=None)
def plane_scene(W, H, n0, nframes, seed, f=700.0, c=None, traj=None, hopeless=37, p3_sigma=0.0, patch=None, patch_from=4):
    """-> (frames, p, p3, vp, K): a textured plane seen by camera(W, H, f, c) on the path traj (default: PlaneMotion's, which also recedes, so the
    tracks drift towards the principal point), n0 grid tracks with their analytic world points.  Every `hopeless`-th track (window far outside the
    frame) dies at once, so the masks and the compaction actually change.
    p3_sigma: the world points carry N(0, p3_sigma^2) metres of error, as points measured from a plate do.
    patch: the rectangle (x0, y0, x1, y1) of every frame from patch_from on is fresh noise, so the tracks inside fail the forward-backward gate there."""
    K = camera(W, H, f, c)
    m = synth.PlaneMotion(K, z0=3.6, traj=traj)
    frames = [synth.render_frame(W, H, m, k, seed=seed).numpy() for k in range(nframes)]
    if patch:
        x0, y0, x1, y1 = patch
        for k in range(patch_from, nframes):
            frames[k] = frames[k].copy()
            frames[k][y0:y1, x0:x1] = np.random.default_rng(seed * 1000 + k).integers(0, 256, (y1 - y0, x1 - x0), dtype=np.uint8)
    p = synth.grid_tracks(n0, W, H, seed=seed & 0xFF)
    p[::hopeless] = np.float32([-40.0, -40.0])
    p3 = m.world_points(p)
    if p3_sigma:
        p3 = p3 + np.random.default_rng(seed).normal(0.0, p3_sigma, (n0, 3))
    vp = (p[:, 0] > W * 0.3) & (p[:, 0] < W * 0.7) & (p[:, 1] > H * 0.3) & (p[:, 1] < H * 0.7)
    return (frozen(*frames),) + frozen(p, p3, vp, K)


@functools.lru_cache(maxsize=None)
def scenes3(n0=150, nhist=10, slot2_seed=433, p3_sigma=0.0, patch=None):
    """The three streams of two cameras of the refinement tests: 320 x 240 at f = 700, 256 x 192 at f = 560 and 320 x 240 again.  In these short clean
    clips only the hopeless tracks die (145 survivors of 150 in every stream with the recipe's 37), so the streams get different strides to keep
    different numbers of tracks.  patch: of the third stream (see plane_scene)."""
    return (plane_scene(320, 240, n0, nhist, 411, 700.0, p3_sigma=p3_sigma), plane_scene(256, 192, n0, nhist, 422, 560.0, hopeless=11, p3_sigma=p3_sigma),
            plane_scene(320, 240, n0, nhist, slot2_seed, 700.0, hopeless=7, p3_sigma=p3_sigma, patch=patch))


@functools.lru_cache(maxsize=None)
def _plate_clip(W, H, f, n, seed, plate_xy, traj):
    K = camera(W, H, f)
    m = synth.PlaneMotion(K, z0=3.6, traj=traj)
    frames = np.stack([synth.render_frame(W, H, m, k, seed=seed).numpy() for k in range(n)])
    return frozen(frames, plate_quad(K, plate_xy[0], plate_xy[1], 3.6), np.arange(n, dtype=np.float32) / np.float32(25.0), K)


def plate_clip(W, H, f, n, seed, name, plate_xy=(0.1, -0.05), traj=None):
    """A clip for the drivers: n frames of the plane of plane_scene at 25 frames per second, with the licence plate clicked at plate_xy metres
    beside the optical axis.  The dict is the caller's, its arrays are shared."""
    frames, q, times, K = _plate_clip(W, H, f, n, seed, plate_xy, traj)
    return dict(frames=frames, q=q, times=times, name=name, K=K)


@functools.lru_cache(maxsize=None)
def load_stills():
    return np.load(os.path.join(ROOT, "tests", "golden", "stills_gray.npz"))


@pytest.fixture(scope="module")
def stills():
    """The reference's stills (sequences a and b: frames, plate corners, intrinsics, times)."""
    return load_stills()
