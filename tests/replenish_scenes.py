"""The scenes of tests/test_replenish_cpu.py and tests/test_gpu_replenish.py: a textured plane that slides out of a 640 x 360 frame, so that a clip
loses a good part of its frame-0 tracks, with the settings the issue fixes for the small shapes (nhist 16, MSV frame 3, a birth every 2 frames,
baseline 3).  test_replenish_cpu.py asserts on these very scenes that no newborn's gate and no prefix cut is a near-tie, which is what lets the GPU
comparison run without exclusions."""
import functools

import numpy as np

import gftt_ref as G
import scenes as S
from oracle import klt_oracle as KO
from velocity_amd import synth
from velocity_amd.driver import Frame0Settings, Replenish

W, H = 640, 360
NHIST, MSV_FRAME = 16, 3
T0 = np.float32([1.5, 0.45, 3.6])
DET = Frame0Settings(max_corners=124, quality=0.01, block=5, harris_k=0.04, subpix=(5, 100, 0.001), use_harris=True, min_distance=10.0)
REP = Replenish(every=2, baseline=3, target=None, max_new=64, min_distance=10.0, border=(0, 0), max_reproj=1.0)
SPARE = 64


def camera(w=W, h=H, f=700.0):
    return S.camera(w, h, f)


def motion(K, dx=0.085, dy=0.004, dz=0.02):
    """Metres per frame: at z0 = 3.6 m and f = 700 the plane slides about 16 pixels per frame to the right."""
    return synth.PlaneMotion(K, z0=3.6, traj=lambda k: np.array([dx * k, dy * k, dz * k]))


@functools.lru_cache(maxsize=None)
def scene(seed=777, w=W, h=H, n0=128, nframes=NHIST, dx=0.085):
    """-> dict(frames, p, p3, vp, K, motion): frame-0 tracks are real corners of frame 0 (at most n0, 10 pixels apart, sub-pixel refined), their world
    points the analytic plane points."""
    K = camera(w, h)
    m = motion(K, dx=dx)
    frames = [synth.render_frame(w, h, m, k, seed=seed).numpy() for k in range(nframes)]
    c = G.good_features(frames[0], n0, DET.quality, DET.min_distance, None, DET.block, DET.use_harris, DET.harris_k)
    p = KO.corner_subpix(frames[0], c, *DET.subpix)
    p3 = m.world_points(p)
    vp = (p[:, 0] > w * 0.3) & (p[:, 0] < w * 0.7) & (p[:, 1] > h * 0.3) & (p[:, 1] < h * 0.7)
    return dict(frames=frames, p=p, p3=p3, vp=vp, K=K, motion=m)


# a gate strict enough to reject some of the scene's newborns (their errors lie between 0.003 and 0.025 pixels: the scene is noise-free)
REP_STRICT = Replenish(every=2, baseline=3, target=None, max_new=64, min_distance=10.0, border=(0, 0), max_reproj=0.0125)


@functools.lru_cache(maxsize=None)
def plate_clip(seed=2024, n=12):
    """A clip for the drivers: the same sliding plane with a licence plate clicked right of the centre of frame 0 (the ROI around it reaches the right
    edge, where the plane slides out), so that frame 0 goes through admit() and the clip has lost tracks by its first birth frame."""
    K = camera()
    m = motion(K)
    frames = np.stack([synth.render_frame(W, H, m, k, seed=seed).numpy() for k in range(n)])
    return dict(frames=frames, q=S.plate_quad(K, 0.2, 0.1, 3.6), times=np.arange(n, dtype=np.float32) / np.float32(25.0), name="sliding plane", K=K)
