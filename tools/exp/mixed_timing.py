"""What it costs to keep two camera types in ONE session set instead of one set per type, on one MI355X.  64 synthetic clips of 20 frames, 1000 corners,
roi_border (700, 500), frames resident as CUDA tensors (synth.render_frame, one seed per clip): 32 at 1920 x 1080 with synth.K_1080P and 32 at 1280 x 720
with that K scaled by 2/3, each clip's plate quad projected through its own K.

  (i)   one run_sequences call on all 64: the sessions are created at 1920 x 1080 and every launch of a step is sized for it -- the surplus workgroups of
        a 720p stream leave at once;
  (ii)  two run_sequences calls, one per camera type, one after the other (what a deployment had to do while a session had one frame size);
  (iii) 64 clips, all at 1920 x 1080: the ceiling of (i).

For each: the median of --reps runs after a warm-up, each run ending in a device synchronise; tracked frames/s (a clip of n frames has n - 1).  The ratios
(i) / (ii) and (i) / (iii) are of the medians; `mixed_slower_than_split_by_more_than_3_spreads` states the README's rule: (i) slower than (ii) by more than
three times the spread (max - min) of (ii)'s runs.

    python tools/exp/mixed_timing.py --out profiles/mixed_cameras/timing.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from velocity_amd import _lib as L  # noqa: E402
from velocity_amd import driver as D  # noqa: E402
from velocity_amd import synth  # noqa: E402
from velocity_amd.common import worldPointsLicensePlate  # noqa: E402

BORDER, MC = (700, 500), 1000
BIG, SMALL = (1920, 1080), (1280, 720)


def camera(size):
    K = synth.K_1080P.copy()
    s = size[0] / 1920.0
    K[0, 0] *= s
    K[1, 1] *= s
    K[2, 0] *= s
    K[2, 1] *= s
    return K


def plate_quad(b, K):
    rng = np.random.default_rng(1000 + b)
    X, Y, Z = rng.uniform(-0.6, 0.6), rng.uniform(-0.3, 0.3), rng.uniform(3.5, 5.0)
    P = worldPointsLicensePlate("Chile").astype(np.float64) + np.array([X, Y, Z])
    uvw = P @ K.astype(np.float64)
    return (uvw[:, :2] / uvw[:, 2:]).astype(np.float32)


def make_clip(b, size, n):
    W, H = size
    K = camera(size)
    m = synth.AffineMotion(W, H, s=0.999, theta_deg=0.02, tx=(2.0 + 0.01 * b) * W / 1920.0, ty=-0.5 * W / 1920.0)
    fr = [synth.render_frame(W, H, m, k, seed=0xC0FFEE + 7919 * b, device="cuda").contiguous() for k in range(n)]
    return dict(frames=fr, q=plate_quad(b, K), times=np.arange(n, dtype=np.float32) / 30.0, K=K, name=f"clip {b} {W} x {H}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clips", type=int, default=64, help="clips in all (half per camera type)")
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch = L.torch_cuda()
    half = a.clips // 2
    big = [make_clip(b, BIG, a.frames) for b in range(a.clips)]          # (iii) uses all of them, (i) and (ii) the first half
    small = [make_clip(half + b, SMALL, a.frames) for b in range(half)]
    torch.cuda.synchronize()
    K0 = camera(BIG)
    kw = dict(roi_border=BORDER, max_corners=MC)
    mixed = [c for pair in zip(big[:half], small) for c in pair]         # the camera types alternate over the slots
    legs = {"i_one_call_mixed": lambda: D.run_sequences(mixed, K0, **kw),
            "ii_one_call_per_camera_type": lambda: (D.run_sequences(big[:half], K0, **kw), D.run_sequences(small, K0, **kw)),
            "iii_all_1080p": lambda: D.run_sequences(big, K0, **kw)}
    tracked = a.clips * (a.frames - 1)
    rows = {}
    for name, fn in legs.items():
        fn()  # warm-up: allocations, first launches
        torch.cuda.synchronize()
        secs = []
        for _ in range(a.reps):
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t)
        s = float(np.median(secs))
        rows[name] = dict(seconds=secs, seconds_median=s, seconds_min=float(min(secs)), seconds_max=float(max(secs)), reps=a.reps,
                          tracked_frames=tracked, tracked_frames_per_s=tracked / s, sessions=D.run_sequences.last_stats["sessions"])
        print(name, json.dumps(rows[name]), flush=True)
    t1, t2, t3 = (rows[k]["seconds_median"] for k in legs)
    spread2 = rows["ii_one_call_per_camera_type"]["seconds_max"] - rows["ii_one_call_per_camera_type"]["seconds_min"]
    out = dict(what=f"{a.clips} clips of {a.frames} frames, {MC} corners, frames resident as CUDA tensors; half at 1920 x 1080, half at 1280 x 720, each with its "
                    "own K: one run_sequences call on all (i) vs one call per camera type (ii) vs all clips at 1080p (iii); host clock around runs that end in "
                    "a device synchronise, median of the runs after one warm-up",
               build_id=L.build_info()["build_id"], device=torch.cuda.get_device_name(0), clips=a.clips, frames=a.frames, rows=rows,
               time_i_over_ii=t1 / t2, time_i_over_iii=t1 / t3, spread_of_ii_seconds=spread2,
               mixed_slower_than_split_by_more_than_3_spreads=bool(t1 - t2 > 3 * spread2))
    print(json.dumps({k: out[k] for k in ("time_i_over_ii", "time_i_over_iii", "spread_of_ii_seconds", "mixed_slower_than_split_by_more_than_3_spreads")}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
