"""What replacing lost tracks costs a frame step and what it keeps alive, on one MI355X.  Load: 64 clips of 40 frames at 1920 x 1080 on synth.HardScene
(8 distinct seeds; clip b shows seed b % 8 from phase 5 (b // 8)), 1000 corners, roi_border (700, 500), frames resident as CUDA tensors.

  legs:  run_sequences without the option and with Replenish() (every 5, baseline 5, 256 new corners at most) and 512 spare rows, alternating: the
         run by a host clock around a call that ends in a device synchronise, and the tracks alive at the last frame.
  steps: ONE TrackerSession of 64 streams stepped by hand, HIP events around every step: the step time on birth frames, promotion frames, frames that
         are both and plain frames, with the option on, beside the same frames with it off.

Median of --reps runs after one warm-up per leg; no figure is fixed in advance.

    python tools/exp/replenish_timing.py --out profiles/replenish/timing.json
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

BORDER, MC, SIZE, MSV = (700, 500), 1000, (1920, 1080), 5


def plate_quad(b, K):
    rng = np.random.default_rng(1000 + b)
    X, Y, Z = rng.uniform(-0.6, 0.6), rng.uniform(-0.3, 0.3), rng.uniform(3.5, 5.0)
    P = worldPointsLicensePlate("Chile").astype(np.float64) + np.array([X, Y, Z])
    uvw = P @ K.astype(np.float64)
    return (uvw[:, :2] / uvw[:, 2:]).astype(np.float32)


def kind_of(f, rep, n):
    birth = f > MSV and (f - MSV) % rep.every == 0 and f + rep.baseline < n
    g = f - rep.baseline
    promo = g > MSV and (g - MSV) % rep.every == 0
    return "both" if birth and promo else "birth" if birth else "promotion" if promo else "plain"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--spare", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch = L.torch_cuda()
    W, H = SIZE
    K = synth.K_1080P.copy()
    n, rep = a.frames, D.Replenish()
    scene = synth.HardScene(K, W, H)
    rendered = {}

    def frame(seed, k):
        if (seed, k) not in rendered:
            rendered[(seed, k)] = scene.frame(k, seed=0xC0FFEE + 7919 * seed, device="cuda").contiguous()
        return rendered[(seed, k)]

    clips = [dict(frames=[frame(b % 8, 5 * (b // 8) + k) for k in range(n)], q=plate_quad(b, K), times=np.arange(n, dtype=np.float32) / 30.0, K=K, name=f"clip {b}")
             for b in range(a.clips)]
    torch.cuda.synchronize()
    kw = dict(roi_border=BORDER, max_corners=MC, msv_frame=MSV)
    legs = {"off": {}, "on": dict(replenish=rep, spare=a.spare)}
    runs = {k: [] for k in legs}
    alive, summary = {}, {}
    for r in range(a.reps + 1):  # (round 0: the warm-up of both legs)
        for name, extra in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = D.run_sequences(clips, K, **kw, **extra)
            torch.cuda.synchronize()
            if r:
                runs[name].append(time.perf_counter() - t0)
            alive[name] = [int(x["S"][-1, 2]) for x in res]
            if name == "on":
                summary = dict(born=int(sum(x["replenish"]["born"].sum() for x in res)), promoted=int(sum(x["replenish"]["promoted"].sum() for x in res)),
                               rejected=int(sum(x["replenish"]["rejected"].sum() for x in res)), rows_left_min=int(min(x["replenish"]["rows_left"] for x in res)),
                               tracks_frame0=[int(x["n_tracks0"]) for x in res])
    # one session of every stream, stepped by hand: the time of each step by events
    settings = D.Frame0Settings(roi_border=BORDER, max_corners=MC)
    steps = {}
    for name, extra in legs.items():
        per = {}
        for r in range(a.reps + 1):
            skw = dict(replenish=extra["replenish"], spare=extra["spare"], replenish_settings=settings) if extra else {}
            ses = D.TrackerSession(K, W, H, settings.cap, nhist=n, batch=a.clips, msv_frame=MSV, **skw)
            ses.admit([(b, c["frames"][0], c["q"], c["times"][0], 0) for b, c in enumerate(clips)], settings)
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
            for i in range(1, n):
                ev[i][0].record()
                ses.step([c["frames"][i] for c in clips], time_s=[float(c["times"][i]) for c in clips], frame_no=[float(i)] * a.clips)
                ev[i][1].record()
            torch.cuda.synchronize()
            if r:
                for i in range(1, n):
                    per.setdefault(kind_of(i, rep, n), []).append(ev[i][0].elapsed_time(ev[i][1]))
            del ses
        steps[name] = {k: dict(frames=len(v) // a.reps, median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v))) for k, v in sorted(per.items())}
    out = dict(load=dict(clips=a.clips, frames=n, size=list(SIZE), max_corners=MC, roi_border=list(BORDER), msv_frame=MSV, scene="synth.HardScene, 8 seeds", spare=a.spare,
                         replenish=dict(every=rep.every, baseline=rep.baseline, max_new=rep.max_new, min_distance=rep.min_distance, max_reproj=rep.max_reproj)),
               reps=a.reps, build=L.build_info()["build_id"],
               run_sequences_s={k: dict(median=float(np.median(v)), all=[float(x) for x in v]) for k, v in runs.items()},
               tracks_alive_last_frame={k: dict(mean=float(np.mean(v)), min=int(min(v)), max=int(max(v))) for k, v in alive.items()},
               tracks_frame0_mean=float(np.mean(summary["tracks_frame0"])), replenished=dict((k, v) for k, v in summary.items() if k != "tracks_frame0"),
               step_ms_by_frame_kind=steps,
               note="step times: HIP events around TrackerSession.step of ONE session of all the streams; a frame of the kind 'birth' / 'promotion' / 'both' with the option "
                    "off is the same frame index, for comparison")
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
