"""What a refinement with partial tracks (refine_min_obs) costs and buys, on one MI355X.  Load: the replenish bullet's -- 64 clips of 40 frames at
1920 x 1080 on synth.HardScene (8 seeds), 1000 corners, Replenish() with 512 spare rows: where tracks die and are born.

The clips are tracked ONCE into a session of 64 streams; then the refinement requests alone are timed on that session (HIP events around
TrackerSession.refine_windows, records copied to pinned memory included), legs alternating, medians of --reps after one warm-up round:
  whole clip (one window of 40 frames per clip) and refine_window = 8 (6 windows per clip), each
    without the option | with min_obs = 3 | with min_obs = 3 and start_reproj = 1.0
Recorded per leg: tracks per window, partial tracks, triangulated and rejected starts, observed measurement pairs, iterations.

    python tools/exp/refine_partial_timing.py --out profiles/refine_partial/timing.json
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from velocity_amd import _lib as L  # noqa: E402
from velocity_amd import driver as D  # noqa: E402
from velocity_amd import synth  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from replenish_timing import BORDER, MC, MSV, SIZE, plate_quad  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--spare", type=int, default=512)
    ap.add_argument("--window", type=int, default=8)
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

    clips = [dict(frames=[frame(b % 8, 5 * (b // 8) + k) for k in range(n)], q=plate_quad(b, K), times=np.arange(n, dtype=np.float32) / 30.0) for b in range(a.clips)]
    settings = D.Frame0Settings(roi_border=BORDER, max_corners=MC)
    ses = D.TrackerSession(K, W, H, settings.cap, nhist=n, batch=a.clips, msv_frame=MSV, replenish=rep, spare=a.spare, replenish_settings=settings)
    ses.admit([(b, c["frames"][0], c["q"], c["times"][0], 0) for b, c in enumerate(clips)], settings)
    for i in range(1, n):
        ses.step([c["frames"][i] for c in clips], time_s=[float(c["times"][i]) for c in clips], frame_no=[float(i)] * a.clips)
    torch.cuda.synchronize()
    shapes = {"whole clip": (n, [(b, 0) for b in range(a.clips)]),
              f"windows of {a.window}": (a.window, [(b, f) for b in range(a.clips) for f in D.refine_window_starts(n, a.window)])}
    options = {"off": {}, "min_obs 3": dict(min_obs=3), "min_obs 3, start_reproj 1.0": dict(min_obs=3, start_reproj=1.0)}
    ms = {(s, o): [] for s in shapes for o in options}
    seen = {}
    for r in range(a.reps + 1):  # (round 0: the warm-up of every leg)
        for s, (nf, wins) in shapes.items():
            for o, kw in options.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                h = ses.refine_windows(wins, nf, **kw)
                e1.record()
                res = h.result()
                torch.cuda.synchronize()
                if r:
                    ms[s, o].append(e0.elapsed_time(e1))
                nt = np.array([w["nt"] for w in res])
                rec = dict(windows=len(res), nf=nf, tracks_per_window=dict(mean=float(nt.mean()), min=int(nt.min()), max=int(nt.max())),
                           iterations=dict(mean=float(np.mean([w["iterations"] for w in res])), max=int(max(w["iterations"] for w in res))),
                           converged=int(sum(w["converged"] for w in res)), speed_mean=float(np.mean([w["speed_mean"] for w in res])),
                           f_last_median=float(np.nanmedian([w["f_last"] for w in res])))
                if kw:
                    rec.update(partial_per_window=float(np.mean([w["npart"] for w in res])), triangulated_per_window=float(np.mean([w["ntri"] for w in res])),
                               rejected_per_window=float(np.mean([w["nrej"] for w in res])),
                               observed_fraction=float(sum(w["nobs"] for w in res) / max(1, sum(w["nt"] for w in res) * nf)))
                seen[s, o] = rec
    out = dict(load=dict(clips=a.clips, frames=n, size=list(SIZE), max_corners=MC, roi_border=list(BORDER), msv_frame=MSV, scene="synth.HardScene, 8 seeds", spare=a.spare,
                         rows=ses.n0, replenish=dict(every=rep.every, baseline=rep.baseline, max_new=rep.max_new)),
               reps=a.reps, build=L.build_info()["build_id"],
               legs={s: {o: dict(ms=dict(median=float(np.median(ms[s, o])), all=[float(x) for x in ms[s, o]]), **seen[s, o]) for o in options} for s in shapes},
               note="ms: HIP events around one TrackerSession.refine_windows request for all the clips (pack, one BA launch sequence, unpack, copy to pinned memory); "
                    "the solve is dense over the session's rows x nf, so a request's time follows the rows and the iterations, not the tracks it takes")
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
