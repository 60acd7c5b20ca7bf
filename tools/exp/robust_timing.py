"""What Huber weights cost a refine request, on one MI355X.  The load of tools/exp/anchor_timing.py: 64 synthetic clips of 20 frames at 1920 x 1080,
1000 corners, roi_border (700, 500), frames resident as CUDA tensors, run_sequences.

  legs:  refine="ba" on the whole clip and with refine_window=8 (3 windows per clip), each without and with refine_robust=1.0, alternating.
  Per leg the run (host clock around a run that ends in a device synchronise) and the refine requests alone, by HIP events recorded on each session's
  stream around TrackerSession.refine / refine_windows (the sessions run side by side: the figure is the longest of them per run).  Also the counts
  of down-weighted measurements, the iterations taken and the refined speeds, plain beside robust.

Median of --reps runs after one warm-up per leg; no figure is fixed in advance.  The ratio is stated next to the free leg's own spread.

    python tools/exp/robust_timing.py --out profiles/ba_robust/timing.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from anchor_timing import BORDER, MC, SIZE, make_clip  # noqa: E402  (the same clips)
from velocity_amd import _lib as L  # noqa: E402
from velocity_amd import driver as D  # noqa: E402
from velocity_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--delta", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch = L.torch_cuda()
    clips = [make_clip(b, a.frames) for b in range(a.clips)]
    torch.cuda.synchronize()
    K0 = synth.K_1080P.copy()
    kw = dict(roi_border=BORDER, max_corners=MC, refine="ba")
    calls = []

    def timed(inner):
        def call(self, items, *args, **kwargs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            h = inner(self, items, *args, **kwargs)
            e1.record()
            calls.append((e0, e1, id(self)))
            return h
        return call

    D.TrackerSession.refine = timed(D.TrackerSession.refine)
    D.TrackerSession.refine_windows = timed(D.TrackerSession.refine_windows)
    legs = {"whole_clip_plain": dict(), "whole_clip_robust": dict(refine_robust=a.delta),
            "window_plain": dict(refine_window=a.window), "window_robust": dict(refine_window=a.window, refine_robust=a.delta)}
    last, secs, req = {}, {k: [] for k in legs}, {k: [] for k in legs}
    for name, extra in legs.items():  # warm-up: allocations, first launches, graph capture
        last[name] = D.run_sequences(clips, K0, **kw, **extra)
        torch.cuda.synchronize()
    for _ in range(a.reps):  # the legs alternate, so drift of the box lands on all of them
        for name, extra in legs.items():
            del calls[:]
            t = time.perf_counter()
            last[name] = D.run_sequences(clips, K0, **kw, **extra)
            torch.cuda.synchronize()
            secs[name].append(time.perf_counter() - t)
            per = {}
            for e0, e1, who in calls:
                per[who] = per.get(who, 0.0) + e0.elapsed_time(e1)
            req[name].append(max(per.values()))

    def stats(v):
        v = np.asarray(v, np.float64)
        return dict(min=float(v.min()), median=float(np.median(v)), max=float(v.max()))

    rows = {k: dict(seconds=secs[k], seconds_median=float(np.median(secs[k])), refine_ms_longest_session=req[k], refine_ms_median=float(np.median(req[k])),
                    refine_ms_spread=float(max(req[k]) - min(req[k]))) for k in legs}
    ba = {k: [r["ba"] for r in last[k]] for k in legs}
    out = dict(what=f"{a.clips} clips of {a.frames} frames at {SIZE[0]} x {SIZE[1]}, {MC} corners, frames resident as CUDA tensors, run_sequences(refine='ba'): the whole "
                    f"clip and refine_window={a.window}, each without and with refine_robust={a.delta:g}, legs alternating, median of {a.reps} runs after one warm-up; "
                    "the refine requests alone by HIP events on each session's stream (the longest session per run)",
               build_id=L.build_info()["build_id"], device=torch.cuda.get_device_name(0), rows=rows,
               whole_clip_request_robust_over_plain=rows["whole_clip_robust"]["refine_ms_median"] / rows["whole_clip_plain"]["refine_ms_median"],
               whole_clip_plain_spread_over_median=rows["whole_clip_plain"]["refine_ms_spread"] / rows["whole_clip_plain"]["refine_ms_median"],
               window_request_robust_over_plain=rows["window_robust"]["refine_ms_median"] / rows["window_plain"]["refine_ms_median"],
               window_plain_spread_over_median=rows["window_plain"]["refine_ms_spread"] / rows["window_plain"]["refine_ms_median"],
               nout_first_whole_clip=stats([b["nout_first"] for b in ba["whole_clip_robust"]]), nout_last_whole_clip=stats([b["nout_last"] for b in ba["whole_clip_robust"]]),
               nout_last_per_window=stats(np.concatenate([b["nout_last"] for b in ba["window_robust"]])),
               tracks_whole_clip=stats([b["nt"] for b in ba["whole_clip_robust"]]),
               speed_mean={k: stats([b["speed_mean"] for b in ba[k]]) for k in legs},
               iterations={k: sorted({int(i) for b in ba[k] for i in np.atleast_1d(b["iterations"])}) for k in legs})
    print(json.dumps({k: out[k] for k in out if k != "what"}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
