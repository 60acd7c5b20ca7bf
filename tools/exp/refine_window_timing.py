"""What refining in windows costs beside the whole-clip refinement, on one MI355X.  The load of tools/exp/refine_timing.py: 64 synthetic clips of 20
frames at 1920 x 1080, 1000 corners, roi_border (700, 500), frames resident as CUDA tensors.

  run_sequences legs (all 64 clips):  (i) no refinement;  (ii) refine="ba", the whole clip;  (iii) refine="ba", refine_window=8, default stride
  (3 windows per clip: starts 0, 7, 12).  For (ii) and (iii) also the refine requests alone, by HIP events recorded on each session's stream around
  TrackerSession.refine / refine_windows (the sessions run side by side: the figure is the longest of them per run).
  run_queue leg (64 clips of 8 .. 32 frames, 16 resident streams):  (iv) whole-clip mode, one TrackerSession.refine per clip length among the clips
  that finish at a step;  (v) refine_window=8, one TrackerSession.refine_windows request per session and step.  Requests are counted.

Host clock around runs that end in a device synchronise, median of --reps runs after one warm-up; no figure is fixed in advance.

    python tools/exp/refine_window_timing.py --out profiles/refine_windows/timing.json
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

BORDER, MC, SIZE = (700, 500), 1000, (1920, 1080)


def plate_quad(b, K):
    rng = np.random.default_rng(1000 + b)
    X, Y, Z = rng.uniform(-0.6, 0.6), rng.uniform(-0.3, 0.3), rng.uniform(3.5, 5.0)
    P = worldPointsLicensePlate("Chile").astype(np.float64) + np.array([X, Y, Z])
    uvw = P @ K.astype(np.float64)
    return (uvw[:, :2] / uvw[:, 2:]).astype(np.float32)


def make_clip(b, n):
    W, H = SIZE
    K = synth.K_1080P.copy()
    m = synth.AffineMotion(W, H, s=0.999, theta_deg=0.02, tx=2.0 + 0.01 * b, ty=-0.5)
    fr = [synth.render_frame(W, H, m, k, seed=0xC0FFEE + 7919 * b, device="cuda").contiguous() for k in range(n)]
    return dict(frames=fr, q=plate_quad(b, K), times=np.arange(n, dtype=np.float32) / 30.0, K=K, name=f"clip {b}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--streams", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch = L.torch_cuda()
    longest = 32
    lengths = [int(n) for n in np.random.default_rng(5).integers(a.window, longest + 1, a.clips)]
    full = [make_clip(b, max(a.frames, lengths[b])) for b in range(a.clips)]
    clips = [dict(c, frames=c["frames"][: a.frames], times=c["times"][: a.frames]) for c in full]
    qclips = [dict(c, frames=c["frames"][:n], times=c["times"][:n]) for c, n in zip(full, lengths)]
    torch.cuda.synchronize()
    K0 = synth.K_1080P.copy()
    kw = dict(roi_border=BORDER, max_corners=MC)

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
    last = {}
    qkw = dict(streams=a.streams, max_frames=longest, max_size=(SIZE[1], SIZE[0]), **kw)
    legs = {"i_run_sequences": lambda: D.run_sequences(clips, K0, **kw),
            "ii_run_sequences_refine_ba_whole_clip": lambda: D.run_sequences(clips, K0, refine="ba", **kw),
            "iii_run_sequences_refine_window": lambda: D.run_sequences(clips, K0, refine="ba", refine_window=a.window, **kw),
            "iv_run_queue_whole_clip_per_length": lambda: D.run_queue(qclips, K0, refine="ba", **qkw),
            "v_run_queue_refine_window": lambda: D.run_queue(qclips, K0, refine="ba", refine_window=a.window, **qkw)}
    rows = {}
    for name, fn in legs.items():
        last[name] = fn()  # warm-up: allocations, first launches
        torch.cuda.synchronize()
        del calls[:]
        secs, req_ms, req_n = [], [], []
        for _ in range(a.reps):
            t = time.perf_counter()
            last[name] = fn()
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t)
            per = {}
            for e0, e1, who in calls:
                per[who] = per.get(who, 0.0) + e0.elapsed_time(e1)
            req_ms.append(sorted(per.values()))
            req_n.append(len(calls))
            del calls[:]
        rows[name] = dict(seconds=secs, seconds_median=float(np.median(secs)), seconds_min=float(min(secs)), seconds_max=float(max(secs)), reps=a.reps,
                          refine_requests=req_n[-1], refine_ms_per_session_and_run=req_ms,
                          refine_ms_longest_session_median=float(np.median([max(r) for r in req_ms])) if req_ms[0] else None)
        print(name, json.dumps(rows[name]), flush=True)
    whole = [r["ba"] for r in last["ii_run_sequences_refine_ba_whole_clip"]]
    wins = [r["ba"] for r in last["iii_run_sequences_refine_window"]]
    qwhole = [r["ba"] for r in last["iv_run_queue_whole_clip_per_length"]]
    qwins = [r["ba"] for r in last["v_run_queue_refine_window"]]

    def stats(v):
        v = np.asarray(v, np.float64)
        return dict(min=float(v.min()), median=float(np.median(v)), max=float(v.max()))

    t = {k: rows[k]["seconds_median"] for k in rows}
    out = dict(what=f"{a.clips} clips at {SIZE[0]} x {SIZE[1]}, {MC} corners, frames resident as CUDA tensors. run_sequences on {a.frames} frames each: no refinement (i), "
                    f"refine='ba' on the whole clip (ii), refine_window={a.window} with the default stride (iii). run_queue on clips of {a.window}..{longest} frames over "
                    f"{a.streams} streams: whole-clip mode, one refine per clip length and step (iv), refine_window={a.window}, one request per session and step (v). "
                    "Host clock around runs that end in a device synchronise, median of the runs after one warm-up; the refine requests alone by HIP events",
               build_id=L.build_info()["build_id"], device=torch.cuda.get_device_name(0), clips=a.clips, frames=a.frames, window=a.window,
               queue_lengths=lengths, rows=rows,
               windows_per_clip=len(D.refine_window_starts(a.frames, a.window)),
               tracks_whole_clip=stats([b["nt"] for b in whole]), tracks_per_window=stats(np.concatenate([b["nt"] for b in wins])),
               tracks_per_window_over_whole_clip=stats(np.concatenate([b["nt"] / max(w["nt"], 1) for b, w in zip(wins, whole)])),
               iterations_whole_clip=sorted({int(b["iterations"]) for b in whole}), iterations_windows=sorted({int(i) for b in wins for i in b["iterations"]}),
               speed_mean_whole_clip=stats([b["speed_mean"] for b in whole]), speed_mean_windows=stats([b["speed_mean"] for b in wins]),
               queue_tracks_whole_clip=stats([b["nt"] for b in qwhole]), queue_tracks_per_window=stats(np.concatenate([b["nt"] for b in qwins])),
               queue_windows_per_clip=stats([len(b["first"]) for b in qwins]),
               time_ii_over_i=t["ii_run_sequences_refine_ba_whole_clip"] / t["i_run_sequences"], time_iii_over_i=t["iii_run_sequences_refine_window"] / t["i_run_sequences"],
               time_v_over_iv=t["v_run_queue_refine_window"] / t["iv_run_queue_whole_clip_per_length"])
    print(json.dumps({k: out[k] for k in out if k not in ("rows", "what", "queue_lengths")}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
