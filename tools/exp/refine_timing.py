"""What refine="ba" costs, and what it saves against the route a user had before it, on one MI355X.  64 synthetic clips of 20 frames at 1920 x 1080,
1000 corners, roi_border (700, 500), frames resident as CUDA tensors (the clips of tools/exp/mixed_timing.py's leg iii).

  (i)   run_sequences on all 64 clips, as ever;
  (ii)  the same call with refine="ba": after the last frame every session refines its clips in ONE TrackerSession.refine (pack, one BA launch sequence
        over windows of different track counts, unpack, one copy);
  (iii) the refine calls of (ii) alone, by HIP events recorded on each session's stream around the call (the sessions run side by side: the figure is
        the longest of them per run);
  (iv)  the 64 clips of (i) refined one at a time from the host arrays its results hold: NLS.fcnNLS_batch(K, P, p3, B[:, 3:6]) per clip -- track filter
        and packing in NumPy, upload, one vh_nls_batch, download.

(i), (ii) and (iv): host clock around runs that end in a device synchronise, median of --reps runs after one warm-up.

    python tools/exp/refine_timing.py --out profiles/refine/timing.json
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from velocity_amd import NLS  # noqa: E402
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch = L.torch_cuda()
    clips = [make_clip(b, a.frames) for b in range(a.clips)]
    torch.cuda.synchronize()
    K0 = synth.K_1080P.copy()
    kw = dict(roi_border=BORDER, max_corners=MC)

    # (iii): events around every TrackerSession.refine of a run, on the stream the call is issued on
    calls, inner = [], D.TrackerSession.refine

    def timed_refine(self, slots, *args, **kwargs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        h = inner(self, slots, *args, **kwargs)
        e1.record()
        calls.append((e0, e1, len(slots)))
        return h

    D.TrackerSession.refine = timed_refine
    last = {}

    def one_at_a_time():
        with contextlib.redirect_stdout(io.StringIO()):  # fcnNLS_batch prints its trace like the reference
            for r in last["plain"]:
                NLS.fcnNLS_batch(K0, r["P"], r["p3"], r["B"][:, 3:6])

    legs = {"i_run_sequences": lambda: last.__setitem__("plain", D.run_sequences(clips, K0, **kw)),
            "ii_run_sequences_refine_ba": lambda: last.__setitem__("ba", D.run_sequences(clips, K0, refine="ba", **kw)),
            "iv_one_vh_nls_batch_per_clip_from_host_arrays": one_at_a_time}
    rows, refine_ms = {}, []
    for name, fn in legs.items():
        fn()  # warm-up: allocations, first launches
        torch.cuda.synchronize()
        del calls[:]
        secs = []
        for _ in range(a.reps):
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t)
            if calls:
                refine_ms.append([e0.elapsed_time(e1) for e0, e1, _ in calls])
                del calls[:]
        s = float(np.median(secs))
        rows[name] = dict(seconds=secs, seconds_median=s, seconds_min=float(min(secs)), seconds_max=float(max(secs)), reps=a.reps)
        print(name, json.dumps(rows[name]), flush=True)
    ba = [r["ba"] for r in last["ba"]]
    longest = [max(run) for run in refine_ms]
    rows["iii_refine_calls_alone"] = dict(ms_per_session_and_run=refine_ms, ms_longest_session_median=float(np.median(longest)), sessions=len(refine_ms[0]))
    t1, t2, t4 = (rows[k]["seconds_median"] for k in legs)
    t3 = rows["iii_refine_calls_alone"]["ms_longest_session_median"] / 1e3
    out = dict(what=f"{a.clips} clips of {a.frames} frames at {SIZE[0]} x {SIZE[1]}, {MC} corners, frames resident as CUDA tensors: run_sequences without (i) and with "
                    "(ii) refine='ba', the refine calls alone by HIP events (iii), and the same clips refined one vh_nls_batch at a time from the exported "
                    "host arrays (iv); host clock around runs that end in a device synchronise, median of the runs after one warm-up",
               build_id=L.build_info()["build_id"], device=torch.cuda.get_device_name(0), clips=a.clips, frames=a.frames, rows=rows,
               tracks_per_clip=dict(min=int(min(b["nt"] for b in ba)), median=float(np.median([b["nt"] for b in ba])), max=int(max(b["nt"] for b in ba))),
               iterations=sorted({int(b["iterations"]) for b in ba}),
               time_ii_over_i=t2 / t1, refine_share_of_ii=t3 / t2, time_iv_over_iii=t4 / t3, seconds_ii_minus_i=t2 - t1)
    print(json.dumps({k: out[k] for k in ("time_ii_over_i", "refine_share_of_ii", "time_iv_over_iii", "seconds_ii_minus_i", "tracks_per_clip", "iterations")}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
