"""What the frame-0 detector settings cost: one frame-0 batch call per session + vh_session_init_dev per clip (run_sequences' frame 0) on synthetic
1920 x 1080 clips (tools/exp/frame0_batch_timing.py's clips and sessions), roi_border (700, 500), 1000 corners, for four detector settings:
Harris md 0 (vh_frame0_init_batch, the reference's call), Shi-Tomasi md 0 / 10 / 30 (vh_frame0_init_batch2).  Warmed up, each repetition ends in a
device synchronise, the settings alternate; median / min / max, and the mean corners kept per clip.

    python tools/exp/gftt_timing.py --out profiles/frame0/r08_gftt.json
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/exp/gftt_timing.py --profile 256     (every setting once per rep)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from frame0_batch_timing import BORDER, MC, SUBPIX, H, W, Setup, make_clips, stats  # noqa: E402
from velocity_amd import _lib as L  # noqa: E402
from velocity_amd import driver as D  # noqa: E402

SETTINGS = (("harris_md0", True, 0.0), ("shi_tomasi_md0", False, 0.0), ("shi_tomasi_md10", False, 10.0), ("shi_tomasi_md30", False, 30.0))


def run(s, use_harris, md):
    """frame 0 of every clip: one batch call per session + vh_session_init_dev per clip, as run_sequences does it."""
    for g, mem in enumerate(s.members):
        ses = s.sess[g]
        bufs = s.bufs["b"][g]
        p, p3, vp, t0, R0, res0, n0 = bufs
        with s.torch.cuda.stream(s.streams[g]):
            D._frame0_batch_call(ses.lib, ses.ws, [s.clips[b]["frames"][0] for b in mem], [s.clips[b]["q"] for b in mem], W, H, ses.K64, s.plate, BORDER, MC,
                                 0.01, 5, 0.04, SUBPIX, bufs, use_harris, md)
            for j, b in enumerate(mem):
                L.check(ses.lib.vh_session_init_dev(ses.handle, j, L.dptr(s.clips[b]["frames"][0]), W, L.dptr(p[j]), L.dptr(p3[j]), L.dptr(vp[j]),
                                                    L.dptr(t0[j]), L.dptr(res0[j]), L.dptr(n0[j]), 0.0, 0.0, L.stream_ptr()), "vh_session_init_dev")
    s.torch.cuda.synchronize()


def corners_kept(s):
    return float(np.mean(np.concatenate([b[6].cpu().numpy() for b in s.bufs["b"]]) - 4))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 8, 64, 256])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--profile", type=int, default=0, help="only this many clips (for rocprofv3)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch = L.torch_cuda()
    if a.profile:
        s = Setup(make_clips(a.profile, frames=1))
        for _ in range(a.warmup + a.reps):
            for _, h, md in SETTINGS:
                run(s, h, md)
        print(f"profiled {a.warmup + a.reps} passes of {len(SETTINGS)} settings at {a.profile} clips")
        return
    rows = []
    for n in a.sizes:
        s = Setup(make_clips(n, frames=1))
        for _ in range(a.warmup):
            for _, h, md in SETTINGS:
                run(s, h, md)
        times = {name: [] for name, _, _ in SETTINGS}
        kept = {}
        for _ in range(a.reps):
            for name, h, md in SETTINGS:
                t = time.perf_counter()
                run(s, h, md)
                times[name].append(time.perf_counter() - t)
                kept[name] = corners_kept(s)
        row = dict(nclips=n, sessions=len(s.members))
        for name, _, _ in SETTINGS:
            row[name] = dict(stats(times[name]), corners_per_clip=kept[name])
        row["st_md10_over_harris_md0"] = row["shi_tomasi_md10"]["median_ms"] / row["harris_md0"]["median_ms"]
        print(json.dumps(row), flush=True)
        rows.append(row)
        del s
        torch.cuda.empty_cache()
    out = dict(what="frame 0 of nclips 1920x1080 clips (one batch call per session + vh_session_init_dev per clip) for four goodFeaturesToTrack settings, "
                    "host clock around work ending in a device synchronise",
               build_id=L.build_info()["build_id"], device=torch.cuda.get_device_name(0), roi_border=list(BORDER), max_corners=MC, rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
