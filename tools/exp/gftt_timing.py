"""What the frame-0 detector settings cost: one frame-0 batch call per session + vh_session_init_dev per clip (run_sequences' frame 0) on synthetic
1920 x 1080 clips (tools/exp/frame0_batch_timing.py's clips and sessions), roi_border (700, 500), 1000 corners, for four detector settings:
Harris md 0 (vh_frame0_init_batch, the reference's call), Shi-Tomasi md 0 / 10 / 30 (vh_frame0_init_batch2).  Warmed up, each repetition ends in a
device synchronise, the settings alternate; median / min / max, and the mean corners kept per clip.

    python tools/exp/gftt_timing.py --out profiles/frame0/r08_gftt.json
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/exp/gftt_timing.py --profile 256     (every setting once per rep)
"""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from frame0_batch_timing import BORDER, MC, SETTINGS as HARRIS_MD0, Setup, make_clips, stats  # noqa: E402
from velocity_amd import _lib as L  # noqa: E402

SETTINGS = (("harris_md0", HARRIS_MD0),) + tuple((f"shi_tomasi_md{md}", dataclasses.replace(HARRIS_MD0, use_harris=False, min_distance=float(md))) for md in (0, 10, 30))


def run(s, settings):
    """frame 0 of every clip: TrackerSession.admit per session (one batch call + vh_session_init_dev per clip), as run_sequences does it."""
    for ses, hs, mem in zip(s.sess, s.streams, s.members):
        with s.torch.cuda.stream(hs):
            ses.admit([(j, s.clips[b]["frames"][0], s.clips[b]["q"], 0.0, 0.0) for j, b in enumerate(mem)], settings)
    s.torch.cuda.synchronize()


def corners_kept(s):
    """Mean corners per clip of the last admission: the streams' track counts without the 4 plate corners."""
    return float(np.mean([ses._rd(ses.view(j).n_cur, 1, np.int32)[0] for ses in s.sess for j in range(ses.batch)]) - 4)


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
            for _, settings in SETTINGS:
                run(s, settings)
        print(f"profiled {a.warmup + a.reps} passes of {len(SETTINGS)} settings at {a.profile} clips")
        return
    rows = []
    for n in a.sizes:
        s = Setup(make_clips(n, frames=1))
        for _ in range(a.warmup):
            for _, settings in SETTINGS:
                run(s, settings)
        times = {name: [] for name, _ in SETTINGS}
        kept = {}
        for _ in range(a.reps):
            for name, settings in SETTINGS:
                t = time.perf_counter()
                run(s, settings)
                times[name].append(time.perf_counter() - t)
                kept[name] = corners_kept(s)
        row = dict(nclips=n, sessions=len(s.members))
        for name, _ in SETTINGS:
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
