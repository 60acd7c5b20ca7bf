"""What the recovery by feature matching costs: one vh_match_affine call (HIP events around the launch sequence, warmed up, median of --reps) on
  stills A frame 0 -> 1 (1024 x 768, the frame-0 tracks of the drop-in loop: the pair on which KLTmain loses every track), and
  a synthetic 1920 x 1080 pair shifted by 200 px with 2000 grid tracks,
next to what it buys: a KLTmain call on the same frames through the drop-in route (host clock, upload and read-back included, as a caller sees it),
without and with fallback=True.

    python tools/exp/match_timing.py --out profiles/fallback/r09_match.json
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/exp/match_timing.py --profile      (the per-kernel split)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from velocity_amd import KLT, synth  # noqa: E402
from velocity_amd import _lib as L  # noqa: E402


def cases():
    from tools.dropin_loop import DropinLoop

    st = np.load(os.path.join(ROOT, "tests", "golden", "stills_gray.npz"))
    fr = st["a_frames"]
    loop = DropinLoop(st["a_K"], 2, roi_border=(233, 167))
    loop.first(fr[0], st["a_q"], 0.0, 0)
    yield "stills_a_1024x768", fr[0], fr[1], loop.pts.astype(np.float32)
    W, H = 1920, 1080
    m = synth.AffineMotion(W, H, s=1.0, theta_deg=0, tx=200, ty=0)
    yield "synthetic_1920x1080_shift200", synth.render_frame(W, H, m, 0).numpy(), synth.render_frame(W, H, m, 1).numpy(), synth.grid_tracks(2000, W, H, frac=0.5)


def stats(ms):
    ms = sorted(ms)
    return dict(median_ms=float(np.median(ms)), min_ms=ms[0], max_ms=ms[-1], reps=len(ms))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--profile", action="store_true", help="only the matching calls (for rocprofv3)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch = L.torch_cuda()
    rows = []
    for name, f0, f1, p0 in cases():
        d0, d1, dp = torch.from_numpy(f0).cuda(), torch.from_numpy(f1).cuda(), torch.from_numpy(p0).cuda()
        for _ in range(a.warmup):
            out = KLT._match_call(d0, d1, dp, None)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = KLT._match_call(d0, d1, dp, None)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        info = out[3].cpu().numpy()
        row = dict(case=name, width=int(f0.shape[1]), height=int(f0.shape[0]), tracks=int(len(p0)), info=[int(x) for x in info], match_affine=stats(ms))
        if not a.profile:
            import contextlib
            import io

            for key, kw in (("kltmain_dropin", {}), ("kltmain_dropin_fallback", dict(fallback=True))):
                wall = []
                with contextlib.redirect_stdout(io.StringIO()):
                    for k in range(a.warmup + a.reps):
                        t = time.perf_counter()
                        p, v, _ = KLT.KLTmain(f1, f0, None, p0, **kw)
                        if k >= a.warmup:
                            wall.append(1e3 * (time.perf_counter() - t))
                row[key] = dict(stats(wall), tracks_kept=int(v.sum()))
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out and not a.profile:
        res = dict(what="one vh_match_affine call (HIP events, device only) and KLTmain through the drop-in route on the same frames (host clock), default parameters",
                   build_id=L.build_info()["build_id"], device=torch.cuda.get_device_name(0), params=dict(L.MATCH_DEFAULTS), rows=rows)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
