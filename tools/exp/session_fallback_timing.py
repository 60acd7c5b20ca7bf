"""What the recovery by feature matching costs on the product route (TrackerSession(fallback=True)); HIP events or the host clock, warmed up, median of --reps.

  match     one vh_match_affine call on the two cases of tools/exp/match_timing.py (stills A at 1024 x 768; synthetic 1920 x 1080, 2000 tracks).  Run the same
            section from a checkout of the parent commit in the same job to compare the ten-pass detector with the one-pass one (the loader binds every
            declared symbol, so an older library cannot be loaded into this tree through VH_LIB).
  option    the price of the option on a clip that never fails: ms per frame step (host clock over a run of steps, one synchronisation at the end) with
            fallback=False and True, at 1 and 64 streams of 1920 x 1080 with 2000 tracks.
  failing   a failing step: stills A frame 1 through a one-stream session with the option on (host clock, the step and its synchronisation), next to the same
            step with the option off; and 8 failed pairs in one vh_match_affine_batch call against 8 vh_match_affine calls (HIP events).

    python tools/exp/session_fallback_timing.py --out profiles/fallback/r11_session.json
    python tools/exp/session_fallback_timing.py --only match                                  (also runs in the parent's checkout)
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/exp/session_fallback_timing.py --only failing --reps 5
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
from tools.exp.match_timing import cases, stats  # noqa: E402


def events(torch, fn, warmup, reps):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return stats(ms), out


def sec_match(torch, a):
    rows = []
    for name, f0, f1, p0 in cases():
        d0, d1, dp = torch.from_numpy(f0).cuda(), torch.from_numpy(f1).cuda(), torch.from_numpy(p0).cuda()
        st, out = events(torch, lambda: KLT._match_call(d0, d1, dp, None), a.warmup, a.reps)
        rows.append(dict(case=name, width=int(f0.shape[1]), height=int(f0.shape[0]), tracks=int(len(p0)), info=[int(x) for x in out[3].cpu().numpy()],
                         match_affine=st))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def sec_option(torch, a):
    from velocity_amd.driver import TrackerSession

    W, H, n0, steps = 1920, 1080, 2000, 12
    K = synth.K_1080P.copy()
    m = synth.PlaneMotion(K, z0=3.6)
    frames = [synth.render_frame(W, H, m, k, device="cuda").contiguous() for k in range(steps + 1)]
    p = synth.grid_tracks(n0, W, H)
    p3, vp, t0 = m.world_points(p), np.ones(n0, bool), np.float32([1.5, 0.45, 3.6])
    rows = []
    for streams in (1, 64):
        row = dict(streams=streams, width=W, height=H, tracks=n0, steps_per_run=steps)
        for fb in (False, True):
            ses = TrackerSession(K, W, H, n0, nhist=steps + 1, batch=streams, msv_frame=0, fallback=fb)
            runs = []
            for rep in range(a.warmup // 2 + 1 + a.reps // 3):
                for b in range(streams):
                    ses.init_stream(b, frames[0], p, p3, vp, t0)
                torch.cuda.synchronize()
                t = time.perf_counter()
                for i in range(1, steps + 1):
                    ses.step([frames[i]] * streams, time_s=i / 30.0, frame_no=i)
                torch.cuda.synchronize()
                if rep > a.warmup // 2:
                    runs.append(1e3 * (time.perf_counter() - t) / steps)
            row["fallback" if fb else "plain"] = dict(stats(runs), tracks_alive=int(ses.state(0)["n_cur"]), recoveries=ses.recoveries().sum(0).tolist())
            del ses
        row["extra_ms_per_step"] = row["fallback"]["median_ms"] - row["plain"]["median_ms"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def sec_failing(torch, a):
    from velocity_amd.driver import TrackerSession, frame0_batch

    st = np.load(os.path.join(ROOT, "tests", "golden", "stills_gray.npz"))
    fr, K = st["a_frames"], st["a_K"]
    f0 = frame0_batch([fr[0]], [st["a_q"]], K, roi_border=(233, 167))[0]
    n0 = len(f0["p"])
    H, W = fr[0].shape
    d = [torch.from_numpy(fr[k]).cuda() for k in (0, 1)]
    row = dict(case="stills_a_frame_1", width=W, height=H, tracks=n0)
    for fb in (False, True):
        ses = TrackerSession(K, W, H, n0, nhist=4, batch=1, msv_frame=0, fallback=fb)
        wall = []
        for rep in range(a.warmup + a.reps):
            ses.init_stream(0, d[0], f0["p"], f0["p3"], f0["vp"], f0["t"])
            torch.cuda.synchronize()
            t = time.perf_counter()
            ses.step([d[1]], time_s=1.0, frame_no=1)
            torch.cuda.synchronize()
            if rep >= a.warmup:
                wall.append(1e3 * (time.perf_counter() - t))
        s1 = ses.state(0)
        row["step_fallback" if fb else "step_plain"] = dict(stats(wall), tracks_alive=int(s1["n_cur"]), klt_flags=int(s1["klt_flags"]) & 7)
    print(json.dumps(row), flush=True)
    nb = 8
    dp = torch.from_numpy(f0["p"]).cuda()
    one, _ = events(torch, lambda: [KLT._match_call(d[0], d[1], dp, None) for _ in range(nb)], a.warmup, a.reps)
    many, out = events(torch, lambda: KLT._match_call_batch([d[0]] * nb, [d[1]] * nb, [dp] * nb, None), a.warmup, a.reps)
    row2 = dict(case="stills_a_8_failed_streams", pairs=nb, eight_single_calls=one, one_batch_call=many, info=out[3].cpu().numpy().tolist()[0])
    print(json.dumps(row2), flush=True)
    return [row, row2]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=("match", "option", "failing"), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch = L.torch_cuda()
    res = dict(what=__doc__.split("\n\n")[0], build_id=L.build_info()["build_id"], device=torch.cuda.get_device_name(0), params=dict(L.MATCH_DEFAULTS))
    for name, fn in (("match", sec_match), ("option", sec_option), ("failing", sec_failing)):
        if a.only in (None, name):
            res[name] = fn(torch, a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
