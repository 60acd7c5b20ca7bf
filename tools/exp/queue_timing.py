"""What a queue of clips of different lengths costs on a fixed set of resident streams: run_queue against what a user could do before it existed, on one
MI355X.  C2 size (1920 x 1080, 1000 corners, roi_border (700, 500)); 256 synthetic clips (synth.render_frame, one seed per clip, the plate quad of
tools/exp/frame0_batch_timing.py) whose lengths are a seeded uniform draw over 8..32.  Frames are CUDA tensors, so no upload blurs the figures.

  (a) run_queue with 64 streams;
  (b) run_sequences once per group of clips of equal length (what the driver offered for such a queue: every group is a lockstep batch of its own);
  (c) run_sequences on 256 clips of the mean length: the lockstep ideal, every stream busy at every step.

For each: clips/s and tracked frames/s (a clip of n frames has n - 1 tracked frames), median of --reps runs after a warm-up, each run ending in a device
synchronise; the device time spent in admissions (frame 0 + vh_session_init_dev, HIP events around them on the session's stream, summed over the
sessions) and its share of sessions x wall time; the mean number of idle slots per step.

    python tools/exp/queue_timing.py --out profiles/queue/queue_timing.json
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

W, H, BORDER, MC = 1920, 1080, (700, 500), 1000


def plate_quad(b):
    rng = np.random.default_rng(1000 + b)
    X, Y, Z = rng.uniform(-0.6, 0.6), rng.uniform(-0.3, 0.3), rng.uniform(3.5, 5.0)
    P = worldPointsLicensePlate("Chile").astype(np.float64) + np.array([X, Y, Z])
    uvw = P @ synth.K_1080P.astype(np.float64)
    return (uvw[:, :2] / uvw[:, 2:]).astype(np.float32)


def make_clips(lengths, least):
    """One clip per length; each is rendered to max(length, least) frames so that the lockstep leg can cut `least` frames out of every clip."""
    torch = L.torch_cuda()
    clips = []
    for b, n in enumerate(lengths):
        m = synth.AffineMotion(W, H, s=0.999, theta_deg=0.02, tx=2.0 + 0.01 * b, ty=-0.5)
        fr = [synth.render_frame(W, H, m, k, seed=0xC0FFEE + 7919 * b, device="cuda").contiguous() for k in range(max(n, least))]
        clips.append(dict(frames=fr, q=plate_quad(b), times=np.arange(len(fr), dtype=np.float32) / 30.0, n=n))
    torch.cuda.synchronize()
    return clips


def cut(c, n):
    return dict(frames=c["frames"][:n], q=c["q"], times=c["times"][:n])


def leg_queue(clips, streams):
    D.run_queue([cut(c, c["n"]) for c in clips], synth.K_1080P, streams=streams, roi_border=BORDER, max_corners=MC)
    st = D.run_queue.last_stats
    return dict(admission_ms=st["admission_ms"], sessions=st["sessions"], steps=st["steps"], idle=st["mean_idle_slots"])


def leg_groups(clips):
    by_len = {}
    for c in clips:
        by_len.setdefault(c["n"], []).append(cut(c, c["n"]))
    adm = ses_wall = 0.0
    steps = 0
    for n in sorted(by_len):
        t = time.perf_counter()
        D.run_sequences(by_len[n], synth.K_1080P, roi_border=BORDER, max_corners=MC)
        st = D.run_sequences.last_stats
        adm += st["admission_ms"]
        ses_wall += st["sessions"] * (time.perf_counter() - t)
        steps += st["steps"]
    return dict(admission_ms=adm, session_seconds=ses_wall, steps=steps, idle=0.0, groups=len(by_len))


def leg_lockstep(clips, n):
    D.run_sequences([cut(c, n) for c in clips], synth.K_1080P, roi_border=BORDER, max_corners=MC)
    st = D.run_sequences.last_stats
    return dict(admission_ms=st["admission_ms"], sessions=st["sessions"], steps=st["steps"], idle=0.0)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20240607)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch = L.torch_cuda()
    lengths = [int(n) for n in np.random.default_rng(a.seed).integers(8, 33, a.clips)]
    mean = int(round(float(np.mean(lengths))))
    clips = make_clips(lengths, mean)
    legs = {"a_run_queue": (lambda: leg_queue(clips, a.streams), sum(lengths) - len(lengths)),
            "b_run_sequences_per_length": (lambda: leg_groups(clips), sum(lengths) - len(lengths)),
            "c_lockstep_mean_length": (lambda: leg_lockstep(clips, mean), len(lengths) * (mean - 1))}
    rows = {}
    for name, (fn, tracked) in legs.items():
        fn()  # warm-up: allocations, first launches
        torch.cuda.synchronize()
        secs, last = [], None
        for _ in range(a.reps):
            t = time.perf_counter()
            last = fn()
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t)
        s = float(np.median(secs))
        ses_seconds = last.get("session_seconds", last.get("sessions", 1) * secs[-1])
        rows[name] = dict(seconds_median=s, seconds_min=float(min(secs)), seconds_max=float(max(secs)), reps=a.reps, clips_per_s=len(lengths) / s,
                          tracked_frames=tracked, tracked_frames_per_s=tracked / s, steps=last["steps"], mean_idle_slots_per_step=last["idle"],
                          admission_ms_last_run=last["admission_ms"], admission_share_of_session_time_last_run=last["admission_ms"] * 1e-3 / ses_seconds,
                          **{k: last[k] for k in ("sessions", "groups") if k in last})
        print(name, json.dumps(rows[name]), flush=True)
    out = dict(what="256 clips of 8..32 frames (seeded uniform draw), 1920 x 1080, 1000 corners, frames resident as CUDA tensors: run_queue on 64 streams vs "
                    "run_sequences per group of equal length vs run_sequences on 256 clips of the mean length; host clock around runs that end in a device "
                    "synchronise, admissions from HIP events on the sessions' streams",
               build_id=L.build_info()["build_id"], device=torch.cuda.get_device_name(0), clips=len(lengths), streams=a.streams, lengths=lengths,
               mean_length=mean, seed=a.seed, rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
