"""What frame 0 costs per clip: a per-clip loop of vh_frame0_init calls -- each a batch of ONE clip through the same kernels; until vh_version 106 the
loop run_sequences ran, then on the first-generation detector that sorted every ROI pixel -- against one vh_frame0_init_batch call per session, on synthetic 1920 x 1080 clips (synth.render_frame, one seed per clip; the plate quad is worldPointsLicensePlate("Chile") projected through
synth.K_1080P at 3.5 - 5 m, a different position per clip), roi_border (700, 500), 1000 corners.  Clips are grouped into sessions as run_sequences groups them.

For every size: (a) vh_frame0_init (a one-clip batch per call) + vh_session_init_dev per clip, (b) vh_frame0_init_batch per session + vh_session_init_dev per clip; warmed up, each
repetition ends in a device synchronise, a and b alternate; median / min / max.  The outputs of both paths are compared (n, p, t, R bit for bit).  For scale
it also times the 19-step tracking loop of the same clips (run_sequences' loop_seconds).

    python tools/exp/frame0_batch_timing.py --out r07_frame0_batch.json
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/exp/frame0_batch_timing.py --profile 256     (the batched call only)
"""
import argparse
import ctypes as C
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

W, H, BORDER, MC, NFR = 1920, 1080, (700, 500), 1000, 20
SUBPIX = (5, 100, 0.001)
SETTINGS = D.Frame0Settings(roi_border=BORDER, max_corners=MC, subpix=SUBPIX)  # (everything else: the reference's call)


def plate_quad(b):
    rng = np.random.default_rng(1000 + b)
    X, Y, Z = rng.uniform(-0.6, 0.6), rng.uniform(-0.3, 0.3), rng.uniform(3.5, 5.0)
    P = worldPointsLicensePlate("Chile").astype(np.float64) + np.array([X, Y, Z])
    uvw = P @ synth.K_1080P.astype(np.float64)
    return (uvw[:, :2] / uvw[:, 2:]).astype(np.float32)


def make_clips(n, frames=NFR):
    torch = L.torch_cuda()
    clips = []
    for b in range(n):
        m = synth.AffineMotion(W, H, s=0.999, theta_deg=0.02, tx=2.0 + 0.01 * b, ty=-0.5)
        fr = [synth.render_frame(W, H, m, k, seed=0xC0FFEE + 7919 * b, device="cuda").contiguous() for k in range(frames)]
        clips.append(dict(frames=fr, q=plate_quad(b), times=np.arange(frames, dtype=np.float32) / 30.0))
    torch.cuda.synchronize()
    return clips


class Setup:
    """Sessions and streams of one size, as run_sequences builds them, and the output buffers of path (a)."""

    def __init__(self, clips):
        torch = L.torch_cuda()
        self.torch, self.clips = torch, clips
        n = len(clips)
        G = D.session_groups(n, MC)
        owner = [b * G // n for b in range(n)]
        self.members = [[b for b in range(n) if owner[b] == g] for g in range(G)]
        self.streams = D.session_streams(G)
        self.sess = []
        for g in range(G):
            with torch.cuda.stream(self.streams[g]):
                self.sess.append(D.TrackerSession(synth.K_1080P, W, H, SETTINGS.cap, nhist=NFR, batch=len(self.members[g])))
        self.bufs = [SETTINGS.outputs(len(m)) for m in self.members]
        torch.cuda.synchronize()

    def run_a(self):
        """vh_frame0_init (a one-clip batch per call) + vh_session_init_dev per clip (the loop run_sequences ran before vh_frame0_init_batch)."""
        win, it, eps = SUBPIX
        for g, mem in enumerate(self.members):
            ses = self.sess[g]
            p, p3, vp, t0, R0, res0, n0 = self.bufs[g]
            with self.torch.cuda.stream(self.streams[g]):
                for j, b in enumerate(mem):
                    f0 = self.clips[b]["frames"][0]
                    q = np.ascontiguousarray(self.clips[b]["q"])
                    rois = (C.c_int * 8)()
                    L.check(ses.lib.vh_frame0_init(ses.ws.handle, L.dptr(f0), W, H, W, q.ctypes.data_as(L.f32p), ses.K64.ctypes.data_as(L.f64p),
                                                   SETTINGS.plate_w.ctypes.data_as(L.f64p), BORDER[0], BORDER[1], MC, 0.01, 5, 0.04, win, it, eps, L.dptr(p[j]),
                                                   L.dptr(p3[j]), L.dptr(vp[j]), L.dptr(t0[j]), L.dptr(R0[j]), L.dptr(res0[j]), L.dptr(n0[j]), rois,
                                                   L.stream_ptr()), "vh_frame0_init")
                    L.check(ses.lib.vh_session_init_dev(ses.handle, j, L.dptr(f0), W, L.dptr(p[j]), L.dptr(p3[j]), L.dptr(vp[j]), L.dptr(t0[j]),
                                                        L.dptr(res0[j]), L.dptr(n0[j]), 0.0, 0.0, L.stream_ptr()), "vh_session_init_dev")
        self.torch.cuda.synchronize()

    def run_b(self):
        """TrackerSession.admit per session: one vh_frame0_init_batch + vh_session_init_dev per clip (run_sequences since vh_version 106)."""
        self.admitted = []
        for ses, hs, mem in zip(self.sess, self.streams, self.members):
            with self.torch.cuda.stream(hs):
                self.admitted.append(ses.admit([(j, self.clips[b]["frames"][0], self.clips[b]["q"], 0.0, 0.0) for j, b in enumerate(mem)], SETTINGS))
        self.torch.cuda.synchronize()

    def same(self):
        """Both paths computed the same frame 0 (n, p[:n], t, R bit for bit): the outputs of (a) against what the admission of (b), the last to run, left
        in the sessions."""
        for ses, adm, ba in zip(self.sess, self.admitted, self.bufs):
            pa, _, _, ta, Ra, _, na = (x.cpu().numpy() for x in ba)
            for j in range(ses.batch):
                st = ses.state(j)
                if not (st["n_cur"] == na[j] and np.array_equal(st["p"], pa[j, :na[j]]) and np.array_equal(st["t"], ta[j])
                        and np.array_equal(adm[j].R0.cpu().numpy(), Ra[j])):
                    return False
        return True


def stats(xs):
    xs = np.asarray(xs)
    return dict(median_ms=float(np.median(xs) * 1e3), min_ms=float(xs.min() * 1e3), max_ms=float(xs.max() * 1e3), reps=len(xs))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 8, 64, 256])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-loop", action="store_true", help="skip the tracking-loop reference")
    ap.add_argument("--profile", type=int, default=0, help="only the batched path at this many clips (for rocprofv3)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch = L.torch_cuda()
    if a.profile:
        s = Setup(make_clips(a.profile, frames=1))
        for _ in range(a.warmup + a.reps):
            s.run_b()
        print(f"profiled {a.warmup + a.reps} batched frame-0 passes at {a.profile} clips")
        return
    rows = []
    for n in a.sizes:
        clips = make_clips(n, frames=1 if a.no_loop else NFR)
        s = Setup(clips)
        for _ in range(a.warmup):
            s.run_a()
            s.run_b()
        ta, tb = [], []
        for _ in range(a.reps):
            t = time.perf_counter()
            s.run_a()
            ta.append(time.perf_counter() - t)
            t = time.perf_counter()
            s.run_b()
            tb.append(time.perf_counter() - t)
        row = dict(nclips=n, sessions=len(s.members), old_loop=stats(ta), batched=stats(tb), same_results=s.same())
        row["old_us_per_clip"] = row["old_loop"]["median_ms"] * 1e3 / n
        row["batched_us_per_clip"] = row["batched"]["median_ms"] * 1e3 / n
        row["speedup"] = row["old_loop"]["median_ms"] / row["batched"]["median_ms"]
        del s
        if not a.no_loop:
            D.run_sequences(clips, synth.K_1080P, roi_border=BORDER, max_corners=MC)  # warm-up
            r = D.run_sequences(clips, synth.K_1080P, roi_border=BORDER, max_corners=MC)
            row["tracking_loop_19_steps_ms"] = r[0]["ms_per_frame"] * (NFR - 1)
            row["tracking_loop_us_per_stream_frame"] = r[0]["ms_per_frame"] * 1e3 / n
            row["tracks0_mean"] = float(np.mean([x["n_tracks0"] for x in r]))
        print(json.dumps(row), flush=True)
        rows.append(row)
        del clips
        torch.cuda.empty_cache()
    out = dict(what="frame-0 initialisation of nclips 1920x1080 clips: per-clip vh_frame0_init loop vs one vh_frame0_init_batch per session "
                    "(+ vh_session_init_dev per clip in both), host clock around work ending in a device synchronise",
               build_id=L.build_info()["build_id"], device=torch.cuda.get_device_name(0), roi_border=list(BORDER), max_corners=MC, rows=rows)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
