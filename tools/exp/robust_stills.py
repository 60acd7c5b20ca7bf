"""An observation, not a claim: sequence B of the real stills (tests/golden/stills_gray.npz, label 40 km/h) tracked by the CPU oracle loop
(tests/test_oracle_stills.py), then refined by the NumPy model tests/robust_ref.py -- the whole clip and windows of 4 frames, plain and with Huber
weights of 0.5 and 1.0 pixels, free and with the four plate corners anchored at their frame-0 points.  No GPU.
-> profiles/ba_robust/stills_b.json"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import robust_ref as RB  # noqa: E402
from oracle import klt_oracle as KO  # noqa: E402
from oracle import nls_oracle as NO  # noqa: E402
from oracle.session_oracle import SessionOracle  # noqa: E402
from velocity_amd.driver import merge_window_speeds, refine_window_starts  # noqa: E402

MSV = 5


def main():
    d = np.load(os.path.join(ROOT, "tests", "golden", "stills_gray.npz"))
    fr, times, q, K = d["b_frames"], d["b_times"], d["b_q"], d["b_K"]
    H, W = fr[0].shape
    boxa, boxb = KO.bounding_rect(q, (H, W), (0, 0)), KO.bounding_rect(q, (H, W), (180, 140))
    roi = fr[0][boxb[2]:boxb[3], boxb[0]:boxb[1]]
    p = KO.corner_subpix(fr[0], KO.good_features(roi, 1000, 0.01, 5, 0.04) + np.float32([boxb[0], boxb[2]]), 5, 100, 0.001)
    p = np.concatenate((q, p)).astype(np.float32)
    t, R, res, _ = NO.estimate_world_camera_pose(K, q, NO.plate_world_points("Chile"), findR=True)
    p3 = NO.hom0(NO.image_to_world(K, R.astype(float), t, p).astype(float)) @ R.astype(float) + t
    vp = (p[:, 0] > boxa[0]) & (p[:, 0] < boxa[1]) & (p[:, 1] > boxa[2]) & (p[:, 1] < boxa[3])
    n = len(fr)
    plate = (np.arange(4), np.asarray(p3[:4], np.float64).copy())  # what refine_anchor="plate" anchors: the frame-0 points of tracks 0..3
    orc = SessionOracle(K, fr[0], p, p3, vp, t, time0=np.float32(times[0]), res0=res, nhist=n, msv_frame=MSV)
    for i in range(1, n):
        orc.step(fr[i], np.float32(times[i]), i)
    sp = orc.S[1:, 8]
    out = dict(what=__doc__.split("->")[0].strip(), tracks_frame0=len(p), alive_last_frame=int(orc.vg.sum()),
               tracker=f"Speed = {sp.mean():.2f} +/- {sp.std():.2f} km/h",
               earlier={"free, plain (profiles/ba_anchor/stills_b.json)": "42.34 +/- 1.26 km/h", "plate, plain": "41.61 +/- 1.26 km/h"}, legs={})
    for name, nf in (("whole clip", n), ("windows of 4", 4)):
        starts = [0] if nf == n else refine_window_starts(n, nf)
        for anchor_name, anchors in (("free", None), ("plate", plate)):
            for delta in (0.0, 1.0, 0.5):  # 0: plain least squares (the model without a threshold is anchor_ref, bit for bit)
                wins = [RB.refine_window_robust_ref(orc.K, orc.P, orc.p3, orc.B, f, nf, delta, anchors) for f in starts]
                mg = merge_window_speeds(n, wins)
                key = f"{name}, {anchor_name}, " + ("plain" if delta == 0 else f"huber {delta:g} px")
                out["legs"][key] = dict(first=starts, nt=[w["nt"] for w in wins], nfix=[w["nfix"] for w in wins], iterations=[w["iterations"] for w in wins],
                                        nout_first=[w["nout_first"] for w in wins], nout_last=[w["nout_last"] for w in wins],
                                        measurements=[w["nt"] * nf for w in wins], f_first=[float(w["f_first"]) for w in wins],
                                        f_last=[float(w["f_last"]) for w in wins], speed_mean=mg["speed_mean"], speed_std=mg["speed_std"],
                                        line=f"BA speed = {mg['speed_mean']:.2f} +/- {mg['speed_std']:.2f} km/h")
    path = os.path.join(ROOT, "profiles", "ba_robust", "stills_b.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    for k, v in out["legs"].items():
        print(k, v["nt"], v["nfix"], v["nout_first"], v["nout_last"], v["line"], np.round(v["f_last"], 3))
    print(out["tracker"])


if __name__ == "__main__":
    main()
