"""An observation, not a claim: sequence B of the real stills (tests/golden/stills_gray.npz, label 40 km/h) tracked by the CPU oracle loop
(tests/test_oracle_stills.py), then refined by the NumPy model tests/refine_partial_ref.py -- the whole clip as one window and in windows of 4 frames,
with full-length tracks only (min_obs = nf) against min_obs = 3, without and with triangulated starts.  No GPU.
-> profiles/refine_partial/stills_b.json"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import refine_partial_ref as RP  # noqa: E402
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
    orc = SessionOracle(K, fr[0], p, p3, vp, t, time0=np.float32(times[0]), res0=res, nhist=n, msv_frame=MSV)
    for i in range(1, n):
        orc.step(fr[i], np.float32(times[i]), i)
    sp = orc.S[1:, 8]
    out = dict(what=__doc__.split("->")[0].strip(), tracks_frame0=len(p), alive_last_frame=int(orc.vg.sum()),
               tracker=f"Speed = {sp.mean():.2f} +/- {sp.std():.2f} km/h", legs={})
    for name, nf in (("whole clip", n), ("windows of 4", 4)):
        starts = [0] if nf == n else refine_window_starts(n, nf)
        for leg, (m, gate) in (("full-length only", (nf, 0.0)), ("min_obs 3", (3, 0.0)), ("min_obs 3, start_reproj 1.0", (3, 1.0))):
            wins = [RP.refine_partial_ref(orc.K, orc.P, orc.p3, orc.B, f, nf, n - 1, MSV, min(m, nf), gate) for f in starts]
            mg = merge_window_speeds(n, wins)
            out["legs"][f"{name}, {leg}"] = dict(first=starts, nt=[w["nt"] for w in wins], npart=[w["npart"] for w in wins], ntri=[w["ntri"] for w in wins],
                                                 nrej=[w["nrej"] for w in wins], nobs=[w["nobs"] for w in wins], iterations=[w["iterations"] for w in wins],
                                                 f_last=[float(w["f_last"]) for w in wins], speed_mean=mg["speed_mean"], speed_std=mg["speed_std"],
                                                 line=f"BA speed = {mg['speed_mean']:.2f} +/- {mg['speed_std']:.2f} km/h")
    path = os.path.join(ROOT, "profiles", "refine_partial", "stills_b.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    for k, v in out["legs"].items():
        print(k, v["nt"], v["npart"], v["ntri"], v["nrej"], v["line"], np.round(v["f_last"], 3))
    print(out["tracker"])


if __name__ == "__main__":
    main()
