"""The truth experiment of the partial refinement, on the NumPy model (no GPU): analytic windows of 8 frames with 6 full-length and 34 partial tracks
(lives of 2..7 frames), 0.1 px noise; the worst relative error of the per-step displacements (scale-free) with full-length tracks only against
min_obs = 2.  -> profiles/refine_partial/truth.json.  tests/test_refine_partial_cpu.py asserts the comparison of the medians on the first 8 seeds."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import refine_partial_ref as RP  # noqa: E402


def main(seeds=16):
    rows = []
    for seed in range(seeds):
        K, P, pw0, cw0, cw = RP.analytic_window(seed)
        a, na = RP.solve_analytic(K, P, pw0, cw0, P.shape[2])
        b, nb = RP.solve_analytic(K, P, pw0, cw0, 2)
        rows.append(dict(seed=seed, tracks_full=na, tracks_min_obs_2=nb, full_only=RP.step_error(a, cw), min_obs_2=RP.step_error(b, cw)))
    full, part = np.array([r["full_only"] for r in rows]), np.array([r["min_obs_2"] for r in rows])
    out = dict(what="worst relative error of the per-step camera displacements, each profile normalised by its own mean (scale-free)",
               scene="refine_partial_ref.analytic_window: 8 frames, 6 full-length + 34 partial tracks of 2..7 frames, 0.1 px noise, start 1 % / 2 % off",
               median_full_only_8=float(np.median(full[:8])), median_min_obs_2_8=float(np.median(part[:8])),
               median_full_only=float(np.median(full)), median_min_obs_2=float(np.median(part)),
               seeds_where_partial_is_worse=[r["seed"] for r in rows if r["min_obs_2"] > r["full_only"]], per_seed=rows)
    path = os.path.join(ROOT, "profiles", "refine_partial", "truth.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "per_seed"}))


if __name__ == "__main__":
    main()
