"""Bit parity of the bundle-adjustment entry points between two builds of the library: one call per route, a SHA-256 of every array each call returns.
Run it once per library (the experiment override VH_LIB=<path> selects the other one, as tools/exp/ab_libs.sh does) and compare the files:
    python tools/exp/ba_host_parity.py a.json;  VH_LIB=$PWD/_exp/lib_parent.so python tools/exp/ba_host_parity.py b.json
    python tools/exp/ba_host_parity.py --compare a.json b.json [more.json ...]
Same device code and same launches => equal hashes; a difference is a host-side bug, not rounding.  One column is kept apart: rms(delta), the second
column of the trace, is a sum of per-workgroup partials added with floating-point atomics (k_ba_update*), so its last bits depend on the order in
which the workgroups finish and differ between two runs of ONE library.  Nothing else a solve returns depends on it beyond the convergence flag."""
import contextlib
import hashlib
import io
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(f"{a.dtype}{a.shape}".encode() + a.tobytes()).hexdigest()


def digests(res):
    """(cw, pw[, x], trace) -> one hash per array, the trace by column."""
    names = ("cw", "pw", "x", "trace") if len(res) == 4 else ("cw", "pw", "trace")
    out = {n: digest(a) for n, a in zip(names, res)}
    tr = np.asarray(res[-1])
    del out["trace"]
    out["trace_rms_residual"], out["trace_rms_delta"] = digest(tr[:, 0]), digest(tr[:, 1])
    return out


def compare(paths):
    runs = [json.load(open(p))["cases"] for p in paths]
    bad = 0
    for case in runs[0]:
        for key in runs[0][case]:
            n = len({r[case][key] for r in runs})
            if n > 1:
                print(f"{case}.{key}: {n} different values over {len(runs)} runs")
                bad += key != "trace_rms_delta"
    print("every array but trace_rms_delta equal in all runs" if not bad else f"{bad} DIFFERENCES outside trace_rms_delta")
    return 1 if bad else 0


def main(out_path):
    from velocity_amd import _lib as L
    from velocity_amd import synth
    from velocity_amd.dist import fcnNLS_batch_sharded
    from velocity_amd.NLS import fcnNLS_batch, fcnNLS_batch2, fcnNLS_batch_windows

    K = synth.K_1080P
    out = {"build": L.build_info(), "cases": {}}

    def case(name, fn):
        with contextlib.redirect_stdout(io.StringIO()):
            res = fn()
        out["cases"][name] = digests(res) if isinstance(res, tuple) else {f"w{w}.{k}": v for w, r in enumerate(res) for k, v in digests(r).items()}
        print(name, "ok", flush=True)

    # (cw, pw, x, trace): x and the trace cut at info[0] carry everything the entry point wrote
    for nt, nf in ((40, 4), (40, 22), (60, 23), (60, 44)):  # MFMA128 + GJ on the matrix cores | MFMA128 + VALU GJ | MFMA256 + Cholesky | SYRK + Cholesky
        case(f"batch_{nt}_{nf}", lambda: fcnNLS_batch(K, *synth.ba_scene(nt, nf, seed=11 + nf), return_info=True))
    L.load().vh_debug_ba_force_valu(1)
    try:
        case("batch_40_4_valu", lambda: fcnNLS_batch(K, *synth.ba_scene(40, 4, seed=15), return_info=True))
    finally:
        L.load().vh_debug_ba_force_valu(0)
    case("batch2_40_6", lambda: fcnNLS_batch2(K, *synth.ba_scene(40, 6, seed=17), return_info=True))

    def windows():
        Ks, scenes = [], []
        for w, cnt in enumerate((40, 31, 0)):
            Kw = K.astype(np.float64).copy()
            Kw[0, 0] *= 1.0 + 0.01 * w
            Kw[1, 1] *= 1.0 + 0.01 * w
            P, pw0, cw0 = synth.ba_scene(40, 4, seed=21 + w, K=Kw)
            P[:, cnt:, 2:] = np.nan  # tracks behind the window's count lose their last frames: the track filter drops them
            Ks.append(Kw)
            scenes.append((P, pw0, cw0))
        return fcnNLS_batch_windows(np.stack(Ks), *zip(*scenes), return_info=True)

    case("windows_40_31_0", windows)
    case("sharded_one_rank_40_4", lambda: fcnNLS_batch_sharded(K, *synth.ba_scene(40, 4, seed=15)))  # the four phases, no process group
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, default=str)


if __name__ == "__main__":
    sys.exit(compare(sys.argv[2:]) if sys.argv[1] == "--compare" else main(sys.argv[1]))
