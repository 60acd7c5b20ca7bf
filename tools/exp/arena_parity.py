"""Parity of everything that lives in a carved device block between two builds of the library (the parent commit's and this tree's): SHA-256 of every array
the drivers and the small-shape entries return, the offsets of the pointers the three *_ptrs entries hand out (relative to the first one) and the four public
size functions.  The Python is this tree's in every run; only the library differs (VH_LIB, as tools/exp/ab_libs.sh selects it).

    python tools/exp/arena_parity.py --parent _exp/lib_parent.so --out profiles/arena/parity.json

runs the parent twice, then this tree, each in a child process.  Every entry must be equal between the parent and this tree.  The exceptions are the entries that do not repeat
between the parent's own two runs, which the result lists; the project documents three, all sums of squares accumulated with floating-point atomics
across workgroups by the bundle adjustment (k_ba_update*, profiles/ba_host/resources.md): the rms(delta) column of a refined window's trace and the record
fields f_first and f_last read from the same sums.  Of the three a driver's result carries `f_last` (one entry per window), hashed apart from the speeds,
covers, track counts, iteration counts and convergence flags of the same windows, which are compared exactly.  The procTime column of S is wall time and is
zeroed before hashing.

Inputs: sequence B of the stills (1024 x 768, tests/golden/stills_gray.npz) for the drivers, and the shapes of tests/test_gpu_arena.py for the rest (restated
here: a tool imports no test module)."""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

MATCH = dict(levels=2, query_per_level=64, train_per_level=64, border_x=4, border_y=4, min_good=3)


def sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(f"{a.dtype}{a.shape}".encode() + a.tobytes()).hexdigest()[:24]


def clip_units(r):
    S = r["S"].copy()
    S[:, 1] = 0
    return dict({k: sha(r[k]) for k in ("B", "P", "vg", "vp", "p", "p3", "ids", "t0", "R0")}, S=sha(S))


def ba_units(ba):
    """a clip refined in windows (driver._merged_ba): every array and scalar of the merged result, one hash each"""
    return {k: sha(np.asarray(v)) for k, v in sorted(ba.items())}


def frame(w, h, k=0):
    from velocity_amd import synth

    return synth.render_frame(w, h, synth.AffineMotion(w, h, s=1.0, theta_deg=0.0, tx=3.0, ty=0.0), k).numpy()


def offsets(struct, names):
    first = getattr(struct, names[0])
    return {n: (getattr(struct, n) or 0) - first for n in names}


def child(out_path):
    import torch

    from velocity_amd import KLT, synth
    from velocity_amd import _lib as L
    from velocity_amd import driver as D
    from velocity_amd import images

    lib = L.load()
    cases = {}

    def case(name, units):
        cases[name] = units
        print(name, "ok", flush=True)

    # the drivers on one 1024 x 768 clip of the stills (two for run_sequences, three of different lengths for the queue)
    st = np.load(os.path.join(ROOT, "tests", "golden", "stills_gray.npz"))
    fr, q, K, t = st["b_frames"], st["b_q"], st["b_K"], st["b_times"]
    kw = dict(roi_border=(180, 140))
    clips = [dict(frames=fr, q=q, times=t, name="b"), dict(frames=fr[:4], q=q, times=t[:4], name="b[:4]"), dict(frames=fr[:6], q=q, times=t[:6], name="b[:6]")]
    case("run_sequence", clip_units(D.run_sequence(fr, q, K, times=t, out=None, live=False, name="b", **kw)))
    case("run_sequence_fallback", clip_units(D.run_sequence(st["a_frames"], st["a_q"], st["a_K"], times=st["a_times"], roi_border=(233, 167), fallback=True,
                                                            out=None, live=False, name="a")))
    case("run_sequences", {f"clip{k}.{f}": v for k, r in enumerate(D.run_sequences([clips[0], clips[0]], K, sessions=1, **kw)) for f, v in clip_units(r).items()})
    case("run_queue", {f"clip{k}.{f}": v for k, r in enumerate(D.run_queue(clips, K, streams=2, sessions=1, **kw)) for f, v in clip_units(r).items()})
    res = D.run_sequences([clips[0], clips[0]], K, sessions=1, refine="ba", refine_window=4, **kw)
    case("refine_windows", {f"clip{k}.{f}": v for k, r in enumerate(res) for f, v in ba_units(r["ba"]).items()})
    f0 = D.frame0_batch([fr[0], fr[1]], [q, q], K, **kw)
    f0 += D.frame0_batch([frame(96, 80), frame(96, 80, 1)], [np.float32([[30, 30], [60, 30], [60, 50], [30, 50]])] * 2, K, roi_border=(20, 20), max_corners=50)
    case("frame0_batch", {f"clip{k}.{f}": sha(np.asarray(v)) for k, r in enumerate(f0) for f, v in r.items()})
    for w, h, mc in ((32, 32, 50), (96, 80, 50), (96, 80, 2050), (32, 32, 50)):  # first block, its growth, the sort block, the small image again
        case(f"good_features_{w}x{h}_{mc}" + ("_again" if f"good_features_{w}x{h}_{mc}" in cases else ""), dict(corners=sha(images.goodFeaturesToTrack(frame(w, h), mc, 0.001, 0, blockSize=3, useHarrisDetector=False))))
    for w, h in ((64, 48), (96, 80), (64, 48)):
        T, inl = KLT.estimateAffine2D_SURF(frame(w, h), frame(w, h, 1), synth.grid_tracks(20, w, h, frac=0.5), **MATCH)
        case(f"estimateAffine2D_SURF_{w}x{h}" + ("_again" if f"estimateAffine2D_SURF_{w}x{h}" in cases else ""),
             dict(T=sha(np.zeros(0) if T is None else T), inliers=sha(inl)))
    T, inl = KLT.estimateAffine2D_SURF(st["a_frames"][0], st["a_frames"][1], st["a_q"])
    case("estimateAffine2D_SURF_stills_a", dict(T=sha(np.zeros(0) if T is None else T), inliers=sha(inl)))

    # pointer offsets and sizes: the session of tests/test_gpu_arena.py, its two-stream context, the matcher after the call above
    ses = D.TrackerSession(synth.K_1080P, 16, 12, 5, nhist=3, batch=2)
    names = ["vg", "vp", "p", "ids", "p3", "P", "B", "S", "n_cur", "n_pose", "t", "res", "frame_i", "klt_flags", "pose_info", "sel_pw", "p_proj"]
    v0, v1 = ses.view(0), ses.view(1)
    case("vh_session_ptrs", dict({f"slot0.{n}": o for n, o in offsets(v0, names).items()}, **{f"slot1.{n}": getattr(v1, n) - v0.vg for n in names}))
    ks = [L.KltStages(), L.KltStages()]
    for b in (0, 1):
        L.check(lib.vh_klt_stage_ptrs(ses.ws.handle, b, C.byref(ks[b])), "vh_klt_stage_ptrs")
    kn = [n for n, _ in L.KltStages._fields_]
    case("vh_klt_stage_ptrs", dict({f"slot0.{n}": o for n, o in offsets(ks[0], kn).items()}, **{f"slot1.{n}": getattr(ks[1], n) - ks[0].p_small for n in kn}))
    ws = L.workspace(64, 48, 128)
    ms = L.MatchStages()
    L.check(lib.vh_match_stage_ptrs(ws.handle, C.byref(ms)), "vh_match_stage_ptrs")
    flat = {f"kp{i}{l}": ms.kp[i][l] for i in (0, 1) for l in range(ms.levels)}
    flat.update(cnt=ms.cnt, pos0=ms.pos[0], pos1=ms.pos[1], desc0=ms.desc[0], desc1=ms.desc[1], nn=ms.nn, good=ms.good, roi=ms.roi)
    case("vh_match_stage_ptrs", {k: (v or 0) - flat["kp00"] for k, v in flat.items()})
    case("sizes", dict(vh_session_export_size=lib.vh_session_export_size(ses.handle, None), vh_session_refine_workspace=lib.vh_session_refine_workspace(ses.handle, 2, 3),
                       vh_session_refine_windows_workspace=lib.vh_session_refine_windows_workspace(ses.handle, 3, 2),
                       vh_nls_batch_workspace=lib.vh_nls_batch_workspace(40, 3)))
    del torch
    with open(out_path, "w") as f:
        json.dump(dict(build=L.build_info(), cases=cases), f, default=str)


def compare(pa, pb, head, out_path):
    runs = [json.load(open(p)) for p in (pa, pb, head)]
    a, b, h = (r["cases"] for r in runs)
    out = dict(what=__doc__.split("\n\n")[0].replace("\n", " "), parent_build=runs[0]["build"], head_build=runs[2]["build"], cases={})
    bad, unstable = 0, []
    for name in a:
        assert a[name].keys() == b[name].keys() == h[name].keys(), name
        rows = {}
        for unit, va in a[name].items():
            if va != b[name][unit]:  # does not repeat in the parent itself
                unstable.append(f"{name}.{unit}")
                continue
            rows[unit] = dict(parent=va, head=h[name][unit], equal=va == h[name][unit])
            bad += va != h[name][unit]
        out["cases"][name] = dict(equal=all(r["equal"] for r in rows.values()), units=rows)
        print(f"{name}: {len(rows)} entries -> {'all equal' if out['cases'][name]['equal'] else 'DIFFER'}")
    out["not_repeatable_in_the_parent"] = unstable
    out["differences"] = bad
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print("not repeatable in the parent itself:", sorted({u.rsplit(".", 1)[1] for u in unstable}) or "-")
    print("parity holds" if not bad else f"{bad} DIFFERENCES")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent", help="the parent commit's library (python -m velocity_amd._build --out=... in a checkout of the parent)")
    ap.add_argument("--out", default="profiles/arena/parity.json")
    ap.add_argument("--child", help="(internal) run the cases with the library the environment selects and write them here")
    ap.add_argument("--timeout", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--runs", help="keep the three runs' files in this directory (default: a temporary one)")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    tmp = a.runs or tempfile.mkdtemp()
    os.makedirs(tmp, exist_ok=True)
    paths = []
    for k, lib in enumerate((a.parent, a.parent, None)):
        env = dict(os.environ)
        env.pop("VH_LIB", None)
        if lib:
            env["VH_LIB"] = os.path.abspath(lib)
        paths.append(os.path.join(tmp, f"run{k}.json"))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", paths[-1]], env=env, timeout=a.timeout)
        if r.returncode:  # nothing more is started on a GPU a run has just failed on
            print(f"arena_parity: run {k} failed ({r.returncode}): stopping")
            return 1
    return compare(*paths, a.out)


if __name__ == "__main__":
    sys.exit(main())
