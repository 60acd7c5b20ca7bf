"""Parity of the refinement entry points and of the drivers' refine="ba" between two builds of the library (the parent commit's and this tree's), by the
bytes of every record and of every array the drivers return.  The Python is this tree's in every run; only the library differs (VH_LIB, as
tools/exp/ab_libs.sh selects it).  Each run is a fresh child process:

    python tools/exp/refine_parity.py --parent _exp/lib_parent.so --out profiles/refine_one_path/parity.json

runs the parent twice, then this tree.  A field whose every unit (case, record) repeats bit for bit between the two parent runs must be SHA-identical
between the parent and this tree in every unit; a field with a unit that does not repeat (sums of squares accumulated with floating-point atomics: the
trace) is compared as float64 at rtol = 1e-12 in every unit.  The unit `rest` of a record is every byte outside trace, f_first and f_last: every other
field AND the padding between them.  The device record buffer is filled with 0xFF before each call, so a byte a call leaves unwritten shows up there.

Inputs: the three-stream session of tests/test_gpu_refine.py at its last frame, and the stills clips of tests/test_gpu_queue.py (restated here: a tool
imports no test module)."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N0, NF, NHIST, W4 = 150, 8, 10, 4


def _camera(W, H, f):
    from velocity_amd import synth

    K = synth.K_1080P.copy()
    K[0, 0] = K[1, 1] = f
    K[2, 0], K[2, 1] = W / 2 + 0.5, H / 2 + 0.5
    return K


def _scene(W, H, seed, f, hopeless):
    from velocity_amd import synth

    K = _camera(W, H, f)
    m = synth.PlaneMotion(K, z0=3.6)
    frames = [synth.render_frame(W, H, m, k, seed=seed).numpy() for k in range(NHIST)]
    p = synth.grid_tracks(N0, W, H, seed=seed & 0xFF)
    p[::hopeless] = np.float32([-40.0, -40.0])
    vp = (p[:, 0] > W * 0.3) & (p[:, 0] < W * 0.7) & (p[:, 1] > H * 0.3) & (p[:, 1] < H * 0.7)
    return frames, p, m.world_points(p), vp, K


def _session():
    import torch

    from velocity_amd.driver import TrackerSession

    scenes = [_scene(320, 240, 411, 700.0, 37), _scene(256, 192, 422, 560.0, 11), _scene(320, 240, 433, 700.0, 7)]
    ses = TrackerSession(scenes[0][4], 320, 240, N0, nhist=NHIST, batch=3, msv_frame=5)
    for b, (frames, p, p3, vp, Kb) in enumerate(scenes):
        ses.init_stream(b, frames[0], p, p3, vp, np.float32([1.5, 0.45, 3.6]), time0=10.0 * b, K=Kb)
    for k in range(1, NF):
        ses.step([torch.from_numpy(sc[0][k]).cuda() for sc in scenes], time_s=[np.float32(10.0 * b + k / (25.0 + b)) for b in range(3)], frame_no=[k] * 3)
    return ses


def _stills_clips():
    st = np.load(os.path.join(ROOT, "tests", "golden", "stills_gray.npz"))
    back = [0, 1, 2, 3, 4, 5, 6, 5, 4, 3, 2, 1]
    t7 = st["b_times"]
    frames, q = np.ascontiguousarray(st["b_frames"][back]), st["b_q"]
    times = np.concatenate([t7, t7[6] + np.cumsum(np.diff(t7)[::-1])[:5]])
    qm = q.copy()
    qm[:, 0] = (frames.shape[2] - 1) - qm[:, 0]
    qm = qm[[1, 0, 3, 2]]
    mirrored = np.ascontiguousarray(frames[:, :, ::-1])
    return [dict(frames=frames, q=q, times=times, name="b"), dict(frames=frames[:4], q=q, times=times[:4], name="b[:4]"),
            dict(frames=mirrored[:7], q=qm, times=times[:7], name="b mirrored[:7]"),
            dict(frames=frames[:9], q=q, times=(times * np.float32(1.5) + np.float32(2.0))[:9], frame_numbers=list(range(100, 109)), name="b slow[:9]"),
            dict(frames=frames[:2], q=q, times=times[:2], name="b[:2]"), dict(frames=mirrored, q=qm, times=times, name="b mirrored"),
            dict(frames=frames[:3], q=q, times=times[:3], name="b[:3]")], st["b_K"]


def _record_units(raw, lay):
    """{field: hex bytes} of one record: the fields read from the solve's sums of squares by name (whether they repeat is for the parent's two runs to
    say), `rest` = the record with their ranges zeroed."""
    raw = np.array(raw, np.uint8)
    spans = dict(trace=(lay.trace, 16 * lay.max_iter), f_first=(lay.f_first, 8), f_last=(lay.f_last, 8))
    out = {k: raw[o:o + n].tobytes().hex() for k, (o, n) in spans.items()}
    for o, n in spans.values():
        raw[o:o + n] = 0
    out["rest"] = raw.tobytes().hex()
    return out


def _dict_units(d):
    return {k: ("f8:" if np.asarray(v).dtype == np.float64 else "") + np.ascontiguousarray(v).tobytes().hex() for k, v in sorted(d.items()) if k != "anchor"}


def child(out_path):
    from velocity_amd import _lib as L
    from velocity_amd import driver as D

    cases = {}
    ses = _session()
    wins = [(0, 0), (0, 3), (1, 0), (1, 4), (2, 2), (2, 4)]
    requests = {"refine": lambda: ses.refine([0, 1, 2]), "refine_windows": lambda: ses.refine_windows(wins, W4),
                "refine_windows_points": lambda: ses.refine_windows(wins, W4, with_points=True)}
    for tag in ("", "_anchored"):
        if tag:  # slots 0 and 2 anchored (four surviving tracks at their current p3), slot 1 free: a request of both kinds
            ses.set_anchors(0, [1, 2, 3, 4])
            ses.set_anchors(2, [1, 2, 3, 4])
        for name, fn in requests.items():
            fn().result()  # (sizes the session's device record buffer)
            ses._refine_dev.fill_(0xFF)
            h = fn()
            h.result()
            assert name != "refine" or [r["nfix"] > 0 for r in h.result()] == ([True, False, True] if tag else [False] * 3)
            cases[name + tag] = {f"rec{k}.{f}": v for k, b in enumerate(h.bufs) for f, v in _record_units(b.numpy(), h.layout).items()}
            print(name + tag, "ok", flush=True)
    clips, K = _stills_clips()
    kw = dict(roi_border=(180, 140), refine="ba")
    for tag, more in (("", {}), ("_window", dict(refine_window=W4)), ("_window_plate", dict(refine_window=W4, refine_anchor="plate"))):
        c = clips[0]
        runs = {"run_sequence": lambda: [D.run_sequence(c["frames"], c["q"], K, times=c["times"], out=None, live=False, name=c["name"], **kw, **more)],
                "run_sequences": lambda: D.run_sequences([clips[0], clips[5]], K, sessions=1, **kw, **more),
                "run_queue": lambda: D.run_queue(clips, K, streams=3, sessions=1, **kw, **more)}
        for name, fn in runs.items():
            res = fn()
            cases[name + tag] = {f"clip{k}.{f}": v for k, r in enumerate(res) for f, v in
                                 dict(_dict_units(r["ba"]), ba_line=r["lines"][-1].encode().hex()).items()}
            print(name + tag, "ok", flush=True)
    with open(out_path, "w") as f:
        json.dump(dict(build=L.build_info(), cases=cases), f, default=str)


def sha(hexed):
    return hashlib.sha256(hexed.encode()).hexdigest()[:16]


def compare(pa, pb, head, out_path):
    runs = [json.load(open(p)) for p in (pa, pb, head)]
    a, b, h = (r["cases"] for r in runs)
    out = dict(what=__doc__.split("\n\n")[0].replace("\n", " "), parent_build=runs[0]["build"], head_build=runs[2]["build"], rtol=1e-12, cases={})
    bad = 0
    field = lambda unit: unit.split(".", 1)[1]
    unstable = sorted({field(u) for case in a for u in a[case] if a[case][u] != b[case][u]})  # fields that do not repeat in the parent itself
    out["fields_not_bit_repeatable_in_the_parent"] = unstable
    for case in a:
        assert a[case].keys() == b[case].keys() == h[case].keys(), case
        exact, loose = {}, {}
        for unit in a[case]:
            va, vb, vh = a[case][unit], b[case][unit], h[case][unit]
            if field(unit) not in unstable:  # repeats bit for bit in the parent: must be identical here
                exact[unit] = dict(parent=sha(va), head=sha(vh), equal=va == vh)
                bad += va != vh
            else:
                raw = [bytes.fromhex(v[3:] if v.startswith("f8:") else v) for v in (va, vb, vh)]
                xs = [np.frombuffer(r[: len(r) // 8 * 8], np.float64) for r in raw]  # (a unit of another type that does not repeat fails below: its bytes differ)
                pp, ph = (float(np.max(np.abs(x - xs[0]) / np.maximum(np.abs(xs[0]), 1e-300), initial=0.0)) if x.shape == xs[0].shape else None for x in xs[1:])
                ok = ph is not None and bool(np.allclose(xs[2], xs[0], rtol=1e-12, atol=0.0, equal_nan=True))
                loose[unit] = dict(parent_vs_parent_max_rel=pp, head_vs_parent_max_rel=ph, within_rtol=ok)
                bad += not ok
        fields = lambda units: sorted({field(u) for u in units})
        out["cases"][case] = dict(units=len(a[case]), bit_identical_fields=fields(exact), bit_identical=all(v["equal"] for v in exact.values()),
                                  rtol_fields=fields(loose), rtol_ok=all(v["within_rtol"] for v in loose.values()), exact=exact, loose=loose)
        print(f"{case}: {len(exact)} units bit-identical in the parent -> {'all equal here' if out['cases'][case]['bit_identical'] else 'DIFFER'}; "
              f"{len(loose)} compared at rtol 1e-12 ({', '.join(fields(loose)) or '-'}) -> {'ok' if out['cases'][case]['rtol_ok'] else 'OUTSIDE'}")
    out["differences"] = bad
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print("parity holds" if not bad else f"{bad} DIFFERENCES")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent", help="the parent commit's library (python -m velocity_amd._build --out=... in a checkout of the parent)")
    ap.add_argument("--out", default="profiles/refine_one_path/parity.json")
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
            print(f"refine_parity: run {k} failed ({r.returncode}): stopping")
            return 1
    return compare(*paths, a.out)


if __name__ == "__main__":
    sys.exit(main())
