"""Every output of the two one-image frame-0 entries, saved to one .npz, for comparing two builds of the library bit for bit (the build under test is
chosen through the VH_LIB override, velocity_amd/_lib.py):

  vh_good_features  on the full first frame of both stills sequences and on the 640 x 480 synthetic image, max_corners 300, 1000 and 3000;
  vh_frame0_init    on the five mixed 1024 x 768 clips of tests/test_gpu_frame0_batch.py (border 180 x 140) and on a 1920 x 1080 synthetic clip with
                    border 700 x 500: p, p3, vp, t, R, res, n, rois.

    python tools/exp/frame0_outputs.py --out A.npz;  VH_LIB=other.so python tools/exp/frame0_outputs.py --out B.npz
    python tools/exp/frame0_outputs.py --compare A.npz B.npz --json verdict.json
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def collect():
    import test_gpu_frame0_batch as T
    from frame0_batch_timing import plate_quad
    from velocity_amd import _lib as L
    from velocity_amd import synth

    torch = L.torch_cuda()
    stills = np.load(os.path.join(ROOT, "tests", "golden", "stills_gray.npz"))
    out = {"build_id": np.array(L.build_info()["build_id"])}
    images = dict(stills_a=stills["a_frames"][0], stills_b=stills["b_frames"][0],
                  synthetic=synth.render_frame(640, 480, synth.AffineMotion(640, 480), 0, seed=0x5EED).numpy())
    for name, img in images.items():
        h, w = img.shape
        t = torch.from_numpy(np.ascontiguousarray(img)).cuda()
        ws = L.Workspace(1, w, h, 64)
        for mc in (300, 1000, 3000):
            corners = torch.full((mc, 2), -7.0, dtype=torch.float32, device="cuda")
            cnt = torch.full((1,), -5, dtype=torch.int32, device="cuda")
            L.check(ws.lib.vh_good_features(ws.handle, L.dptr(t), w, h, w, mc, 0.01, 5, 0.04, L.dptr(corners), L.dptr(cnt), L.stream_ptr()), "vh_good_features")
            n = int(cnt.item())
            out[f"gf/{name}/{mc}/n"] = np.array(n)
            out[f"gf/{name}/{mc}/corners"] = corners[:n].cpu().numpy()
    K, clips = T._mixed_clips(stills)
    jobs = [(f"mixed{b}", f, q, K, T.BORDER) for b, (f, q) in enumerate(clips)]
    jobs.append(("synthetic_1080p", synth.render_frame(1920, 1080, synth.AffineMotion(1920, 1080), 0, seed=0xC0FFEE).numpy(), plate_quad(0), synth.K_1080P, (700, 500)))
    for name, f, q, Kc, border in jobs:
        one = T._single(f, q, Kc, border=border)
        n = one["n"]
        for key, val in one.items():
            out[f"f0/{name}/{key}"] = np.asarray(val)[:n] if key == "p" else np.asarray(val)  # rows of p beyond n are never written
    return out


def compare(a, b):
    A, B = np.load(a), np.load(b)
    keys = sorted(set(A.files) | set(B.files))
    differ = [k for k in keys if k != "build_id" and not (k in A.files and k in B.files and A[k].shape == B[k].shape and A[k].tobytes() == B[k].tobytes())]
    return dict(builds=[str(A["build_id"]), str(B["build_id"])], arrays=len(keys) - 1, differing=differ, bit_identical=not differ)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--json")
    a = ap.parse_args()
    if a.compare:
        v = compare(*a.compare)
        print(json.dumps(v))
        if a.json:
            with open(a.json, "w") as f:
                json.dump(v, f, indent=1)
        sys.exit(0 if v["bit_identical"] else 1)
    out = collect()
    np.savez(a.out, **out)
    print(f"{len(out) - 1} arrays from build {out['build_id']} -> {a.out}")


if __name__ == "__main__":
    main()
