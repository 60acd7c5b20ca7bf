"""What the two one-image frame-0 entries cost on the device: vh_frame0_init at 1920 x 1080 with roi_border (700, 500) and 1000 corners (the clip of
tools/exp/frame0_batch_timing.py) and vh_good_features on the full 1920 x 1080 frame with 1000 corners.  HIP events around one call, warmed up, median
of 30.  The library is chosen through the VH_LIB override; to compare builds on one box, run this once per build, alternating, several rounds:
the spread between rounds of the same build is the noise a difference has to exceed.

    python tools/exp/frame0_entry_timing.py            -> one JSON line
"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from frame0_batch_timing import BORDER, MC, SETTINGS, SUBPIX, H, W, plate_quad  # noqa: E402
from velocity_amd import _lib as L  # noqa: E402
from velocity_amd import synth  # noqa: E402

REPS, WARMUP = 30, 5


def timed(torch, fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), reps=REPS)


def main():
    torch = L.torch_cuda()
    f = synth.render_frame(W, H, synth.AffineMotion(W, H), 0, seed=0xC0FFEE, device="cuda").contiguous()
    ws = L.Workspace(1, W, H, SETTINGS.cap)
    lib = ws.lib
    q = np.ascontiguousarray(plate_quad(0))
    K64 = L.host_K(synth.K_1080P)
    plate = SETTINGS.plate_w
    p, p3, vp, t0, R0, res0, n0 = (x[0] for x in SETTINGS.outputs(1))
    rois = (C.c_int * 8)()
    win, it, eps = SUBPIX
    corners = torch.zeros((MC, 2), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")

    def frame0():
        L.check(lib.vh_frame0_init(ws.handle, L.dptr(f), W, H, W, q.ctypes.data_as(L.f32p), K64.ctypes.data_as(L.f64p), plate.ctypes.data_as(L.f64p), BORDER[0],
                                   BORDER[1], MC, 0.01, 5, 0.04, win, it, eps, L.dptr(p), L.dptr(p3), L.dptr(vp), L.dptr(t0), L.dptr(R0), L.dptr(res0), L.dptr(n0),
                                   rois, L.stream_ptr()), "vh_frame0_init")

    def features():
        L.check(lib.vh_good_features(ws.handle, L.dptr(f), W, H, W, MC, 0.01, 5, 0.04, L.dptr(corners), L.dptr(cnt), L.stream_ptr()), "vh_good_features")

    row = dict(build_id=L.build_info()["build_id"], device=torch.cuda.get_device_name(0), vh_frame0_init=timed(torch, frame0),
               vh_good_features=timed(torch, features), n_frame0=int(n0.item()), n_features=int(cnt.item()))
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
