"""The NumPy model of the recovery by feature matching (tests/match_ref.py: the definition vh_match_affine is held to on the GPU, tests/test_gpu_match.py)
on its own: does the algorithm recover the motions the tracker loses?  Plus the CPU-side checks of the new boundary (pair table, struct size, version)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import match_ref as MR
from oracle import driver_oracle as DO
from oracle import klt_oracle as KO
from scenes import load_stills as stills
from velocity_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 960, 540


@functools.lru_cache(maxsize=None)
def stills_a():
    """Frames 0 and 1 of sequence A, the driver oracle's frame-0 tracks, the model's result."""
    st = stills()
    fr = st["a_frames"]
    p0 = DO.frame0(fr[0], st["a_q"], st["a_K"], roi_border=(233, 167))["p"]
    return fr[0], fr[1], p0, MR.match_affine(fr[0], fr[1], p0)


@functools.lru_cache(maxsize=None)
def synthetic(s, theta, tx, ty):
    m = synth.AffineMotion(W, H, s=s, theta_deg=theta, tx=tx, ty=ty)
    a, b = synth.render_frame(W, H, m, 0).numpy(), synth.render_frame(W, H, m, 1).numpy()
    g = synth.grid_tracks(300, W, H, frac=0.5)
    A = m.matrix(1)
    return a, b, g, g.astype(np.float64) @ A[:, :2].T + A[:, 2], MR.match_affine(a, b, g)


def _err(M, g, truth):
    return float(np.abs(g.astype(np.float64) @ M[:, :2].T + M[:, 2] - truth).max())


def test_model_recovers_the_motion_of_stills_a():
    """Sequence A, frame 0 -> 1 (the car moves ~200 px and shrinks to 0.73x; KLTmain loses all 149 tracks).  The model reaches: 1374 query and 4925 train
    keypoints, 222 good matches, 154 RANSAC inliers, sqrt(det) = 0.7333; the fine stage with its affine keeps 114 of 149 tracks, all four plate corners."""
    f0, f1, p0, r = stills_a()
    assert len(p0) == 149
    print("stills A:", r["info"], r["M"])
    assert r["M"] is not None and r["status"] == 1
    assert r["info"][2] >= 60
    assert 0.68 <= np.sqrt(np.linalg.det(r["M"][:, :2])) <= 0.78
    p, v, _, _ = KO.klt_regional(f0, f1, p0, r["M"].T, KO.LK_FINE, 0.3)
    print("fine stage keeps", int(v.sum()))
    assert v.sum() >= 90 and v[:4].all()


def test_model_recovers_a_200_px_shift_the_tracker_loses():
    """960 x 540, pure shift of 200 px, 300 grid tracks: klt_main sets flag bit 0 and keeps 2 tracks; the model (2129 good matches, 2099 inliers) is within
    0.059 px of the truth at the tracks, and the fine stage with it keeps 300 of 300 within 0.017 px."""
    a, b, g, truth, r = synthetic(1.0, 0, 200, 0)
    _, ev, _, S = KO.klt_main(b, a, None, g, stages=True)
    assert S["flags"] & 1 and ev.sum() <= 10
    assert r["M"] is not None
    e = _err(r["M"], g, truth)
    print("200 px shift:", r["info"], "max error", e)
    assert e <= 1.0
    p, v, _, _ = KO.klt_regional(a, b, g, r["M"].T, KO.LK_FINE, 0.3)
    assert v.sum() >= 270
    assert np.abs(p[v] - truth[v]).max() <= 0.1


@pytest.mark.parametrize("s,theta,tx,ty", [(0.75, 2, 120, -40), (1.3, -3, -90, 60)])
def test_model_recovers_scale_and_rotation(s, theta, tx, ty):
    """The model's affine at the tracks: 0.050 px from the truth for (0.75, 2 deg, 120, -40), 0.302 px for (1.3, -3 deg, -90, 60)."""
    a, b, g, truth, r = synthetic(s, theta, tx, ty)
    assert r["M"] is not None
    e = _err(r["M"], g, truth)
    print((s, theta, tx, ty), r["info"], "max error", e)
    assert e <= 1.0


def test_model_at_half_scale_stays_within_two_pixels():
    """estimateAffine2D_SURF(..., scale=0.5) on the 200-px pair (the bound the GPU test holds the shim to): the model is 0.101 px off."""
    a, b, g, truth, _ = synthetic(1.0, 0, 200, 0)
    M, inl = MR.estimate_affine_surf(a, b, g, scale=0.5)
    assert M is not None and inl.shape[1] == 1
    assert _err(M, g, truth) <= 2.0


def test_failure_is_reported_not_raised():
    a, b, g, _, _ = synthetic(1.0, 0, 200, 0)
    flat = np.full((H, W), 117, np.uint8)
    r = MR.match_affine(flat, flat, g)
    assert r["status"] == 0 and r["M"] is None and tuple(r["info"]) == (0, 0, 0, 0)
    assert MR.estimate_affine_surf(flat, flat, g)[0] is None
    # fewer than min_good good matches: stills A reaches 222
    f0, f1, p0, ra = stills_a()
    few = MR.match_affine(f0, f1, p0, min_good=int(ra["info"][1]) + 1)
    assert few["status"] == 0 and few["M"] is None and few["info"][1] == ra["info"][1] and few["info"][2] == 0 and not few["inl"].any()
    assert MR.estimate_affine_surf(f0, f1, p0, min_good=int(ra["info"][1]) + 1)[0] is None
    # two unrelated frames: whatever comes back, nothing raises
    other = synth.render_frame(W, H, synth.AffineMotion(W, H), 0, seed=0xBEEF).numpy()
    r = MR.match_affine(a, other, g)
    assert r["status"] in (0, 1) and len(r["inl"]) == r["info"][1]


def test_no_tracks_is_an_error_at_the_c_entry_and_none_from_the_shim():
    from velocity_amd import KLT

    L = _lib.load()
    assert L.vh_match_affine(None, None, None, 64, 64, 64, 64, None, 0, None, None, None, None, None, None) == -1
    T, inl = KLT.estimateAffine2D_SURF(np.zeros((64, 64), np.uint8), np.zeros((64, 64), np.uint8), np.zeros((0, 2), np.float32))
    assert T is None and inl.shape == (0, 1)


def test_the_kernel_and_the_model_read_one_pair_table():
    L = _lib.load()
    assert L.vh_version() >= 108
    got = np.zeros((256, 4), np.int32)
    assert L.vh_match_pairs(got.ctypes.data_as(_lib.i32p)) == 0
    model = MR.pair_table()
    assert model.shape == (256, 4) and np.array_equal(got, model)
    assert np.abs(model).max() <= 13
    assert not ((model[:, 0] == model[:, 2]) & (model[:, 1] == model[:, 3])).any(), "a pair that compares a pixel with itself carries no information"


def test_match_structs_have_the_size_of_the_c_structs(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "velocity_hip.h"\nint main(void) { printf("%zu %zu\\n", sizeof(vh_match_params), sizeof(vh_match_stages)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    a, b = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert (a, b) == (C.sizeof(_lib.MatchParams), C.sizeof(_lib.MatchStages))
    d = _lib.match_params()
    assert (d.levels, d.query_per_level, d.train_per_level, d.block, d.border_x, d.border_y, d.ratio_num, d.ratio_den, d.min_good, d.quality) == (
        5, 500, 1000, 5, 50, 50, 4, 5, 10, 0.01)
    assert dict(MR.DEFAULTS) == dict(_lib.MATCH_DEFAULTS)
    with pytest.raises(TypeError):
        _lib.match_params(dict(levles=3))


def test_fallback_is_off_by_default_everywhere():
    import inspect

    from tools import dropin_loop
    from velocity_amd import KLT

    assert inspect.signature(KLT.KLTmain).parameters["fallback"].default is False
    assert inspect.signature(dropin_loop.run_sequence_dropin).parameters["fallback"].default is False
    assert inspect.signature(dropin_loop.DropinLoop.__init__).parameters["fallback"].default is False
    assert list(inspect.signature(KLT.estimateAffine2D_SURF).parameters)[:4] == ["im1", "im2", "p1", "scale"]  # utils/KLT.py:10
