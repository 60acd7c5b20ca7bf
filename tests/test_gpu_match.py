"""Recovery by feature matching on the MI355X: vh_match_affine against its NumPy model (tests/match_ref.py) bit for bit -- every stage is integer or already
pinned bit-exact against its checker (remap, detector, RANSAC) -- then the shim, the torch op, KLTmain(fallback=True) and the drop-in loop built on it."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import match_ref as MR  # noqa: E402
from oracle import driver_oracle as DO  # noqa: E402 (checker only)
from oracle import klt_oracle as KO  # noqa: E402 (checker only)
from scenes import load_stills as stills  # noqa: E402
from velocity_amd import synth  # noqa: E402

W, H = 960, 540
SYNTH = {"shift200": (1.0, 0, 200, 0), "shrink": (0.75, 2, 120, -40), "grow": (1.3, -3, -90, 60)}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (im1, im2, p1, truth at p1 or None)."""
    if name in ("a", "b"):
        st = stills()
        fr = st[f"{name}_frames"]
        border = (233, 167) if name == "a" else (180, 140)
        return fr[0], fr[1], DO.frame0(fr[0], st[f"{name}_q"], st[f"{name}_K"], roi_border=border)["p"], None
    s, th, tx, ty = SYNTH[name]
    m = synth.AffineMotion(W, H, s=s, theta_deg=th, tx=tx, ty=ty)
    g = synth.grid_tracks(300, W, H, frac=0.5)
    A = m.matrix(1)
    return synth.render_frame(W, H, m, 0).numpy(), synth.render_frame(W, H, m, 1).numpy(), g, g.astype(np.float64) @ A[:, :2].T + A[:, 2]


@functools.lru_cache(maxsize=None)
def model(name):
    a, b, p, _ = case(name)
    return MR.match_affine(a, b, p)


def c_entry(a, b, p, **params):
    """vh_match_affine through ctypes -> host copies of (M [2,3], inl [cap], pairs [cap,4], info [4])."""
    from velocity_amd import KLT

    M, inl, pairs, info = KLT._match_call(a, b, p, params)
    return M.cpu().numpy().reshape(2, 3), inl.cpu().numpy(), pairs.cpu().numpy(), info.cpu().numpy()


@pytest.mark.parametrize("name", ["a", "b", "shift200", "shrink", "grow"])
def test_match_affine_equals_the_model_bit_for_bit(name):
    from velocity_amd import KLT

    a, b, p, _ = case(name)
    ref = model(name)
    M, inl, pairs, info = c_entry(a, b, p)
    S = KLT.match_stages()
    print(name, "info", info, "model", ref["info"])
    assert tuple(S["roi"]) == tuple(ref["box"])
    for l in range(5):
        assert S["dims"][l] == MR.level_dims(a.shape[1], a.shape[0], l)
    for i, f in enumerate((ref["q"], ref["t"])):
        for l in range(5):
            assert np.array_equal(S["kp"][i][l], f["kp"][l]), (name, "keypoints", i, l)
        assert np.array_equal(S["pos"][i], f["pos"]), (name, "positions", i)
        assert np.array_equal(S["desc"][i], f["desc"]), (name, "descriptors", i)
    assert np.array_equal(S["nn"], ref["nn"]), (name, "nearest / second nearest")
    assert np.array_equal(S["good"].astype(bool), ref["good"])
    ng = int(ref["info"][1])
    assert np.array_equal(info, ref["info"])
    assert np.array_equal(pairs[:ng], ref["pairs"]) and not pairs[ng:].any()
    assert np.array_equal(inl[:ng], ref["inl"]) and not inl[ng:].any()
    assert ref["M"] is not None and np.array_equal(M, ref["M"]), (M, ref["M"])


def test_failures_are_reported_like_the_model_reports_them():
    from velocity_amd import KLT, _lib as L

    a, b, p, _ = case("a")
    ref = model("a")
    ng = int(ref["info"][1])
    M, inl, pairs, info = c_entry(a, b, p, min_good=ng + 1)
    assert tuple(info) == (0, ng, 0, int(ref["info"][3])) and not M.any() and not inl.any() and np.array_equal(pairs[:ng], ref["pairs"])
    T, i2 = KLT.estimateAffine2D_SURF(a, b, p, min_good=ng + 1)
    assert T is None and i2.shape == (ng, 1) and not i2.any()
    flat = np.full((H, W), 117, np.uint8)
    g = case("shift200")[2]
    M, inl, pairs, info = c_entry(flat, flat, g)
    assert tuple(info) == (0, 0, 0, 0) and not M.any()
    assert KLT.estimateAffine2D_SURF(flat, flat, g)[0] is None
    # two unrelated frames: whatever the model returns
    x = case("shift200")[0]
    other = synth.render_frame(W, H, synth.AffineMotion(W, H), 0, seed=0xBEEF).numpy()
    ref = MR.match_affine(x, other, g)
    M, inl, pairs, info = c_entry(x, other, g)
    assert np.array_equal(info, ref["info"]) and np.array_equal(inl[: info[1]], ref["inl"])
    assert (ref["M"] is None and not M.any()) or np.array_equal(M, ref["M"])
    # bad arguments: -1 before anything is queued
    import torch

    ws = L.workspace(W, H, 2500)
    im = torch.from_numpy(x).cuda()
    pt = torch.from_numpy(g).cuda()
    out = [torch.zeros(6, dtype=torch.float64, device="cuda"), torch.zeros(2500, dtype=torch.uint8, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")]
    before = ws.lib.vh_match_launch_count()

    def call(n, mp):
        return ws.lib.vh_match_affine(ws.handle, L.dptr(im), L.dptr(im), W, H, W, W, L.dptr(pt), n, C.byref(mp) if mp else None, L.dptr(out[0]), L.dptr(out[1]),
                                      None, L.dptr(out[2]), L.stream_ptr())

    assert call(0, None) == -1
    for bad in (dict(levels=0), dict(levels=9), dict(query_per_level=0), dict(train_per_level=4096), dict(ratio_den=0), dict(quality=0.0), dict(min_good=-1)):
        assert call(len(g), L.match_params(bad)) == -1, bad
    assert ws.lib.vh_match_launch_count() == before


def test_a_reserved_context_of_its_own_gives_the_same_result():
    """vh_match_reserve sizes the scratch of a fresh context (what a caller does ahead of a stream capture); the call on it then equals the default one,
    launched plainly and replayed from a captured graph."""
    import torch

    from velocity_amd import _lib as L

    a, b, p, _ = case("shrink")
    ref = model("shrink")
    ws = L.Workspace(1, W, H, 2500)
    assert ws.lib.vh_match_reserve(ws.handle, W, H, None, L.stream_ptr()) == 0
    assert ws.lib.vh_match_reserve(ws.handle, W, H, C.byref(L.match_params(dict(levels=0))), L.stream_ptr()) == -1
    st = L.MatchStages()
    assert ws.lib.vh_match_stage_ptrs(ws.handle, C.byref(st)) == -1, "no call on this context yet"
    im1, im2, pt = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(p).cuda()
    M, inl, info = torch.zeros(6, dtype=torch.float64, device="cuda"), torch.zeros(2500, dtype=torch.uint8, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    for _ in range(2):  # the second call reuses everything
        L.check(ws.lib.vh_match_affine(ws.handle, L.dptr(im1), L.dptr(im2), W, H, W, W, L.dptr(pt), len(p), None, L.dptr(M), L.dptr(inl), None, L.dptr(info),
                                       L.stream_ptr()), "vh_match_affine")
        assert np.array_equal(info.cpu().numpy(), ref["info"]) and np.array_equal(M.cpu().numpy().reshape(2, 3), ref["M"])
        assert np.array_equal(inl.cpu().numpy()[: ref["info"][1]], ref["inl"])
    # with the scratch in place a call only queues work: it can be captured and replayed
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = ws.lib.vh_match_affine(ws.handle, L.dptr(im1), L.dptr(im2), W, H, W, W, L.dptr(pt), len(p), None, L.dptr(M), L.dptr(inl), None, L.dptr(info),
                                    L.stream_ptr())
    assert rc == 0, ws.lib.vh_last_error()
    for _ in range(2):
        M.fill_(3)
        inl.fill_(3)
        info.fill_(3)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(info.cpu().numpy(), ref["info"]) and np.array_equal(M.cpu().numpy().reshape(2, 3), ref["M"])
        assert np.array_equal(inl.cpu().numpy()[: ref["info"][1]], ref["inl"]) and not inl.cpu().numpy()[ref["info"][1]:].any()
    del g
    # a context too small for the query budget is refused
    small = L.Workspace(1, W, H, 1000)
    assert small.lib.vh_match_affine(small.handle, L.dptr(im1), L.dptr(im2), W, H, W, W, L.dptr(pt), len(p), None, L.dptr(M), L.dptr(inl), None, L.dptr(info),
                                     L.stream_ptr()) == -1


def test_shim_and_torch_op_return_what_the_c_entry_returns():
    import torch

    import velocity_amd.torch_ops  # noqa: F401
    from velocity_amd import KLT

    for name in ("a", "shift200"):
        a, b, p, _ = case(name)
        M, inl, pairs, info = c_entry(a, b, p)
        ng = int(info[1])
        T, i2 = KLT.estimateAffine2D_SURF(a, b, p)
        assert T.dtype == np.float64 and T.shape == (2, 3) and np.array_equal(T, M)
        assert i2.dtype == np.uint8 and i2.shape == (ng, 1) and np.array_equal(i2.ravel(), inl[:ng])
        Mt, it, nt = torch.ops.velocity_hip.match_affine(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(p).cuda())
        assert np.array_equal(Mt.cpu().numpy(), M) and np.array_equal(it.cpu().numpy(), inl) and np.array_equal(nt.cpu().numpy(), info)
    a, b, g, truth = case("shift200")
    T, i2 = KLT.estimateAffine2D_SURF(a, b, g, scale=0.5)
    Tm, im_ = MR.estimate_affine_surf(a, b, g, scale=0.5)
    assert np.array_equal(T, Tm) and np.array_equal(i2, im_)
    assert np.abs(g.astype(np.float64) @ T[:, :2].T + T[:, 2] - truth).max() <= 2.0


@pytest.mark.parametrize("name", ["a", "shift200"])
def test_kltmain_with_fallback_runs_the_fine_stage_with_the_matched_affine(name):
    from velocity_amd import KLT

    a, b, p0, _ = case(name)
    today = KLT.KLTmain(b, a, None, p0, return_all=True)
    off = KLT.KLTmain(b, a, None, p0, fallback=False, return_all=True)
    assert off[4] == today[4] and off[4] & 1 and not off[4] & 6
    for x, y in zip(today[:4], off[:4]):
        assert np.array_equal(x, y)
    if name == "a":
        assert today[1].sum() == 0
    p, v, small, p_all, flags = KLT.KLTmain(b, a, None, p0, fallback=True, return_all=True)
    assert flags & 7 == 7, "coarse-affine failure, the recovery ran, it found a model"
    ep, ev, _, _ = KO.klt_regional(a, b, p0, model(name)["M"].T, KO.LK_FINE, fbt=0.3)
    print(name, "tracks kept with the fallback:", int(v.sum()), "of", len(p0))
    assert np.array_equal(v, ev) and np.array_equal(p, ep[ev]) and np.array_equal(p_all[ev], ep[ev])
    assert np.array_equal(small, today[2])
    assert v.sum() >= (90 if name == "a" else 270)


def test_kltmain_fallback_changes_nothing_where_the_tracker_succeeds():
    from velocity_amd import KLT, _lib as L

    a, b, p0, _ = case("b")
    before = L.load().vh_match_launch_count()
    today = KLT.KLTmain(b, a, None, p0, return_all=True)
    got = KLT.KLTmain(b, a, None, p0, fallback=True, return_all=True)
    assert L.load().vh_match_launch_count() == before, "the recovery must not run when the coarse stage succeeds"
    assert got[4] == today[4] and not got[4] & 7 and today[1].sum() > 50
    for x, y in zip(today[:4], got[:4]):
        assert np.array_equal(x, y)


def test_a_default_kltmain_call_queues_no_kernel_of_the_matcher():
    from velocity_amd import KLT, _lib as L

    a, b, p0, _ = case("a")
    lib = L.load()
    before = lib.vh_match_launch_count()
    p, v, _ = KLT.KLTmain(b, a, None, p0)  # the failing pair, option off
    assert v.sum() == 0 and lib.vh_match_launch_count() == before
    KLT.KLTmain(b, a, None, p0, fallback=True)
    assert lib.vh_match_launch_count() == before + 6  # mask, box sums, descriptors, matching, compaction, info: one launch each


def test_drop_in_loop_with_fallback_measures_the_labelled_speed_on_stills_a(monkeypatch):
    """Sequence A through run_sequence_dropin(fallback=True) against the oracle driver whose klt_main is wrapped with the same recovery (the model +
    klt_regional): without the fallback the clip loses every track at frame 1 and reports no speed; the reference labels it 40 km/h."""
    from _helpers import same_table
    from tools.dropin_loop import run_sequence_dropin

    st = stills()
    frames, times, q, K = st["a_frames"], st["a_times"], st["a_q"], st["a_K"]
    real = KO.klt_main
    ran = []

    def klt_main_recovering(im, im0, im0_small, p0, lk_coarse=None, lk_fine=None, stages=False, L=None):
        p, v, small, S = real(im, im0, im0_small, p0, lk_coarse=lk_coarse, lk_fine=lk_fine, stages=True, L=L)
        if S["flags"] & 1 and len(p0):
            ran.append(len(p0))
            rec = MR.recover(im0, im, p0)
            if rec is not None:
                p_all, v = rec[0], rec[1]
                p = p_all[v]
        return (p, v, small, S) if stages else (p, v, small)

    monkeypatch.setattr(KO, "klt_main", klt_main_recovering)
    with np.errstate(all="ignore"):
        ref = DO.run_sequence(frames, q, K, times, roi_border=(233, 167))
    monkeypatch.setattr(KO, "klt_main", real)
    got = run_sequence_dropin(frames, q, K, times=times, roi_border=(233, 167), clock=lambda: 0.0, out=None, fallback=True)
    print("\n".join(got["lines"]))
    print("the oracle's recovery ran", len(ran), "time(s); tracks alive per frame:", got["S"][:, 2])
    assert len(ran) == 1, "the fallback runs once; frames 2 and 3 track normally"
    assert np.array_equal(got["S"][:, 2], ref["S"][:, 2]) and got["S"][1:, 2].min() >= 90
    assert np.array_equal(got["vg"], ref["vg"]) and np.array_equal(got["vp"], ref["vp"]) and np.array_equal(got["p"], ref["p"])
    for r in (0, 1, 4):
        assert np.array_equal(got["P"][r], ref["P"][r], equal_nan=True)
    np.testing.assert_allclose(got["B"], ref["B"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(got["S"][1:, [0, 2, 4, 5]], ref["S"][1:, [0, 2, 4, 5]], rtol=0, atol=0)
    np.testing.assert_allclose(got["S"][1:, [3, 6, 7, 8]], ref["S"][1:, [3, 6, 7, 8]], rtol=1e-4)
    same_table(got["lines"][:-1], ref["lines"])
    speed = got["S"][1:, 8]
    assert np.all((speed > 33) & (speed < 46)), speed
