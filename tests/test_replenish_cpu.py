"""The NumPy model of track replenishment (tests/replenish_ref.py) on the scenes of tests/replenish_scenes.py: what the option is for, its invariants,
the conditions on the scenes that let tests/test_gpu_replenish.py compare without exclusions, and the accuracy of the points it triangulates."""
import json
import os

import numpy as np

import replenish_scenes as RS
from oracle.session_oracle import SessionOracle
from replenish_ref import ReplenishOracle, birth_due, exclusion_mask
from velocity_amd.driver import Replenish

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_RUNS = {}


def _run(name):
    """One model run per scene and setting, shared by the tests (-> the oracle after its last frame, and n_cur after every step)."""
    if name not in _RUNS:
        seed, kw, rep, spare = {"main": (777, {}, RS.REP, RS.SPARE), "second": (1234, {}, RS.REP, RS.SPARE), "small": (4321, dict(w=480, h=270, n0=96), RS.REP, RS.SPARE),
                                "strict": (777, {}, RS.REP_STRICT, RS.SPARE), "few rows": (777, {}, RS.REP, 10), "plain": (777, {}, None, 0)}[name]
        sc = RS.scene(seed=seed, **kw)
        args = (sc["K"], sc["frames"][0], sc["p"], sc["p3"], sc["vp"], RS.T0)
        if rep is None:
            orc = SessionOracle(*args, nhist=RS.NHIST, msv_frame=RS.MSV_FRAME)
        else:
            orc = ReplenishOracle(*args, rep, RS.DET, spare=spare, nhist=RS.NHIST, msv_frame=RS.MSV_FRAME)
        n_cur, msv = [len(orc.p)], None
        for k in range(1, RS.NHIST):
            orc.step(sc["frames"][k], np.float32(k / 25.0), k)
            n_cur.append(len(orc.p))
            if k == RS.MSV_FRAME:
                msv = dict(ids=np.nonzero(orc.vg)[0], p3=orc.p3[orc.vg].copy())  # fcnMSV1_t's own points: p3[vg] = b0 - t
        _RUNS[name] = (orc, n_cur, msv, sc)
    return _RUNS[name]


def test_the_scene_loses_a_quarter_of_its_tracks_without_the_option():
    orc, n_cur, _, sc = _run("plain")
    assert n_cur[0] == len(sc["p"]) == 128 and n_cur[-1] <= 0.75 * n_cur[0], n_cur
    assert orc.S[-1, 2] == n_cur[-1]


def test_births_refill_to_the_target_ids_ascend_and_no_history_row_has_a_gap():
    for name in ("main", "second", "small"):
        orc, n_cur, _, sc = _run(name)
        n0 = len(sc["p"])
        assert len(orc.births) >= 3, name
        for b in orc.births:
            assert b["found"] >= b["entered"] == min(b["found"], orc.target - b["n_cur"], b["rows_left"]), (name, b)
            if b["rows_left"] >= orc.target - b["n_cur"] <= b["found"]:  # a birth that has rows left
                assert n_cur[b["frame"]] == orc.target == n0, (name, b)
            assert birth_due(b["frame"], RS.MSV_FRAME, RS.REP.every, RS.REP.baseline, RS.NHIST)
            assert orc.S[b["frame"], 2] == b["n_cur"]  # S keeps the count from before the birth
        ids = np.nonzero(orc.vg)[0]
        assert np.all(np.diff(ids) > 0) and len(ids) == len(orc.p) and ids.max() < orc.n_rows <= orc.N0
        seen = np.isfinite(orc.P[4])
        for g in range(orc.N0):
            fr = np.nonzero(seen[g])[0]
            if g >= orc.n_rows:
                assert len(fr) == 0 and orc.born[g] == -1
            else:
                assert fr[0] == orc.born[g] and np.array_equal(fr, np.arange(fr[0], fr[-1] + 1)), (name, g)  # one track per row, no gap
        assert not orc.vp[orc.tri == 0].any() and (orc.tri[orc.born == 0] == 1).all()
        # a newborn keeps min_distance from every track that was alive at its birth
        for b in orc.births:
            f = b["frame"]
            new = orc.P[0:2, orc.born == f, f].T
            old = orc.P[0:2, (orc.born < f) & (orc.born >= 0), f].T
            old = old[np.isfinite(old[:, 0])]
            d = np.abs(new[:, None, :] - old[None, :, :]).max(2)
            # (the integer corner lies outside the square around the ROUNDED track; cornerSubPix then moves it by at most its window's half-size)
            assert d.min() > RS.REP.min_distance - 0.5 - RS.DET.subpix[0], (name, f, d.min())


def test_rows_run_out():
    orc, n_cur, _, sc = _run("few rows")
    assert [b["entered"] for b in orc.births] == [10] and orc.n_rows == orc.N0 == len(sc["p"]) + 10 and n_cur[-1] < len(sc["p"])


def test_the_mask_is_a_square_around_every_rounded_track():
    m = exclusion_mask(np.float32([[10.5, 7.49], [2.0, 30.0]]), (3, 23, 2, 12), 2.5)  # rint(10.5) = 10 (half to even); the second track lies outside
    want = np.full((10, 20), 255, np.uint8)
    want[3:8, 5:10] = 0
    assert np.array_equal(m, want)
    assert (exclusion_mask(np.float32([[5, 5]]), (1, 11, 1, 11), 0.5) == 255).sum() == 99  # abs(d) < 0.5: the track's own pixel only


def test_no_gate_and_no_prefix_cut_of_the_scenes_is_a_near_tie():
    """What lets the GPU comparison run without exclusions: every newborn's largest reprojection error is at least 1e-3 pixels away from max_reproj, and
    the corner strengths on either side of every prefix cut differ.  (The strict gate of REP_STRICT sits inside the scene's noise-free errors of about
    0.01 pixels, where a margin of 1e-3 cannot exist; the device's error differs from the model's through the float32 translations B[:, 3:6], one ulp of
    which -- 2.4e-7 m at 3.6 m -- moves a reprojection by 5e-5 pixels at f = 700, so 2.5e-4 pixels is asked for there.)"""
    for name, margin in (("main", 1e-3), ("second", 1e-3), ("small", 1e-3), ("few rows", 1e-3), ("strict", 2.5e-4)):
        orc = _run(name)[0]
        err = np.array(list(orc.reproj.values()))
        assert len(err) > 0 and np.abs(err[np.isfinite(err)] - orc.rep.max_reproj).min() >= margin, (name, np.sort(err))
        for b in orc.births:
            m, s = b["entered"], b["strength"]
            assert np.all(np.diff(s) <= 0), name
            if 0 < m < len(s):
                assert s[m - 1] != s[m], (name, b["frame"])
    strict = _run("strict")[0]
    assert strict.counts["promoted"].sum() > 0 and strict.counts["rejected"].sum() > 0


def test_promoted_points_are_as_good_as_the_re_triangulation():
    """Truth: the analytic plane point of a promoted row's birth pixel, in the coordinates p3 lives in.  p3[g] + B[f, 3:6] is the point in camera f, so
    the truth of a row born at f is backproject(P[0:2, g, f]) at the plane's depth in camera f, minus the TRUE translation of camera f.  The yardstick
    is fcnMSV1_t's own error at the MSV frame of the same scene, measured the same way from the frame-0 pixels: the same number of views (baseline =
    msv_frame).  Both values go to profiles/replenish/truth.json."""
    orc, _, msv, sc = _run("main")
    m, K = sc["motion"], sc["K"].astype(np.float64)

    def truth(pix, f):
        depth = m.z0 + m.t(f)[2]
        xy = (pix.astype(np.float64) - K[2, 0:2]) / np.array([K[0, 0], K[1, 1]]) * depth
        return np.concatenate([xy, np.full((len(xy), 1), depth)], 1) - m.t(f)

    rows = np.nonzero((orc.born > 0) & (orc.tri == 1))[0]
    assert len(rows) >= 20
    e_new = np.array([np.linalg.norm(orc.p3[g] - truth(orc.P[0:2, g:g + 1, orc.born[g]].T, int(orc.born[g]))[0]) for g in rows])
    e_msv = np.linalg.norm(msv["p3"] - truth(orc.P[0:2, msv["ids"], 0].T, 0), axis=1)
    out = dict(scene="tests/replenish_scenes.py::scene()", promoted_rows=int(len(rows)), median_error_promoted_m=float(np.median(e_new)), msv_rows=int(len(msv["ids"])),
               median_error_msv_m=float(np.median(e_msv)), ratio=float(np.median(e_new) / np.median(e_msv)), bound=2.0,
               reason_for_bound="the same geometry and number of views, plus the tracker's pose error in the ray origins")
    path = os.path.join(ROOT, "profiles", "replenish", "truth.json")
    try:  # (a record for the reader; a read-only checkout still runs the assertion)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    except OSError:
        pass
    print(out)
    assert np.median(e_new) <= 2.0 * np.median(e_msv), out


def test_the_parameters_are_checked():
    import pytest

    assert Replenish().every == 5 and Replenish().baseline == 5 and Replenish().target is None and Replenish().max_new == 256
    assert Replenish().min_distance == 10.0 and Replenish().border == (0, 0) and Replenish().max_reproj == 1.0
    for bad in (dict(every=0), dict(baseline=0), dict(max_new=0), dict(max_new=2049), dict(target=0), dict(min_distance=float("nan"))):
        with pytest.raises(ValueError):
            Replenish(**bad)


def test_the_library_has_the_entries_and_every_default_is_off():
    import inspect

    from velocity_amd import _lib, driver

    lib = _lib.load()
    assert hasattr(lib, "vh_session_set_replenish") and hasattr(lib, "vh_session_replenish_state")
    for fn in (driver.TrackerSession.__init__, driver.run_sequence, driver.run_sequences, driver.run_queue):
        sig = inspect.signature(fn).parameters
        assert sig["replenish"].default is None and sig["spare"].default == 0, fn
