"""The model of bundle adjustment with anchored points (tests/anchor_ref.py): against oracle.ba_schur_step with no anchor, against the dense solve
with the anchors' columns zeroed, the scale it recovers from a mis-scaled start (and the free solve does not), padding, the session's packing with
anchors on hand-made histories, and the drivers' argument checks.  No GPU."""
import numpy as np
import pytest

import anchor_ref as AR
import refine_ref as RR
import refine_window_ref as RW
from oracle import nls_oracle as O
from velocity_amd import synth

SHAPES = [(24, 4, 700), (50, 6, 400), (24, 22, 701)]  # (nt, nf, seed): the matrix-core Gauss-Jordan, a C5-like window, the register Gauss-Jordan


def _packed(nt, nf, seed):
    K = synth.K_1080P.astype(float)
    z, bad, x0, nt, nc = O.ba_pack(K, *synth.ba_scene(nt, nf, seed=seed))
    return K, z, bad, x0, nt, nc


@pytest.mark.parametrize("nt,nf,seed", SHAPES)
def test_no_anchor_is_the_oracle_step_bit_for_bit(nt, nf, seed):
    K, z, bad, x0, nt, nc = _packed(nt, nf, seed)
    ed, ef = O.ba_schur_step(x0, z, K, nc, nt, bad=bad)
    for fixed in (None, np.zeros(nt, bool)):
        d, f = AR.anchored_step(x0, z, K, nc, nt, fixed=fixed, bad=bad)
        assert d.tobytes() == ed.tobytes() and f == ef


@pytest.mark.parametrize("nt,nf,seed", SHAPES)
def test_anchored_step_is_the_dense_solve_with_zeroed_columns(nt, nf, seed):
    """atol 1e-8: measured 9.9e-10 / 2.8e-10 / 7.7e-11 on these starts (steps of 0.4-1.6; 1.1e-10 at worst on the mis-scaled starts of the scale
    experiment): forward-difference cancellation, which moves with the scene, leaves a margin of 10 to 100."""
    K, z, bad, x0, nt, nc = _packed(nt, nf, seed)
    assert not bad.any()
    fixed = np.zeros(nt, bool)
    fixed[:4] = True
    d, _ = AR.anchored_step(x0, z, K, nc, nt, fixed=fixed)
    dense = AR.dense_step(x0, z, K, nc, nt, fixed)
    print(f"({nt}, {nf}, {seed}): max |schur - dense| = {np.abs(d - dense).max():.3g}, max |step| = {np.abs(d).max():.3g}")
    np.testing.assert_allclose(d, dense, rtol=0, atol=1e-8)
    assert np.all(d[:12] == 0.0) and np.all(dense[:12] == 0.0)
    assert np.abs(d[12: 3 * nt]).min() > 0.0  # every other point moves


@pytest.mark.parametrize("nt,nf,seed", SHAPES)
def test_anchors_recover_the_scale_and_the_free_solve_does_not(nt, nf, seed):
    """The start is the truth scaled by 1.08 except the four anchors.  Measured |last camera| / truth after 10 iterations: free 1.0676 / 1.0722 /
    1.0675, anchored 0.9962 / 0.9985 / 1.0006."""
    K, z, x0, nt, nc, fixed, truth = AR.scale_problem(nt, nf, seed)
    bad = np.zeros(z.size, bool)
    xf, _ = AR.solve_anchored(K, z, bad, x0, nt, nt, nc, fixed=None)
    xa, _ = AR.solve_anchored(K, z, bad, x0, nt, nt, nc, fixed=fixed)
    free, anch = AR.scale_ratio(xf, nt, nc, truth), AR.scale_ratio(xa, nt, nc, truth)
    print(f"({nt}, {nf}, {seed}): free {free:.4f}, anchored {anch:.4f}")
    assert abs(AR.scale_ratio(x0, nt, nc, truth) - 1.08) < 1e-12
    assert abs(anch - 1.0) <= 0.01
    assert free >= 1.05
    assert np.array_equal(xa[:12], x0[:12]) and not np.array_equal(xf[:12], x0[:12])


@pytest.mark.parametrize("nt,nf,pad", [(24, 4, 8), (17, 22, 7), (4, 6, 20)])
def test_a_padded_window_with_anchors_is_the_unpadded_one(nt, nf, pad):
    K, z, bad, x0, nt, nc = _packed(nt, nf, 60 + nt)
    fixed = np.zeros(nt, bool)
    fixed[:4] = True
    ex, etr = AR.solve_anchored(K, z, bad, x0, nt, nt, nc, fixed=fixed)
    zp, bp, xp0 = RR.pad_window(z, bad, x0, nt, nc, nt + pad)
    xp, tr = AR.solve_anchored(K, zp, bp, xp0, nt, nt + pad, nc, fixed=np.concatenate((fixed, np.zeros(pad, bool))))
    assert len(tr) == len(etr)
    assert np.array_equal(np.concatenate((xp[: 3 * nt], xp[3 * (nt + pad):])), ex)
    assert xp[3 * nt: 3 * (nt + pad)].tobytes() == xp0[3 * nt: 3 * (nt + pad)].tobytes()
    assert np.array_equal(xp[:12], x0[:12])
    np.testing.assert_allclose(tr, etr, rtol=1e-14)


def _history(nt=20, nf=8, seed=31):
    """A hand-made clip: track 1 dies after frame 4, track 2 after frame 2, tracks 0..3 all die before the last two frames' window [6, 8) except
    that nobody else does; B carries the truth's camera path and a clock."""
    P, pw0, cw0 = synth.ba_scene(nt, nf, seed=seed)
    P[:, 1, 5:] = np.nan
    P[:, 2, 3:] = np.nan
    P[:, 0, 7:] = np.nan
    P[:, 3, 6:] = np.nan
    B = np.zeros((nf, 14), np.float32)
    B[:, 3:6] = cw0
    B[:, 12] = np.arange(nf, dtype=np.float32) / np.float32(25.0)
    return synth.K_1080P, P, pw0, B


def test_packing_with_anchors_on_hand_made_histories():
    K, P, p3, B = _history()
    ids = np.array([0, 1, 2, 3])
    xyz = p3[ids] + np.array([[0.01, -0.02, 0.03]])  # not the session's points: the anchors' own coordinates must be the ones that start the solve
    anchors = (ids, xyz)
    # frames [0, 3): all four alive; the anchors come back as given, everything else moves
    a = AR.refine_window_anchored_ref(K, P, p3, B, 0, 3, anchors)
    assert a["nfix"] == 4 and np.array_equal(a["ids"][:4], ids) and np.array_equal(a["pw"][:4], xyz)
    free = RW.refine_window_ref(K, P, p3, B, 0, 3)
    assert np.array_equal(a["ids"], free["ids"]) and not np.array_equal(a["cw"], free["cw"])
    # frames [2, 5): first > 0 and track 2 is dead: three anchors, at xyz + B[2, 3:6] formed in double from the float32 record
    b = AR.refine_window_anchored_ref(K, P, p3, B, 2, 3, anchors)
    shift = B[2, 3:6].astype(np.float64)
    assert b["nfix"] == 3 and list(b["ids"][:3]) == [0, 1, 3] and b["first"] == 2
    assert np.array_equal(b["pw"][:3], xyz[[0, 1, 3]] + shift)
    # frames [6, 8): every anchored track is dead or dying: solved free, and says so -- equal to the model without anchors
    c = AR.refine_window_anchored_ref(K, P, p3, B, 6, 2, anchors)
    cf = RW.refine_window_ref(K, P, p3, B, 6, 2)
    assert c["nfix"] == 0 and not set(c["ids"]) & set(ids)
    for key in cf:
        assert np.array_equal(np.asarray(c[key]), np.asarray(cf[key]), equal_nan=True), key
    # the whole clip (8 frames): no anchored track survives it
    w = AR.refine_anchored_ref(K, P, p3, B, 8, anchors)
    wf = RR.refine_ref(K, P, p3, B, 8)
    assert w["nfix"] == 0 and np.array_equal(w["cw"], wf["cw"]) and np.array_equal(w["pw"], wf["pw"])
    # ... and of a clip cut to 3 frames: all four, coordinates replaced, no shift (B[0, 3:6] = 0)
    w3 = AR.refine_anchored_ref(K, P, p3, B, 3, anchors)
    assert w3["nfix"] == 4 and np.array_equal(w3["pw"][:4], xyz) and np.array_equal(w3["cw"], a["cw"])
    # no anchors: the models of refine_ref / refine_window_ref, bit for bit
    n0 = AR.refine_window_anchored_ref(K, P, p3, B, 2, 3, None)
    f0 = RW.refine_window_ref(K, P, p3, B, 2, 3)
    assert n0.pop("nfix") == 0 and all(np.array_equal(np.asarray(n0[k]), np.asarray(f0[k]), equal_nan=True) for k in f0)


def test_pack_windows_filters_the_mask_like_the_tracks():
    from velocity_amd.NLS import pack_windows

    scenes = []
    for w, n in enumerate([24, 17, 4, 0]):
        P, pw0, cw0 = synth.ba_scene(24, 4, seed=80 + w)
        P[:, n:, 2:] = np.nan
        scenes.append((P, pw0, cw0))
    plain = pack_windows(*zip(*scenes))
    assert len(plain) == 5  # no mask: what it always returned
    first4 = np.zeros(24, bool)
    first4[:4] = True
    last = np.zeros(24, bool)
    last[20:] = True  # rows the filter of window 1 drops
    z, x0, cnt, nt, nc, fx = pack_windows(*zip(*scenes), fixed=[first4, first4 | last, np.ones(24, bool), None])
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip((z, x0, cnt), plain[:3])) and (nt, nc) == plain[3:]
    assert fx.dtype == np.uint8 and fx.shape == (4, 24)
    assert fx[0].tolist() == [1] * 4 + [0] * 20 and fx[1].tolist() == [1] * 4 + [0] * 20 and fx[2].tolist() == [1] * 4 + [0] * 20 and not fx[3].any()
    with pytest.raises(ValueError, match="bool mask"):
        pack_windows(*zip(*scenes), fixed=[np.zeros(23, bool)] * 4)
    with pytest.raises(ValueError, match="masks for 4 windows"):
        pack_windows(*zip(*scenes), fixed=[first4])


def test_refine_anchor_is_checked_before_anything_runs():
    from velocity_amd.driver import _check_refine, run_queue, run_sequence, run_sequences

    assert _check_refine("ba", None, None, "plate") == (True, None, None) and _check_refine("ba", 8, None, "plate") == (True, 8, 7)
    assert _check_refine(None) == (False, None, None) and _check_refine("ba", 8, 3) == (True, 8, 3)
    for call in (lambda: run_sequence([None, None], None, None, fps=25.0, refine_anchor="plate"), lambda: run_sequences([], None, refine_anchor="plate"),
                 lambda: run_queue([], None, 2, refine_anchor="plate")):
        with pytest.raises(ValueError, match="refine_anchor needs refine='ba'"):
            call()
    for call in (lambda: run_sequence([None, None], None, None, fps=25.0, refine="ba", refine_anchor="corners"),
                 lambda: run_sequences([], None, refine="ba", refine_anchor=True), lambda: run_queue([], None, 2, refine="ba", refine_anchor=[0, 1, 2, 3])):
        with pytest.raises(ValueError, match="refine_anchor must be None or 'plate'"):
            call()


def test_merge_and_lines_carry_nfix():
    from velocity_amd.driver import _merged_ba, _tag_anchor, ba_line, merge_window_speeds

    nan = np.nan
    wins = [dict(first=0, speed=np.array([nan, 10.0, 12.0]), nt=30, nfix=4, iterations=10, converged=0, f_last=0.5),
            dict(first=2, speed=np.array([nan, 20.0, 22.0]), nt=25, nfix=0, iterations=7, converged=1, f_last=0.75)]
    m = merge_window_speeds(5, wins)
    assert m["nfix"].tolist() == [4, 0] and m["nfix"].dtype == np.int64
    assert merge_window_speeds(5, [{k: v for k, v in w.items() if k != "nfix"} for w in wins])["nfix"].tolist() == [0, 0]
    ba = _merged_ba(5, wins, 3, 2)
    assert ba_line(ba) == "BA speed = 16.00 +/- 5.10 km/h (2 windows of 3 frames, 25-30 tracks, f = 0.750 pixels)"  # not asked for: the line it was
    assert ba_line(_tag_anchor(ba, "plate")) == "BA speed = 16.00 +/- 5.10 km/h (2 windows of 3 frames, 25-30 tracks, 0-4 anchors, f = 0.750 pixels)"
    whole = dict(nt=2, nfix=4, speed_mean=40.456, speed_std=1.0049, f_last=0.08449, iterations=10, converged=0)
    assert ba_line(whole) == "BA speed = 40.46 +/- 1.00 km/h (2 tracks, f = 0.084 pixels)"
    assert ba_line(_tag_anchor(whole, "plate")) == "BA speed = 40.46 +/- 1.00 km/h (2 tracks, 4 anchors, f = 0.084 pixels)"
    assert _tag_anchor(whole, None) is whole and _tag_anchor(None, "plate") is None


def test_the_anchor_entry_points_are_declared_and_bound():
    from velocity_amd import _lib as L

    declared = L.declared_symbols()
    for s in ("vh_nls_batch_windows_fixed", "vh_session_set_anchors", "vh_session_anchors"):
        assert s in declared and s in L._SIGS and hasattr(L.load(), s), s
    assert len(L._SIGS["vh_nls_batch_windows_fixed"][1]) == len(L._SIGS["vh_nls_batch_windows"][1]) + 1
    # no older member of either struct of offsets changed place: nfix is the last member of the one and the last offset of the other
    assert [n for n, _ in L.RefineRecord._fields_][-4:] == ["n0", "nhist", "max_iter", "nfix"]
    assert [n for n, _ in L.RefineWindowRecord._fields_][-6:] == ["pw", "nfix", "n0", "nf", "max_iter", "with_points"]
