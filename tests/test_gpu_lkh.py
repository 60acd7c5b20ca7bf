"""k_lk_h<15> (route 9): sixteen tracks per wavefront, four lanes per track, four window rows per lane.

Held bit for bit -- position, status, err (and fbe where it is asked for) -- against the CPU oracle, the generic k_lk (route 1) and k_lk_o (route 8).
What can go wrong in this kernel and nowhere else: a quad reading its neighbour quad through DPP (lane 3's dummy row), partial wavefronts and a last
quad group that is not full, tracks of one wavefront leaving the Newton loop at different iterations, the byte phase of the row loads with six / four
rows per lane, and the int32 partial sums of a lane that now holds 60 samples (0.93 of 2^31 at worst-case contrast).  The shapes are those of
tests/test_gpu_lko_alignment.py: 96 x 80 images taken as views with base phase 0..3 and rows 132..135 bytes apart, three levels, 64 tracks of which
24 touch or cross an edge or a corner."""
import numpy as np
import pytest

import lk_ref as R
from lk_support import assert_same_bits as _assert_same
from lk_support import SMALL, bits, pyr_lk_forced, small, strided_view, texture_pair, to_dev  # noqa: F401 (small: a fixture)
from oracle import klt_oracle as KO  # (checker only)
from oracle.session_oracle import SessionOracle  # (checker only)
from velocity_amd import synth

pytestmark = pytest.mark.gpu

WIN, LEVELS, MAX_COUNT, EPS = 15, 2, 10, 0.03
assert dict(win=WIN, max_level=LEVELS, max_count=MAX_COUNT, eps=EPS) == SMALL  # the `small` fixture's oracle ran with these
ROUTE = 9
PITCHES = (132, 133, 134, 135)


def _run(I, J, pts, fbt, mode, max_level=LEVELS, max_count=MAX_COUNT, eps=EPS, want_err=True, want_fbe=False):
    return pyr_lk_forced(I, J, pts, fbt, mode, WIN, max_level, max_count, eps, want_err, want_fbe)


@pytest.mark.parametrize("pitch", PITCHES)
def test_every_phase_and_pitch(small, pitch):
    """Route 9 against routes 1 and 8 and the oracle at every base phase and row pitch, forward and forward-backward."""
    I, J, pts, oracle = small
    for phase in range(4):
        a, b = strided_view(I, pitch, phase), strided_view(J, pitch + (phase & 1), (phase + 1 + (pitch & 1)) & 3)
        for fbt in (None, 1.0):
            res = {mode: _run(a, b, pts, fbt, mode) for mode in (ROUTE, 8, 1)}
            for mode in (8, 1):
                _assert_same(res[ROUTE], res[mode], (pitch, phase, fbt, "route", mode))
            _assert_same(res[ROUTE], oracle[fbt], (pitch, phase, fbt, "oracle"))
            assert res[ROUTE][1].sum() >= 40, (pitch, phase, fbt, int(res[ROUTE][1].sum()))  # the interior tracks are tracked: not a comparison of failures


@pytest.mark.parametrize("n", (1, 3, 15, 16, 17, 33, 64))
def test_track_counts(small, n):
    """Partial wavefronts and a last quad group that is not full: the LAST n tracks of the set, so that every count has edge and corner tracks (tracks
    are independent: the oracle's rows of the same tracks)."""
    I, J, pts, oracle = small
    a, b = strided_view(I, 133, 1), strided_view(J, 134, 3)
    for fbt in (None, 1.0):
        got = _run(a, b, pts[-n:], fbt, ROUTE)
        _assert_same(got, tuple(x[-n:] for x in oracle[fbt]), (n, fbt))


def _spread_scene():
    """192 x 80 pair in four bands of 48 columns: the moved texture, a static copy (J = I: the first Newton step is zero), a flat patch (the
    min-eigenvalue gate rejects it on level 0) and a textured ramp that is 60 grey levels brighter in J (Newton steps of tens of pixels: the window leaves the
    level during the iterations).  Tracks of the four kinds INTERLEAVED, so that every wavefront -- and most quads' neighbours -- hold all of them."""
    I, J = texture_pair(192, 80, 9)
    I, J = I.copy(), J.copy()
    J[:, 48:96] = I[:, 48:96]
    I[:, 96:144] = J[:, 96:144] = 128
    rng = np.random.default_rng(3)
    ramp = np.clip(1.5 * np.arange(48)[None, :] + 0.5 * np.arange(80)[:, None] + rng.integers(0, 12, (80, 48)), 0, 180)
    I[:, 144:] = ramp.astype(np.uint8)
    J[:, 144:] = (ramp + 60).astype(np.uint8)
    kinds = []
    for i in range(16):
        y = 12.0 + 3.5 * i + 0.21 * (i % 4)
        kinds.append([(12.0 + 1.6 * i + 0.3 * (i % 3), y), (64.0 + 1.1 * i + 0.17 * (i % 5), y), (112.0 + 1.3 * i, y + 0.5), (160.0 + 1.2 * i + 0.41 * (i % 2), y)])
    pts = np.array([p for four in kinds for p in four], np.float32)
    return I, J, pts, np.arange(64) % 4


@pytest.fixture(scope="module")
def spread():
    I, J, pts, kind = _spread_scene()
    oracle = {fbt: KO.lk_fb(I, J, pts, fbt=fbt, win=WIN, max_level=LEVELS, max_count=MAX_COUNT, eps=EPS) for fbt in (None, 1.0)}
    return I, J, pts, kind, oracle


def test_spread_inside_one_wavefront(spread):
    """Tracks that stop at different iterations, are rejected by the gate or walk out of the level share wavefronts in caller order; every quad holds
    the oracle's bits whatever its neighbours do (the same tracks in another order land beside other neighbours), and a track whose forward status
    is 0 skips the backward pass: v = 0 and the forward point returned."""
    I, J, pts, kind, oracle = spread
    p, v, e = oracle[None]
    # the scene does what it is built for
    assert v[kind == 0].all() and v[kind == 1].all(), (v[kind == 0], v[kind == 1])
    assert np.abs(p[kind == 1] - pts[kind == 1]).max() < 0.05  # static copy: done after the first Newton step (the upper levels see a little of the bands beside it)
    assert not v[kind == 2].any()  # flat: rejected on level 0
    assert not v[kind == 3].any() and (np.abs(p[kind == 3] - pts[kind == 3]).max(1) > 50).all()  # the ramp tracks walk out of the level
    a, b = to_dev(I), to_dev(J)
    orders = [np.arange(64), np.arange(64)[::-1], np.roll(np.arange(64), 5), np.argsort(kind, kind="stable")]
    fwd = None
    for k, order in enumerate(orders):
        for fbt in (None, 1.0):
            got = _run(a, b, pts[order], fbt, ROUTE)
            _assert_same(got, tuple(x[order] for x in oracle[fbt]), (k, fbt, "oracle"))
            _assert_same(got, _run(a, b, pts[order], fbt, 1), (k, fbt, "generic"))
            if k == 0 and fbt is None:
                fwd = got
            if k == 0 and fbt is not None:
                dead = ~fwd[1]
                assert dead.sum() >= 24 and not got[1][dead].any()
                assert (bits(got[0][dead]) == bits(fwd[0][dead])).all()


@pytest.mark.parametrize("max_level", (0, 2, 4))
def test_levels_criteria_and_optional_outputs(small, max_level):
    """max_level 0 / 2 / 4, max_count 1 / 2 / 10, with and without the err and fbe outputs (with fbe the backward pass of dead tracks runs)."""
    I, J, pts, _ = small
    a, b = strided_view(I, 135, 2), strided_view(J, 132, 0)
    for max_count in (1, 2, 10):
        for fbt in (None, 1.0):
            exp = KO.lk_fb(I, J, pts, fbt=fbt, win=WIN, max_level=max_level, max_count=max_count, eps=EPS, return_fbe=True)
            for want_err, want_fbe in ((True, True), (True, False), (False, True), (False, False)):
                ctx = (max_level, max_count, fbt, want_err, want_fbe)
                got = _run(a, b, pts, fbt, ROUTE, max_level, max_count, EPS, want_err, want_fbe)
                _assert_same(got, exp if fbt is not None else exp[:3], ctx + ("oracle",))
                _assert_same(got, _run(a, b, pts, fbt, 8, max_level, max_count, EPS, want_err, want_fbe), ctx + ("route 8",))


@pytest.mark.parametrize("scene", sorted(R.SCENES))
def test_worst_case_contrast(scene):
    """The binary scenes of lk_ref (bars, transposed bars, the negated variant, checkerboards) at window 15: a lane's 60-sample partial sums at the
    largest gradients and differences 8-bit images hold, integer-position tracks included; the settings of tests/test_gpu_lk_extremes.py."""
    I, J = (np.array(x) for x in R.SCENES[scene]())
    sets = [R.tracks(WIN, o) for o in R.OFFSETS]
    pts = np.concatenate(sets)
    lens = np.array([len(s) for s in sets])
    ends = np.cumsum(lens)
    a, b = to_dev(I), to_dev(J)
    for fbt in (None, 1.0):
        for lvl in (0, 2):
            for mc, eps in R.CRITERIA:
                ctx = (scene, fbt, lvl, mc, eps)
                got = _run(a, b, pts, fbt, ROUTE, lvl, mc, eps)
                _assert_same(got, KO.lk_fb(I, J, pts, fbt=fbt, win=WIN, max_level=lvl, max_count=mc, eps=eps), ctx)
                if lvl == 0 and fbt is None:  # the exact-integer model directly
                    for o, lo, hi in zip(R.OFFSETS, ends - lens, ends):
                        _assert_same(tuple(x[lo:hi] for x in got[:3]), R.model(scene, WIN, o, mc, eps)[:3], ctx + (o, "model"))


def test_session_above_the_threshold_takes_k_lk_h():
    """NATURAL routing, no hook: one session of 256 streams x 504 tracks on 640 x 360 frames = 129 024 tracks in flight, just over the 128 000 from
    which vh_lk_route sends window 15 to k_lk_h<15>.  Both coarse stages report it, and the first, a middle and the last stream match SessionOracle
    for 3 frames: masks, ids and points bit for bit, pose and residual to 1e-5."""
    from velocity_amd.driver import TrackerSession

    W, H, N, B, nframes, ring = 640, 360, 504, 256, 4, 60
    K = synth.K_1080P.copy()
    K[:2, :2] *= W / 1920.0
    K[2, 0], K[2, 1] = W / 2 + 0.5, H / 2 + 0.5
    m = synth.PlaneMotion(K, z0=3.6, traj=synth.oscillating_traj(period=float(ring)))
    lkc = dict(max_level=2)
    checked = {0: (0, 11), 131: (9, 22), 255: (31, 33)}  # stream -> (motion phase, texture); every other stream replays one of three filler clips
    filler = [(3, 44), (17, 55), (40, 66)]
    clips = {}

    def clip(ph, tex):
        if (ph, tex) not in clips:
            clips[(ph, tex)] = [synth.render_frame(W, H, m, ph + k, seed=0xC0FFEE + 104729 * tex, device="cuda") for k in range(nframes)]
        return clips[(ph, tex)]

    of = [checked.get(b, filler[b % 3]) for b in range(B)]
    p0 = synth.grid_tracks(N, W, H, seed=0xEF)
    p3 = m.world_points(p0)
    vp = np.ones(N, bool)
    ses = TrackerSession(K, W, H, N, nhist=nframes + 1, batch=B, lk_coarse=lkc, lk_fine={}, msv_frame=0)
    orcs = {}
    for b, (ph, tex) in enumerate(of):
        pb = m.apply(ph, p0.astype(float)).astype(np.float32)
        p3b = p3 + m.t(ph)
        ses.init_stream(b, clip(ph, tex)[0], pb, p3b, vp, np.float32([0, 0, 0]))
        if b in checked:
            orcs[b] = SessionOracle(K, clip(ph, tex)[0].cpu().numpy(), pb, p3b, vp, np.float32([0, 0, 0]), nhist=nframes + 1, lk_coarse=lkc, lk_fine={}, msv_frame=0)
    for i in range(1, nframes):
        ts = np.float32(i / 30.0)
        ses.step([clip(*of[b])[i] for b in range(B)], time_s=ts, frame_no=i)
        rec = ses.lk_launches()
        assert rec["kernels"] == ["k_lk_h<15>", "k_lk_h<15>", "k_lk3<51, 1, 4>"], rec
        for b, o in orcs.items():
            o.step(clip(*of[b])[i].cpu().numpy(), ts, i)
            st = ses.state(b)
            assert np.array_equal(st["vg"], o.vg) and np.array_equal(st["vp"], o.vp), (i, b)
            assert np.array_equal(st["ids"], np.nonzero(o.vg)[0]) and np.array_equal(st["p"], o.p), (i, b)
            np.testing.assert_allclose(st["t"], o.t, rtol=1e-5, atol=1e-7)
            np.testing.assert_allclose(st["res"], o.residuals, rtol=1e-5)
    for b in orcs:
        assert ses.state(b)["n_cur"] > 0.9 * N  # the tracker really follows the scene
