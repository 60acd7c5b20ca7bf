"""The library launches what the step plan says (velocity_amd/csrc/vh_step_plan.hpp): sessions whose launch extent -- streams x track rows, which decides
the route, whatever the number of live tracks -- sits on both sides of every LK threshold that a small session reaches.  Each is stepped once; its launch
record (vh_profile_lk_routes, vh_profile_lk_tpw) must be the plan that the g++ probe of tests/step_plan_probe.py computes from the same header for the
same (batch, rows, window, max_level), and its streams must be on the session oracle bit for bit.  One 96 x 64 clip of 50 tracks (48 survive the step) in
every stream of every session; the rows behind the 50 are spare rows."""
import contextlib

import numpy as np
import pytest

from oracle.session_oracle import SessionOracle
from scenes import T0, plane_scene, to_cuda
from step_plan_probe import lk, probe  # noqa: F401 (probe: the fixture)

pytestmark = pytest.mark.gpu

W, H, N = 96, 64, 50
TIME1 = np.float32(1 / 30.0)


@pytest.fixture(scope="module")
def clip():
    """-> (scene, oracle after frame 1): computed once, read by every case"""
    sc = plane_scene(W, H, N, 2, 87, 100.0)
    frames, p, p3, vp, K = sc
    orc = SessionOracle(K, frames[0], p, p3, vp, T0, nhist=3, msv_frame=0)
    orc.step(frames[1], TIME1, 1)
    assert orc.vg.sum() == 48  # (the two hopeless tracks of the scene die)
    return sc, orc


def stepped(clip, batch, rows):
    """A session of `batch` streams x `rows` track rows, every stream on the clip, after frame 1."""
    from velocity_amd.driver import TrackerSession

    (frames, p, p3, vp, K), _ = clip
    ses = TrackerSession(K, W, H, N, nhist=3, batch=batch, msv_frame=0, spare=rows - N)
    f0, f1 = to_cuda(frames[0]), to_cuda(frames[1])
    for b in range(batch):
        ses.init_stream(b, f0, p, p3, vp, T0)
    ses.step([f1] * batch, time_s=TIME1, frame_no=1)
    return ses


def on_the_oracle(ses, clip, where):
    _, orc = clip
    for b in sorted({0, ses.batch // 2, ses.batch - 1}):
        st = ses.state(b)
        assert np.array_equal(st["vg"][:N], orc.vg) and not st["vg"][N:].any(), (where, b)
        assert np.array_equal(st["ids"], np.nonzero(orc.vg)[0]) and np.array_equal(st["p"], orc.p), (where, b)


def planned(probe, batch, rows, force=0, tpw=0, one_level=1):  # noqa: F811
    from velocity_amd import _lib as L

    stages = [L.LK_COARSE, L.LK_COARSE, L.LK_FINE]  # quarter scale, coarse ROI, fine
    return lk(probe, [(batch, rows, s["win"], s["max_level"], force, tpw, one_level) for s in stages])


def assert_launched(ses, plans, where):
    rec = ses.lk_launches()
    assert rec["routes"] == [p["route"] for p in plans], (where, rec, plans)
    assert rec["kernels"] == [p["name"] for p in plans], (where, rec, plans)
    assert rec["slots_per_workgroup"] == [p["tpw"] for p in plans], (where, rec, plans)


# (streams, rows) -> the routes DESIGN.md section 4 gives, written out: the probe must say the same
EXTENTS = [((1, 639), [2, 2, 7]), ((1, 640), [2, 2, 5]), ((1, 2999), [2, 2, 5]), ((1, 3000), [4, 4, 5]), ((4, 2500), [8, 8, 5]),
           ((64, 1999), [8, 8, 5]), ((64, 2000), [9, 9, 5]), ((64, 768), [8, 8, 5]), ((64, 1536), [8, 8, 5])]
SLOTS = {(64, 768): 2, (64, 1536): 4, (64, 1999): 4, (64, 2000): 4}  # of the fine stage: 2 from 49 152 rows in flight, 4 from 98 304 (1 below)


@pytest.mark.parametrize("extent,routes", EXTENTS, ids=["%dx%d" % e for e, _ in EXTENTS])
def test_a_session_launches_the_plan(clip, probe, extent, routes):  # noqa: F811
    plans = planned(probe, *extent)
    assert [p["route"] for p in plans] == routes and [p["tpw"] for p in plans] == [1, 1, SLOTS.get(extent, 1)], plans
    ses = stepped(clip, *extent)
    assert_launched(ses, plans, extent)
    on_the_oracle(ses, clip, extent)


@contextlib.contextmanager
def hook(name, value, rest):
    from velocity_amd import _lib as L

    fn = getattr(L.load(), name)
    try:
        fn(value)
        yield
    finally:
        fn(rest)


# setter, value, default, what the plan is asked with: the two hooks whose effect the launch record shows (route, kernel name, slots per workgroup)
REPORTED = [("vh_debug_force_generic_lk", 4, 0, dict(force=4)), ("vh_debug_force_generic_lk", 6, 0, dict(force=6)), ("vh_debug_lk3_tpw", 3, 0, dict(tpw=3)),
            ("vh_debug_lk3_tpw", 100, 0, dict(tpw=100)), ("vh_debug_lk3_tpw", -5, 0, dict(tpw=0))]
# the hooks of a step that the ABI gives no read-back for: neither the launch record nor the profile records (one per launcher call) tell the level form of
# k_lk3, the track order, the RANSAC path or the rows per thread of pyrDown apart
UNREPORTED = [("vh_debug_lk3_one_level", 0, 1), ("vh_debug_klt_order", 1, -1), ("vh_debug_ransac_path", 1, 0), ("vh_debug_pyr_rows", 8, 0)]


def under_hook(clip, probe, name, value, rest, tuning):  # noqa: F811
    extent = (1, 640)
    plans = planned(probe, *extent, **tuning)
    with hook(name, value, rest):
        ses = stepped(clip, *extent)
        assert_launched(ses, plans, (name, value))
        on_the_oracle(ses, clip, (name, value))
    again = stepped(clip, *extent)  # the default is back
    assert_launched(again, planned(probe, *extent), (name, "restored"))
    return plans


@pytest.mark.parametrize("name,value,rest,tuning", REPORTED, ids=["%s=%d" % h[:2] for h in REPORTED])
def test_a_hook_reaches_the_next_launch(clip, probe, name, value, rest, tuning):  # noqa: F811
    """The value set is what the next launch reports, the setter's normalisation included (100 slots act as 8, -5 is 0: by load); the default is restored."""
    plans = under_hook(clip, probe, name, value, rest, tuning)
    if name == "vh_debug_force_generic_lk":
        assert [p["route"] for p in plans] == {4: [4, 4, 2], 6: [2, 2, 6]}[value], plans  # (4: other windows than 15 as in 2; 6: others by load)
    else:
        assert plans[2]["tpw"] == {3: 3, 100: 8, -5: 1}[value], plans


@pytest.mark.parametrize("name,value,rest", UNREPORTED, ids=["%s=%d" % h[:2] for h in UNREPORTED])
def test_a_step_under_an_unreported_hook_is_only_checked_to_stay_bit_exact(clip, probe, name, value, rest):  # noqa: F811
    """NOT a check that the setter has an effect: a step under the hook keeps the default LK launches and the oracle's bits, and would do so with a setter
    that did nothing.  What these hooks select is exercised where it shows: tests/test_gpu_lk3_staging.py (level form), tests/test_gpu_session.py (order),
    tests/test_gpu_ransac.py and tests/test_gpu_klt.py (RANSAC path, pyrDown rows).  vh_debug_ba_force_valu has no case here: a session step runs no bundle
    adjustment (tests/test_gpu_nls.py compares the two Schur kernels it selects)."""
    under_hook(clip, probe, name, value, rest, {})
