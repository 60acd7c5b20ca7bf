"""k_lk3's track loop against the CPU oracle, bit for bit: the lane map a workgroup writes to LDS once (LK3::OFF_TAB) must serve every launch slot the
workgroup solves after it -- whatever the slots before it did (left before any set-up, took the border set-up, stopped on minEig) -- in every
instantiation of the kernel, for every slot count, with and without the forward-backward gate and the err / fbe outputs."""
import functools

import numpy as np
import pytest

from oracle import klt_oracle as KO  # (checker only)
from lk_support import forced_route, lk3_slots
from test_gpu_klt import _lib, _pyr_lk_raw

OOF, INT, BRD, FLAT = "out-of-frame", "interior", "border", "textureless"
# launch order = slot order (vh_pyr_lk keeps the caller's order): with 4 slots per workgroup every workgroup starts on an out-of-frame track, which leaves
# before any set-up, and a textureless track (forward status 0: no backward pass) is followed by a live one inside the workgroup (6 -> 7, 10 -> 11).
# 13 tracks: no slot count but 1 divides them
KINDS = [OOF, INT, BRD, FLAT, OOF, INT, FLAT, INT, OOF, BRD, FLAT, INT, OOF]
# frame size, the textureless rectangle (x0, y0, x1, y1) and the tracks of each kind.  224 x 192 is the smallest frame that holds interior 51 x 51 windows
# with their search margin beside a textureless block a window fits in, and whose second pyramid level (112 x 96) still holds the window; 160 x 128 does
# the same for 15 x 15 down to pyramid level 3
SCENES = {
    51: dict(W=224, H=192, flat=(146, 0, 224, 80),
             pts={OOF: [(-140.0, 50.0), (400.5, 90.25), (90.0, -160.0), (120.0, 420.0)],
                  INT: [(60.0, 60.0), (100.25, 120.5), (70.5, 138.75), (118.0, 92.3)],
                  BRD: [(10.5, 100.25), (100.7, 185.5)],
                  FLAT: [(185.0, 38.0), (184.5, 40.25), (186.2, 39.0)]}),
    15: dict(W=160, H=128, flat=(110, 0, 160, 40),
             pts={OOF: [(-140.0, 50.0), (400.5, 90.25), (90.0, -160.0), (120.0, 420.0)],
                  INT: [(40.0, 40.0), (80.25, 70.5), (60.5, 100.75), (90.0, 52.3)],
                  BRD: [(3.5, 60.25), (80.7, 125.5)],
                  FLAT: [(135.0, 20.0), (134.5, 19.25), (136.2, 21.0)]}),
}
LK = {
    (51, 0): dict(win=51, max_level=0, max_count=30, eps=0.001),
    (51, 1): dict(win=51, max_level=1, max_count=30, eps=0.001),
    (15, 3): dict(win=15, max_level=3, max_count=10, eps=0.1),
}
FBT = {51: 0.3, 15: 0.3}


def _bilinear(img, x, y):
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    ax, ay = x - x0, y - y0
    return ((1 - ay) * ((1 - ax) * img[y0, x0] + ax * img[y0, x0 + 1]) + ay * ((1 - ax) * img[y0 + 1, x0] + ax * img[y0 + 1, x0 + 1]))


@functools.lru_cache(maxsize=None)
def _scene(win):
    """A seeded frame pair: smoothed noise, the second frame displaced by (1.3, -0.7) pixels; one rectangle is constant in both frames."""
    sc = SCENES[win]
    W, H = sc["W"], sc["H"]
    rng = np.random.default_rng(5100 + win)
    big = rng.random((H + 24, W + 24))
    k = np.ones(5) / 5.0
    for _ in range(2):
        big = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 0, big)
        big = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 1, big)
    big = 255.0 * (big - big.min()) / (big.max() - big.min())
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    f0 = np.rint(_bilinear(big, xx + 12.0, yy + 12.0)).astype(np.uint8)
    f1 = np.rint(_bilinear(big, xx + 12.0 - 1.3, yy + 12.0 + 0.7)).astype(np.uint8)
    x0, y0, x1, y1 = sc["flat"]
    f0[y0:y1, x0:x1] = 128
    f1[y0:y1, x0:x1] = 128
    left = {k: list(v) for k, v in sc["pts"].items()}
    pts = np.array([left[k].pop(0) for k in KINDS], np.float32)
    return np.ascontiguousarray(f0), np.ascontiguousarray(f1), pts


@functools.lru_cache(maxsize=None)
def _oracle(win, max_level, fbt, n):
    """(p, status, err, fbe | None) of the first n tracks: computed once, shared by every test, never written to."""
    f0, f1, pts = _scene(win)
    lk = LK[(win, max_level)]
    if fbt is None:
        p, v, err = KO.lk_fb(f0, f1, pts[:n], fbt=None, **lk)
        fbe = None
    else:
        p, v, err, fbe = KO.lk_fb(f0, f1, pts[:n], fbt=fbt, return_fbe=True, **lk)
    for a in (p, v, err) + (() if fbe is None else (fbe,)):
        a.setflags(write=False)
    return p, v, err, fbe


@pytest.mark.parametrize("win, max_level", sorted(LK))
def test_the_oracle_alone_gives_live_and_dead_tracks_of_every_kind_it_can(win, max_level):
    """CPU only.  Out-of-frame and textureless tracks are dead by construction (every one must be); interior and border tracks must be alive on the forward
    pass, and the forward-backward gate must keep at least one of each of those two kinds alive."""
    f0, f1, pts = _scene(win)
    kinds = np.array(KINDS)
    fwd = KO.pyr_lk(f0, f1, pts, **LK[(win, max_level)])[1]
    assert not fwd[kinds == OOF].any() and not fwd[kinds == FLAT].any(), fwd
    assert fwd[kinds == INT].all() and fwd[kinds == BRD].all(), fwd
    v = _oracle(win, max_level, FBT[win], len(pts))[1]
    assert v[kinds == INT].any() and v[kinds == BRD].any() and not v[kinds == OOF].any() and not v[kinds == FLAT].any(), v
    assert len(pts) == 13 and all(len(pts) % t for t in (2, 3, 4, 8))


@pytest.mark.gpu
@pytest.mark.parametrize("mode, win, max_level", [(5, 51, 0), (5, 51, 1), (6, 51, 0), (6, 51, 1), (7, 51, 0), (7, 51, 1), (3, 15, 3)])
def test_every_slot_of_a_workgroup_gets_the_oracles_bits(mode, win, max_level):
    """p, status, err and fbe of EVERY track equal the oracle's, for 1 / 2 / 3 / 4 / 8 launch slots per workgroup (13 tracks: the last workgroup is short;
    3 tracks: fewer tracks than slots), with and without the gate and the optional outputs.  The kernels of two and four wavefronts per track solve one slot
    per workgroup whatever the hook says, and must report that."""
    L, C, torch = _lib()
    f0, f1, pts = _scene(win)
    lk = LK[(win, max_level)]
    H, W = f0.shape
    a, b = torch.from_numpy(f0).cuda(), torch.from_numpy(f1).cuda()
    ws = L.workspace(W, H, len(pts))
    with forced_route(mode):
        for n in (len(pts), 3):
            for fbt in (None, FBT[win]):
                ep, ev, eerr, efbe = _oracle(win, max_level, fbt, n)
                for tpw in ((1, 2, 3, 4, 8) if n == len(pts) else (4, 8)):
                    with lk3_slots(tpw):
                        for want_err, want_fbe in ((True, False), (False, False), (True, True), (False, True)):
                            if want_fbe and fbt is None:
                                continue
                            p2, v, err, fbe, route, used = _pyr_lk_raw(ws, a, b, W, H, pts[:n], lk, fbt, want_err, want_fbe)
                            ctx = (mode, win, max_level, n, fbt, tpw, want_err, want_fbe)
                            assert route == mode and used == (tpw if mode in (3, 5) else 1), (ctx, route, used)
                            assert np.array_equal(v, ev), (ctx, v, ev)
                            assert np.array_equal(p2, ep), (ctx, p2, ep)
                            if want_err:
                                assert np.array_equal(err, eerr), (ctx, err, eerr)
                            if want_fbe:
                                assert np.array_equal(fbe, efbe), (ctx, fbe, efbe)
