"""k_lk_h<15> (route 9) with part of a lane's template in LDS: four wavefronts per SIMD.

A lane keeps the y gradients of its four window rows, the last strip of the x gradients and what a track carries from level to level in a slice of
LDS of its own: 16 bytes of every 1024-byte chunk of its wavefront's 10 240 bytes.  What can go wrong here and nowhere else: a lane reading a
neighbour's 16 bytes or another chunk, wavefronts of one CU reading each other's slices, a set-up that leaves a chunk unwritten (two set-ups write
them: the interior one and the one of border windows), the err pass and the next pass or level reusing the slots, and a build that does not reach the
residency the move is for.  Everything is held bit for bit -- position, status, err, fbe -- against k_lk_o (route 8) and the CPU oracle on one
320 x 240 scene whose gradients differ strongly from track to track: with any slot mixed up, a track solves for another track's template."""
import ctypes as C

import numpy as np
import pytest

from lk_support import assert_same_bits as _assert_same
from lk_support import pyr_lk_forced
from oracle import klt_oracle as KO  # (checker only)

pytestmark = pytest.mark.gpu

W, H, WIN, MAX_COUNT, EPS, FBT = 320, 240, 15, 10, 0.03, 1.0
ROUTE, NMAX = 9, 4096
FLAT = (150, 100, 44, 40)  # x, y, w, h of a constant patch: the min-eigenvalue gate kills its tracks on level 0 of the forward pass


def _cells_pair():
    """Box-filtered noise whose contrast and grain change from cell to cell of a 16 x 16 px grid (the gradients of two tracks a few pixels apart share
    little), a constant patch, and the same image moved by (+1.5, -1) px."""
    rng = np.random.default_rng(41)
    n = rng.integers(0, 256, (H + 12, W + 12)).astype(np.float64)
    k3, k7 = np.ones(3) / 3.0, np.ones(7) / 7.0

    def blur(a, k):
        a = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), 1, a)
        return np.apply_along_axis(lambda c: np.convolve(c, k, "same"), 0, a)

    fine, coarse = blur(n, k3), blur(n, k7)
    cells = (H + 12 + 15) // 16, (W + 12 + 15) // 16
    mix = np.kron(rng.random(cells), np.ones((16, 16)))[:H + 12, :W + 12]
    gain = np.kron(0.25 + 0.75 * rng.random(cells), np.ones((16, 16)))[:H + 12, :W + 12]
    t = mix * fine + (1.0 - mix) * coarse
    t = (t - t.mean()) * gain
    t = (t - t.min()) / (t.max() - t.min()) * 255.0
    x, y, w, h = FLAT
    t[6 + y - 2:6 + y + h + 2, 6 + x - 3:6 + x + w + 3] = 128.0
    a = t[6:6 + H, 6:6 + W]
    b = 0.5 * (t[7:7 + H, 4:4 + W] + t[7:7 + H, 5:5 + W])
    return np.rint(a).astype(np.uint8), np.rint(b).astype(np.uint8)


def _border_tracks(n, rng):
    """n points within 8 px of the left, right, top and bottom border in turn (their 15 x 15 window crosses it: the border set-up on level 0)."""
    pts = []
    for i in range(n):
        d = 0.25 + 7.5 * rng.random()
        u = rng.random()
        side = i % 4
        if side == 0: pts.append((d, 10.0 + u * (H - 20)))
        elif side == 1: pts.append((W - 1 - d, 10.0 + u * (H - 20)))
        elif side == 2: pts.append((10.0 + u * (W - 20), d))
        else: pts.append((10.0 + u * (W - 20), H - 1 - d))
    return np.array(pts, np.float32)


def _interior_tracks(n, rng):
    return np.stack([12.0 + rng.random(n) * (W - 24), 12.0 + rng.random(n) * (H - 24)], 1).astype(np.float32)


def _flat_tracks(n, rng):
    x, y, w, h = FLAT
    return np.stack([x + 10.0 + rng.random(n) * (w - 20), y + 10.0 + rng.random(n) * (h - 20)], 1).astype(np.float32)


def _tracks():
    """NMAX points: of every 8 consecutive ones 5 are interior, 2 lie at a border and 1 in the flat patch, so that every wavefront -- and the first 15
    tracks already -- holds slices filled by both set-ups and a track whose backward pass is skipped."""
    rng = np.random.default_rng(7)
    kinds = np.array([0, 1, 0, 0, 2, 0, 1, 0] * (NMAX // 8))
    pts = np.zeros((NMAX, 2), np.float32)
    pts[kinds == 0] = _interior_tracks(int((kinds == 0).sum()), rng)
    pts[kinds == 1] = _border_tracks(int((kinds == 1).sum()), rng)
    pts[kinds == 2] = _flat_tracks(int((kinds == 2).sum()), rng)
    return pts, kinds


def _run(I, J, pts, fbt, mode, max_level, want_err=True, want_fbe=True):
    return pyr_lk_forced(I, J, pts, fbt, mode, WIN, max_level, MAX_COUNT, EPS, want_err, want_fbe)


@pytest.fixture(scope="module")
def scene():
    import torch

    I, J = _cells_pair()
    pts, kinds = _tracks()
    oracle = {(lvl, fbt): KO.lk_fb(I, J, pts, fbt=fbt, win=WIN, max_level=lvl, max_count=MAX_COUNT, eps=EPS, return_fbe=True)
              for lvl in (0, 2) for fbt in (None, FBT)}
    return I, J, torch.from_numpy(I).cuda(), torch.from_numpy(J).cuda(), pts, kinds, oracle


def test_the_coarse_kernel_is_resident_as_designed():
    """16 workgroups per CU (4 wavefronts per SIMD), at most 128 registers, no scratch, at most 10 240 bytes of LDS: conditions, asked of the runtime."""
    from velocity_amd import _lib as L

    L.torch_cuda()
    out = (C.c_int * 4)()
    L.check(L.load().vh_debug_lkh_residency(out), "vh_debug_lkh_residency")
    blocks, regs, scratch, lds = (int(x) for x in out)
    print(f"k_lk_h<15>: {blocks} workgroups per CU, {regs} registers, {scratch} bytes of scratch, {lds} bytes of LDS")
    assert blocks >= 16, out[:]
    assert regs <= 128, out[:]
    assert scratch == 0, out[:]
    assert lds <= 160 * 1024 // 16, out[:]


def test_the_scene_does_what_it_is_built_for(scene):
    """The oracle alone: interior and border tracks are tracked through the forward-backward gate, the flat ones die on level 0 of the forward pass, and
    neighbouring tracks have little in common (their err values spread over a wide range)."""
    _, _, _, _, pts, kinds, oracle = scene
    p, v, err, fbe = oracle[(2, FBT)]
    assert v[kinds == 0].mean() > 0.9 and v[kinds == 1].mean() > 0.5, (v[kinds == 0].mean(), v[kinds == 1].mean())
    assert not oracle[(2, None)][1][kinds == 2].any() and not oracle[(0, None)][1][kinds == 2].any()
    e = err[v]
    assert np.percentile(e, 90) > 3.0 * np.percentile(e, 10), (np.percentile(e, 10), np.percentile(e, 90))


@pytest.mark.parametrize("n", (1, 15, 16, 17, 31, 33, NMAX))
def test_slices_are_isolated(scene, n):
    """A lane reads only its own 16 bytes of each chunk, a wavefront only its own 10 240 bytes: partial wavefronts, one and two wavefronts, and 256
    wavefronts of which several share a CU (their slices are neighbours in its LDS).  Three levels, forward-backward, err and fbe."""
    I, J, a, b, pts, kinds, oracle = scene
    got = _run(a, b, pts[:n], FBT, ROUTE, 2)
    _assert_same(got, _run(a, b, pts[:n], FBT, 8, 2), (n, "route 8"))
    _assert_same(got, tuple(x[:n] for x in oracle[(2, FBT)]), (n, "oracle"))
    if n == NMAX:
        assert got[1].sum() > 0.6 * n, int(got[1].sum())  # not a comparison of failures


@pytest.mark.parametrize("max_level", (0, 2))
@pytest.mark.parametrize("want_err", (True, False))
def test_both_setups_fill_the_slices(scene, max_level, want_err):
    """Border and interior tracks in ONE launch, mixed inside every wavefront, with the flat tracks whose forward status is 0 (without the fbe output
    their backward pass is skipped, and the next pass to touch the slots is another track's or another level's); one level and three; with and
    without the err pass, which borrows the slots once the template is dead."""
    I, J, a, b, pts, kinds, oracle = scene
    n = 512
    assert (kinds[:n] == 1).sum() >= 100 and (kinds[:n] == 2).sum() >= 50
    for fbt in (None, FBT):
        for want_fbe in (False, True):
            ctx = (max_level, want_err, fbt, want_fbe)
            got = _run(a, b, pts[:n], fbt, ROUTE, max_level, want_err, want_fbe)
            _assert_same(got, _run(a, b, pts[:n], fbt, 8, max_level, want_err, want_fbe), ctx + ("route 8",))
            _assert_same(got, tuple(x[:n] for x in oracle[(max_level, fbt)]), ctx + ("oracle",))
            assert not got[1][kinds[:n] == 2].any(), ctx
    # the border tracks alone, and the interior ones alone: wavefronts whose slices all come from one set-up
    for kind in (1, 0):
        sel = np.flatnonzero(kinds == kind)[:200]
        got = _run(a, b, pts[sel], FBT, ROUTE, max_level, want_err, True)
        _assert_same(got, _run(a, b, pts[sel], FBT, 8, max_level, want_err, True), (max_level, want_err, kind, "route 8"))
        _assert_same(got, tuple(x[sel] for x in oracle[(max_level, FBT)]), (max_level, want_err, kind, "oracle"))
