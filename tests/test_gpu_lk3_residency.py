"""k_lk3<51, 1, 4>, the dominant kernel of a step, at the residency it is built for, and its restage path through the lane-table words it now reads from LDS
where they are used.

Residency: the register file (512 VGPRs per lane and SIMD) holds four wavefronts at 128 VGPRs or fewer, LDS (160 KiB per CU) holds sixteen one-wavefront
workgroups at 10 240 bytes or fewer, and a kernel with scratch pays for every spilled register in every track -- three CONDITIONS of the design (DESIGN.md
section 5), asked of the runtime through vh_debug_lk3_residency; none is a measurement.

Restage: test_gpu_lk3_track_loop displaces its frames by (1.3, -0.7) px, inside the +-4 px the staged search region holds, so no Newton iteration there ever
stages the region again.  Here the displacement is (4.6, -5.3) px: every live track leaves the first region in both axes."""
import functools

import numpy as np
import pytest

from oracle import klt_oracle as KO  # (checker only)
from lk_support import forced_route, lk3_slots
from test_gpu_klt import _lib, _pyr_lk_raw
from test_gpu_lk3_track_loop import SCENES, _bilinear

W, H = SCENES[51]["W"], SCENES[51]["H"]  # 224 x 192
SEED = 5151
SHIFT = (4.6, -5.3)
M = 4  # search margin of the staged region (LK3<51, NW, 4>)
PTS = np.array([(60, 60), (100.25, 120.5), (70.5, 138.75), (118, 92.3), (150.4, 70.2), (10.5, 100.25), (100.7, 185.5), (210.3, 60), (90.2, 6.5)], np.float32)
BORDER = np.array([0, 0, 0, 0, 0, 1, 1, 1, 1], bool)  # the 51 x 51 window of the track reaches over the frame's edge
LK = dict(win=51, max_level=0, max_count=30, eps=0.001)
FBT = 0.3


@functools.lru_cache(maxsize=None)
def _shifted_pair():
    """The frame pair of test_gpu_lk3_track_loop._scene(51) -- same generator, same seed -- displaced by SHIFT instead of (1.3, -0.7), and textured all over:
    without that scene's constant rectangle, which would hold two of the nine tracks in place."""
    rng = np.random.default_rng(SEED)
    big = rng.random((H + 24, W + 24))
    k = np.ones(5) / 5.0
    for _ in range(2):
        big = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 0, big)
        big = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 1, big)
    big = 255.0 * (big - big.min()) / (big.max() - big.min())
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    f0 = np.rint(_bilinear(big, xx + 12.0, yy + 12.0)).astype(np.uint8)
    f1 = np.rint(_bilinear(big, xx + 12.0 - SHIFT[0], yy + 12.0 - SHIFT[1])).astype(np.uint8)
    return np.ascontiguousarray(f0), np.ascontiguousarray(f1)


@functools.lru_cache(maxsize=None)
def _oracle():
    """(p, status, err, fbe) of the nine tracks: computed once, shared, never written to."""
    f0, f1 = _shifted_pair()
    out = KO.lk_fb(f0, f1, PTS, fbt=FBT, return_fbe=True, **LK)
    for a in out:
        a.setflags(write=False)
    return out


def _assert_oracle_restages():
    p, v, _, _ = _oracle()
    assert v.sum() >= 7 and (v & BORDER).sum() >= 2, v
    moved = np.abs(p - PTS)
    assert (moved[v] > M).all(), moved


def test_the_oracle_alone_moves_every_live_track_out_of_the_staged_region():
    """CPU only: at least 7 of the 9 tracks alive after the gate, at least 2 of them border tracks, every live one moved more than 4 px in both axes."""
    _assert_oracle_restages()
    assert (W, H) == (224, 192) and SEED == 5100 + 51


@pytest.mark.gpu
def test_the_fine_kernel_is_resident_as_designed():
    """16 workgroups per CU (4 wavefronts per SIMD), at most 128 registers, no scratch."""
    L, C, torch = _lib()
    L.torch_cuda()
    out = (C.c_int * 4)()
    L.check(L.load().vh_debug_lk3_residency(out), "vh_debug_lk3_residency")
    blocks, regs, scratch, lds = (int(x) for x in out)
    print(f"k_lk3<51, 1, 4>: {blocks} workgroups per CU, {regs} registers, {scratch} bytes of scratch, {lds} bytes of LDS")
    assert blocks == 16, out[:]
    assert regs <= 128, out[:]
    assert scratch == 0, out[:]
    assert 0 < lds <= 160 * 1024 // 16, out[:]


@pytest.mark.gpu
def test_restaged_tracks_get_the_oracles_bits_in_every_instantiation():
    """Modes 5 / 6 / 7 (1 / 2 / 4 wavefronts per track) x 1 / 2 / 4 / 8 launch slots per workgroup: p, status, err and fbe of every track, bit for bit."""
    _assert_oracle_restages()
    L, C, torch = _lib()
    f0, f1 = _shifted_pair()
    ep, ev, eerr, efbe = _oracle()
    a, b = torch.from_numpy(f0).cuda(), torch.from_numpy(f1).cuda()
    ws = L.workspace(W, H, len(PTS))
    for mode in (5, 6, 7):
        for tpw in (1, 2, 4, 8):
            with forced_route(mode), lk3_slots(tpw):
                p2, v, err, fbe, route, used = _pyr_lk_raw(ws, a, b, W, H, PTS, LK, FBT, True, True)
                ctx = (mode, tpw)
                assert route == mode and used == (tpw if mode == 5 else 1), (ctx, route, used)
                assert np.array_equal(v, ev), (ctx, v, ev)
                assert np.array_equal(p2, ep), (ctx, p2, ep)
                assert np.array_equal(err, eerr), (ctx, err, eerr)
                assert np.array_equal(fbe, efbe), (ctx, fbe, efbe)
