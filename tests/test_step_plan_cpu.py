"""The host decisions of a frame step (velocity_amd/csrc/vh_step_plan.hpp), checked without a GPU: a small program compiled with g++ against the header
prints the plan of every launch at both sides of every threshold.  The expectations are DESIGN.md sections 4 and 5 and include/velocity_hip.h, written
out here; the LK route rule is additionally compared, over a grid of hooks, windows and loads, with a transcription of vh_lk_route as commit 6fa1685
had it, before the rule moved into the header."""
import itertools
import os
import subprocess

from step_plan_probe import CSRC, ints, lk, probe  # noqa: F401 (probe: the fixture)

ROTATE = 0x10000  # LK_GRP_ROTATE: the streams of a set are rotated off the XCDs below 64 streams
NAMES = {1: "k_lk", 3: "k_lk3<15, 1, 6>", 4: "k_lk_q<15>", 5: "k_lk3<51, 1, 4>", 6: "k_lk3<51, 2, 4>", 7: "k_lk3<51, 4, 4>", 8: "k_lk_o<15>",
         9: "k_lk_h<15>"}


def test_the_header_is_plain_cxx17(tmp_path):
    """g++ compiles the header on its own: no HIP include, no getenv and no atomics (the record of the switches is the library's; a plan reads a snapshot)."""
    src = tmp_path / "alone.cpp"
    src.write_text('#include "vh_step_plan.hpp"\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", CSRC, str(src)], check=True)
    text = open(os.path.join(CSRC, "vh_step_plan.hpp")).read()
    assert "hip/" not in text and "getenv" not in text and "std::atomic" not in text and "<atomic>" not in text and "vh_common" not in text
    # the word itself only where the measurement record beside the LK thresholds speaks of the statistics atomics of round 5: never in code
    assert "atomic" not in "\n".join(line.split("//")[0] for line in text.splitlines())


def test_the_defaults_are_the_librarys(probe):
    assert ints(probe, "d", [(0,)])[0] == [0, 0, 1, -1, 0, 0, 0, 64, 64, 16, 0, 10000, 128000, 0, 0, 0]


def both_ways(tracks):
    """a load reached with one stream, and as batch x max_n"""
    for b in (64, 32, 16, 8, 5, 3, 2):
        if tracks % b == 0:
            return [(1, tracks), (b, tracks // b)]
    return [(1, tracks), (tracks, 1)]


# (window, tracks in flight) -> route, DESIGN.md section 4: both sides of every boundary at default tuning
BOUNDARIES = [(51, 639, 7), (51, 640, 5), (15, 2999, 2), (15, 3000, 4), (15, 9999, 4), (15, 10000, 8), (15, 127999, 8), (15, 128000, 9),
              (21, 2999, 2), (21, 128000, 2), (63, 2, 2), (63, 128000, 2), (64, 2, 1), (64, 128000, 1), (65, 3000, 1), (165, 2, 1), (165, 128000, 1)]


def test_lk_routes_at_every_boundary(probe):
    cases, want = [], []
    for win, tracks, route in BOUNDARIES:
        for batch, max_n in both_ways(tracks):
            cases.append((batch, max_n, win))
            want.append(route)
    assert all(b > 1 for b, _, _ in cases[1::2])  # every boundary is reached as a product too
    for c, route, p in zip(cases, want, lk(probe, cases)):
        assert p["rc"] == 0 and p["route"] == route, (c, p)
    # a window that no kernel holds in LDS: refused, whatever the load and the hook
    for p in lk(probe, [(1, 100, 166), (64, 2000, 166), (1, 100, 166, -1, 2), (1, 100, 1000)]):
        assert p["rc"] == -2 and p["route"] == 1, p
    # no track slot: nothing to launch
    for p in lk(probe, [(4, 0, 15), (4, -3, 51)]):
        assert p["rc"] == 0 and p["route"] == 0 and p["name"] == "none" and p["tpw"] == 1, p


def test_lk_names(probe):
    cases = [(1, 100, 15, -1, f) for f in range(1, 10)] + [(1, 100, 51, -1, f) for f in range(1, 10)] + [(1, 100, w, -1, f) for w in (21, 63, 64, 165) for f in (0, 1, 2)]
    for c, p in zip(cases, lk(probe, cases)):
        win, route = c[2], p["route"]
        if route == 2:
            assert p["name"] == ("k_lk_strip<%d>" % (win if win in (15, 51) else 0)) and p["strip_win"] == (win if win in (15, 51) else 0), (c, p)
        else:
            assert p["name"] == NAMES[route], (c, p)
    got = {(c[2], c[4]): p["route"] for c, p in zip(cases, lk(probe, cases))}
    assert [got[15, f] for f in range(1, 10)] == [1, 2, 3, 4, 2, 2, 2, 8, 9]  # 5..7 with another window than 51: default routing (100 tracks: strip)
    assert [got[51, f] for f in range(1, 10)] == [1, 2, 7, 2, 5, 6, 7, 2, 2]  # 3 at window 51: four wavefronts per track
    assert all(got[w, f] == (1 if f == 1 or w > 63 else 2) for w in (21, 63, 64, 165) for f in (0, 1, 2))


def test_lk_grids_blocks_and_lds(probe):
    sizes = [(1, 1), (1, 15), (1, 16), (1, 17), (3, 2001), (64, 2000)]
    per = {1: 1, 2: 1, 4: 4, 8: 8, 9: 16}
    for force, win in ((1, 15), (2, 15), (2, 51), (2, 33), (4, 15), (8, 15), (9, 15), (1, 99)):
        cases = [(b, n, win, -1, force) for b, n in sizes]
        for (b, n), p in zip(sizes, lk(probe, cases)):
            what = (force, win, b, n, p)
            assert p["route"] == force and p["grid_x"] == -(-n // per[force]) and p["grid_y"] == b and p["block"] == 64, what
            assert p["tracks_per_wave"] == per[force] and p["waves_per_track"] == 1 and p["tpw"] == 1 and p["one_level"] == 0, what
            if force in (4, 8, 9):  # sets of 64 streams, rotated off the XCDs below 64 streams; no dynamic LDS
                assert p["group"] == (64 | (ROTATE if b < 64 else 0)) and p["lds"] == 0 and p["needs_big_lds"] == 0, what
            elif force == 2:  # 24 bytes per strip of 4 window pixels, in whole passes of the wavefront
                strips = -(-win // 4) * win
                assert p["group"] == 0 and p["lds"] == -(-strips // 64) * 64 * 24 and p["needs_big_lds"] == (p["lds"] > 65536), what
            else:  # 6 bytes per window pixel, in whole passes of the wavefront
                assert p["group"] == 0 and p["lds"] == -(-win * win // 64) * 64 * 6 and p["needs_big_lds"] == (p["lds"] > 65536), what
    lds = {c[2]: p for c, p in zip([(1, 8, w, -1, f) for w, f in ((15, 2), (51, 2), (63, 2), (64, 1), (104, 1), (105, 1), (165, 1))],
                                    lk(probe, [(1, 8, w, -1, f) for w, f in ((15, 2), (51, 2), (63, 2), (64, 1), (104, 1), (105, 1), (165, 1))]))}
    assert [lds[w]["lds"] for w in (15, 51, 63, 64, 104, 105, 165)] == [1536, 16896, 24576, 24576, 64896, 66432, 163584]
    assert [lds[w]["needs_big_lds"] for w in (15, 51, 63, 64, 104, 105, 165)] == [0, 0, 0, 0, 0, 1, 1]
    # k_lk3: NW wavefronts per track, sets of 16 streams, the plan carries only the experiment's LDS pad
    cases = [(b, n, win, -1, force, 0, 1, -1, -1, pad) for force, win in ((3, 15), (5, 51), (6, 51), (7, 51)) for b, n in sizes for pad in (0, 4096)]
    for c, p in zip(cases, lk(probe, cases)):
        nw = {3: 1, 5: 1, 6: 2, 7: 4}[c[4]]
        assert p["route"] == c[4] and p["block"] == 64 * nw and p["waves_per_track"] == nw and p["tracks_per_wave"] == 1, (c, p)
        assert p["grid_x"] == -(-c[1] // p["tpw"]) and p["grid_y"] == c[0] and p["group"] == (16 | (ROTATE if c[0] < 64 else 0)), (c, p)
        assert p["lds"] == c[9] and p["needs_big_lds"] == 0, (c, p)


def test_lk3_slots_per_workgroup(probe):
    loads = {49151: 1, 49152: 2, 98303: 2, 98304: 4}
    for tracks, want in loads.items():
        for batch, max_n in both_ways(tracks):  # (49 152 = 64 x 768, 98 304 = 64 x 1536)
            one, four, coarse = lk(probe, [(batch, max_n, 51, -1, 5), (batch, max_n, 51, -1, 7), (batch, max_n, 15, -1, 3)])
            assert one["tpw"] == want and one["grid_x"] == -(-max_n // want), (batch, max_n, one)
            assert coarse["tpw"] == want, (batch, max_n, coarse)
            assert four["tpw"] == 1 and four["grid_x"] == max_n, (batch, max_n, four)  # NW != 1: one slot
    # the hook: n slots whatever the load, clamped to 8; ignored by the kernels with more than one wavefront per track
    for hook, want in ((1, 1), (3, 3), (8, 8), (9, 8), (100, 8), (0, 4)):
        one, two = lk(probe, [(64, 2000, 51, -1, 5, hook), (64, 2000, 51, -1, 6, hook)])
        assert one["tpw"] == want and one["grid_x"] == -(-2000 // want) and two["tpw"] == 1, (hook, one, two)
    # default routing at the headline's load: one wavefront per track, four slots
    p = lk(probe, [(256, 2000, 51, 0)])[0]
    assert (p["route"], p["tpw"], p["grid_x"], p["grid_y"], p["one_level"]) == (5, 4, 500, 256, 1)


def test_lk3_single_level_form(probe):
    cases = [(1, 700, 51, lvl, 0, 0, sw) for lvl in (-1, 0, 1, 3) for sw in (0, 1)]
    for c, p in zip(cases, lk(probe, cases)):
        assert p["one_level"] == (1 if c[3] == 0 and c[6] == 1 else 0), (c, p)
    assert all(p["one_level"] == 0 for p in lk(probe, [(1, 700, 15, 0), (1, 7000, 15, 0), (1, 70, 33, 0), (1, 70, 99, 0)]))  # no other kernel has one


def test_lk_rotate_bit(probe):
    for force, win, g in ((4, 15, 64), (8, 15, 64), (9, 15, 64), (3, 15, 16), (5, 51, 16)):
        a, b = lk(probe, [(63, 100, win, -1, force), (64, 100, win, -1, force)])
        assert a["group"] == (g | ROTATE) and b["group"] == g, (force, a, b)


def parent_route(batch, max_n, win, force, lko_min=10000, lkh_min=128000):
    """vh_lk_route of commit 6fa1685, statement by statement"""
    tracks = max_n * batch
    force_nw = 5 <= force <= 7
    if force == 0 or force == 3 or (force_nw and win == 51):
        if win == 15 and force == 3:
            return 3
        if win == 51:
            nw = (1 << (force - 5)) if force_nw else (4 if force == 3 else 1 if tracks >= 640 else 4)
            return 5 if nw == 1 else 6 if nw == 2 else 7
    if win == 15 and (force == 9 or ((force == 0 or force_nw) and tracks >= lkh_min)):
        return 9
    if win == 15 and (force == 8 or ((force == 0 or force_nw) and tracks >= lko_min)):
        return 8
    if win == 15 and (force == 4 or ((force == 0 or force_nw) and tracks >= 3000)):
        return 4
    if force != 1 and win <= 63:
        return 2
    return 1


def test_the_route_rule_is_the_parents(probe):
    loads = [(1, t) for t in (1, 639, 640, 2999, 3000, 9999, 10000, 49151, 49152, 98303, 98304, 127999, 128000)]
    loads += [(3, 213), (64, 10), (4, 750), (8, 1250), (64, 2000), (256, 500), (65535, 65535)]  # (the last product is beyond 2^31)
    wins = (1, 5, 15, 21, 51, 63, 64, 65, 165)
    cases, want = [], []
    for (lko, lkh), force, win, (b, n) in itertools.product(((-1, -1), (2000, 4000), (200000, 100000), (0, 0)), range(-1, 11), wins, loads):
        cases.append((b, n, win, -1, force, 0, 1, lko, lkh))
        want.append(parent_route(b, n, win, force, *((10000, 128000) if lko < 0 else (lko, lkh))))
    got = lk(probe, cases)
    bad = [(c, w, p["route"]) for c, w, p in zip(cases, want, got) if p["route"] != w or p["rc"] != 0]
    assert not bad, (len(bad), bad[:10])
    assert set(want) == set(range(1, 10))


def test_lk_window_fit(probe):
    rows = dict(zip((0, 1, 64, 165, 166, 1000), ints(probe, "f", [(w,) for w in (0, 1, 64, 165, 166, 1000)])))
    assert [rows[w][0] for w in (0, 1, 64, 165, 166, 1000)] == [0, 1, 1, 1, 0, 0]
    assert all(r[1] == 165 for r in rows.values())  # vh_lk_max_window
    assert rows[165][2] == 163584 <= 160 * 1024 < rows[166][2] == 165504


def test_pyramid(probe):
    keys = ["w", "h", "rows", "block_x", "block_y", "grid_x", "grid_y", "grid_z", "ring_groups"]

    def plans(cases):
        return [dict(zip(keys, r)) for r in ints(probe, "p", cases)]

    # rows per thread by the pixels of the level over the whole launch: 2^20 = 1024 x 1024, 2^25 = 32 x 2^20
    cases = [(0, 2048, 2046, 1, 0), (0, 2048, 2048, 1, 0), (0, 2048, 2048, 31, 0), (0, 2048, 2048, 32, 0), (0, 2046, 2048, 32, 0), (1, 4096, 4096, 1, 0),
             (1, 4096, 4092, 1, 0)]
    assert [p["rows"] for p in plans(cases)] == [2, 4, 4, 8, 4, 4, 2]
    sizes = [(0, 96, 64, 1), (0, 1920, 1080, 256), (0, 4096, 4096, 64)]
    for rows in (2, 4, 8):  # forced
        assert all(p["rows"] == rows for p in plans([c + (rows,) for c in sizes]))
    assert [p["rows"] for p in plans([c + (0,) for c in sizes])] == [2, 8, 8]
    # level sizes and grids: 64 x 4 threads, 4 pixels of `rows` rows per thread, both pyramids of a stream
    for lvl, w0, h0, batch, rows, w, h in ((0, 1920, 1080, 1, 2, 960, 540), (1, 1920, 1080, 1, 2, 480, 270), (2, 1920, 1080, 8, 2, 240, 135),
                                           (0, 1920, 1080, 256, 8, 960, 540), (0, 1533, 903, 3, 2, 767, 452), (1, 1533, 903, 3, 2, 384, 226),
                                           (3, 1533, 903, 3, 2, 96, 57), (0, 1533, 903, 3, 4, 767, 452), (0, 1, 1, 1, 2, 1, 1)):
        p = plans([(lvl, w0, h0, batch, rows if (lvl, batch) == (0, 3) else 0)])[0]
        assert (p["w"], p["h"], p["rows"]) == (w, h, rows), p
        assert (p["block_x"], p["block_y"]) == (64, 4), p
        assert (p["grid_x"], p["grid_y"], p["grid_z"]) == (-(-w // 256), -(-h // (4 * rows)), 2 * batch), p
    assert [p["ring_groups"] for p in plans([(0, 96, 64, b, 0) for b in (1, 15, 16, 256)])] == [32, 32, 4, 4]


def test_roi_warp(probe):
    # 16 x 16 threads, 8 pixels of one row per thread: 128 x 16 pixels per workgroup; XCD bands: rows of workgroups padded to a multiple of 8
    cases = [(1636, 902, 256, 0), (1636, 902, 256, 1), (128, 16, 1, 0), (129, 17, 1, 0), (129, 17, 1, 1), (96, 128, 3, 1), (96, 129, 3, 1), (96, 129, 3, 0)]
    want = [(13, 57, 256, 0), (13, 64, 256, 1), (1, 1, 1, 0), (2, 2, 1, 0), (2, 8, 1, 1), (1, 8, 3, 1), (1, 16, 3, 1), (1, 9, 3, 0)]
    for c, w, r in zip(cases, want, ints(probe, "w", cases)):
        assert r[:2] == [16, 16] and tuple(r[2:]) == w, (c, r)


def test_ransac(probe):
    def plans(cases):
        return [dict(zip(["fused", "glue", "glue_ran", "try_attribute"], r)) for r in ints(probe, "r", cases)]

    # (max_n, glue, workspace given, attribute state, path)
    for path in (0, 1, 2):
        a, b = plans([(3072, 0, 0, 1, path), (3073, 0, 0, 1, path)])
        assert a["fused"] == (path != 1) and b["fused"] == 0, (path, a, b)
    # the dynamic-LDS attribute of the device: not asked yet -> ask first; refused -> the three kernels
    assert plans([(100, 1, 1, 0, 0)])[0] == dict(fused=1, glue=1, glue_ran=1, try_attribute=1)
    assert plans([(100, 1, 1, 1, 0)])[0] == dict(fused=1, glue=1, glue_ran=1, try_attribute=0)
    assert plans([(100, 1, 1, -1, 0)])[0] == dict(fused=0, glue=0, glue_ran=0, try_attribute=0)
    assert plans([(100, 1, 1, -1, 2)])[0]["fused"] == 0 and plans([(3073, 1, 1, 0, 2)])[0]["try_attribute"] == 0
    # the glue runs only as the epilogue of the fused kernel, and only with the streams' workspaces
    for glue, ws, state, path, want in ((1, 1, 1, 0, (1, 1, 1)), (2, 1, 1, 0, (1, 2, 1)), (2, 1, 1, 2, (1, 2, 1)), (0, 1, 1, 0, (1, 0, 0)), (1, 0, 1, 0, (1, 0, 0)),
                                        (2, 0, 1, 0, (1, 0, 0)), (1, 1, 1, 1, (0, 0, 0)), (2, 1, -1, 0, (0, 0, 0))):
        p = plans([(2000, glue, ws, state, path)])[0]
        assert (p["fused"], p["glue"], p["glue_ran"]) == want, (glue, ws, state, path, p)
    assert plans([(4000, 1, 1, 1, 0)])[0] == dict(fused=0, glue=0, glue_ran=0, try_attribute=0)


def test_track_order_session_and_msv(probe):
    # spatial order from 24 000 tracks in flight; the hook's value goes to the kernel as it is
    cases = [(1, 23999, -1), (1, 24000, -1), (12, 2000, -1), (11, 2000, -1), (65535, 65535, -1), (256, 2000, 0), (1, 10, 1), (1, 10, 0), (256, 2000, 1)]
    assert [r[0] for r in ints(probe, "o", cases)] == [0, 1, 1, 0, 1, 0, 1, 0, 1]
    # one session kernel up to 4096 track slots per stream, else three launches
    assert [r[0] for r in ints(probe, "s", [(1,), (4096,), (4097,), (20000,)])] == [1, 1, 3, 3]
    # fcnMSV1_t fires at frame msv_frame: at least 1, at most 2047 (2048 frames), and inside the history
    cases = [(0, 10), (1, 10), (9, 10), (10, 10), (2047, 4000), (2048, 4000), (-1, 10)]
    assert [r[0] for r in ints(probe, "m", cases)] == [0, 1, 1, 0, 1, 0, 0]
