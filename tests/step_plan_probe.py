"""What the tests of the step plan share (velocity_amd/csrc/vh_step_plan.hpp): a small program that g++ compiles against the header and that prints the
plan of a launch for the sizes and the tuning on its command line, and its output as dicts.  No GPU, no HIP: the GPU test asks it what the library
must have launched."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "velocity_amd", "csrc")

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "vh_step_plan.hpp"
int main(int argc, char** argv)
{
    for (int a = 1; a < argc; a++) {
        long long v[10] = {0};
        const char kind = argv[a][0];
        sscanf(argv[a] + 2, "%lld,%lld,%lld,%lld,%lld,%lld,%lld,%lld,%lld,%lld", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8, v + 9);
        VhTuning t;
        if (kind == 'l') {  // batch, max_n, win, max_level, lk_force, lk3_tpw, lk3_one_level, lko_min_tracks, lkh_min_tracks (-1: the default), lk_lds_pad
            t.lk_force = (int)v[4]; t.lk3_tpw = (int)v[5]; t.lk3_one_level = (int)v[6]; t.lk_lds_pad = (int)v[9];
            if (v[7] >= 0) t.lko_min_tracks = v[7];
            if (v[8] >= 0) t.lkh_min_tracks = v[8];
            const LkPlan p = lk_plan((int)v[0], (int)v[1], (int)v[2], (int)v[3], t);
            if (p.route != lk_route((int)v[0], (int)v[1], (int)v[2], t) && v[1] > 0) return 3;
            if (strcmp(p.name, lk_route_name(p.route, (int)v[2]))) return 4;
            printf("%d %d %u %u %u %d %d %d %d %d %u %zu %d|%s\n", p.rc, (int)p.route, p.grid_x, p.grid_y, p.block, p.tracks_per_wave, p.waves_per_track, p.tpw,
                   p.one_level, p.strip_win, p.group, p.lds, p.needs_big_lds, p.name);
        } else if (kind == 'p') {  // lvl, max_w0, max_h0, batch, pyr_rows
            t.pyr_rows = (int)v[4];
            const PyrPlan p = pyr_plan((int)v[0], (int)v[1], (int)v[2], (int)v[3], t);
            printf("%d %d %d %u %u %u %u %u %u\n", p.w, p.h, p.rows, p.block_x, p.block_y, p.grid_x, p.grid_y, p.grid_z, p.ring_groups);
        } else if (kind == 'w') {  // max_w, max_h, batch, rw_xcd_bands
            t.rw_xcd_bands = (int)v[3];
            const RoiWarpPlan p = roi_warp_plan((int)v[0], (int)v[1], (int)v[2], t);
            printf("%u %u %u %u %u %d\n", p.block_x, p.block_y, p.grid_x, p.grid_y, p.grid_z, p.xcd_bands);
        } else if (kind == 'r') {  // max_n, glue, glue_ws_given, attribute_state, ransac_path
            t.ransac_path = (int)v[4];
            const RansacPlan p = ransac_plan((int)v[0], (int)v[1], v[2] != 0, (int)v[3], t);
            printf("%d %d %d %d\n", p.fused, p.glue, p.glue_ran, p.try_attribute);
        } else if (kind == 'o') {  // count, mn, klt_order
            t.klt_order = (int)v[2];
            printf("%d\n", klt_track_order((int)v[0], (int)v[1], t));
        } else if (kind == 's') {  // N0
            printf("%d\n", session_frame_plan((int)v[0]));
        } else if (kind == 'm') {  // msv_frame, nhist
            printf("%d\n", sess_msv_fires((int)v[0], (int)v[1]) ? 1 : 0);
        } else if (kind == 'f') {  // win
            printf("%d %d %zu\n", lk_window_fits((int)v[0]) ? 1 : 0, lk_max_window(), lk_per_sample_lds((int)v[0]));
        } else {  // the defaults of the record
            printf("%d %d %d %d %d %d %d %d %d %d %d %lld %lld %d %d %d\n", t.lk_force, t.lk3_tpw, t.lk3_one_level, t.klt_order, t.ransac_path, t.pyr_rows,
                   t.ba_force_valu, t.lko_group, t.lkq_group, t.lk3_group, t.lk_lds_pad, t.lko_min_tracks, t.lkh_min_tracks, t.rw_xcd_bands, t.ba_parts,
                   t.ba_graph_off);
        }
    }
    return 0;
}
"""


def build_probe(d):
    """Compiles the program in directory d -> run(kind, cases): one output line per case."""
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(MAIN)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def run(kind, cases):
        rows = []
        for k in range(0, len(cases), 2000):  # (a command line has a length limit)
            args = [kind + ":" + ",".join(str(int(x)) for x in c) for c in cases[k:k + 2000]]
            rows += subprocess.run([str(exe)] + args, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(rows) == len(cases)
        return rows

    return run


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return build_probe(tmp_path_factory.mktemp("step_plan"))


LK_KEYS = ["rc", "route", "grid_x", "grid_y", "block", "tracks_per_wave", "waves_per_track", "tpw", "one_level", "strip_win", "group", "lds", "needs_big_lds"]


def lk(probe, cases):
    """cases: (batch, max_n, win) + optional max_level, force, tpw hook, one-level switch, k_lk_o threshold, k_lk_h threshold, LDS pad"""
    dflt = (-1, 0, 0, 1, -1, -1, 0)
    out = []
    for row in probe("l", [tuple(c) + dflt[len(c) - 3:] for c in cases]):
        nums, name = row.split("|")
        p = dict(zip(LK_KEYS, (int(x) for x in nums.split())))
        p["name"] = name
        out.append(p)
    return out


def ints(probe, kind, cases):
    return [[int(x) for x in row.split()] for row in probe(kind, cases)]
