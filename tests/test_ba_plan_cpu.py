"""The host decisions of the batched bundle adjustment (velocity_amd/csrc/vh_ba_plan.hpp), checked without a GPU: a small program compiled with g++
against the header prints the plan at every route boundary, the carved workspace and its size.  The expectations are DESIGN.md section 6 and
include/velocity_hip.h, written out here; the sizes are the figures vh_nls_batch_workspace returned before the layout had one description."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["camR", "r", "Jp", "Jc", "tp", "Lc", "Y", "Spart", "Rpart", "Dpart", "Sfull", "dc", "done"]  # the documented order (done = start of the flag block)

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "vh_ba_plan.hpp"
int main(int argc, char** argv)
{
    for (int a = 1; a < argc; a++) {
        int v[8] = {0};
        char kind = argv[a][0];
        sscanf(argv[a] + 2, "%d,%d,%d,%d,%d,%d,%d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6);
        if (kind == 'p') {  // nt, nc, nwin, model, force_valu, dbg
            BaPlan p;
            const int nparts = ba_nparts(v[0], v[1], v[2], 0);
            const int rc = ba_plan(v[0], v[1], nparts, v[2], v[3], v[4], v[5], &p);
            printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %zu %zu %d\n", rc, p.nq, (int)p.schur, (int)p.solve, (int)p.update, p.zmode, p.npass, p.nsplit, p.nm,
                   p.npairs, p.nzb, p.upd_blocks, p.reduce_ns, p.needs_big_lds, p.lds_valu, p.lds_mfma, p.nparts);
        } else {  // nt, nc, nwin: nparts, sized bytes, then the carved fields as byte offsets from the base
            const int nparts = ba_nparts(v[0], v[1], v[2], 0);
            const size_t bytes = ba_workspace_bytes(v[0], v[1], nparts);
            char* base = static_cast<char*>(aligned_alloc(256, bytes));  // never touched: only addresses are compared
            BaFields f;
            const size_t carved = ba_workspace_walk(v[0], v[1], nparts, base, &f);
            const void* q[] = {f.camR, f.r, f.Jp, f.Jc, f.tp, f.Lc, f.Y, f.Spart, f.Rpart, f.Dpart, f.Sfull, f.dc, f.done, f.acc, f.ticket, f.rslot};
            printf("%d %zu %zu", nparts, bytes, carved);
            for (const void* x : q) printf(" %td", static_cast<const char*>(x) - base);
            printf("\n");
            free(base);
        }
    }
    return 0;
}
"""

VALU, MFMA128, MFMA256, SYRK = range(4)
GJ_MFMA, GJ_VALU, CHOL_LEFT, CHOL_RIGHT = range(4)
POINTS, Z_LATENCY, Z4 = range(3)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("ba_plan")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(MAIN)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "velocity_amd", "csrc"), str(src), "-o", str(exe)], check=True)

    def run(kind, cases):
        out = subprocess.run([str(exe)] + [kind + ":" + ",".join(str(int(x)) for x in c) for c in cases], capture_output=True, text=True, check=True).stdout
        rows = [[int(x) for x in line.split()] for line in out.splitlines()]
        assert len(rows) == len(cases)
        return rows

    return run


def plans(probe, cases):
    keys = ["rc", "nq", "schur", "solve", "update", "zmode", "npass", "nsplit", "nm", "npairs", "nzb", "upd_blocks", "reduce_ns", "needs_big_lds", "lds_valu",
            "lds_mfma", "nparts"]
    return [dict(zip(keys, row)) for row in probe("p", cases)]


def test_the_header_is_plain_cxx17(tmp_path):
    """g++ compiles the header on its own: no HIP include, no getenv (the experiment switches are read by the callers and passed in)."""
    src = tmp_path / "alone.cpp"
    src.write_text('#include "vh_ba_plan.hpp"\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "velocity_amd", "csrc"), str(src)], check=True)
    text = open(os.path.join(ROOT, "velocity_amd", "csrc", "vh_ba_plan.hpp")).read()
    assert "hip/" not in text and "getenv" not in text and "vh_common" not in text


# (nc, model, force_valu, dbg) -> (nq or None, Schur, solve or None); rc = -3 where the solve is refused
ROUTES = [
    ((1, 0, 0, 0), (6, MFMA128, GJ_MFMA)),
    ((20, 0, 0, 0), (120, MFMA128, GJ_MFMA)),
    ((20, 0, 0, 64), (120, MFMA128, GJ_VALU)),
    ((21, 0, 0, 0), (126, MFMA128, GJ_VALU)),
    ((22, 0, 0, 0), (132, MFMA256, CHOL_LEFT)),
    ((22, 0, 0, 256), (132, MFMA256, CHOL_RIGHT)),
    ((42, 0, 0, 0), (252, MFMA256, CHOL_LEFT)),
    ((43, 0, 0, 0), (258, SYRK, None)),
    ((128, 0, 1, 0), (768, VALU, None)),
    ((129, 0, 1, 0), (774, SYRK, None)),  # the hook is ignored where the VALU Schur kernel does not exist
    ((255, 0, 0, 0), (1530, SYRK, None)),
    ((256, 0, 0, 0), None),
    ((119, 1, 0, 0), (124, VALU, GJ_MFMA)),
    ((120, 1, 0, 0), (125, VALU, GJ_VALU)),
    ((255, 1, 0, 0), (260, VALU, CHOL_LEFT)),
]


def test_routes_at_every_boundary(probe):
    got = plans(probe, [(100, nc, 1, model, fv, dbg) for (nc, model, fv, dbg), _ in ROUTES])
    for ((nc, model, fv, dbg), want), p in zip(ROUTES, got):
        what = f"nc={nc} model={model} force_valu={fv} dbg={dbg}: {p}"
        if want is None:
            assert p["rc"] == -3, what
            continue
        nq, schur, solve = want
        assert p["rc"] == 0 and p["nq"] == nq and p["schur"] == schur, what
        if solve is not None:
            assert p["solve"] == solve, what
        assert p["zmode"] == (schur != VALU), what
        assert p["update"] == (POINTS if schur == VALU else Z_LATENCY), what
        assert p["reduce_ns"] == (16 if p["nsplit"] >= 128 else 4), what
        # k_ba_schur_mfma<256, *> (more than 64 KB of LDS) and k_ba_chol_left (above 124 unknowns) need their dynamic-LDS limit raised first
        assert p["needs_big_lds"] == (nq > 124 or (schur == MFMA256)), what
        if schur == VALU:
            assert p["npass"] == -(-nq * nq // (256 * 64)) and p["lds_valu"] == 8 * (6 * nq + 12 * (nc + 1) + 16), what
        if schur in (MFMA128, MFMA256):
            assert p["lds_mfma"] <= (64 if schur == MFMA128 else 158) * 1024, what
        if schur != SYRK:
            assert p["nsplit"] == p["nparts"] and p["nzb"] == 0, what
    # the trajectory model and the hook at their largest sizes are not refused
    assert all(p["rc"] == 0 for p in plans(probe, [(100, 255, 1, 1, 1, 0), (100, 128, 1, 0, 1, 0)]))


def test_update_route(probe):
    cases = [((100, 4, 1, 0, 0, 0), Z_LATENCY), ((20000, 4, 1, 0, 0, 0), Z_LATENCY), ((20001, 4, 1, 0, 0, 0), Z4), ((100, 4, 201, 0, 0, 0), Z4),
             ((100, 50, 1, 0, 0, 0), Z_LATENCY), ((20001, 50, 1, 0, 0, 0), Z4),
             ((100, 4, 1, 0, 1, 0), POINTS), ((20001, 4, 1, 0, 1, 0), POINTS), ((100, 4, 201, 0, 1, 0), POINTS), ((100, 4, 1, 1, 0, 0), POINTS),
             ((20001, 128, 1, 0, 1, 0), POINTS)]
    for (c, want), p in zip(cases, plans(probe, [c for c, _ in cases])):
        assert p["rc"] == 0 and p["update"] == want, (c, p)
        assert 1 <= p["upd_blocks"] <= 256, (c, p)


def test_syrk_grids_are_never_empty(probe):
    cases = [(nt, nc, nwin, 0, 0, 0) for nc in (43, 128, 129, 255) for nt, nwin in ((1, 1), (1, 65535), (100, 65535), (11, 2), (5000, 1), (5000, 64))]
    for c, p in zip(cases, plans(probe, cases)):
        assert p["rc"] == 0 and p["schur"] == SYRK, (c, p)
        assert 1 <= p["nsplit"] <= max(1, p["nparts"]) and 1 <= p["nzb"] <= 256, (c, p)
        assert p["nm"] == -(-p["nq"] // 128) and p["npairs"] == p["nm"] * (p["nm"] + 1) // 2, (c, p)


# (nt, nc, nwin) -> bytes of one window's workspace as the library sized it before this header existed (vh_nls_batch_workspace; the 64-window rows with the
# per-window cap of vh_nls_batch_multi: 512 / 64 < 16 -> 16 partial systems)
SIZES = {
    (1, 1, 1): 5120, (40, 3, 1): 57600, (300, 24, 1): 5443072, (200, 42, 1): 9247232, (200, 43, 1): 13301248, (60, 128, 1): 32284928,
    (1000, 9, 1): 4470272, (16, 255, 1): 60732672,
    (2000, 4, 64): 2980864, (4096, 2, 64): 3464448, (8000, 9, 64): 24152832,
}


def test_the_size_is_what_it_always_was(probe):
    for c, row in zip(SIZES, probe("w", list(SIZES))):
        assert row[1] == SIZES[c], (c, row[:3])
    assert [row[0] for row in probe("w", [(2000, 4, 64), (4096, 2, 64), (8000, 9, 64), (8000, 9, 512), (8000, 9, 16), (100, 9, 64)])] == [16, 16, 16, 16, 32, 6]


def test_sizing_equals_carving(probe):
    shapes = [(1, 1), (40, 3), (300, 24), (200, 42), (200, 43), (60, 128), (1000, 9), (16, 255)]
    for (nt, nc), row in zip(shapes, probe("w", [(nt, nc, 1) for nt, nc in shapes])):
        nparts, sized, carved = row[:3]
        off = dict(zip(FIELDS + ["acc", "ticket", "rslot"], row[3:]))
        nq, m, big = 6 * nc, nt * (nc + 1), 6 * nc > 252
        doubles = {"camR": 36 * (nc + 1), "r": 2 * m, "Jp": 6 * m, "Jc": 12 * m, "tp": 3 * nt, "Lc": 6 * nt, "Y": 3 * nq * nt, "Spart": nparts * nq * nq,
                   "Rpart": (max(nparts, 256) if big else nparts) * nq, "Dpart": 256 * 36 * nc if big else 0, "Sfull": nq * (nq + 1) + 4, "dc": nq,
                   "done": 32}  # vh_ba.hpp, field by field
        assert sized == carved, (nt, nc)
        assert off["camR"] == 0
        for a, b in zip(FIELDS, FIELDS[1:]):
            assert off[a] % 256 == 0 and off[b] % 256 == 0, (nt, nc, a, b)
            assert off[a] + 8 * doubles[a] <= off[b], (nt, nc, a, b, off)  # in order, no overlap
            assert off[b] - off[a] < 8 * doubles[a] + 256, (nt, nc, a, b, off)  # and rounded up to 256 bytes, no further
        assert off["acc"] == off["Sfull"] + 8 * nq * (nq + 1)  # [Sfull | acc]: one all-reduce span
        assert off["ticket"] == off["done"] + 16 and off["rslot"] == off["done"] + 64
        assert off["done"] + 8 * 32 + 1024 == sized, (nt, nc)
