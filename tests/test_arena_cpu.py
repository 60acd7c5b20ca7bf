"""The carver every host layout goes through (velocity_amd/csrc/vh_arena.hpp), checked without a GPU: a small program compiled with g++ against the header
runs a sequence of takes twice -- sizes only (null base), then on a real block -- and prints the offsets.  The expectations are written out here by hand."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "velocity_amd", "csrc")

# argv: a list of takes "<type><count>" (b: uint8_t, h: uint16_t, i: int, d: double, q: a 24-byte struct); "x<count>" is a take<double> of SIZE_MAX / 8 - count
# objects, i.e. one whose byte count does not fit beside what has been taken.  Output, one line per take: the size-only pass's offset before the take, whether it
# returned null, the pointer pass's offset of the returned pointer from the base (-1: null) and its address modulo 256; then "total <size-only> <pointer>".
MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include "vh_arena.hpp"
struct Q { double a; int b[4]; };
static_assert(sizeof(Q) == 24, "the probe's odd-sized record");
template <class T> static void* take(VhCarver& A, size_t n) { return A.take<T>(n); }
static void* one(VhCarver& A, const char* arg)
{
    const size_t n = strtoull(arg + 1, nullptr, 10);
    switch (arg[0]) {
    case 'b': return take<uint8_t>(A, n);
    case 'h': return take<uint16_t>(A, n);
    case 'i': return take<int>(A, n);
    case 'd': return take<double>(A, n);
    case 'q': return take<Q>(A, n);
    default: return take<double>(A, SIZE_MAX / 8 - n);
    }
}
int main(int argc, char** argv)
{
    char* block = static_cast<char*>(aligned_alloc(256, 1 << 20));  // never touched: only addresses are compared
    VhCarver sizes(nullptr), ptrs(block);
    for (int a = 1; a < argc; a++) {
        const size_t before = sizes.off;
        const void* p0 = one(sizes, argv[a]);
        const char* p1 = static_cast<const char*>(one(ptrs, argv[a]));
        printf("%zu %d %td %d\n", before, p0 == nullptr, p1 ? p1 - block : (ptrdiff_t)-1, p1 ? (int)(reinterpret_cast<uintptr_t>(p1) % 256) : 0);
    }
    printf("total %zu %zu %d\n", sizes.bytes(), ptrs.bytes(), sizes.bytes() == VH_CARVE_OVERFLOW);
    free(block);
    return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("arena")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(MAIN)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def run(takes):
        out = subprocess.run([str(exe)] + list(takes), capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(takes) + 1
        rows = [[int(x) for x in line.split()] for line in out[:-1]]
        return rows, [int(x) for x in out[-1].split()[1:]]

    return run


def test_the_carver_is_plain_cxx17(tmp_path):
    """g++ compiles the header on its own; nothing of HIP stands above the guard that separates the carver from the owners."""
    src = tmp_path / "alone.cpp"
    src.write_text('#include "vh_arena.hpp"\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", CSRC, str(src)], check=True)
    text = open(os.path.join(CSRC, "vh_arena.hpp")).read()
    carver = text[:text.index("#ifdef __HIPCC__")]
    includes = [line for line in carver.splitlines() if line.lstrip().startswith("#include")]
    assert includes and not any("hip" in line.lower() or "vh_" in line for line in includes)


# counts of 0 and 1, a non-multiple of 256, a double after a single byte, an odd-sized record; the offsets by hand (every take rounds up to 256)
SEQUENCE = ["b1", "d1", "b0", "i0", "b257", "i64", "i65", "q11", "d0", "h128", "h129"]
OFFSETS = [0, 256, 512, 512, 512, 1024, 1280, 1792, 2304, 2304, 2560]
TOTAL = 3072


def test_sizing_equals_carving(probe):
    rows, (sized, carved, overflow) = probe(SEQUENCE)
    assert [r[0] for r in rows] == OFFSETS and [r[2] for r in rows] == OFFSETS
    assert all(r[1] == 1 for r in rows), "the size-only pass hands out null"
    assert all(r[3] == 0 for r in rows), "every pointer is aligned to 256"
    assert sized == carved == TOTAL and not overflow


def test_a_zero_count_take_moves_nothing(probe):
    rows, (sized, carved, _) = probe(["i3", "b0", "d0", "i3"])
    assert [r[2] for r in rows] == [0, 256, 256, 256]  # the current position, three times
    assert sized == carved == 512


def test_overflow_is_reported_not_wrapped(probe):
    # SIZE_MAX / 8 doubles are 2^64 - 8 bytes: beside the 256 already taken (and the rounding) they do not fit
    rows, (sized, carved, overflow) = probe(["b1", "x0", "b1"])
    assert overflow and sized == carved == 2**64 - 1
    assert rows[1][2] == -1 and rows[2][2] == -1, "an overflowed carver hands out nothing more"
    # the largest take that still fits stays exact: 2^61 - 32 doubles = 2^64 - 256 bytes from offset 0
    _, (sized, _, overflow) = probe(["x31"])
    assert not overflow and sized == 2**64 - 256
    _, (sized, _, overflow) = probe(["x30"])
    assert overflow and sized == 2**64 - 1


def match_total(px, budget):
    """{0, px, 2 px, 8 budget} bytes, each rounded up to 256: one level-0 image of match_carve (no image of its own, mask, box sums, keypoints)."""
    up = lambda v: (v + 255) // 256 * 256
    return up(0) + up(px) + up(2 * px) + up(8 * budget)


def test_the_match_carve_sequence(probe):
    for px, budget, want in ((1, 1, 768), (257, 1, 1536), (257, 33, 1792)):
        assert match_total(px, budget) == want  # the helper agrees with the figures written here by hand
        takes = ["b0", "b%d" % px, "h%d" % px, "i%d" % (2 * budget)]  # (float and int are both 4 bytes)
        rows, (sized, carved, _) = probe(takes)
        assert sized == carved == want, (px, budget)
        assert rows[0][2] == rows[1][2] == 0, "the absent level-0 image shares the mask's position"
