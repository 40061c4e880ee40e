"""csrc/tile_walk.h -- the XCD-contiguous tile walk of the persistent kernels and the grid their launch functions size for it -- without a
GPU.

A small host program includes the header and, for ``num_cus`` in {8, 32, 256} and every ``n_tiles`` in 0 .. 1199, takes
``grid = xcd_grid(n_tiles, num_cus)`` and prints, per block, ``my_tiles``, the tiles of ``tile_at(0 .. my_tiles - 1)`` and
``tile_at_clamped`` at and past the end.  It is built with the address and undefined-behaviour sanitizers (a stand-alone host program:
nothing is preloaded).

The output is held to ``want_walk`` below, a restatement of the formulas every kernel spelled out before the header existed
(``per_xcd``, ``xcd_lo``, ``xcd_hi``, ``my_tiles`` and the two ``tile_at`` flavours, e.g. csrc/dec_halo_x3.hip at 4378f1c), and to the
properties the kernels and their launch functions rely on."""
import os
import shutil
import subprocess

import pytest

NUM_CUS = (8, 32, 256)
N_TILES = range(1200)

_PROBE = r"""
#include "tile_walk.h"
#include <cstdio>
using namespace sbbseg;

struct U3 { unsigned x; };

int main()
{
    const int cus[3] = {8, 32, 256};
    for (int num_cus : cus)
        for (int n_tiles = 0; n_tiles < 1200; ++n_tiles) {
            const int grid = xcd_grid(n_tiles, num_cus);
            printf("L %d %d %d\n", num_cus, n_tiles, grid);
            for (int b = 0; b < grid; ++b) {
                const XcdWalk w = xcd_walk(n_tiles, U3{(unsigned)b}, U3{(unsigned)grid});
                printf("B %d %d %d %d %d", b, w.xcd_lo, w.slot, w.GX, w.my_tiles);
                for (int it = 0; it < w.my_tiles; ++it) printf(" %d", w.tile_at(it));
                // the clamped flavour: equal inside the range, the last tile at and past its end (only asked of a block that has tiles)
                if (w.my_tiles > 0) {
                    for (int it = 0; it < w.my_tiles; ++it)
                        if (w.tile_at_clamped(it) != w.tile_at(it)) { printf(" clamped-differs-at-%d", it); return 1; }
                    printf(" | %d %d %d", w.tile_at_clamped(w.my_tiles), w.tile_at_clamped(w.my_tiles + 1), w.tile_at_clamped(w.my_tiles + 1000));
                }
                printf("\n");
            }
        }
    return 0;
}
"""


def want_walk(n, block, grid):
    """(xcd range, my_tiles, tiles) of one block: the formulas as the kernels had them"""
    xcd, slot, GX = block & 7, block >> 3, grid >> 3
    per_xcd = (n + 7) >> 3
    xcd_lo = xcd * per_xcd
    xcd_hi = min(n, xcd_lo + per_xcd)
    my = (xcd_hi - xcd_lo - slot + GX - 1) // GX if xcd_lo + slot < xcd_hi else 0
    return xcd_lo, xcd_hi, slot, GX, my, [xcd_lo + slot + it * GX for it in range(my)]


@pytest.fixture(scope="module")
def launches(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("xcd_walk")
    (d / "probe.cpp").write_text(_PROBE)
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sbb_textline_detection_amd", "csrc")
    # the walk is plain arithmetic: host pass only, and the program never calls the HIP runtime
    res = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                          "-Xarch_host", "-fno-sanitize-recover=all", "-I", csrc, str(d / "probe.cpp"), "-o", str(d / "probe")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    out = subprocess.run([str(d / "probe")], capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, (out.stdout[-300:], out.stderr[-3000:])      # (a sanitizer report ends the program with a status)
    got = {}                                      # (num_cus, n_tiles) -> (grid, [block rows])
    cur = None
    for line in out.stdout.splitlines():
        f = line.split()
        if f[0] == "L":
            cur = (int(f[1]), int(f[2]))
            got[cur] = (int(f[3]), [])
        else:
            head, _, tail = line[2:].partition(" | ")
            v = [int(x) for x in head.split()]
            got[cur][1].append((v[0], v[1], v[2], v[3], v[4], v[5:], [int(x) for x in tail.split()]))
    return got


def test_the_sweep_is_complete(launches):
    assert sorted(launches) == sorted((c, n) for c in NUM_CUS for n in N_TILES)
    assert all([r[0] for r in rows] == list(range(grid)) for grid, rows in launches.values())


def test_grid_is_a_multiple_of_8_within_the_machine(launches):
    for (num_cus, n), (grid, _) in launches.items():
        assert grid % 8 == 0 and grid <= ((num_cus + 7) & ~7), (num_cus, n, grid)
        assert grid == ((min(n, num_cus) + 7) & ~7), (num_cus, n, grid)           # what every launch function spelled out
        assert grid >= min(n, num_cus)


def test_walk_matches_the_kernels_formulas(launches):
    bad = []
    for (num_cus, n), (grid, rows) in launches.items():
        for b, xcd_lo, slot, GX, my, tiles, _ in rows:
            w_lo, _, w_slot, w_GX, w_my, w_tiles = want_walk(n, b, grid)
            if (xcd_lo, slot, GX, my, tiles) != (w_lo, w_slot, w_GX, w_my, w_tiles):
                bad.append((num_cus, n, b, (xcd_lo, slot, GX, my, tiles[:4]), (w_lo, w_slot, w_GX, w_my, w_tiles[:4])))
    assert not bad, (len(bad), bad[:4])


def test_every_tile_is_visited_exactly_once(launches):
    for (num_cus, n), (grid, rows) in launches.items():
        seen = sorted(t for r in rows for t in r[5])
        assert seen == list(range(n)), (num_cus, n, grid)


def test_no_block_leaves_its_xcd_range(launches):
    for (num_cus, n), (grid, rows) in launches.items():
        for b, xcd_lo, slot, GX, my, tiles, _ in rows:
            lo, hi = want_walk(n, b, grid)[:2]
            assert xcd_lo == lo and all(lo <= t < hi for t in tiles), (num_cus, n, b)


def test_clamped_walk_repeats_the_last_tile(launches):
    for (num_cus, n), (grid, rows) in launches.items():
        for b, _, _, _, my, tiles, past in rows:
            if my > 0:
                assert past == [tiles[-1]] * 3, (num_cus, n, b, tiles[-1], past)
            else:
                assert tiles == [] and past == []
