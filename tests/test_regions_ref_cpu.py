"""tests/regions_ref.py -- the restatement the GPU test of the owned-region launches (tests/test_gpu_region_steps.py) measures the
device against -- held to the library's closed forms and to figures worked out by hand.  No GPU.

(1) Per axis it agrees with ``_capi.owned_range`` / ``_capi.region_rows`` (csrc/region.h region_own / region_down) on the extent lists
of tests/test_regions_cpu.py, with and without the deduplicated last tile.  (2) On the pages of the GPU test every table covers the
needed box, stays inside the tensor, and counts at least the pixels it writes; a tile that owns nothing has no entry anywhere.
(3) Two axes are pinned level by level, so that the restatement cannot drift together with the header."""
import numpy as np
import pytest

import regions_ref as rr
import test_regions_cpu as trc
from sbb_textline_detection_amd import _capi

AXES = [(448, 44, trc.EXTENTS_448), (224, 22, list(range(224, 1100, 13))), (320, 48, list(range(320, 1500, 29))), (480, 48, list(range(480, 2000, 41)))]
# (model side, classes, page rows, page columns) of tests/test_gpu_region_steps.py
PAGES = [(224, 583, 700), (224, 404, 405), (448, 1000, 1234)]


def level_sizes(side, levels=5):
    return [(side >> k, side >> k) for k in range(levels)]


def _same(a, b):
    return (a[0] >= a[1] and b[0] >= b[1]) or tuple(a) == tuple(b)          # every empty range is the same range


@pytest.mark.parametrize("tile,margin,extents", AXES, ids=[f"{a[0]}-{a[1]}" for a in AXES])
def test_axis_functions_agree_with_the_library(tile, margin, extents):
    sizes = [tile >> k for k in range(5)]
    seen_dedupe = seen_empty = 0
    for extent in extents:
        n_full = rr.axis_count(extent, tile, margin)
        n_short = rr.axis_count(extent, tile, margin, dedupe=True)
        assert n_full == len(trc.tiling.axis_tiles(extent, tile, margin)) and n_short in (n_full, n_full - 1)
        seen_dedupe += n_short < n_full
        for n in sorted({n_full, n_short}):
            a = rr.Axis(extent, tile, margin, n)
            for t in range(n):
                lib = _capi.owned_range(extent, tile, margin, n, t)
                assert _same(rr.own(a, t), lib), (extent, n, t, rr.own(a, t), lib)
                seen_empty += lib[0] >= lib[1]
                rows = _capi.region_rows(extent, tile, margin, n, t, sizes)
                for k in range(5):
                    assert _same(rr.needed(a, t, k, sizes), rows[k]), (extent, n, t, k, rr.needed(a, t, k, sizes), rows[k].tolist())
    assert seen_dedupe > 0 and seen_empty > 0                                # the lists reach both regimes


def _geoms():
    for side, hp, wp in PAGES:
        for dedupe in (False, True):
            yield side, hp, wp, dedupe, rr.make_geom(hp, wp, side, side, level_sizes(side), dedupe)


def test_page_geometries_are_the_ones_the_gpu_test_describes():
    g = {(s, hp, wp, d): geom for s, hp, wp, d, geom in _geoms()}
    a, a_full = g[(224, 583, 700, True)], g[(224, 583, 700, False)]
    assert (a.ax.n, a.ay.n) == (4, 3) and (a_full.ax.n, a_full.ay.n) == (4, 4)                 # rows: tile 2 is clamped to 359 already, tile 3 repeats it
    assert [rr.origin(a_full.ay, t) for t in range(4)] == [0, 180, 359, 359] and rr.own(a_full.ay, 2) == (0, 0)
    assert [rr.origin(a.ax, t) for t in range(4)] == [0, 180, 360, 476]                        # columns: first, interior, short penultimate, clamped last
    assert [rr.own(a.ax, t) for t in range(4)] == [(0, 202), (22, 202), (22, 138), (22, 224)]
    b, b_full = g[(224, 404, 405, True)], g[(224, 404, 405, False)]
    assert (b_full.ax.n, b_full.ay.n) == (3, 3) and (b.ax.n, b.ay.n) == (3, 2)                 # 404 repeats its clamped tile; 405 clamps to 181:
    assert rr.origin(b_full.ay, 1) == rr.origin(b_full.ay, 2) == 180 and rr.own(b_full.ay, 1) == (0, 0)
    assert rr.origin(b.ax, 2) == 181 and rr.own(b.ax, 1) == (22, 23)                           # tile 1 keeps ONE column
    c = g[(448, 1000, 1234, True)]
    assert (c.ax.n, c.ay.n) == (4, 3) and g[(448, 1000, 1234, False)] == c


@pytest.mark.parametrize("side,hp,wp,dedupe", [(s, hp, wp, d) for s, hp, wp, d, _ in _geoms()], ids=lambda v: str(v))
def test_tables_cover_the_needed_box_inside_the_tensor(side, hp, wp, dedupe):
    geom = rr.make_geom(hp, wp, side, side, level_sizes(side), dedupe)
    owns = np.zeros((hp, wp), np.int32)
    for g in range(geom.tpp):
        i, j = rr.grid_ij(geom, g)
        ylo, yhi, xlo, xhi = rr.needed_box(geom, g, 0)
        owns[rr.origin(geom.ay, j) + ylo:rr.origin(geom.ay, j) + yhi, rr.origin(geom.ax, i) + xlo:rr.origin(geom.ax, i) + xhi] += 1
        empty = yhi <= ylo
        assert empty == (rr.own(geom.ay, j) == (0, 0) or rr.own(geom.ax, i) == (0, 0))
        for level in range(len(geom.Rh)):
            box = rr.needed_box(geom, g, level)
            need = rr.needed_mask(geom, g, level)
            assert need.sum() == (box[1] - box[0]) * (box[3] - box[2]) and (need.sum() == 0) == empty
            for kind in (0, 1):
                if (kind == 0 and min(geom.Rh[level], geom.Rw[level]) < 16) or (kind == 1 and level == 0):
                    continue                                                 # (no such launch: the tail has tiles only, a tile is 16 x 16)
                e = rr.entries(geom, g, level, kind)
                f = rr.footprint(geom, g, level, kind)                       # (asserts that every entry lies inside the tensor)
                assert f.shape == (geom.Rh[level], geom.Rw[level])
                assert not (need & ~f).any(), (g, level, kind)
                assert len(e) * (4 if kind else 256) >= f.sum(), (g, level, kind)
                assert (len(e) == 0) == empty and (f.sum() == 0) == empty, (g, level, kind)
                if kind == 1:                                                # the four classes never share a pixel: the count is exact
                    assert len(e) * 4 == f.sum()
                    ys, xs = np.nonzero(f)
                    assert (ys.max() + 1 - ys.min()) % 2 == 0 and (xs.max() + 1 - xs.min()) % 2 == 0 if len(e) else True
    assert (owns == 1).all()                                                 # the owned boxes tile the page


def test_pinned_boxes_of_two_axes():
    """Worked out from the header's rules by hand (mid = 448 - 88 = 360):
    extent 1234: origins 0, 360, 720, 786; tile 2 keeps [44, 404) cut at tile 3's first kept pixel 786 + 44 - 720 = 110;
    extent 1000: origins 0, 360, 552; tile 1 keeps [44, 404) cut at 552 + 44 - 360 = 236;
    a level below reads rows (lo - 1) >> 1 ... hi >> 1 (the last row hi - 1 reads up to hi, which is row hi >> 1 below)."""
    sizes = [448, 224, 112, 56, 28]
    a = rr.Axis(1234, 448, 44, 4)
    assert [rr.needed(a, 2, k, sizes) for k in range(5)] == [(44, 110), (21, 56), (10, 29), (4, 15), (1, 8)]
    b = rr.Axis(1000, 448, 44, 3)
    assert [rr.needed(b, 1, k, sizes) for k in range(5)] == [(44, 236), (21, 119), (10, 60), (4, 31), (1, 16)]
    assert _capi.region_rows(1234, 448, 44, 4, 2, sizes).tolist() == [[44, 110], [21, 56], [10, 29], [4, 15], [1, 8]]
    assert _capi.region_rows(1000, 448, 44, 3, 1, sizes).tolist() == [[44, 236], [21, 119], [10, 60], [4, 31], [1, 16]]
    geom = rr.make_geom(1000, 1234, 448, 448, [(s, s) for s in sizes])
    g = 2 * geom.ny + 1                                                      # x tile 2, y tile 1
    assert [rr.needed_box(geom, g, k) for k in range(5)] == [(44, 236, 44, 110), (21, 119, 21, 56), (10, 60, 10, 29), (4, 31, 4, 15), (1, 16, 1, 8)]


def test_table_layouts_on_small_cases():
    assert rr.tile_origins(44, 110, 16, 448) == [32, 48, 64, 80, 96] and rr.tile_origins(44, 110, 2, 448) == [44, 60, 76, 92, 108]
    assert rr.tile_origins(200, 224, 2, 224) == [200, 208] and rr.tile_origins(21, 21, 2, 224) == []       # the last tile pulled inside
    assert rr.even(3, 8, 28) == (3, 9) and rr.even(21, 28, 28) == (20, 28) and rr.even(4, 8, 28) == (4, 8)
    assert rr.class_rows(3, 8, 0, 28) == [2, 3, 4] and rr.class_rows(3, 8, 1, 28) == [1, 2, 3]              # rows 4 6 8 / 3 5 7
    assert rr.down(44, 110, 224) == (21, 56) and rr.down(0, 224, 112) == (0, 112) and rr.down(5, 5, 112) == (0, 0)


# ------------------------------------------------------------------------------------------------ the header itself, compiled for the host
# region_even, region_tiles16, region_tile_origin and region_entries have no export: a small host program includes csrc/region.h and
# prints them for a page geometry (hipcc compiles host code without a GPU; no HIP call is made).
_HEADER_PROBE = r"""
#include "region.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace sbbseg;
int main(int argc, char** argv)
{
    if (argc < 9) return 2;
    RegionGeom g;
    memset(&g, 0, sizeof(g));
    int a = 1;
    const int Hp = atoi(argv[a++]), Wp = atoi(argv[a++]), H = atoi(argv[a++]), W = atoi(argv[a++]), margin = atoi(argv[a++]);
    const int nx = atoi(argv[a++]), ny = atoi(argv[a++]);
    g.n_levels = atoi(argv[a++]);
    if (g.n_levels > kRegionMaxLevels || argc != 9 + 2 * g.n_levels) return 2;
    g.ax = {Wp, W, margin, W - 2 * margin, nx};
    g.ay = {Hp, H, margin, H - 2 * margin, ny};
    g.tpp = nx * ny; g.ny = ny;
    for (int L = 0; L < g.n_levels; ++L) { g.Rh[L] = atoi(argv[a++]); g.Rw[L] = atoi(argv[a++]); g.align_x[L] = L == 0 ? 16 : 2; }
    for (int kind = 0; kind < 2; ++kind)
        for (int L = 0; L < g.n_levels; ++L) {
            g.kind[L] = kind;
            for (int t = 0; t < g.tpp; ++t) {
                const int i = t / g.ny, j = t % g.ny;
                int ylo, yhi, xlo, xhi;
                region_needed(g, i, j, L, ylo, yhi, xlo, xhi);
                printf("%d %d %d  %d %d %d %d  %d ", kind, L, t, ylo, yhi, xlo, xhi, region_entries(g, i, j, L));
                if (kind == 0) {
                    const int ty = region_tiles16(ylo, yhi, 2), tx = region_tiles16(xlo, xhi, g.align_x[L]);
                    printf(" %d %d ", ty, tx);
                    for (int k = 0; k < ty; ++k) printf(" %d", region_tile_origin(ylo, 2, k, g.Rh[L]));
                    for (int k = 0; k < tx; ++k) printf(" %d", region_tile_origin(xlo, g.align_x[L], k, g.Rw[L]));
                } else {
                    region_even(ylo, yhi, g.Rh[L]);
                    region_even(xlo, xhi, g.Rw[L]);
                    printf(" %d %d %d %d", ylo, yhi, xlo, xhi);
                }
                printf("\n");
            }
        }
    return 0;
}
"""


@pytest.fixture(scope="module")
def header_probe(tmp_path_factory):
    import os
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("region_header")
    (d / "probe.cpp").write_text(_HEADER_PROBE)
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sbb_textline_detection_amd", "csrc")
    res = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-I", csrc, str(d / "probe.cpp"), "-o", str(d / "probe")],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]

    def run(geom, model_h, model_w):
        args = [geom.ay.extent, geom.ax.extent, model_h, model_w, geom.ax.margin, geom.ax.n, geom.ay.n, len(geom.Rh)]
        for h, w in zip(geom.Rh, geom.Rw):
            args += [h, w]
        out = subprocess.run([str(d / "probe")] + [str(v) for v in args], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        return [[int(v) for v in line.split()] for line in out.stdout.splitlines()]
    return run


@pytest.mark.parametrize("side,hp,wp,dedupe", [(s, hp, wp, d) for s, hp, wp, d, _ in _geoms()] + [(448, 1441, 809, True), (224, 225, 672, False)],
                         ids=lambda v: str(v))
def test_header_tables_equal_the_restatement(header_probe, side, hp, wp, dedupe):
    """region_needed, region_entries, the kind-0 tile origins and the kind-1 even ranges of csrc/region.h, for every tile and level."""
    geom = rr.make_geom(hp, wp, side, side, level_sizes(side), dedupe)
    rows = header_probe(geom, side, side)
    assert len(rows) == 2 * len(geom.Rh) * geom.tpp
    for row in rows:
        kind, L, g = row[:3]
        where = (kind, L, g)
        box = rr.needed_box(geom, g, L)
        assert tuple(row[3:7]) == box or (row[4] <= row[3] and box == (0, 0, 0, 0)), (where, row[3:7], box)
        if (kind == 0 and min(geom.Rh[L], geom.Rw[L]) < 16) or (kind == 1 and L == 0):
            continue
        e = rr.entries(geom, g, L, kind)
        assert row[7] == len(e), (where, row[7], len(e))
        if kind == 0:
            ty, tx = row[8:10]
            ys, xs = row[10:10 + ty], row[10 + ty:10 + ty + tx]
            assert [(y, x) for y in ys for x in xs] == e, (where, ys, xs)
        elif e:
            ylo, yhi, xlo, xhi = row[8:12]
            assert (ylo, yhi) == rr.even(box[0], box[1], geom.Rh[L]) and (xlo, xhi) == rr.even(box[2], box[3], geom.Rw[L]), (where, row[8:12], box)
            assert (yhi - ylo) * (xhi - xlo) == 4 * len(e)
