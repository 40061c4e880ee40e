"""Plain restatement of csrc/region.h (owned-region decoder launches), written from the header's comments -- test helper, no GPU.

Where the header has a closed form this file has the loop the closed form stands for: the owned range is read off a painted axis
(every tile pastes its margin-cropped range, later tiles over earlier ones), the rows a level reads are collected tap by tap, the
class grid is filtered by parity.  Only the table layouts the kernels consume are taken over as they are: 16-pixel tiles from the
needed range rounded down to the alignment, the last pulled inside the tensor (kind 0); the range grown to an even length (kind 1).

Geometry: ``make_geom(page_h, page_w, model_h, model_w, level_sizes, dedupe)``; level 0 is the network output, level k the decoder
conv k steps below it.  Grid index g -> (i, j) = (g // ny, g % ny): i along x (outer loop of the reference), j along y.
All ranges are half open, in the coordinates of the level's own tensor."""
import functools
from collections import namedtuple

import numpy as np

Axis = namedtuple("Axis", "extent tile margin n")
Geom = namedtuple("Geom", "ax ay ny tpp Rh Rw")            # Rh / Rw: output rows / columns per level


def axis_count(extent, tile, margin, dedupe=False):
    """Tiles of an axis: ceil(extent / mid) (main.py:246-257); `dedupe` drops the last one when it repeats its neighbour's origin."""
    mid = tile - 2 * margin
    n = 0
    while n * mid < extent:
        n += 1
    if dedupe and n >= 2 and origin(Axis(extent, tile, margin, n), n - 1) == origin(Axis(extent, tile, margin, n), n - 2):
        n -= 1
    return n


def make_geom(page_h, page_w, model_h, model_w, level_sizes, dedupe=False):
    margin = int(0.1 * model_w)                            # main.py:233: from the WIDTH, for both axes
    ax = Axis(page_w, model_w, margin, axis_count(page_w, model_w, margin, dedupe))
    ay = Axis(page_h, model_h, margin, axis_count(page_h, model_h, margin, dedupe))
    return Geom(ax, ay, ay.n, ax.n * ay.n, tuple(int(s[0]) for s in level_sizes), tuple(int(s[1]) for s in level_sizes))


# ------------------------------------------------------------------------------------------------ one axis
def origin(a, t):
    mid = a.tile - 2 * a.margin
    return min(t * mid, a.extent - a.tile)


@functools.lru_cache(maxsize=64)
def paint(a):
    """The paste loop along one axis: owner[q] = the LAST tile whose margin-cropped range covers page coordinate q."""
    owner = [-1] * a.extent
    for s in range(a.n):
        lo = 0 if s == 0 else a.margin
        hi = a.tile if s == a.n - 1 else a.tile - a.margin
        for q in range(origin(a, s) + lo, origin(a, s) + hi):
            owner[q] = s
    assert -1 not in owner, a
    return tuple(owner)


def own(a, t):
    """[lo, hi) in tile coordinates of what the stitch keeps of tile t; (0, 0) when nothing survives."""
    mine = [q for q, s in enumerate(paint(a)) if s == t]
    if not mine:
        return 0, 0
    assert mine == list(range(mine[0], mine[-1] + 1)), (a, t)          # one run
    return mine[0] - origin(a, t), mine[-1] + 1 - origin(a, t)


def down(lo, hi, rows_below):
    """Rows of the level below that rows [lo, hi) read: a zero-padded 3x3 conv over the nearest-x2 upsampling of `rows_below` rows."""
    need = set()
    for y in range(lo, hi):
        for dy in (-1, 0, 1):
            u = y + dy
            if 0 <= u < 2 * rows_below:
                need.add(u >> 1)
    if not need:
        return 0, 0
    return min(need), max(need) + 1


def needed(a, t, level, sizes):
    """Rows of `level` tile t must produce; sizes[k] = rows of level k."""
    lo, hi = own(a, t)
    for k in range(1, level + 1):
        lo, hi = down(lo, hi, sizes[k])
    return lo, hi


def even(lo, hi, rows):
    """kind 1: grown to an even length (upwards while there is room), so that both parities have as many class rows."""
    if (hi - lo) % 2:
        if hi < rows:
            hi += 1
        else:
            lo -= 1
    return lo, hi


def tile_origins(lo, hi, align, rows):
    """kind 0: 16-pixel tiles from `lo` rounded down to `align`, the last pulled inside the tensor."""
    out = []
    if hi <= lo:
        return out
    o = lo - lo % align
    while o < hi:
        out.append(min(o, rows - 16))
        o += 16
    return out


def class_rows(lo, hi, parity, rows):
    """kind 1: rows of the parity class's own grid (row y of it is row 2 y + parity of the tensor)."""
    lo, hi = even(lo, hi, rows)
    return [y >> 1 for y in range(lo, hi) if y % 2 == parity]


# ------------------------------------------------------------------------------------------------ the grid
def grid_ij(geom, g):
    return g // geom.ny, g % geom.ny


def needed_box(geom, g, level):
    """(ylo, yhi, xlo, xhi) of `level` that tile g must produce; all zero for a tile that owns nothing."""
    i, j = grid_ij(geom, g)
    ylo, yhi = needed(geom.ay, j, level, geom.Rh)
    xlo, xhi = needed(geom.ax, i, level, geom.Rw)
    if yhi <= ylo or xhi <= xlo:
        return 0, 0, 0, 0
    return ylo, yhi, xlo, xhi


@functools.lru_cache(maxsize=None)
def entries(geom, g, level, kind):
    """The table entries of tile g at `level`.  kind 0: [(y0, x0)] origins of 16 x 16 output tiles, y outer (x aligned to 16 at
    level 0 -- label rows are stored 16 bytes at a time -- and to 2 elsewhere, y to 2).  kind 1: [{(py, px): (y, x)}], one entry per
    pixel of a parity class's grid holding the pixel of each of the four classes; len() is the count PER CLASS."""
    ylo, yhi, xlo, xhi = needed_box(geom, g, level)
    if yhi <= ylo:
        return []
    R_h, R_w = geom.Rh[level], geom.Rw[level]
    if kind == 0:
        ys = tile_origins(ylo, yhi, 2, R_h)
        xs = tile_origins(xlo, xhi, 16 if level == 0 else 2, R_w)
        return [(y, x) for y in ys for x in xs]
    rows = {p: class_rows(ylo, yhi, p, R_h) for p in (0, 1)}
    cols = {p: class_rows(xlo, xhi, p, R_w) for p in (0, 1)}
    assert len(rows[0]) == len(rows[1]) and len(cols[0]) == len(cols[1])
    return [{(py, px): (rows[py][r], cols[px][c]) for py in (0, 1) for px in (0, 1)}
            for r in range(len(rows[0])) for c in range(len(cols[0]))]


@functools.lru_cache(maxsize=None)
def footprint(geom, g, level, kind):
    """bool [Rh, Rw]: the pixels of the level's tensor the launch writes for tile g."""
    R_h, R_w = geom.Rh[level], geom.Rw[level]
    f = np.zeros((R_h, R_w), bool)
    for e in entries(geom, g, level, kind):
        if kind == 0:
            assert 0 <= e[0] <= R_h - 16 and 0 <= e[1] <= R_w - 16, ("tile outside the tensor", g, level, e)
            f[e[0]:e[0] + 16, e[1]:e[1] + 16] = True
        else:
            for (py, px), (y, x) in e.items():
                assert 0 <= 2 * y + py < R_h and 0 <= 2 * x + px < R_w, ("pixel outside the tensor", g, level, e)
                f[2 * y + py, 2 * x + px] = True
    f.setflags(write=False)                                # (cached: shared among callers)
    return f


def needed_mask(geom, g, level):
    ylo, yhi, xlo, xhi = needed_box(geom, g, level)
    m = np.zeros((geom.Rh[level], geom.Rw[level]), bool)
    m[ylo:yhi, xlo:xhi] = True
    return m
