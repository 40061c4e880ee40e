"""Seeded planes for the device's connected-component labelling (tests/test_cc_planes_cpu.py, tests/test_gpu_components.py): the shapes
a lock-free union-find labeller gets wrong -- runs across 64-pixel chunks, components joined through a diagonal neighbour only, hundreds
of row runs that meet late, islands in holes several deep, holes that open to the frame through one cell, hundreds of equal components.
Everything is generated; nothing here is product code, nothing touches the GPU, and nothing is recorded from the reference.

The entry points apply morphology before they label -- dilate x 6 (one 25 x 25 maximum) for the page box, OPEN then CLOSE with 5 x 5 for
the region calls -- so the INPUT is shaped for the structure to survive it: region planes are drawn on a coarse grid and blown up to 6 - 8
pixels per cell, page-box planes are single pixels and small seeds 25 / 26 apart.  ``region_mask`` / ``page_mask`` give the plane that is
labelled (by the oracle's literal morphology); tests/test_cc_planes_cpu.py checks on it that every family holds what it claims."""
import functools

import numpy as np

from oracle import stage_glue as sg


def up(grid, s):
    """A coarse grid blown up to s x s pixels per cell."""
    return np.kron(np.asarray(grid, np.uint8), np.ones((s, s), np.uint8))


def region_mask(plane, label=1):
    """The 0 / 255 plane the region calls label: class mask, MORPH_OPEN, MORPH_CLOSE (oracle/stage_glue.morph, one 5 x 5 pass each)."""
    p = np.where(np.asarray(plane) == label, 255, 0).astype(np.uint8)
    p = sg.morph(sg.morph(p, "erode", 5, 1), "dilate", 5, 1)
    return sg.morph(sg.morph(p, "dilate", 5, 1), "erode", 5, 1)


def page_mask(plane):
    """The 0 / 255 plane the page box labels: > 0, dilate x 6."""
    return sg.morph(np.where(np.asarray(plane) > 0, 255, 0).astype(np.uint8), "dilate", 5, 6)


def cell_area2(comp):
    """The device's LOWER bound of twice a component's contour area: 2 x 2 cells with four pixels inside count 2, with three 1 (holes not
    filled).  Restated here to check which planes leave the device's ranking open; equal to the contour area for a component without holes."""
    f = np.asarray(comp).astype(np.int64)
    k = f[:-1, :-1] + f[:-1, 1:] + f[1:, :-1] + f[1:, 1:]
    return int(2 * (k == 4).sum() + (k == 3).sum())


# ------------------------------------------------------------------------------------------------ coarse shapes
def spiral_grid(n):
    """A square spiral of one-cell arms and one-cell gaps on n x n cells, walked inwards from the top left corner."""
    g = np.zeros((n, n), np.uint8)
    y = x = 0
    dy, dx = 0, 1
    g[0, 0] = 1

    def free(y, x, dy, dx):
        ny, nx = y + dy, x + dx
        if not (0 <= ny < n and 0 <= nx < n) or g[ny, nx]:
            return False
        ay, ax = ny + dy, nx + dx                                 # the cell after the next stays a gap
        return not (0 <= ay < n and 0 <= ax < n and g[ay, ax])
    turns = 0
    while True:
        if free(y, x, dy, dx):
            y, x = y + dy, x + dx
            g[y, x] = 1
            continue
        dy, dx = dx, -dy                                          # turn right (y points down)
        if not free(y, x, dy, dx):
            return g, turns
        turns += 1


def serpentine_grid(turns, width):
    """Full rows joined alternately at the right and the left end: 2 * turns + 1 rows."""
    g = np.zeros((2 * turns + 1, width), np.uint8)
    g[0::2] = 1
    for k in range(turns):
        g[2 * k + 1, width - 1 if k % 2 == 0 else 0] = 1
    return g


def comb_grid(teeth, height):
    """`teeth` one-cell columns, a cell apart, joined only along the bottom row."""
    g = np.zeros((height, 2 * teeth - 1), np.uint8)
    g[:, 0::2] = 1
    g[-1] = 1
    return g


def rings_grid(depth, margin=1, h_extra=0, w_extra=0, centre=True):
    """`depth` concentric one-cell rings a cell apart (each the island in the hole of the one before) and a centre cell in the last hole."""
    h, w = 4 * depth + 1 + h_extra, 4 * depth + 1 + w_extra
    g = np.zeros((h, w), np.uint8)
    for k in range(depth):
        a = 2 * k
        g[a, a:w - a] = g[h - 1 - a, a:w - a] = 1
        g[a:h - a, a] = g[a:h - a, w - 1 - a] = 1
    if centre and h_extra == 0 and w_extra == 0:
        g[h // 2, w // 2] = 1
    return np.pad(g, margin)


def cut_channel(g, cells):
    """A one-cell channel along the middle row, from the plane's left edge `cells` cells inwards."""
    g = g.copy()
    g[g.shape[0] // 2, :cells] = 0
    return g


def _tile(tiles, cols, gap=1):
    """Coarse tiles (padded to one size) laid out `cols` to a row, `gap` empty cells apart."""
    th, tw = max(t.shape[0] for t in tiles), max(t.shape[1] for t in tiles)
    rows = (len(tiles) + cols - 1) // cols
    g = np.zeros((rows * (th + gap) + gap, cols * (tw + gap) + gap), np.uint8)
    for k, t in enumerate(tiles):
        y, x = gap + (k // cols) * (th + gap), gap + (k % cols) * (tw + gap)
        g[y:y + t.shape[0], x:x + t.shape[1]] = t
    return g


# ------------------------------------------------------------------------------------------------ region planes (label 1)
def _grids():
    out = {}
    for k, (h, w) in enumerate(((11, 40), (30, 12), (18, 18))):
        for j, fill in enumerate((0.3, 0.5, 0.7)):
            rng = np.random.RandomState(100 + 10 * k + j)
            out[f"grid_{h}x{w}_fill{int(fill * 10)}"] = up(rng.rand(h, w) < fill, 6 + (k + j) % 3)
    return out


def _paths():
    out = {}
    out["serpentine"] = up(np.pad(serpentine_grid(12, 12), 1), 6)            # 27 x 14 cells: 162 x 84
    out["spiral"] = up(spiral_grid(49)[0], 6)                                # 294 x 294, touches all four edges
    comb = comb_grid(21, 18)
    out["comb"] = up(comb, 6)                                                # 108 x 246
    out["comb_upside_down"] = up(comb[::-1], 6)
    small = [spiral_grid(9)[0], comb_grid(5, 7), serpentine_grid(3, 7), comb_grid(5, 7)[::-1], serpentine_grid(4, 5).T, spiral_grid(7)[0][:, ::-1]]
    out["paths_field"] = up(_tile([small[k % len(small)] for k in range(16)], 4), 6)
    return out


def _rings():
    out = {}
    for s in (6, 7, 8):
        out[f"rings_s{s}"] = up(rings_grid(4), s)
    closed = rings_grid(4)                                                   # 19 x 19 cells: rings at cells 1, 3, 5, 7 of the middle row
    out["rings_channel"] = up(cut_channel(closed, closed.shape[1] // 2), 7)  # from the innermost hole to the frame: nothing is an island any more
    out["rings_half_channel"] = up(cut_channel(closed, 5), 7)                # through the two outer rings only: the third still holds islands
    out["rings_rect"] = up(rings_grid(3, 1, h_extra=0, w_extra=14, centre=False), 6)
    out["rings_edges_s6"] = up(rings_grid(4, 0), 6)                          # the outer ring runs along all four plane edges
    out["rings_edges_s8"] = up(rings_grid(3, 0, h_extra=3, w_extra=0, centre=False), 8)
    two = rings_grid(2)                                                      # 11 x 11 cells
    out["rings_field"] = up(_tile([cut_channel(two, 5) if k % 2 else two for k in range(12)], 4, gap=0), 6)
    return out


def _interleaved():
    out = {}
    i, j = np.mgrid[0:20, 0:24]
    other = np.where(i % 2 == 0, 2, 3)
    out["checker"] = up(np.where((i + j) % 2 == 0, 1, other), 6)             # label-1 cells meet corner to corner only
    out["stripes"] = up(np.where(j % 2 == 0, 1, other), 6)
    out["rows_of_cells"] = up(np.where((i % 2 == 0) & (j % 2 == 0), 1, other), 7)
    rng = np.random.RandomState(7)
    out["random_labels"] = up(rng.randint(0, 4, (25, 25)), 7)
    return out


def _narrow():
    """Planes narrower than the 5 x 5 kernel (no 5 x 5 square fits: the boxes call sizes its root list by the pixel count), and uniform ones."""
    out = {}
    for name, (h, w) in (("narrow_3x40", (3, 40)), ("narrow_40x4", (40, 4)), ("narrow_4x260", (4, 260)), ("narrow_260x3", (260, 3))):
        along = (np.arange(max(h, w)) % 10 < 5).astype(np.uint8)             # runs of five, five apart
        line = np.where(along == 1, 1, 2).astype(np.uint8)
        out[name] = np.ascontiguousarray(np.broadcast_to(line[None, :] if w > h else line[:, None], (h, w)))
    out["all_ones"] = np.ones((50, 70), np.uint8)
    out["all_zero"] = np.zeros((64, 64), np.uint8)
    out["no_label_1"] = np.full((33, 65), 2, np.uint8)
    return out


RIVAL_PITCH, RIVAL_N = 20, 17


def _rivals():
    """17 x 17 small components 20 apart, the smallest shapes OPEN and CLOSE leave alone (arms and holes five wide).  The first is a 14 x 15
    block (contour area 13 x 14 = 182: the largest LOWER bound on the plane), the last in raster order a 15 x 15 ring with a 5 x 5 hole
    (lower bound 162, contour area 196: the true winner), and the 287 L shapes between them have a bounding-box bound of 196 > 182: more
    undecided rivals than the device lists, and the winner is among them."""
    ell = np.zeros((15, 15), np.uint8)
    ell[:, :5] = 1
    ell[10:, :] = 1
    ring = np.ones((15, 15), np.uint8)
    ring[5:10, 5:10] = 0
    side = RIVAL_PITCH * RIVAL_N + 1
    p = np.full((side, side), 3, np.uint8)
    for a in range(RIVAL_N):
        for b in range(RIVAL_N):
            t = np.ones((15, 14), np.uint8) if (a, b) == (0, 0) else ring if (a, b) == (RIVAL_N - 1, RIVAL_N - 1) else ell
            y, x = 3 + RIVAL_PITCH * a, 3 + RIVAL_PITCH * b
            p[y:y + t.shape[0], x:x + t.shape[1]][t > 0] = 1
    return {"rivals_ring_last": p}


@functools.lru_cache(maxsize=None)
def region_families():
    """{family: {name: uint8 label plane}} for sbbseg_text_region_boxes[_dev] / sbbseg_text_regions_present_dev with label 1."""
    return {"grids": _grids(), "paths": _paths(), "rings": _rings(), "interleaved": _interleaved(), "narrow": _narrow(), "rivals": _rivals()}


# ------------------------------------------------------------------------------------------------ page-box planes (> 0)
def _seeds(h, w, points):
    p = np.zeros((h, w), np.uint8)
    for y, x in points:
        p[y, x] = 1
    return p


def _diagonal():
    """25 x 25 blobs (single-pixel seeds, dilated) that touch corner to corner only: a lost diagonal link leaves one 25 x 25 blob as the page."""
    return {
        "diag_down_right": _seeds(80, 110, [(20, 30), (45, 55)]),            # the lower blob sees the upper one as its NW neighbour
        "diag_down_left": _seeds(80, 110, [(20, 55), (45, 30)]),             # ... as its NE neighbour
        "zigzag5": _seeds(150, 110, [(14 + 25 * k, 30 + 25 * (k % 2)) for k in range(5)]),
    }


def _chunks():
    """Row runs against the 64-pixel chunks of the row pass: a run over columns 63 | 64, a run that starts at column 64, a run over two
    chunk boundaries, rows that end at columns 62 / 63 / 64 / 127 / 128, one-row and one-column planes (no 2 x 2 cell pass)."""
    out = {}
    for h, w in ((1, 200), (2, 129), (200, 1), (40, 63), (40, 64), (40, 65), (40, 128)):
        y = h // 2
        tag = f"{h}x{w}"
        if w > 76:
            out[f"chunk_{tag}_51_76"] = _seeds(h, w, [(y, 51), (y, 76)] + ([(y, 150)] if w > 150 else []))      # runs 39..63 + 64..88: one run
            out[f"chunk_{tag}_76"] = _seeds(h, w, [(y, 76)] + ([(y, 20)] if h > 1 else []))                   # a run that starts at column 64
        if w > 52:
            out[f"chunk_{tag}_52"] = _seeds(h, w, [(y, min(52, w - 1))])                                      # 40..64 clipped to the row's end
        row = np.zeros((h, w), np.uint8)
        row[y, :] = 1
        out[f"chunk_{tag}_row"] = row                                                                         # one run over every boundary
        if w == 1:
            out[f"chunk_{tag}_51_76"] = _seeds(h, w, [(51, 0), (76, 0), (150, 0)])
    return out


LATTICE_N, LATTICE_PITCH = 17, 26


def _lattice():
    """17 x 17 seeds 26 apart on 450 x 450: 289 blobs of 25 x 25 a pixel apart.  `equal`: all the same (the last in raster order wins);
    `one_apart`: one seed a pixel wider (it wins by one cell column); `notched`: every seed two pixels on a diagonal (27 apart), so every blob's
    bounding-box bound (25 x 25) lies above every blob's cell count -- 288 undecided rivals, more than the device lists."""
    pts = [(13 + LATTICE_PITCH * a, 13 + LATTICE_PITCH * b) for a in range(LATTICE_N) for b in range(LATTICE_N)]
    equal = _seeds(450, 450, pts)
    one = equal.copy()
    y, x = pts[5 * LATTICE_N + LATTICE_N - 1]                    # in the last column: widened outwards, it stays a pixel from its neighbours
    one[y, x + 1] = 1
    wide = [(13 + (LATTICE_PITCH + 1) * a, 13 + (LATTICE_PITCH + 1) * b) for a in range(LATTICE_N) for b in range(LATTICE_N)]
    notched = _seeds(460, 460, wide + [(y + 1, x + 1) for y, x in wide])
    return {"lattice_equal": equal, "lattice_one_apart": one, "lattice_notched": notched}


def _coarse():
    """30-pixel cells on a 7 x 9 lattice (51 / 46 apart, so that dilated neighbours merge, diagonal ones too) at fill 0.5, on 360 x 420."""
    out = {}
    for seed in (0, 1, 2):
        rng = np.random.RandomState(40 + seed)
        p = np.zeros((360, 420), np.uint8)
        for a, b in zip(*np.nonzero(rng.rand(7, 9) < 0.5)):
            p[3 + 51 * a:33 + 51 * a, 3 + 46 * b:33 + 46 * b] = 1
        out[f"coarse_{seed}"] = p
    return out


@functools.lru_cache(maxsize=None)
def page_families():
    """{family: {name: uint8 0 / 1 plane}} for sbbseg_page_box_dev."""
    return {"diagonal": _diagonal(), "chunks": _chunks(), "lattice": _lattice(), "coarse": _coarse(),
            "empty": {"empty_64x64": np.zeros((64, 64), np.uint8), "empty_1x1": np.zeros((1, 1), np.uint8)}}


# ------------------------------------------------------------------------------------------------ what the oracle says, computed once
@functools.lru_cache(maxsize=None)
def _region_plane(name):
    for planes in region_families().values():
        if name in planes:
            return planes[name]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def oracle_region_boxes(name, min_area, max_area):
    """slopes_ref.oracle_boxes of the named region plane for label 1 (cached: the GPU tests and the CPU test share it; callers do not
    modify the list)."""
    import slopes_ref
    return slopes_ref.oracle_boxes(_region_plane(name), 1, min_area, max_area)


@functools.lru_cache(maxsize=None)
def interior_window(name):
    """(min_area, max_area) fractions for the named region plane, from the oracle's own contour areas (stage_glue.text_region_contour_areas)
    so that the window splits the plane's components: with three or more distinct areas some lie below, some inside and some above; with
    two the smaller ones are kept; with one the window is that area to a quarter pixel above it -- far inside the device's two bounds unless
    the component is a solid rectangle, so the exact tracing decides.  The lower edge IS an area: the comparison is inclusive."""
    plane = _region_plane(name)
    total = float(plane.shape[0] * plane.shape[1])
    areas = sorted(set(sg.text_region_contour_areas(plane, 1, 0.0, 1.0)))
    if not areas:
        return 0.1, 0.5
    k = len(areas)
    i = k // 3
    j = i if k < 3 else max(i, k - 2)
    return areas[i] / total, (areas[j] + 0.25) / total
