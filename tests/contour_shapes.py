"""Small raw masks for the contour tracer, shared by tests/test_contours_cpu.py and tests/test_gpu_contours.py: shapes OPEN and CLOSE can
never leave behind (single pixels, spurs, pinches), the shapes that decide between testing the label and testing the mask (a foreign
blob inside a bounding box, an island in a hole), and seeded random masks."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _canvas(h, w, cells):
    m = np.zeros((h, w), np.uint8)
    for y, x in cells:
        m[y, x] = 1
    return m


def hand_shapes():
    """{name: uint8 0 / 1 mask}; every mask keeps a free one-pixel frame unless its name says otherwise."""
    out = {"single_pixel": _canvas(3, 3, [(1, 1)])}
    for name, (dy, dx) in (("two_east", (0, 1)), ("two_south_east", (1, 1)), ("two_south", (1, 0)), ("two_south_west", (1, -1))):
        out[name] = _canvas(4, 5, [(1, 2), (1 + dy, 2 + dx)])
    out["line_horizontal"] = _canvas(3, 11, [(1, x) for x in range(1, 10)])
    out["line_vertical"] = _canvas(11, 3, [(y, 1) for y in range(1, 10)])
    out["line_diagonal_down"] = _canvas(9, 9, [(k, k) for k in range(1, 8)])
    out["line_diagonal_up"] = _canvas(9, 9, [(k, 8 - k) for k in range(1, 8)])
    pinch = np.zeros((7, 7), np.uint8)                        # two 3 x 3 squares that share the corner pixel (3, 3): entered twice
    pinch[1:4, 1:4] = 1
    pinch[3:6, 3:6] = 1
    out["pinch"] = pinch
    edges = np.zeros((9, 12), np.uint8)                       # touches all four plane edges
    edges[4, :] = 1
    edges[:, 5] = 1
    edges[0:3, 0:2] = 0
    out["touches_all_edges"] = edges
    ring = np.zeros((13, 13), np.uint8)
    ring[1:12, 1:12] = 1
    ring[3:10, 3:10] = 0
    ring[5:8, 5:8] = 1                                        # the island in the hole
    out["ring_with_island"] = ring
    c = np.zeros((12, 12), np.uint8)                          # a C whose bounding box holds a foreign blob
    c[1:11, 1:11] = 1
    c[3:9, 3:11] = 0
    c[5:7, 6:10] = 1
    out["c_with_foreign_blob"] = c
    spur = np.zeros((8, 10), np.uint8)                        # a block with a one-pixel spur: the tip is a kept point
    spur[2:6, 1:5] = 1
    spur[3, 5:9] = 1
    out["spur"] = spur
    return out


def random_masks(n=200, seed=0, max_side=13):
    """n seeded random masks of at most max_side x max_side at fills between 0.2 and 0.8."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        h, w = rng.randint(1, max_side + 1), rng.randint(1, max_side + 1)
        out.append((rng.rand(h, w) < rng.uniform(0.2, 0.8)).astype(np.uint8))
    return out


def pack(masks, width, gap=1):
    """The masks laid out left to right, top to bottom on one plane `width` wide, `gap` empty pixels apart (and around)."""
    x = y = gap
    row_h = 0
    places = []
    for m in masks:
        h, w = m.shape
        if x + w + gap > width:
            x, y, row_h = gap, y + row_h + gap, 0
        places.append((y, x))
        x += w + gap
        row_h = max(row_h, h)
    plane = np.zeros((y + row_h + gap, width), np.uint8)
    for m, (py, px) in zip(masks, places):
        plane[py:py + m.shape[0], px:px + m.shape[1]] = m
    return plane


def widths_plane():
    """Solid and hollow boxes 31, 32, 33, 63, 64 and 65 wide at odd x offsets: the bit map's word stride and the ballot's tail."""
    plane = np.zeros((2 * 6 * 9 + 2, 80), np.uint8)
    y = 1
    for k, w in enumerate((31, 32, 33, 63, 64, 65)):
        x = 1 + 2 * (k % 3)
        plane[y:y + 7, x:x + w] = 1
        plane[y + 2:y + 5, x + 2:x + w - 3] = 0               # hollow, with a notch-free inner border
        y += 9
        x = 3 + 2 * (k % 2)
        plane[y:y + 7, x:x + w] = (np.add.outer(np.arange(7), np.arange(w)) % 3 != 0)      # diagonal stripes: one 8-connected component
        y += 9
    return plane


def staircase(steps):
    """One component of 2 x 2 treads: 4 * steps + O(1) kept points."""
    m = np.zeros((2 * steps + 4, 2 * steps + 4), np.uint8)
    for k in range(steps):
        m[1 + 2 * k:3 + 2 * k, 1 + 2 * k:5 + 2 * k] = 1
    return m


def many_components(rows=36, cols=36):
    """rows x cols isolated components (pixels, and every third a 2 x 1 domino) two pixels apart: more than one tracer launch has blocks."""
    m = np.zeros((3 * rows + 1, 3 * cols + 1), np.uint8)
    m[1::3, 1::3] = 1
    m[1::9, 2::3] = 1
    return m


def frame_plane():
    """A hollow 1024 x 640 frame with 7-pixel walls on a 1040 x 656 label plane (class 1): its bit map is beyond the LDS limit, and it
    survives OPEN and CLOSE."""
    p = np.zeros((656, 1040), np.uint8)
    p[8:648, 8:1032] = 1
    p[15:641, 15:1025] = 0
    return p


def golden_cases():
    """[(regions [H, W, 3], boxes, rings)] of contours_golden.npz, the inputs taken from the glue and slopes fixtures."""
    g = np.load(os.path.join(GOLDEN, "contours_golden.npz"))
    glue, slopes = np.load(os.path.join(GOLDEN, "glue_golden.npz")), np.load(os.path.join(GOLDEN, "slopes_golden.npz"))
    out = []
    for j in range(int(g["n"])):
        from_slopes, k = (int(v) for v in g[f"source{j}"])
        if from_slopes:
            regions = np.repeat(slopes[f"regions{k}"][:, :, None], 3, axis=2)
        else:
            regions = np.repeat(glue[f"regions_map{k}"][:, :, None], 3, axis=2)
            if not int(glue[f"regions_ch1_{k}"]):
                regions[:, :, 1] = 0
        assert regions.shape == tuple(g[f"shape{j}"])
        ends = np.cumsum(g[f"lengths{j}"])
        rings = [g[f"points{j}"][e - n:e].astype(np.uint).reshape(-1, 1, 2) for n, e in zip(g[f"lengths{j}"], ends)]
        out.append((regions, g[f"boxes{j}"].tolist(), rings))
    return out
