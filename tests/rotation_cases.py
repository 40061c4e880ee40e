"""Adversarial crops, shapes, angles and planes for the two device rotations (tests/test_rotation_cases_cpu.py,
tests/test_gpu_rotations.py): the deskew sweep (csrc/region_deskew.hip, csrc/page_glue.hip) and the deskewed line mask
(csrc/region_lines.hip).  Case builders and compositions of the numpy oracles only: nothing here is product code (the rotation matrices
of the sweep are handed in by the tests), nothing here touches the GPU, every seed is fixed.

Every box side is at most 320, so the square of the sweep has a side of at most 448.

Sides of the square.  S = int(1.4 * max(h, w)) in float64 skips values: 45 -> 62 (62.99999999999999), 46 -> 64, 92 -> 128, 93 -> 130, so
no box has S = 63 or S = 129.  The shapes around the 64-lane loop therefore give S = 62, 64, 65 and 127, 128, 130.

Pooled boxes lie in the top rows of their planes (``POOLED_ROWS``): a crop kernel that took another box's plane record would then still
read inside the one allocation the three planes are packed into, and return wrong bytes."""
from collections import namedtuple

import numpy as np

from oracle import deskew as dk

import lines_ref
import slopes_ref

RANDOM_ANGLES = [float(a) for a in np.random.RandomState(46).uniform(-180, 180, 12)]     # (a seed with three values inside the first sweep)
# both sides of |sin| = 1e-7 (5.7296e-6 degrees); the end points of the two sweeps (-90 is already there)
ANGLES = [0.0, 90.0, -90.0, 180.0, 270.0, 360.0, 45.0, -45.0, 45.0001, 1e-9, -1e-9, 5.72e-6, 5.74e-6, 1e-4, 89.99999, 90.00001,
          -25.0, 25.0, -50.0] + RANDOM_ANGLES

KINDS = ["ones", "full", "frame", "corners", "mids", "row", "col", "checker", "bytes", "wrap", "stripes"]
WRAP_BYTES = [0, 1, 2, 3, 128, 254, 255]

TINY = [(1, 1), (2, 2), (3, 3), (4, 4)]                          # the analytic span is off
FIRST_CLIPPED = [(5, 5), (5, 6)]
THIN = [(1, 40), (40, 1), (2, 300), (300, 2)]
LANES = [(45, 30), (20, 46), (47, 47), (91, 60), (64, 92), (93, 93)]           # S = 62, 64, 65, 127, 128, 130
MIXED = [(37, 90), (90, 37), (43, 17)]                           # odd and even sides; S = 125, 125, 60
BIG = [(200, 320)]
SHAPES = TINY + FIRST_CLIPPED + THIN + LANES + MIXED + BIG
SHAPE_CLASSES = {"tiny": TINY, "first_clipped": FIRST_CLIPPED, "thin": THIN, "lanes": LANES, "mixed": MIXED, "big": BIG}

# which plane a shape is placed on, and the widest the packer lets each plane grow (plane 0: one more than its widest box)
PLANE_OF = {(200, 320): 0, (40, 1): 0, (37, 90): 0, (1, 1): 0, (4, 4): 0, (47, 47): 0, (91, 60): 0,
            (2, 300): 1, (1, 40): 1, (90, 37): 1, (2, 2): 1, (5, 5): 1, (20, 46): 1, (64, 92): 1,
            (300, 2): 2, (3, 3): 2, (5, 6): 2, (45, 30): 2, (93, 93): 2, (43, 17): 2}
PLANE_LIMIT = [321, 400, 517]

# the sweep goes through the numpy oracle at every angle: the shapes whose square is small take every kind of crop, the others a few
SWEEP_ALL_KINDS = TINY + FIRST_CLIPPED + [(1, 40), (40, 1), (45, 30), (20, 46), (47, 47), (43, 17)]
SWEEP_SOME = {(91, 60): ["ones", "frame", "bytes", "stripes"], (64, 92): ["ones", "corners", "wrap", "row"],
              (93, 93): ["ones", "mids", "checker", "full"], (37, 90): ["ones", "col", "bytes", "stripes"],
              (90, 37): ["ones", "frame", "wrap", "stripes"], (2, 300): ["ones"], (300, 2): ["bytes"], (200, 320): ["ones"]}

# the larger boxes of the pooled call (the oracle runs two whole sweeps for each): packed first, so they lie in the top rows
POOLED_LARGE = [("stripes", (37, 90)), ("stripes", (90, 37)), ("stripes", (45, 30)), ("wrap", (1, 40)), ("bytes", (5, 6)), ("ones", (20, 46))]
POOLED_ROWS = 130
TINY_RUN = 210

Case = namedtuple("Case", "kind shape plane box")               # box = [x, y, w, h] on planes()[plane]


def side_of(h, w):
    """main.py:1613."""
    return int(max(h, w) * 1.4)


def make_crop(kind, h, w, seed=0):
    """One (h, w) uint8 crop of the named kind."""
    rng = np.random.RandomState(1000 + seed)
    c = np.zeros((h, w), np.uint8)
    if kind == "ones":
        c[:] = 1
    elif kind == "full":
        c[:] = 255
    elif kind == "frame":
        c[0, :] = c[-1, :] = 1
        c[:, 0] = c[:, -1] = 1
    elif kind == "corners":
        c[0, 0] = c[0, -1] = c[-1, 0] = c[-1, -1] = 1
    elif kind == "mids":
        c[0, w // 2] = c[-1, w // 2] = c[h // 2, 0] = c[h // 2, -1] = 1
    elif kind == "row":
        c[h // 2, :] = 1
    elif kind == "col":
        c[:, w // 2] = 1
    elif kind == "checker":
        c[:] = (np.add.outer(np.arange(h), np.arange(w)) & 1) ^ 1
    elif kind == "bytes":
        c[:] = rng.randint(0, 256, (h, w))
    elif kind == "wrap":
        c[:] = rng.choice(WRAP_BYTES, (h, w))
    elif kind == "stripes":                                      # slanted text lines as slopes_ref.random_page draws them
        period, thick, slant = (18, 11, 0.08) if min(h, w) >= 30 else (6, 3, 0.08)
        xs = np.arange(w)
        for y in range(0, max(h - thick, 1), period):
            ys = y + np.round(slant * (xs - w / 2)).astype(int)
            for d in range(thick):
                yy = ys + d
                ok = (yy >= 0) & (yy < h)
                c[yy[ok], xs[ok]] = 1
    else:
        raise ValueError(kind)
    if not c.any():                                              # (a random crop of a pixel or two)
        c[0, 0] = 255
    return c


def _pack(sizes, limit):
    """First-fit shelves: [(x, y)] per (h, w), and the extent (H, W)."""
    shelves, at = [], []                                         # [y, height, next x]
    for h, w in sizes:
        for s in shelves:
            if s[1] >= h and s[2] + w <= limit:
                break
        else:
            s = [shelves[-1][0] + shelves[-1][1] if shelves else 0, h, 0]
            shelves.append(s)
        at.append((s[2], s[0]))
        s[2] += w
    return at, (shelves[-1][0] + shelves[-1][1], max(x + w for (x, _y), (_h, w) in zip(at, sizes)))


_BUILT = None


def _build():
    global _BUILT
    if _BUILT is None:
        planes, cases = [], []
        for k in range(3):
            mine = [(kind, shape) for shape in SHAPES if PLANE_OF[shape] == k for kind in KINDS]
            first = [c for c in POOLED_LARGE if c in mine]
            rest = sorted((c for c in mine if c not in first), key=lambda c: -c[1][0])
            order = first + rest
            at, (H, W) = _pack([shape for _kind, shape in order], PLANE_LIMIT[k])
            plane = np.zeros((H, W), np.uint8)
            placed = []
            for n, ((kind, (h, w)), (x, y)) in enumerate(zip(order, at)):
                plane[y:y + h, x:x + w] = make_crop(kind, h, w, seed=17 * k + n)
                placed.append(Case(kind, (h, w), k, [x, y, w, h]))
            # call order: small and large boxes alternate, so the kernels' binary searches cross small and large neighbours
            by_area = sorted(placed, key=lambda c: (c.shape[0] * c.shape[1], c.kind))
            half = (len(by_area) + 1) // 2
            mixed = [c for pair in zip(by_area[:half], by_area[:half - 1:-1] + [None]) for c in pair if c is not None]
            assert sorted(mixed) == sorted(placed)
            planes.append(plane)
            cases.append(mixed)
        _BUILT = (planes, cases)
    return _BUILT


def planes():
    """The three uint8 planes.  Not to be written to."""
    return _build()[0]


def line_cases(plane=None):
    """Every crop kind x shape as a Case, in call order (of one plane, or of all three)."""
    cases = _build()[1]
    return list(cases[plane]) if plane is not None else [c for cs in cases for c in cs]


def sweep_cases(plane=None):
    """The cases that go through the deskew sweep and its oracle."""
    return [c for c in line_cases(plane) if c.shape in SWEEP_ALL_KINDS or c.kind in SWEEP_SOME.get(c.shape, ())]


def crop_of(case):
    return slopes_ref.crop_of(planes()[case.plane], case.box)


def find(kind, shape):
    return next(c for c in line_cases() if c.kind == kind and c.shape == tuple(shape))


def one_per_shape_class():
    """A sweep case per shape class (two for the thin ones: a row and a column), for the one-region path."""
    picks = [("bytes", (3, 3)), ("wrap", (5, 6)), ("ones", (1, 40)), ("bytes", (300, 2)), ("stripes", (91, 60)), ("stripes", (37, 90)), ("ones", (200, 320))]
    return [find(kind, shape) for kind, shape in picks]


def line_slopes(shape):
    """The slopes a shape's line masks are computed at: the angle list, a seeded third of it for the largest shape."""
    if tuple(shape) in BIG:
        keep = np.random.RandomState(5).permutation(len(ANGLES))[:len(ANGLES) // 3]
        return [ANGLES[i] for i in sorted(keep)]
    return list(ANGLES)


def pooled_case():
    """(boxes, box_plane) for the pooled calls: a larger box, a run of TINY_RUN 1 x 1 .. 3 x 3 boxes that alternate between the three
    planes, then larger boxes and shorter runs in turn.  The tiny boxes lie anywhere in the top rows, the plane's two upper corners among them."""
    rng = np.random.RandomState(23)
    pl = planes()
    sizes = [(1, 1), (2, 2), (3, 3), (1, 3), (3, 1), (2, 3)]

    def tiny(i):
        k = i % 3
        h, w = sizes[(i // 3) % len(sizes)]
        H, W = pl[k].shape
        x, y = int(rng.randint(0, W - w + 1)), int(rng.randint(0, min(H, POOLED_ROWS) - h + 1))
        if i < 3:
            x, y = 0, 0
        elif i < 6:
            x, y = W - w, 0
        return [x, y, w, h], k
    large = [find(kind, shape) for kind, shape in POOLED_LARGE]
    boxes, box_plane, i = [], [], 0
    for n, c in enumerate(large):
        boxes.append(list(c.box))
        box_plane.append(c.plane)
        for _ in range(TINY_RUN if n == 0 else 25):
            b, k = tiny(i)
            boxes.append(b)
            box_plane.append(k)
            i += 1
    assert all(b[1] + b[3] <= POOLED_ROWS for b in boxes)
    assert (POOLED_ROWS + 1) * max(p.shape[1] for p in pl) <= min(p.size for p in pl)
    return boxes, box_plane


def x_scale_matrix():
    """A forward map that is no rotation: an x scale of 2048 / 2049 whose inverse scale is 2049 / 2048, so that m0 * x * 1024 = 1024.5 x
    ends on .5 for odd x, shifted so that the row origin is X0 = -15: at x = 29 round-half-even gives table index 31 of source column
    28, round-half-up index 0 of column 29."""
    s = 2048.0 / 2049.0
    return np.array([[s, 0.0, (31.0 / 1024.0) * s], [0.0, 1.0, 0.0]], np.float64)


def shear_matrix():
    return np.array([[1.0, 0.25, -7.0], [0.1, 1.0, -3.0]], np.float64)


# ---- compositions of the oracles' own functions ---------------------------------------------------------------------------------------
_SWEEP = {}


def sweep_reference(case, erode_iterations, angle, M):
    """sweep_profile of a case's eroded crop at one angle of the list (M: the library's matrix for it), computed once per process."""
    key = (case.kind, case.shape, erode_iterations, angle)
    if key not in _SWEEP:
        _SWEEP[key] = sweep_profile(lines_ref.eroded_crop(crop_of(case), erode_iterations), M)
    return _SWEEP[key]


def sweep_profile(eroded_crop, M):
    """One row profile of the sweep (main.py:1613-1642, 1546) for the forward 2 x 3 map M, by oracle/deskew.py.  A crop of zeros needs no
    rotation: every tap is zero."""
    h, w = eroded_crop.shape
    if not eroded_crop.any():
        return np.zeros(side_of(h, w), np.int64)
    return (dk.warp_affine_cubic_replicate(dk.padded_square(eroded_crop), M) != 0).sum(axis=1).astype(np.int64)


def line_masks_of(crop, slopes, erode_iterations):
    """[lines_ref.line_mask(crop, s, erode_iterations) for s in slopes], with the part that does not depend on the slope computed once."""
    mask = (lines_ref.eroded_crop(crop, erode_iterations) * np.uint8(255)).astype(np.uint8)
    opened = lines_ref.open_close(mask)
    out = []
    for s in slopes:
        dst = (lines_ref.rotate_image_u8(opened, s) != 0).astype(np.uint8)
        out.append((dst, dst.sum(axis=1).astype(np.int64), dst.sum(axis=0).astype(np.int64)))
    return out
