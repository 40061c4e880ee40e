"""Composed references for the boxes + slopes step (tests/test_slopes_cpu.py, tests/test_gpu_slopes.py), built from the oracle's
own functions: nothing here is product code, and nothing here touches the GPU."""
import os

import numpy as np

from oracle import deskew as dk
from oracle import stage_glue as sg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slopes_golden.npz")
SWEEP1 = np.linspace(-25, 25, 80)            # main.py:1620
SWEEP2 = np.linspace(-90, -50, 30)           # main.py:1670


def load_pages():
    """[(regions uint8 [H, W], textlines uint8 [H, W], boxes [[x, y, w, h]], slopes [float])] of the committed fixture."""
    g = np.load(GOLDEN)
    pages = []
    for k in range(int(g["n"])):
        h, w = (int(v) for v in g[f"shape{k}"])
        textlines = np.unpackbits(g[f"textlines{k}"])[:h * w].reshape(h, w)
        pages.append((g[f"regions{k}"], textlines, [[int(v) for v in b] for b in g[f"boxes{k}"]], [float(s) for s in g[f"slopes{k}"]]))
    return pages


def erode2(crop):
    """cv2.erode(crop, 5x5, iterations=2) of main.py:1734, by the oracle."""
    return sg.morph(np.ascontiguousarray(crop, np.uint8), "erode", 5, 2)


def crop_of(textlines, box):
    return sg.crop_image_inside_box(box, textlines)[0]


def cleaned(slope):
    """main.py:1744-1747."""
    return 0 if (slope == 999 or abs(slope) > 120.5) else slope


def oracle_slopes(textlines, boxes, sigma_des=2):
    """The slope half of do_work_of_slopes (main.py:1728-1748) from oracle functions: crop, erode x 2, return_deskew_slope, clean-up."""
    out = []
    for box in boxes:
        try:
            slope = dk.return_deskew_slope(erode2(crop_of(textlines, box)), sigma_des)
        except Exception:
            slope = 999
        out.append(cleaned(slope))
    return out


def oracle_boxes(regions, label=1, min_area=0.00001, max_area=1.0):
    """get_text_region_contours_and_boxes' boxes from oracle functions and scipy.ndimage.label: parentless 8-connected components of the
    opened / closed class mask with an outer-contour area in range; first pixel in raster order, descending."""
    from scipy import ndimage
    a = np.asarray(regions)
    m = np.all(a == label, axis=-1) if a.ndim == 3 else a == label
    p = np.where(m, 255, 0).astype(np.uint8)
    p = sg.morph(sg.morph(p, "erode", 5, 1), "dilate", 5, 1)
    p = sg.morph(sg.morph(p, "dilate", 5, 1), "erode", 5, 1)
    lab, n = ndimage.label(p > 0, structure=np.ones((3, 3), int))
    back, _ = ndimage.label(np.pad(p == 0, 1, constant_values=True), structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    outer = back == back[0, 0]
    total = float(p.shape[0] * p.shape[1])
    boxes = []
    for k in range(n, 0, -1):
        comp = lab == k
        grown = ndimage.binary_dilation(np.pad(comp, 1), structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
        if not (grown & outer).any():
            continue                                            # an island in a hole: it has a parent
        ys, xs = np.nonzero(comp)
        area = sg.outer_contour_area2(comp[ys.min():ys.max() + 1, xs.min():xs.max() + 1]) / 2.0
        if min_area * total <= area <= max_area * total:
            boxes.append([int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)])
    return boxes


def random_page(seed=0, h=1500, w=1300, n_boxes=26):
    """A textline-like 0 / 1 plane and at least 24 boxes on it: from 5 x 5 up to about 600 x 900, some touching the plane's edges, one
    the whole plane.  Boxes may overlap: slopes are per box."""
    rng = np.random.RandomState(seed)
    t = np.zeros((h, w), np.uint8)
    for _ in range(14):                                         # blocks of lines with their own period, thickness and slant
        bh, bw = rng.randint(80, 420), rng.randint(120, 620)
        y0, x0 = rng.randint(0, h - bh), rng.randint(0, w - bw)
        period, thick, slant = rng.randint(18, 40), rng.randint(9, 16), rng.uniform(-0.15, 0.15)
        xs = np.arange(bw)
        for y in range(0, bh - thick, period):
            ys = y + np.round(slant * (xs - bw / 2)).astype(int)
            for d in range(thick):
                yy = ys + d
                ok = (yy >= 0) & (yy < bh)
                t[y0 + yy[ok], x0 + xs[ok]] = 1
    boxes = [[0, 0, w, h], [0, 0, 5, 5], [w - 7, h - 5, 7, 5], [0, h - 600, 900, 600], [w - 300, 0, 300, 200], [10, 10, 1, 1], [400, 0, 40, 9]]
    while len(boxes) < n_boxes:
        bw, bh = int(rng.randint(5, 420)), int(rng.randint(5, 320))
        boxes.append([int(rng.randint(0, w - bw + 1)), int(rng.randint(0, h - bh + 1)), bw, bh])
    return t, boxes
