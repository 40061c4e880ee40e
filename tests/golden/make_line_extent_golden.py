#!/usr/bin/env python3
"""Generate tests/golden/line_extent_golden.npz by running the REFERENCE's OWN ``textline_contours_postprocessing`` (main.py:1472-1524) with its
two real splitters (``seperate_lines`` / ``seperate_lines_vertical``) on the boxes and contours of the five pages of
``make_slopes_golden.page()`` (through the reference's own ``do_work_of_slopes``) and on small synthetic regions, and recording the
``textline_boxes_rot`` it returns.

THIS IS A SELF-CONSISTENCY FIXTURE.  cv2 is not installed: the reference runs on the cv2 stubs of ``make_line_split_golden.py`` /
``make_lines_golden.py``, plus ``cv2.fillPoly``, ``cv2.findContours`` and ``cv2.pointPolygonTest`` taken from the literal Python
restatement of the OpenCV text (tests/line_extent_ref.py).  What the fixture pins is the reference's CONTROL FLOW around those calls --
the coordinate shift by the box, the float64 image, numpy's own ``astype(np.uint8)``, ``np.argmax`` over the list order, which splitter
runs, ``np.linspace``, ``int()`` of the float64 samples, ``np.dot`` and the clamps, the bare except -- not OpenCV itself.  The restated
``findContours`` returns the borders in REVERSE discovery order [EXT, assumed].

Runs only where the reference is available; never on the GPU box.  The fixture holds arrays only: per case the ring, the box, the slope,
``dst`` as the splitter received it (bit-packed) and the polygons.
    python tests/golden/make_line_extent_golden.py [out.npz]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_glue_golden import install_contour_tree_stubs, install_cv2_stubs  # noqa: E402
from make_line_split_golden import stripes  # noqa: E402
from make_slopes_golden import N_PAGES, Sink, page  # noqa: E402
from make_tiling_golden import load_reference  # noqa: E402
from oracle import deskew as dk  # noqa: E402
from oracle import stage_glue as sg  # noqa: E402
import line_extent_ref as ler  # noqa: E402
import lines_ref  # noqa: E402


def synthetic():
    """(textline crop of 0 / 1, slope, ring in box coordinates, box): chosen until the assertions of main() hold."""
    out = []
    lines = stripes(120, 160, 30, 9)
    u = [[10, 5], [50, 5], [50, 90], [110, 90], [110, 5], [150, 5], [150, 115], [10, 115]]
    out.append((lines, 0.0, u, (40, 30, 160, 120)))                   # a U: two inside intervals on the rows of its arms
    out.append((lines, 3.0, u, (40, 30, 160, 120)))
    out.append((lines, -6.0, [[20, 10], [140, 10], [140, 110], [20, 110]], (7, 9, 160, 120)))
    out.append((lines, 2.0, [[5, 5], [80, 5], [80, 60], [155, 60], [155, 115], [5, 115]], (0, 0, 160, 120)))      # an L
    out.append((stripes(70, 50, 36, 8, first=10), -2.0, [[4, 4], [45, 4], [45, 65], [4, 65]], (3, 3, 50, 70)))     # two lines
    out.append((stripes(40, 50, 100, 6, first=15), 1.0, [[4, 4], [45, 4], [45, 35], [4, 35]], (3, 3, 50, 40)))     # one line: keeps 0 .. w
    out.append((stripes(160, 60, 30, 9).T.copy(), -88.0, [[5, 5], [150, 5], [150, 55], [5, 55]], (11, 2, 160, 60)))   # vertical
    out.append((lines, 44.9, [[1, 1]], (5, 5, 160, 120)))             # one pixel rotated out of the frame: no border, np.argmax([]) raises
    blob = np.zeros((120, 160), np.uint8)
    rng = np.random.RandomState(7)
    blob[10:110, 15:150] = rng.rand(100, 135) < 0.7
    blob[55:65, 15:150] = 1
    ring = max((b[1] for b in ler.find_contours_tree(blob) if not b[0]), key=len)
    out.append((lines, 5.0, ring.tolist(), (21, 13, 160, 120)))       # a ragged traced ring
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "line_extent_golden.npz")
    ref = load_reference()
    import cv2
    install_cv2_stubs(cv2, {})
    install_contour_tree_stubs(cv2, ref)
    page_find_contours = cv2.findContours                        # (the page's own contours: the stub contours_golden.npz pins)
    cv2.erode = lambda src, kernel, iterations=1: sg.morph(src, "erode", kernel.shape[0], iterations)

    def warp_affine(src, M, dsize, flags=None, borderMode=None):
        assert flags == cv2.INTER_CUBIC and borderMode == cv2.BORDER_REPLICATE and tuple(dsize) == (src.shape[1], src.shape[0])
        fixed = src.dtype == np.uint8
        planes = [src[:, :, c] for c in range(src.shape[2])] if src.ndim == 3 else [src]
        if src.ndim == 3 and all(np.array_equal(planes[0], p) for p in planes[1:]):
            planes = planes[:1]
        res = [lines_ref.warp_affine_cubic_replicate_u8(p, M) if fixed else dk.warp_affine_cubic_replicate(p, M) for p in planes]
        return np.stack([res[min(c, len(res) - 1)] for c in range(src.shape[2])], axis=2) if src.ndim == 3 else res[0]
    cv2.warpAffine = warp_affine

    def fill_poly(img, pts, color):
        assert len(pts) == 1 and img.ndim == 3 and tuple(color) == (255, 255, 255)
        ring = np.asarray(pts[0]).reshape(-1, 2).astype(np.int64)
        img[ler.fill_poly(ring, img.shape[1], img.shape[0]) != 0] = color
        return img
    cv2.fillPoly = fill_poly
    seen = {}

    def find_rotated(mask, mode, method):
        assert mode == cv2.RETR_TREE and method == cv2.CHAIN_APPROX_SIMPLE and mask.dtype == np.uint8
        borders = ler.find_contours_tree(mask)
        seen["threshrot"], seen["borders"] = mask.copy(), borders
        return [b[1].reshape(-1, 1, 2).astype(np.int32) for b in borders[::-1]], None
    cv2.pointPolygonTest = lambda contour, pt, measure: ler.point_polygon_test(contour, pt)

    det = ref.textline_detector.__new__(ref.textline_detector)
    det.kernel = np.ones((5, 5), np.uint8)                       # main.py:57
    real = {False: det.seperate_lines, True: det.seperate_lines_vertical}

    def splitter(vertical):
        def run(img_patch, contour, slope):
            seen["dst"], seen["vertical"], seen["winner"] = np.array(img_patch, np.uint8), vertical, np.asarray(contour).reshape(-1, 2)
            return real[vertical](img_patch, contour, slope)
        return run
    det.seperate_lines, det.seperate_lines_vertical = splitter(False), splitter(True)

    cases = []                                                   # (crop, slope, ring [N, 1, 2] page coordinates, box, page)
    for k in range(N_PAGES):
        regions, textlines = page(k)
        cv2.findContours = page_find_contours
        contours = det.get_text_region_contours_and_boxes(np.repeat(regions[:, :, None], 3, axis=2))
        boxes = [list(b) for b in det.boxes]
        slopes = [float(s) for s in lines_ref.load_golden()[k][0]]
        assert len(slopes) == len(boxes) == len(contours), (k, len(slopes), len(boxes), len(contours))
        for box, slope, contour in zip(boxes, slopes, contours):
            crop = sg.morph(np.ascontiguousarray(textlines[box[1]:box[1] + box[3], box[0]:box[0] + box[2]]), "erode", 5, 2)      # main.py:1731-1734
            cases.append((crop, slope, np.asarray(contour).astype(np.uint), box, k))
    for crop, slope, ring, box in synthetic():
        ring = (np.array(ring, np.int64) + np.array(box[:2])).astype(np.uint)
        cases.append((crop, slope, np.concatenate([ring, ring[:1]]).reshape(-1, 1, 2), list(box), -1))

    cv2.findContours = find_rotated
    # (only now: get_text_region_contours_and_boxes above needs the real filter)
    det.return_contours_of_image = lambda img: ([], None)        # dead inside the first `try` of the splitters (make_line_split_golden.py)
    det.filter_contours_area_of_image = lambda *a, **k: []
    rows = {key: [] for key in ("ring", "box", "slope", "page", "dst", "status", "polygons", "holes", "is_hole", "tie")}
    kinds = set()
    for crop, slope, ring, box, pg in cases:
        seen.clear()
        polygons = det.textline_contours_postprocessing(crop, slope, ring, box)
        w, h = box[2], box[3]
        assert "borders" in seen, "findContours must be reached: the reference's bare except hides a broken stub"
        none = len(seen["borders"]) == 0
        assert none or "dst" in seen, "a splitter must be reached whenever there is a border"
        dst = seen.get("dst", np.zeros((h, w), np.uint8))
        k, tie = ler.winner(seen["borders"])
        holes = sum(1 for b in seen["borders"] if b[0])
        polygons = np.array(polygons, np.int64).reshape(-1, 4, 2)
        if none:
            kinds.add("none")
        else:
            assert np.array_equal(seen["winner"], seen["borders"][k][1])
            if seen["vertical"]:
                kinds.add("vertical")
            elif len(polygons):
                kinds.add("lines")
        if holes:
            kinds.add("hole")
        for key, v in (("ring", np.asarray(ring, np.int64).reshape(-1, 2)), ("box", box), ("slope", slope), ("page", pg), ("dst", np.packbits(dst)),
                       ("status", int(none)), ("polygons", polygons), ("holes", holes), ("is_hole", 0 if none else int(seen["borders"][k][0])),
                       ("tie", int(tie))):
            rows[key].append(v)
        print("page", pg, "box", box, "slope", slope, "borders", len(seen["borders"]), "holes", holes, "tie", tie, "lines", len(polygons))
    # Which lines were cut, and which rows have two inside intervals, is decided from the recorded polygons by the tests' own restatement
    # (tests/test_line_extent_golden_cpu.py asserts both kinds exist); here: every kind of case the contour half can end in.
    assert kinds >= {"none", "vertical", "lines", "hole"}, kinds
    out = {"ring": np.concatenate(rows["ring"]).astype(np.int32), "ring_off": np.concatenate([[0], np.cumsum([len(v) for v in rows["ring"]])]).astype(np.int64),
           "box": np.array(rows["box"], np.int32), "slope": np.array(rows["slope"], np.float64), "page": np.array(rows["page"], np.int32),
           "dst": np.concatenate(rows["dst"]), "dst_off": np.concatenate([[0], np.cumsum([len(v) for v in rows["dst"]])]).astype(np.int64),
           "status": np.array(rows["status"], np.int32), "holes": np.array(rows["holes"], np.int32), "is_hole": np.array(rows["is_hole"], np.int32),
           "tie": np.array(rows["tie"], np.int32), "polygons": np.concatenate(rows["polygons"]).astype(np.int32),
           "polygon_off": np.concatenate([[0], np.cumsum([len(v) for v in rows["polygons"]])]).astype(np.int64)}
    np.savez_compressed(out_path, **out)
    print("wrote", out_path, os.path.getsize(out_path), "bytes;", len(rows["box"]), "cases, kinds", sorted(kinds))


if __name__ == "__main__":
    main()
