#!/usr/bin/env python3
"""Generate tests/golden/lines_golden.npz by running the REFERENCE's OWN control flow from ``do_work_of_slopes`` (main.py:1721-1758) into
``textline_contours_postprocessing`` (main.py:1472-1524) on the five pages of ``make_slopes_golden.page()``.

Runs only where the reference is available (the build container); never on the GPU box.  The reference is imported exactly as
``make_slopes_golden.py`` imports it, with the same stubs (``install_cv2_stubs``, ``install_contour_tree_stubs``, ``cv2.erode``), and:
  * ``cv2.warpAffine`` sends uint8 sources to ``lines_ref.warp_affine_cubic_replicate_u8`` (OpenCV's fixed-point bicubic path, restated
    [EXT, unpinned]) and float sources to the oracle's float path, channel by channel;
  * ``cv2.fillPoly`` fills the contour's bounding rectangle: it only feeds the contour half of the function, which is out of scope;
  * ``seperate_lines`` / ``seperate_lines_vertical`` on the instance are recorders of their ``img_patch`` argument (``dst``).
The fixture holds arrays only: the slopes, ``dst`` per box (bit-packed) and which of the two splitters was called.
    python tests/golden/make_lines_golden.py [out.npz]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_glue_golden import install_contour_tree_stubs, install_cv2_stubs  # noqa: E402
from make_slopes_golden import N_PAGES, Sink, page  # noqa: E402
from make_tiling_golden import load_reference  # noqa: E402
from oracle import deskew as dk  # noqa: E402
from oracle import stage_glue as sg  # noqa: E402
import lines_ref  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "lines_golden.npz")
    ref = load_reference()
    import cv2
    install_cv2_stubs(cv2, {})
    install_contour_tree_stubs(cv2, ref)
    cv2.erode = lambda src, kernel, iterations=1: sg.morph(src, "erode", kernel.shape[0], iterations)
    disagree = [0]                                              # pixels where the float path's sum != 0 and the fixed-point != 0 differ

    def warp_affine(src, M, dsize, flags=None, borderMode=None):
        assert flags == cv2.INTER_CUBIC and borderMode == cv2.BORDER_REPLICATE and tuple(dsize) == (src.shape[1], src.shape[0])
        fixed = src.dtype == np.uint8
        planes = [src[:, :, c] for c in range(src.shape[2])] if src.ndim == 3 else [src]
        if src.ndim == 3 and all(np.array_equal(planes[0], p) for p in planes[1:]):
            planes = planes[:1]                                 # equal channels: warp one
        res = [lines_ref.warp_affine_cubic_replicate_u8(p, M) if fixed else dk.warp_affine_cubic_replicate(p, M) for p in planes]
        if fixed:
            disagree[0] += int(((dk.warp_affine_cubic_replicate(planes[0], M) != 0) != (res[0] != 0)).sum())
        if src.ndim == 3:
            return np.stack([res[min(c, len(res) - 1)] for c in range(src.shape[2])], axis=2)
        return res[0]
    cv2.warpAffine = warp_affine

    def fill_poly(img, pts, color):
        p = np.asarray(pts[0]).reshape(-1, 2)
        img[max(int(p[:, 1].min()), 0):int(p[:, 1].max()) + 1, max(int(p[:, 0].min()), 0):int(p[:, 0].max()) + 1] = color
        return img
    cv2.fillPoly = fill_poly

    det = ref.textline_detector.__new__(ref.textline_detector)
    det.kernel = np.ones((5, 5), np.uint8)                       # main.py:57
    seen = []

    def recorder(vertical):
        def record(img_patch, contour, slope):
            seen.append((np.array(img_patch, np.uint8), vertical))
            return None, []
        return record
    det.seperate_lines = recorder(0)
    det.seperate_lines_vertical = recorder(1)
    out = {"n": np.int64(N_PAGES)}
    non_empty = vertical_boxes = changed = 0
    for k in range(N_PAGES):
        regions, textlines = page(k)
        contours = det.get_text_region_contours_and_boxes(np.repeat(regions[:, :, None], 3, axis=2))
        boxes = [list(b) for b in det.boxes]
        del seen[:]
        sink = Sink()
        det.do_work_of_slopes(sink, boxes, textlines, contours)
        slopes = [float(s) for s in sink.item[0]]
        assert len(seen) == len(boxes), "a splitter must be reached for every box (the reference's bare except hides a broken stub)"
        out[f"slopes{k}"] = np.array(slopes, np.float64)
        out[f"vertical{k}"] = np.array([v for _d, v in seen], np.uint8)
        for r, (box, (dst, vertical)) in enumerate(zip(boxes, seen)):
            assert dst.shape == (box[3], box[2]) and dst.max(initial=0) <= 1
            assert vertical == int(abs(slopes[r]) > 45)
            out[f"dst{k}_{r}"] = np.packbits(dst)
            non_empty += bool(dst.any())
            vertical_boxes += vertical
            mask = lines_ref.eroded_crop(textlines[box[1]:box[1] + box[3], box[0]:box[0] + box[2]]) * np.uint8(255)
            changed += not np.array_equal(lines_ref.open_close(mask), mask)
        print("page", k, "boxes", boxes, "slopes", slopes, "vertical", [v for _d, v in seen])
    # a fixture of empty masks, one splitter and crops the morphology leaves alone proves nothing
    assert non_empty >= 4 and vertical_boxes >= 1 and changed >= 1 and disagree[0] >= 1, (non_empty, vertical_boxes, changed, disagree[0])
    np.savez_compressed(out_path, **out)
    print("wrote", out_path, os.path.getsize(out_path), "bytes;", non_empty, "non-empty masks,", vertical_boxes, "vertical,", changed,
          "crops changed by OPEN / CLOSE,", disagree[0], "pixels where the float and the fixed-point path disagree")


if __name__ == "__main__":
    main()
