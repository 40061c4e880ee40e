#!/usr/bin/env python3
"""Generate tests/golden/contours_golden.npz by running the REFERENCE's OWN get_text_region_contours_and_boxes (main.py:456-481) on the
eight region maps of the glue fixture and the five pages of the slopes fixture.

Runs only where the reference is checked out; never on the GPU box.  ``main.py`` is imported as ``make_glue_golden.py`` and
``make_slopes_golden.py`` import it (stub modules, the oracle's restatements behind the cv2 calls).  The ``cv2.findContours`` stub is
make_glue_golden's -- list order, holes and hierarchy -- with every component's contour replaced by what ``tests/contours_ref.py``, the
restatement of OpenCV's border follower, traces: OpenCV's start point, OpenCV's counter-clockwise direction, CHAIN_APPROX_SIMPLE.

What this pins: the reference's filter (three points, the area window, `hierarchy[..][3] == -1`), the ring closing of
``polygon.exterior.coords`` (first point repeated), the ``np.uint`` dtype and [N + 1, 1, 2] shape, the list order and ``self.boxes``.
What it cannot pin: the cv2 rules inside the stub ([EXT], cv2 is not installable) -- against them the fixture is a self-consistency check.

The fixture holds the reference's outputs only; the inputs are the region maps the glue and slopes fixtures already hold.
    python tests/golden/make_contours_golden.py [out.npz]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_tiling_golden import load_reference  # noqa: E402
from make_glue_golden import TEXT_REGION_CASES, install_contour_tree_stubs, install_cv2_stubs, text_region_map  # noqa: E402
from make_slopes_golden import N_PAGES, page  # noqa: E402
import contours_ref  # noqa: E402


def install_opencv_order(cv2):
    """cv2.findContours: the glue stub's list with the component contours as OpenCV's follower lists them."""
    from scipy import ndimage
    glue_find = cv2.findContours

    def find_contours(mask, mode, method):
        contours, hierarchy = glue_find(mask, mode, method)
        lab, n = ndimage.label(mask > 0, structure=np.ones((3, 3), int))
        k, last_comp = n, None                               # the stub lists component n, its holes, component n - 1, its holes, ...
        out = []
        for i, c in enumerate(contours):
            if last_comp is not None and hierarchy[0][i][3] == last_comp:
                out.append(c)                                # a hole of the component before it: never kept, but it advances `jv`
                continue
            pts = contours_ref.follow_outer_border(lab == k, simple=True)
            assert sorted(map(tuple, np.asarray(c).reshape(-1, 2).tolist())) == sorted(pts), "the two tracers disagree on the kept points"
            out.append(np.array([[p] for p in pts], np.int32))
            last_comp, k = i, k - 1
        assert k == 0
        return out, hierarchy
    cv2.findContours = find_contours


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "contours_golden.npz")
    ref = load_reference()
    import cv2
    install_cv2_stubs(cv2, {})
    install_contour_tree_stubs(cv2, ref)
    install_opencv_order(cv2)
    det = ref.textline_detector.__new__(ref.textline_detector)
    det.kernel = np.ones((5, 5), np.uint8)                    # main.py:57
    inputs = [("glue", k, text_region_map(h, w, kind)) for k, (h, w, kind) in enumerate(TEXT_REGION_CASES)]
    inputs += [("slopes", k, np.repeat(page(k)[0][:, :, None], 3, axis=2)) for k in range(N_PAGES)]
    out = {"n": np.int64(len(inputs))}
    for j, (source, k, regions) in enumerate(inputs):
        kept = det.get_text_region_contours_and_boxes(regions)
        assert len(kept) == len(det.boxes)
        assert all(c.dtype == np.uint and c.ndim == 3 and c.shape[1:] == (1, 2) and (c[0] == c[-1]).all() for c in kept)
        out[f"source{j}"] = np.array([source == "slopes", k], np.int64)      # the input: regions_map<k> of glue_golden.npz / regions<k> of slopes_golden.npz
        out[f"shape{j}"] = np.array(regions.shape, np.int64)
        out[f"boxes{j}"] = np.array(det.boxes, np.int64).reshape(-1, 4)
        out[f"lengths{j}"] = np.array([len(c) for c in kept], np.int64)
        out[f"points{j}"] = (np.concatenate([c.reshape(-1, 2) for c in kept]) if kept else np.zeros((0, 2))).astype(np.int32)
        print(source, k, regions.shape, "->", len(kept), "contours,", int(out[f"lengths{j}"].sum()), "points")
    np.savez_compressed(out_path, **out)
    print("wrote", out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
