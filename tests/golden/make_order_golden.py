#!/usr/bin/env python3
"""Generate tests/golden/order_golden.npz by running the REFERENCE's OWN order_of_regions and order_and_id_of_texts (main.py:1802-1906) on
the textline planes of the slopes fixture with the rings the contours fixture holds for them, plus a few small synthetic planes
(``tests/order_ref.py: fixture_cases``).

Runs only where the reference is checked out; never on the GPU box.  ``main.py`` is imported as the other generators import it.
``cv2.moments`` and ``cv2.contourArea`` are stubbed by ``tests/order_ref.py``'s restatement of OpenCV's contourMoments ([EXT], cv2 is not
installable): against those rules the fixture is a self-consistency check.  What it pins is everything else -- the padding, the sigma, the
``- 40``, the unclamped edges, the band tests, the argsort and the bookkeeping of order_and_id_of_texts.

The fixture holds the reference's outputs only.
    python tests/golden/make_order_golden.py [out.npz]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_tiling_golden import load_reference  # noqa: E402
import order_ref  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "order_golden.npz")
    ref = load_reference()
    import cv2
    cv2.moments = order_ref.moments
    cv2.contourArea = order_ref.contour_area
    det = ref.textline_detector.__new__(ref.textline_detector)
    cases = order_ref.fixture_cases(HERE)
    out = {"n": np.int64(len(cases))}
    low = high = empty_band = reordered = non_identity = 0
    for j, (plane, contours) in enumerate(cases):
        indexes_sorted, matrix = det.order_of_regions(plane, contours)
        order_of_texts, id_of_texts = det.order_and_id_of_texts(contours, matrix, indexes_sorted)
        out[f"indexes_sorted{j}"] = np.array(indexes_sorted, np.int64)
        out[f"matrix{j}"] = np.asarray(matrix, np.float64)
        out[f"order_of_texts{j}"] = np.array([int(v) for v in order_of_texts], np.int64)
        out[f"id_of_texts{j}"] = np.array(id_of_texts, dtype="U8")
        # what the fixture has to contain to prove anything (the restatement only describes the case; the outputs are the reference's)
        _, _, edges, bands = order_ref.order_of_regions(plane, contours)
        H = plane.shape[0]
        low += any(e < 0 for e in edges[1:-1])
        high += any(e >= H for e in edges[1:-1])
        assert sorted(indexes_sorted) == list(range(len(contours))), "every region in exactly one band"
        for i in range(len(edges) - 1):
            inside = [m for m in range(len(contours)) if bands[m] == i]
            empty_band += not inside
            cxs = [matrix[m, 2] for m in inside]
            assert len(set(cxs)) == len(cxs), "a cx tie inside a band: np.argsort's order would depend on the numpy build"
            reordered += len(inside) >= 3 and sorted(inside, key=lambda m: matrix[m, 2]) != inside
        non_identity += indexes_sorted != list(range(len(contours)))
        print("case", j, plane.shape, len(contours), "regions, edges", edges, "->", indexes_sorted)
    assert low and high and empty_band and reordered and non_identity, (low, high, empty_band, reordered, non_identity)
    np.savez_compressed(out_path, **out)
    print("wrote", out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
