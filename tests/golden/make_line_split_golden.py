#!/usr/bin/env python3
"""Generate tests/golden/line_split_golden.npz by running the REFERENCE's OWN ``seperate_lines`` (main.py:516-991) and
``seperate_lines_vertical`` (main.py:993-1457) on the ``dst`` of every box of the five pages of ``make_slopes_golden.page()`` (as
recorded in lines_golden.npz from the reference's control flow) and on small synthetic stripe masks.

Runs only where the reference is available (the build container); never on the GPU box.  The reference is imported exactly as
``make_lines_golden.py`` imports it, with the same stubs, plus:
  * ``cv2.pointPolygonTest`` returns -1, so the full-width fallback x_min_cont / x_max_cont is taken (the contour half is out of scope);
  * ``return_contours_of_image`` / ``filter_contours_area_of_image`` on the instance return nothing: their results are unused inside the
    first ``try`` (main.py:608-610), and they are taken as non-raising [EXT] unpinned.
The functions return only ``peaks`` and ``textline_boxes_rot``; sigma_gaus, the unrotated boxes and the cluster list are read from the
function's own local variables when it returns or raises (``sys.setprofile``).  An exception that leaves the function is what
``textline_contours_postprocessing``'s bare except turns into [] (main.py:1520): status 1.
The fixture holds arrays only.  On every recorded case the reference's ``np.dot`` corners equal the elementwise form ``a * x + b * y +
d`` of tests/line_split_ref.py (asserted below: no case had to be replaced).
The branch ``len(peaks) < 1`` (main.py:822 / 1288) needs a profile without an interior maximum after the second smoothing: mass at both
ends only, and a sigma_gaus whose radius exceeds the pads, so that ``gaussian_filter1d``'s reflection puts the maxima on the array's ends.
Only the vertical splitter gets there (main.py:1127 takes its maximum over the minima); the horizontal one raises in main.py:646.
    python tests/golden/make_line_split_golden.py [out.npz]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_glue_golden import install_contour_tree_stubs, install_cv2_stubs  # noqa: E402
from make_tiling_golden import load_reference  # noqa: E402
from oracle import deskew as dk  # noqa: E402
import line_split_ref as lr  # noqa: E402
import lines_ref  # noqa: E402


def stripes(h, w, period, thick, first=3, skip=()):
    m = np.zeros((h, w), np.uint8)
    for k, top in enumerate(range(first, h, period)):
        if k not in skip:
            m[top:top + thick, 2:w - 2] = 1
    return m


def synthetic():
    """(dst, slope): small masks chosen until the assertions of main() hold."""
    out = [(np.zeros((30, 40), np.uint8), 0.0), (np.zeros((30, 40), np.uint8), 90.0)]                 # np.max of nothing: [] and sigma 12
    out.append((stripes(40, 50, 100, 6, first=15), 1.0))                                              # one line
    out.append((stripes(40, 50, 100, 6, first=15).T.copy(), 80.0))                                    # one line, vertical: NameError
    out.append((stripes(70, 50, 36, 8, first=10), -2.0))                                              # two lines
    out.append((stripes(160, 60, 30, 9), 3.0))
    out.append((stripes(160, 60, 30, 9).T.copy(), -88.0))
    out.append((stripes(400, 80, 60, 20), 12.0))                                                      # sigma > 3
    out.append((stripes(400, 80, 60, 20).T.copy(), 60.0))
    out.append((stripes(300, 64, 24, 7, skip=(4, 5, 9)), -6.5))                                       # gaps: shallow minima merge
    m = stripes(260, 64, 20, 6)
    m[:, 40:] = 0
    m[100:140, :] = 0
    out.append((m, 20.0))
    ends = np.zeros((50, 300), np.uint8)                                                              # column sums: 50 at both ends only
    ends[:, :3] = 1
    ends[:, -3:] = 1
    out.append((ends, 80.0))                                                                          # no peak left: `pass`, no lines
    out.append((ends.T.copy(), 2.0))                                                                  # the same rows: np.max of nothing
    rng = np.random.RandomState(3)
    for k in range(10):
        h, w = int(rng.randint(20, 330)), int(rng.randint(12, 90))
        m = stripes(h, w, int(rng.randint(6, 70)), int(rng.randint(2, 12)), first=int(rng.randint(0, 9)), skip=tuple(rng.randint(0, 12, 2)))
        m[rng.rand(h, w) < 0.15] = 0
        slope = float(rng.choice([-30.0, -4.0, 0.5, 7.0, 33.0, 50.0, -75.0]))
        out.append((m.T.copy() if abs(slope) > 45 else m, slope))
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "line_split_golden.npz")
    ref = load_reference()
    import cv2
    install_cv2_stubs(cv2, {})
    install_contour_tree_stubs(cv2, ref)
    cv2.pointPolygonTest = lambda contour, point, measure: -1.0
    det = ref.textline_detector.__new__(ref.textline_detector)
    det.kernel = np.ones((5, 5), np.uint8)                       # main.py:57
    det.return_contours_of_image = lambda img: ([], None)
    det.filter_contours_area_of_image = lambda *a, **k: []
    contour = np.zeros((1, 1, 2), np.int32)

    cases = []
    for k, (slopes, masks, vertical) in enumerate(lines_ref.load_golden()):
        cases += [(dst, float(s), k, r) for r, (dst, s) in enumerate(zip(masks, slopes))]
    cases += [(dst, s, -1, r) for r, (dst, s) in enumerate(synthetic())]

    rows = {name: [] for name in ("y", "other", "vertical", "slope", "rot", "status", "sigma", "raised", "branch", "clusters", "peaks", "boxes",
                                  "boxes_rot", "page", "box")}
    clamped = 0
    for dst, slope, page, box in cases:
        vertical = int(abs(slope) > 45)
        name = "seperate_lines_vertical" if vertical else "seperate_lines"
        seen = {}

        def profile(frame, event, arg, name=name, seen=seen):
            if event == "return" and frame.f_code.co_name == name:
                seen.update(frame.f_locals)
        sys.setprofile(profile)
        try:
            try:
                _peaks, boxes_rot = getattr(det, name)(dst, contour, slope)
                status = lr.OK
            except Exception:
                boxes_rot, status = [], lr.NONE
        finally:
            sys.setprofile(None)
        h, w = dst.shape
        y = dst.sum(axis=0 if vertical else 1).astype(np.int32)
        mean = seen.get("y_diff_mean", np.nan)
        raised = not np.isfinite(mean)
        assert raised == (seen["sigma_gaus"] == 12 and raised)
        n_peaks, n_neg = (len(seen["peaks"]), len(seen["peaks_neg"])) if "textline_boxes" in seen else (-1, -1)
        branch = -1 if n_peaks < 0 else 0 if (n_neg == n_peaks + 1 and n_peaks >= 3) else 1 if n_peaks < 1 else 2 if n_peaks == 1 else 3 if n_peaks == 2 else 4
        ok = status == lr.OK
        rec = {"status": status, "sigma": int(seen["sigma_gaus"]), "raised": raised, "branch": branch,
               "peaks": np.array(seen["peaks"] if ok else [], np.int32).reshape(-1),
               "boxes": np.array(seen["textline_boxes"] if ok else [], np.int32).reshape(-1, 4, 2),
               "boxes_rot": np.array(boxes_rot, np.int32).reshape(-1, 4, 2)}
        rec["point_up"], rec["point_down"] = rec["boxes"][:, 0, 1], rec["boxes"][:, 2, 1]
        rot = lr.rotation_terms(w, h, slope, dk.rotation_matrix)
        mine = lr.line_split(y, h if vertical else w, vertical, rot)
        # the restatement (elementwise corners) against the reference's own values (np.dot corners), every field
        assert lr.same(mine, rec), (page, box, slope, {f: (mine[f], rec[f]) for f in lr.FIELDS})
        clusters = len(seen["clusters_to_be_deleted"]) if "peaks_new" in seen and "mean_value_of_peaks" in seen else mine["clusters"]
        assert clusters == mine["clusters"]
        clamped += mine["clamped"]
        for key, v in (("y", y), ("other", h if vertical else w), ("vertical", vertical), ("slope", slope), ("rot", rot), ("status", status),
                       ("sigma", rec["sigma"]), ("raised", raised), ("branch", branch), ("clusters", clusters), ("peaks", rec["peaks"]),
                       ("boxes", rec["boxes"]), ("boxes_rot", rec["boxes_rot"]), ("page", page), ("box", box)):
            rows[key].append(v)
        print(page, box, dst.shape, slope, "status", status, "sigma", rec["sigma"], "raised", raised, "branch", branch, "clusters", clusters,
              "lines", len(rec["peaks"]))

    branches = set(rows["branch"])
    # a fixture that misses any of these proves nothing
    assert {0, 1, 2, 3, 4} <= branches, branches
    assert any(rows["vertical"]) and any(rows["raised"]) and any(s > 3 for s in rows["sigma"]) and any(c > 0 for c in rows["clusters"])
    assert any(s == lr.NONE for s in rows["status"]) and clamped >= 1
    assert any(v and s == lr.OK and len(p) for v, s, p in zip(rows["vertical"], rows["status"], rows["peaks"]))
    out = {"y": np.concatenate(rows["y"]).astype(np.int32), "y_off": np.concatenate([[0], np.cumsum([len(v) for v in rows["y"]])]).astype(np.int64),
           "line_off": np.concatenate([[0], np.cumsum([len(v) for v in rows["peaks"]])]).astype(np.int64),
           "peaks": np.concatenate(rows["peaks"]).astype(np.int32), "boxes": np.concatenate(rows["boxes"]).astype(np.int32),
           "boxes_rot": np.concatenate(rows["boxes_rot"]).astype(np.int32), "rot": np.array(rows["rot"], np.float64),
           "slope": np.array(rows["slope"], np.float64)}
    for key in ("other", "vertical", "status", "sigma", "raised", "branch", "clusters", "page", "box"):
        out[key] = np.array(rows[key], np.int32)
    np.savez_compressed(out_path, **out)
    print("wrote", out_path, os.path.getsize(out_path), "bytes;", len(rows["other"]), "cases, branches", sorted(branches), "clamped lines' regions", clamped)


if __name__ == "__main__":
    main()
