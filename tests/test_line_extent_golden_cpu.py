"""The library's serial host twin of the text-line x extents against tests/golden/line_extent_golden.npz: ``textline_boxes_rot`` as the
reference's OWN ``textline_contours_postprocessing`` and its two real splitters return it for the boxes and contours of the five fixture
pages and for small synthetic regions.  A SELF-CONSISTENCY fixture (tests/golden/make_line_extent_golden.py): the reference ran on cv2
stubs, three of which are the restatement of tests/line_extent_ref.py -- it pins the reference's control flow around the cv2 calls, not
OpenCV.  The line records that go in are the library's own, from the ``dst`` the reference's splitter received."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import line_extent_cases as cases  # noqa: E402
from sbb_textline_detection_amd import _capi  # noqa: E402


def test_host_twin_returns_the_polygons_the_reference_returned():
    golden = cases.golden_cases()
    assert sorted({c["page"] for c in golden}) == [-1, 0, 1, 2, 3, 4]
    kinds = set()
    for c in golden:
        got = _capi.host_region_line_extents(c["ring"], c["box"], c["slope"], c["record"], want_masks=True)
        contour, w = got["contour"], int(c["box"][2])
        assert contour["status"] == c["status"] and contour["holes"] == c["holes"], c["name"]
        polygons = got["boxes_rot"] if got["status"] == _capi.LINES_OK else got["boxes_rot"][:0]
        assert np.array_equal(polygons, c["polygons"]), c["name"]
        if c["status"] != 0:
            kinds.add("none")
            continue
        assert (contour["is_hole"], contour["tie"]) == (c["is_hole"], c["tie"]), c["name"]
        if abs(c["slope"]) > 45:
            kinds.add("vertical")
            continue
        if c["holes"]:
            kinds.add("hole in threshrot")
        for peak, extent in zip(got["peaks"].tolist(), got["extent"].tolist()):
            if tuple(extent) != (0, w):
                kinds.add("differs from 0 .. w")
            row = np.concatenate([[0], contour["threshrot"][peak] != 0, [0]]).astype(np.int8)
            if (np.diff(row) == 1).sum() >= 2 and got["branch"] != 2:
                kinds.add("two inside intervals on a row")
    assert kinds == {"none", "vertical", "hole in threshrot", "differs from 0 .. w", "two inside intervals on a row"}, kinds
