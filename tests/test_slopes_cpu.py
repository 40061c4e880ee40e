"""The boxes + slopes step without a GPU: the host mirror of the box search and the composed oracle against the fixture recorded from
the reference's own control flow (tests/golden/make_slopes_golden.py), the new names of the C ABI, and its argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sbb_textline_detection_amd import _capi, stages

import slopes_ref

NEW_EXPORTS = ["sbbseg_text_region_boxes_dev", "sbbseg_text_region_boxes", "sbbseg_region_deskew_profiles_dev", "sbbseg_region_deskew_profiles"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pages():
    return slopes_ref.load_pages()


def test_fixture_exercises_what_it_must(pages):
    """Boxes of a ring (not of its island), of two blocks joined by CLOSE; slopes that are not 0; the second sweep's angle set."""
    assert len(pages) >= 4
    assert len(pages[0][2]) == 2 and len(pages[1][2]) == 1
    slopes = [s for p in pages for s in p[3]]
    assert sum(1 for s in slopes if s != 0) >= 4
    assert any(s <= -50 for s in slopes), "no slope from the second sweep (30 angles in [-90, -50])"
    allowed = set(float(a) for a in slopes_ref.SWEEP1) | set(float(a) for a in slopes_ref.SWEEP2) | {0.0}
    assert all(s in allowed for s in slopes)


def test_host_mirror_boxes_equal_the_reference(pages):
    """stages.host_text_region_boxes (the library's host tracer, no GPU): the same boxes in the same, documented order."""
    for k, (regions, _t, boxes, _s) in enumerate(pages):
        assert stages.host_text_region_boxes(regions) == boxes, k
        assert stages.host_text_region_boxes(np.repeat(regions[:, :, None], 3, axis=2)) == boxes, k
        assert slopes_ref.oracle_boxes(regions) == boxes, k
    one_channel = np.repeat(pages[1][0][:, :, None], 3, axis=2)
    one_channel[:, :, 1] = 0                                     # main.py:458: np.all(image == (1, 1, 1), axis=-1)
    assert stages.host_text_region_boxes(one_channel) == []


def test_host_mirror_area_filter():
    """min_area x H x W is compared with the outer-contour area (through pixel centres): a 5 x 5 square has area 16."""
    r = np.zeros((1400, 1200), np.uint8)
    r[700:705, 600:605] = 1                                      # area 16 < 16.8
    r[100:105, 100:106] = 1                                      # area 20
    assert stages.host_text_region_boxes(r) == [[100, 100, 6, 5]]
    assert stages.host_text_region_boxes(r, min_area=0.0) == [[600, 700, 5, 5], [100, 100, 6, 5]]
    assert stages.host_text_region_boxes(r, min_area=0.0, max_area=17.0 / r.size) == [[600, 700, 5, 5]]


def test_composed_oracle_slopes_equal_the_reference(pages):
    """crop, erode x 2, oracle return_deskew_slope(., 2), clean-up == what do_work_of_slopes returned."""
    for k, (_r, textlines, boxes, slopes) in enumerate(pages):
        assert slopes_ref.oracle_slopes(textlines, boxes) == slopes, k


def test_new_names_are_exported_and_declared():
    lib = _capi.load_library()
    header = open(os.path.join(ROOT, "include", "sbbseg.h")).read()
    for name in NEW_EXPORTS:
        assert name in _capi.EXPORTS and hasattr(lib, name)
        assert re.search(r"\bint %s\(" % name, header)
    assert lib.sbbseg_abi_version() == 5
    for attr in ("text_region_boxes", "text_region_boxes_dev", "region_deskew_profiles", "region_deskew_profiles_dev"):
        assert callable(getattr(_capi.Context, attr))
    for attr in ("host_text_region_boxes", "get_slopes"):
        assert callable(getattr(stages, attr))
    for attr in ("get_text_region_boxes", "get_slopes", "run_with_slopes"):
        assert callable(getattr(stages.InferenceStages, attr))


def test_packed_offsets_and_bad_boxes():
    """The size query needs no handle: offsets of the packed counts, and every bad box is a RuntimeError with a message."""
    off = _capi.region_deskew_offsets([[0, 0, 5, 5], [10, 20, 100, 40], [0, 0, 300, 200]], 80, 200, 300)
    sides = [int(1.4 * 5), int(1.4 * 100), int(1.4 * 300)]
    assert list(off) == [0, 80 * sides[0], 80 * (sides[0] + sides[1]), 80 * sum(sides)]
    assert [_capi.deskew_side(h, w) for (w, h) in ((5, 5), (100, 40), (300, 200))] == sides
    assert list(_capi.region_deskew_offsets(np.zeros((0, 4), np.int32), 80, 200, 300)) == [0]
    for bad in ([0, 0, 0, 5], [0, 0, 5, 0], [-1, 0, 5, 5], [0, -1, 5, 5], [296, 0, 5, 5], [0, 196, 5, 5], [0, 0, 5, -3]):
        with pytest.raises(RuntimeError, match="box 1"):
            _capi.region_deskew_offsets([[0, 0, 5, 5], bad], 80, 200, 300)
    with pytest.raises(RuntimeError, match="side"):
        _capi.region_deskew_offsets([[0, 0, 5, 30000]], 1, 30000, 5)             # S = 42000 > 32767
    with pytest.raises(RuntimeError):
        _capi.region_deskew_offsets([[0, 0, 5, 5]], 0, 200, 300)                 # no angles


def test_calls_without_a_handle_fail_cleanly():
    """A null handle, a zero cap: a status and a message, never a crash."""
    lib = _capi.load_library()
    n = C.c_int(-1)
    plane = np.zeros((8, 8), np.uint8)
    assert lib.sbbseg_text_region_boxes(None, plane.ctypes.data_as(C.c_void_p), 8, 8, 1, 1e-5, 1.0, None, 0, C.byref(n)) != 0
    assert b"null handle" in lib.sbbseg_last_error()
    boxes = np.array([[0, 0, 5, 5]], np.int32)
    angles = np.zeros(1, np.float64)
    counts, off = np.zeros(7, np.int32), np.zeros(2, np.int64)
    rc = lib.sbbseg_region_deskew_profiles(None, plane.ctypes.data_as(C.c_void_p), 8, 8, boxes.ctypes.data_as(C.c_void_p), 1, 2,
                                           angles.ctypes.data_as(C.c_void_p), 1, counts.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p))
    assert rc != 0 and b"null handle" in lib.sbbseg_last_error()
    with pytest.raises(RuntimeError, match="library handle"):
        stages.get_slopes(plane, [[0, 0, 5, 5]], None)
