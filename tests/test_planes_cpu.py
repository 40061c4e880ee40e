"""The pooled per-box calls (boxes on many device planes) without a GPU: the four symbols exist in the header, the binding and the built
library; the argument errors that the one-plane entry points report before they need a handle are reported by the pooled ones too and name
the box; the page-grouping helper."""
import ctypes as C
import os

import numpy as np
import pytest

from sbb_textline_detection_amd import _build, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["sbbseg_run_pages_planes", "sbbseg_planes_deskew_slopes_dev", "sbbseg_planes_line_masks_dev", "sbbseg_planes_line_boxes_dev"]
FAKE = 0x1000                                                     # a non-null "device pointer": nothing here reaches a launch


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _capi.load_library()


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _planes(sizes, ptr=FAKE):
    arr = (_capi.Plane * len(sizes))()
    for k, (h, w) in enumerate(sizes):
        arr[k].d_hw, arr[k].H, arr[k].W = ptr, h, w
    return arr


def _masks(lib, planes, n_planes, boxes, box_plane):
    """sbbseg_planes_line_masks_dev with a NULL handle: (status, message)."""
    b = np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
    bp = np.ascontiguousarray(box_plane, np.int32)
    n = b.shape[0]
    slopes = np.zeros(max(n, 1), np.float64)
    rows, cols = np.zeros(1 << 12, np.int32), np.zeros(1 << 12, np.int32)
    mo, ro, co = (np.full(n + 1, -1, np.int64) for _ in range(3))
    rc = lib.sbbseg_planes_line_masks_dev(None, planes, n_planes, _p(b), _p(bp), n, 2, _p(slopes), None, _p(rows), _p(cols), _p(mo), _p(ro), _p(co))
    return rc, (lib.sbbseg_last_error() or b"").decode(), (mo, ro, co)


def _line_boxes(lib, planes, n_planes, boxes, box_plane):
    b = np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
    bp = np.ascontiguousarray(box_plane, np.int32)
    n = b.shape[0]
    slopes, rot = np.zeros(max(n, 1), np.float64), np.zeros((max(n, 1), 6), np.float64)
    w, w_off = _capi.line_weight_table()
    info, line_off = np.zeros((max(n, 1), 5), np.int32), np.zeros(n + 1, np.int64)
    big = np.zeros((1 << 12, 8), np.int32)
    rc = lib.sbbseg_planes_line_boxes_dev(None, planes, n_planes, _p(b), _p(bp), n, 2, _p(slopes), _p(rot), _p(w), _p(w_off), _capi.LINE_SIGMA_MAX,
                                          _p(info), _p(line_off), _p(big), _p(big), _p(big))
    return rc, (lib.sbbseg_last_error() or b"").decode()


def test_symbols_are_declared_bound_and_built(lib):
    header = open(os.path.join(ROOT, "include", "sbbseg.h")).read()
    for name in NEW_EXPORTS:
        assert name + "(" in header and name in _capi.EXPORTS and hasattr(lib, name), name
    assert "typedef struct sbbseg_plane { const void* d_hw; int32_t H, W; } sbbseg_plane;" in header
    assert "#define SBBSEG_ABI_VERSION 5" in header and lib.sbbseg_abi_version() == 5
    assert C.sizeof(_capi.Plane) == 16


def test_box_errors_come_before_the_handle_and_name_the_box(lib):
    sizes = [(23, 31), (19, 47), (64, 40)]
    planes = _planes(sizes)
    good = [[0, 0, 31, 23], [40, 10, 7, 9], [0, 0, 40, 64]]
    for call in (_masks, _line_boxes):
        # all boxes fine: the next thing the call needs is the handle
        rc, msg = call(lib, planes, 3, good, [0, 1, 2])[:2]
        assert rc != 0 and "null handle" in msg, msg
        # a box_plane out of range, on either side
        for bad in (3, -1):
            rc, msg = call(lib, planes, 3, good, [0, 1, bad])[:2]
            assert rc != 0 and "box 2" in msg and "plane %d out of range" % bad in msg, msg
        # box 1 fits plane 1 (19 x 47) but is said to lie on plane 0 (23 x 31): it leaves ITS OWN plane
        rc, msg = call(lib, planes, 3, good, [0, 0, 2])[:2]
        assert rc != 0 and "box 1 (40, 10, 7, 9) leaves the 31 x 23 plane 0" in msg, msg
        # ... and the whole of plane 2 does not fit plane 1
        rc, msg = call(lib, planes, 3, good, [0, 1, 1])[:2]
        assert rc != 0 and "box 2 (0, 0, 40, 64) leaves the 47 x 19 plane 1" in msg, msg
        rc, msg = call(lib, planes, 3, [good[0], [0, 0, 0, 5]], [0, 1])[:2]
        assert rc != 0 and "box 1: width 0, height 5" in msg, msg
        # a plane that a box names has no pointer; one that no box names may have none
        holes = _planes(sizes)
        holes[1].d_hw = None
        rc, msg = call(lib, holes, 3, good, [0, 1, 2])[:2]
        assert rc != 0 and "box 1: plane 1 has no device pointer" in msg, msg
        rc, msg = call(lib, holes, 3, [good[0], good[2]], [0, 2])[:2]
        assert rc != 0 and "null handle" in msg, msg
        # boxes but no planes
        rc, msg = call(lib, planes, 0, good, [0, 1, 2])[:2]
        assert rc != 0 and "3 boxes but 0 planes" in msg, msg
        rc, msg = call(lib, None, 3, good, [0, 1, 2])[:2]
        assert rc != 0 and "bad arguments" in msg, msg
        # no boxes: success, without a handle and without planes
        assert call(lib, None, 0, np.zeros((0, 4)), [])[0] == 0
    # the offsets of the size part are written in box order before the handle is needed -- the one-plane call's own sums
    rc, msg, (mo, ro, co) = _masks(lib, planes, 3, good, [0, 1, 2])
    assert mo.tolist() == [0, 31 * 23, 31 * 23 + 63, 31 * 23 + 63 + 40 * 64] and ro.tolist() == [0, 23, 32, 96] and co.tolist() == [0, 31, 38, 78]
    # the pooled limit: the sum of the areas over all planes
    huge = _planes([(40000, 40000)] * 2)
    rc, msg = _masks(lib, huge, 2, [[0, 0, 40000, 40000]] * 2, [0, 1])[:2]
    assert rc != 0 and "too much work for one call" in msg, msg
    # the slopes call needs its handle first, as its one-plane twin does
    slopes = np.zeros(3, np.float64)
    b, bp = np.ascontiguousarray(good, np.int32), np.array([0, 1, 5], np.int32)
    assert lib.sbbseg_planes_deskew_slopes_dev(None, planes, 3, _p(b), _p(bp), 3, 2, None, 0, _p(slopes)) != 0
    assert b"null handle" in lib.sbbseg_last_error()
    # the planes of a run need a handle too
    out = (_capi.Plane * 1)()
    assert lib.sbbseg_run_pages_planes(None, 1, out, out) != 0 and b"null handle" in lib.sbbseg_last_error()
    assert lib.sbbseg_debug_counter(None, 5, None) != 0


def test_pool_planes_packs_in_plane_order():
    arr, n, boxes, box_plane, counts = _capi._pool_planes([(FAKE, 5, 6), (0, 7, 8), (FAKE + 64, 9, 10)], [[[0, 0, 1, 1], [1, 1, 2, 2]], [], [[3, 3, 4, 4]]])
    assert n == 3 and counts == [2, 0, 1] and box_plane.tolist() == [0, 0, 2] and boxes.tolist() == [[0, 0, 1, 1], [1, 1, 2, 2], [3, 3, 4, 4]]
    assert [(arr[k].d_hw, arr[k].H, arr[k].W) for k in range(3)] == [(FAKE, 5, 6), (None, 7, 8), (FAKE + 64, 9, 10)]
    assert _capi._unpool(["a", "b", "c"], counts) == [["a", "b"], [], ["c"]]
    with pytest.raises(ValueError, match="one box list per plane"):
        _capi._pool_planes([(FAKE, 5, 6)], [[], []])
    with pytest.raises(ValueError, match="one slope per box"):
        _capi._pool_planes([(FAKE, 5, 6)], [[[0, 0, 1, 1]]], [[]])


def test_page_groups_split_at_the_limits_and_are_never_empty():
    group = _capi.group_pages_for_lines
    assert group([]) == []
    # areas 100, 100, 100 under a limit of 250: the third page opens a group
    pages = [[[0, 0, 10, 10]]] * 3
    assert group(pages, max_area=250) == [[0, 1], [2]]
    assert group(pages, max_area=200) == [[0, 1], [2]] and group(pages, max_area=199) == [[0], [1], [2]]      # the limit itself is allowed
    # the count limit: n_angles * int(1.4 * max(h, w)) = 80 * 14 = 1120 per box
    assert group(pages, max_counts=2240) == [[0, 1], [2]] and group(pages, max_counts=2239) == [[0], [1], [2]]
    assert group(pages, n_angles=30, max_counts=30 * 14 * 3) == [[0, 1, 2]]
    # S follows the longer side, truncated as the library truncates it: int(1.4 * 7) = 9
    assert group([[[0, 0, 7, 2]], [[0, 0, 2, 7]]], n_angles=1, max_counts=18) == [[0, 1]]
    assert group([[[0, 0, 7, 2]], [[0, 0, 2, 7]]], n_angles=1, max_counts=17) == [[0], [1]]
    # pages without boxes cost nothing and join their neighbours; a page beyond the limit on its own still gets a group
    pages = [[], [[0, 0, 10, 10]], [], [[0, 0, 100, 100]], [], [[0, 0, 10, 10], [0, 0, 10, 10]]]
    got = group(pages, max_area=250)
    assert got == [[0, 1, 2], [3], [4, 5]]
    rng = np.random.RandomState(5)
    for _ in range(50):
        pages = [[[0, 0, int(rng.randint(1, 60)), int(rng.randint(1, 60))] for _ in range(rng.randint(0, 5))] for _ in range(rng.randint(1, 12))]
        lim_a, lim_c = int(rng.randint(1, 6000)), int(rng.randint(1, 40000))
        got = group(pages, max_area=lim_a, max_counts=lim_c)
        assert [k for g in got for k in g] == list(range(len(pages))) and all(got)
        for g in got:
            a = sum(b[2] * b[3] for k in g for b in pages[k])
            c = sum(80 * int(1.4 * max(b[2], b[3])) for k in g for b in pages[k])
            assert (a <= lim_a and c <= lim_c) or len(g) == 1, (g, a, c)          # (a page beyond a limit stands alone)
    # the defaults are the library's own bounds (sums below 2^31)
    assert group([[[0, 0, 40000, 40000]], [[0, 0, 40000, 40000]]]) == [[0], [1]]
