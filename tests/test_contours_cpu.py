"""The contour tracer without a GPU: tests/contours_ref.py (OpenCV's border follower, restated) against the oracle's chain, and the
library's host twin ``sbbseg_mask_contours_host`` -- the same contour_walk.h the device kernels run -- against contours_ref on hand
shapes, seeded random masks and the adversarial planes of tests/cc_planes.py.  Every comparison is exact."""
import numpy as np
import pytest

from oracle import stage_glue as sg

import cc_planes
import contour_shapes
import contours_ref

def _capi():
    from sbb_textline_detection_amd import _capi
    return _capi


def _components(mask):
    from scipy import ndimage
    lab, n = ndimage.label(np.asarray(mask) != 0, structure=np.ones((3, 3), int))
    return [lab == k for k in range(1, n + 1)]


def _direction_changes(chain):
    """The rule of tests/golden/make_glue_golden.py::approx_simple."""
    n = len(chain)
    if n < 3:
        return list(chain)
    keep = []
    for i in range(n):
        (x0, y0), (x1, y1), (x2, y2) = chain[i - 1], chain[i], chain[(i + 1) % n]
        if (x1 - x0, y1 - y0) != (x2 - x1, y2 - y1):
            keep.append(chain[i])
    return keep


def _check_host_against_ref(mask, what):
    """sbbseg_mask_contours_host == contours_ref on all tables; area2 == the oracle's; the box is the component's; the step bound holds."""
    boxes, area2, off, pts = _capi().mask_contours_host_tables(mask)
    want = contours_ref.mask_contours(mask)
    assert len(boxes) == len(want) and off[0] == 0 and off[-1] == len(pts), what
    comps = _components(mask)[::-1]
    for k, (box, a2, p, chain_len) in enumerate(want):
        assert boxes[k].tolist() == box, (what, k)
        assert int(area2[k]) == a2 == sg.outer_contour_area2(comps[k]), (what, k)
        assert np.array_equal(pts[off[k]:off[k + 1]], p), (what, k)
        ys, xs = np.nonzero(comps[k])
        assert box == [xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1], (what, k)
        assert chain_len <= 8 * int(comps[k].sum()), (what, k, chain_len)
    return len(want)


def test_ref_is_the_oracle_chain_reversed():
    """CHAIN_APPROX_NONE of the restated follower = the oracle's clockwise chain walked the other way from the same start; its
    CHAIN_APPROX_SIMPLE list = the direction-change rule on that chain."""
    n = 0
    for mask in contour_shapes.random_masks(120, seed=5):
        for comp in _components(mask):
            chain = sg.outer_contour_chain(comp)
            none = contours_ref.follow_outer_border(comp, simple=False)
            assert none == [chain[0]] + chain[:0:-1]
            simple = contours_ref.follow_outer_border(comp, simple=True)
            assert simple == _direction_changes(none)
            assert simple[0] == none[0]                             # the start pixel is a kept point
            n += 1
    assert n > 300


@pytest.mark.parametrize("name", list(contour_shapes.hand_shapes()))
def test_host_twin_on_hand_shapes(name):
    mask = contour_shapes.hand_shapes()[name]
    n = _check_host_against_ref(mask, name)
    assert n == {"ring_with_island": 2, "c_with_foreign_blob": 2}.get(name, 1)
    _, contours = _capi().mask_contours_host(mask)
    if name == "single_pixel":
        assert contours[0].tolist() == [[1, 1]]
    if name.startswith("two_"):
        assert len(contours[0]) == 2
    if name == "spur":
        assert [8, 3] in contours[-1].tolist()                      # the spur's tip
    if name == "pinch":
        assert contours[0].tolist().count([3, 3]) == 0 and len(contours[0]) == 10      # the pinch pixel lies on two straight runs


def test_host_twin_on_random_masks():
    total = sum(_check_host_against_ref(m, ("random", k)) for k, m in enumerate(contour_shapes.random_masks(200, seed=0)))
    assert total > 400


@pytest.mark.parametrize("family", list(cc_planes.region_families()))
def test_host_twin_on_region_planes(family):
    """The opened / closed masks of every cc_planes region plane (spirals and combs give long chains), and the host mirror's boxes."""
    from sbb_textline_detection_amd import stages
    for name, plane in cc_planes.region_families()[family].items():
        _check_host_against_ref(cc_planes.region_mask(plane), name)
        boxes, contours = stages.host_text_region_contours(plane, 1, 0.0, 1.0)
        assert boxes == [b for b, c in zip(*_all_parentless(plane)) if len(c) >= 3], name
        for box, c in zip(boxes, contours):
            assert box == [c[:, 0].min(), c[:, 1].min(), c[:, 0].max() - c[:, 0].min() + 1, c[:, 1].max() - c[:, 1].min() + 1], name


def _all_parentless(plane):
    """(boxes, contours) of every parentless component of the plane's opened / closed mask, from the oracle's boxes and contours_ref."""
    want = cc_planes.oracle_region_boxes(_plane_name(plane), 0.0, 1.0)
    by_box = {tuple(b): p for b, _, p, _ in contours_ref.mask_contours(cc_planes.region_mask(plane))}
    return [list(b) for b in want], [by_box[tuple(b)] for b in want]


def _plane_name(plane):
    for planes in cc_planes.region_families().values():
        for name, p in planes.items():
            if p is plane or (p.shape == plane.shape and np.array_equal(p, plane)):
                return name
    raise KeyError


def test_counts_query_and_small_capacity():
    import ctypes as C
    capi = _capi()
    lib = capi.load_library()
    mask = np.ascontiguousarray(contour_shapes.hand_shapes()["ring_with_island"])
    n, npts = C.c_int(0), C.c_int64(0)
    assert lib.sbbseg_mask_contours_host(capi._ptr(mask), 13, 13, None, None, None, 0, None, 0, C.byref(n), C.byref(npts)) == 0
    assert (n.value, npts.value) == (2, 8)
    boxes, area2, off, pts = np.full((2, 4), -7, np.int32), np.full(2, -7, np.int64), np.full(3, -7, np.int64), np.full((7, 2), -7, np.int32)
    rc = lib.sbbseg_mask_contours_host(capi._ptr(mask), 13, 13, capi._ptr(boxes), capi._ptr(area2), capi._ptr(off), 2, capi._ptr(pts), 7,
                                       C.byref(n), C.byref(npts))
    assert rc != 0 and b"room for" in lib.sbbseg_last_error()
    assert (boxes == -7).all() and (area2 == -7).all() and (off == -7).all() and (pts == -7).all()


def test_step_bound_is_an_error_not_a_spin():
    """The failure path of the bounded walk, on the host twin: with the bound set artificially small a contour that needs more steps
    ends with an error that names it; with the real bound every plane above closes."""
    capi = _capi()
    mask = contour_shapes.staircase(40)
    capi.set_contour_host_step_bound(50)
    try:
        with pytest.raises(RuntimeError, match="did not close within 50 steps"):
            capi.mask_contours_host(mask)
        assert len(capi.mask_contours_host(contour_shapes.hand_shapes()["pinch"])[1][0]) == 10      # 12 steps: inside the bound
    finally:
        capi.set_contour_host_step_bound(0)
    assert len(capi.mask_contours_host(mask)[1]) == 1


def test_host_mirror_equals_the_fixture():
    """stages.host_text_region_contours + closed_rings == what the reference's get_text_region_contours_and_boxes returned
    (tests/golden/make_contours_golden.py): boxes, list order, ring closing, dtype."""
    from sbb_textline_detection_amd import stages
    for regions, boxes, rings in contour_shapes.golden_cases():
        got_boxes, contours = stages.host_text_region_contours(regions)
        got = stages.closed_rings(contours)
        assert got_boxes == boxes
        assert len(got) == len(rings) and all(g.dtype == np.uint and g.shape == r.shape and np.array_equal(g, r) for g, r in zip(got, rings))
