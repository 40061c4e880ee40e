"""The reading order of text regions on the CPU: the library's serial host twins (csrc/order.h behind sbbseg_region_order_host /
sbbseg_contour_moments_host) and stages.order_of_regions / order_and_id_of_texts against the reference's own outputs
(tests/golden/order_golden.npz) and against the numpy / scipy restatement (tests/order_ref.py) -- every float64 bit-equal, every list
equal."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import order_ref  # noqa: E402
from sbb_textline_detection_amd import _capi, stages  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_against_ref(plane, contours):
    """host twin and stages against order_ref on one input; returns the record"""
    want_sorted, want_matrix, want_edges, want_bands = order_ref.order_of_regions(plane, contours)
    rec = _capi.host_region_order(plane, contours)
    assert rec["edges"].tolist() == want_edges
    assert rec["band"].tolist() == want_bands
    n = len(contours)
    kept = sum(b >= 0 for b in want_bands)
    assert rec["sorted_index"][:kept].tolist() == want_sorted
    assert sorted(rec["sorted_index"].tolist()) == list(range(n))                # a permutation, whatever the bands
    assert (bits(rec["centroids"]) == bits(want_matrix[:, 2:4])).all()
    for m in range(n):
        assert rec["order"][m] == (want_sorted.index(m) if want_bands[m] >= 0 else -1)
    got_sorted, got_matrix = stages.order_of_regions(plane, contours)
    assert got_sorted == want_sorted and got_matrix.dtype == np.float64 and got_matrix.shape == (n, 5)
    assert (bits(got_matrix) == bits(want_matrix)).all()
    return rec


def test_fixture_holds_the_references_outputs():
    golden = np.load(os.path.join(GOLDEN, "order_golden.npz"))
    cases = order_ref.fixture_cases(GOLDEN)
    assert int(golden["n"]) == len(cases)
    for j, (plane, contours) in enumerate(cases):
        indexes_sorted, matrix = stages.order_of_regions(plane, contours)
        assert indexes_sorted == golden[f"indexes_sorted{j}"].tolist(), j
        assert (bits(matrix) == bits(golden[f"matrix{j}"])).all(), j
        order_of_texts, id_of_texts = stages.order_and_id_of_texts(contours, matrix, indexes_sorted)
        assert order_of_texts == golden[f"order_of_texts{j}"].tolist(), j
        assert id_of_texts == golden[f"id_of_texts{j}"].tolist(), j
        assert sorted(indexes_sorted) == list(range(len(contours)))              # every region in exactly one band
        check_against_ref(plane, contours)


def test_random_planes_match_scipy_bit_for_bit():
    rng = np.random.default_rng(5)
    low = high = many = 0
    for case in range(300):
        H, W = int(rng.integers(1, 601)), int(rng.integers(1, 201))
        plane = order_ref.random_plane(rng, H, W)
        contours = [order_ref.random_contour(rng, H, W) for _ in range(int(rng.integers(0, 13)))]
        rec = check_against_ref(plane, contours)
        assert (rec["band"] >= 0).all()                                          # centroids of polygons inside the plane: 0 <= cy < H
        low += bool((rec["edges"][1:-1] < 0).any())
        high += bool((rec["edges"][1:-1] >= H).any())
        many += len(contours) >= 8
    assert low >= 20 and high >= 20 and many >= 50, (low, high, many)            # unclamped edges are normal, not a corner case


def test_stored_values_are_summed_not_counted():
    plane = np.zeros((120, 40), np.uint8)
    plane[10:30, 5:35] = 1
    plane[60:80, 5:35] = 200
    other = (plane != 0).astype(np.uint8)
    assert order_ref.band_edges(plane) != order_ref.band_edges(other)
    check_against_ref(plane, [order_ref._rect(5, 10, 34, 29), order_ref._rect(5, 60, 34, 79)])


def test_moments_are_the_exact_sums_while_prefixes_stay_small():
    rng = np.random.default_rng(11)
    contours = [order_ref.random_contour(rng, 3000, 2000) for _ in range(200)]
    moments, centroids, serial = _capi.host_contour_moments(contours)
    for k, c in enumerate(contours):
        (s00, s10, s01), small = order_ref.exact_sums(c)
        assert small and serial[k] == 0
        sign = 1 if s00 > 0 else -1
        want = (Fraction(s00 * sign, 2), Fraction(s10 * sign, 6), Fraction(s01 * sign, 6)) if s00 else (0, 0, 0)
        ref = order_ref.moments(c)
        assert (bits(moments[k]) == bits([ref["m00"], ref["m10"], ref["m01"]])).all()
        assert Fraction(float(moments[k, 0])) == want[0]                         # a00 / 2 is exact
        for got, exact in zip(moments[k, 1:], want[1:]):                         # one multiply by the rounded 1 / 6: two roundings at the most
            assert abs(Fraction(float(got)) - exact) <= abs(exact) * Fraction(1, 2 ** 51)
        assert (bits(centroids[k]) == bits(order_ref.centroid(c))).all()


def lap_square(laps):
    return np.array([[32767, 0], [32767, 32767], [0, 32767], [0, 0]] * laps, np.int64)


def test_square_walked_300_times_leaves_the_exact_range():
    square = lap_square(300)
    (s00, s10, s01), small = order_ref.exact_sums(square)
    assert not small and max(abs(s10), abs(s01)) >= 2 ** 53
    moments, centroids, serial = _capi.host_contour_moments([square, lap_square(1)])
    assert serial.tolist() == [1, 0]
    ref = order_ref.moments(square)
    assert (bits(moments[0]) == bits([ref["m00"], ref["m10"], ref["m01"]])).all()
    assert (bits(centroids[0]) == bits(order_ref.centroid(square))).all()
    a10 = order_ref.contour_sums(square)[1]
    assert a10 != float(s10) and Fraction(a10) != s10                           # the float64 serial sum is NOT the exact sum here


def test_orientation_and_degenerate_contours():
    ccw = order_ref._rect(10, 20, 50, 90)
    cw = order_ref._rect(10, 20, 50, 90, clockwise=True)
    closed = np.concatenate([ccw, ccw[:1]])                                      # the reference's rings repeat the first point
    degenerate = [np.array([[7, 9]]), np.array([[7, 9], [30, 9]]), np.array([[1, 1], [5, 5], [9, 9]]), np.zeros((0, 2), np.int64)]
    moments, centroids, serial = _capi.host_contour_moments([ccw, cw, closed] + degenerate)
    assert (bits(moments[0]) == bits(moments[1])).all() and (bits(moments[0]) == bits(moments[2])).all()
    assert moments[0, 0] == 40 * 70 and centroids[0].tolist() == [30.0, 55.0] and centroids[1].tolist() == [30.0, 55.0]
    assert (bits(moments[3:]) == 0).all() and (bits(centroids[3:]) == 0).all()   # all zero, cx = cy = +0.0
    assert serial.tolist() == [0] * 7
    for c in [ccw, cw, closed] + degenerate[:3]:
        assert (bits(_capi.host_contour_moments([c])[1][0]) == bits(order_ref.centroid(c))).all()


def test_cx_ties_are_broken_by_region_index():
    plane = np.zeros((200, 100), np.uint8)
    plane[20:60, 5:95] = 1
    plane[120:160, 5:95] = 1
    a, b = order_ref._rect(10, 25, 50, 55), order_ref._rect(20, 30, 40, 50)      # the same centroid
    c, low = order_ref._rect(10, 22, 50, 58), order_ref._rect(5, 125, 30, 155)
    contours = [low, a, b, c, np.array([[3, 3]]), np.array([[4, 4]])]            # two degenerate ones: cx = cy = 0
    rec = check_against_ref(plane, contours)
    assert rec["centroids"][1].tolist() == rec["centroids"][2].tolist() == rec["centroids"][3].tolist()
    assert rec["sorted_index"].tolist() == [4, 5, 1, 2, 3, 0]
    order_of_texts, id_of_texts = stages.order_and_id_of_texts(contours, *stages.order_of_regions(plane, contours)[::-1])
    assert order_of_texts == [5, 2, 3, 4, 0, 1] and id_of_texts == ["r0", "r1", "r2", "r3", "r4", "r5"]


def test_a_region_in_no_band_is_left_out_as_in_the_reference():
    plane = np.zeros((50, 30), np.uint8)
    plane[10:40, 2:28] = 1
    contours = [order_ref._rect(2, 10, 27, 39), order_ref._rect(2, 500, 27, 560)]        # the second lies below the plane
    want_sorted, matrix, _, bands = order_ref.order_of_regions(plane, contours)
    assert bands[1] == -1 and want_sorted == [0]
    rec = check_against_ref(plane, contours)
    assert rec["order"].tolist() == [0, -1] and rec["sorted_index"].tolist() == [0, 1]
    with pytest.raises(IndexError):
        order_ref.order_and_id_of_texts(contours, matrix, want_sorted)
    with pytest.raises(IndexError):
        stages.order_and_id_of_texts(contours, *stages.order_of_regions(plane, contours)[::-1])


def test_no_regions():
    plane = np.zeros((30, 7), np.uint8)
    plane[5:9] = 3
    rec = check_against_ref(plane, [])
    assert rec["sorted_index"].shape == (0,) and rec["edges"][0] == 0 and rec["edges"][-1] == 30
    assert stages.order_and_id_of_texts([], *stages.order_of_regions(plane, [])[::-1]) == ([], [])
    moments, centroids, serial = _capi.host_contour_moments([])
    assert moments.shape == (0, 3) and centroids.shape == (0, 2) and serial.shape == (0,)
    check_against_ref(np.zeros((1, 1), np.uint8), [np.array([[0, 0]])])          # the smallest plane


def test_argument_errors():
    lib = _capi.load_library()
    w = _capi.order_weights()
    assert w.shape == (33,) and (bits(w) == bits(_capi.gaussian_weights(8))).all()
    sums, edges, ne = np.zeros(10, np.int32), np.zeros(47, np.int32), _capi.C.c_int(0)
    pts, off = np.zeros((4, 2), np.int32), np.array([0, 4], np.int64)
    out = [np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros((1, 2), np.float64)]
    ptr = _capi._ptr

    def call(sums_=sums, H=10, w_=w, off_=off, cap=47, n=1):
        return lib.sbbseg_region_order_host(ptr(sums_), H, ptr(w_), ptr(pts), ptr(off_), n, *[ptr(a) for a in out], ptr(edges), cap, _capi.C.byref(ne))
    assert call() == 0 and ne.value >= 2
    assert call(cap=46) != 0 and b"room for 46 edges" in lib.sbbseg_last_error()
    assert call(H=0) != 0 and call(sums_=None) != 0 and call(w_=None) != 0 and call(n=-1) != 0
    assert call(off_=np.array([1, 4], np.int64)) != 0 and b"start at 0" in lib.sbbseg_last_error()
    assert call(off_=np.array([0, -1], np.int64)) != 0
    m, c = np.zeros((1, 3)), np.zeros((1, 2))
    assert lib.sbbseg_contour_moments_host(ptr(pts), ptr(off), 1, ptr(m), ptr(c), None) == 0
    assert lib.sbbseg_contour_moments_host(ptr(pts), ptr(off), 1, None, ptr(c), None) != 0
    assert lib.sbbseg_contour_moments_host(None, ptr(off), 1, ptr(m), ptr(c), None) != 0
    assert lib.sbbseg_contour_moments_host(None, None, 0, None, None, None) == 0
    assert lib.sbbseg_abi_version() == 5
