"""The reading order of text regions on the device (-m gpu; csrc/order.hip) against the library's serial host twins, bit for bit.  The host
twins run the same order.h and tests/test_order_cpu.py holds them to scipy / numpy, so a difference here is the device's: the wide loads
of the row sums, the block scan of the edges, the int64 wave scan of the moments and its serial fallback, the tiled ranking."""
import time

import numpy as np
import pytest

import contour_shapes
import order_ref

pytestmark = pytest.mark.gpu
T0 = time.time()


def _model(seed):
    from sbb_textline_detection_amd.model import SegModel
    from tools.synth_model import calibrated_model
    cfg, w = calibrated_model(2, 224, 224, seed=seed)
    return SegModel(cfg, w, device=0, max_batch=4)                # any finalized handle: these calls do not touch the network


@pytest.fixture(scope="module")
def ctx():
    m = _model(0)
    yield m.ctx
    m.release()
    print(f"[test_gpu_order] module wall time {time.time() - T0:.1f} s")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_record(got, want, what):
    for key in ("edges", "band", "sorted_index", "order"):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (what, key)
    assert np.array_equal(bits(got["centroids"]), bits(want["centroids"])), (what, "centroids")


def test_row_sums_of_unaligned_rows(ctx):
    rng = np.random.default_rng(3)
    for W in (1, 3, 17, 67, 260):
        for H in (1, 2, 45, 300, 2100):
            plane = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
            plane[rng.integers(0, H)] = 255                        # a row of the largest value
            got = ctx.debug_row_sums(plane)
            assert got.dtype == np.int32 and np.array_equal(got, plane.sum(axis=1, dtype=np.int64)), (H, W)


def _shape_planes():
    hand = contour_shapes.pack(list(contour_shapes.hand_shapes().values()), 128)
    return {"hand_shapes": hand, "random_masks": contour_shapes.pack(contour_shapes.random_masks(200, seed=0), 300),
            "widths": contour_shapes.widths_plane(), "many_components": contour_shapes.many_components(), "staircase": contour_shapes.staircase(70)}


@pytest.mark.parametrize("name", ["hand_shapes", "random_masks", "widths", "many_components", "staircase"])
def test_moments_of_the_resident_contours(ctx, name):
    from sbb_textline_detection_amd import _capi
    plane = np.ascontiguousarray(_shape_planes()[name], np.uint8)
    boxes, contours = ctx.debug_mask_contours_dev(ctx.stage(plane), plane.shape[0], plane.shape[1])
    assert len(contours) >= 1
    launches = ctx.order_launches()
    moments, centroids, serial = ctx.contour_moments_dev(None, len(contours))
    assert ctx.order_launches() == launches + 1
    want = _capi.host_contour_moments(contours)
    assert np.array_equal(bits(moments), bits(want[0])) and np.array_equal(bits(centroids), bits(want[1]))
    assert not serial.any() and not want[2].any()
    # and the order, with the plane itself as the textline plane: the table is read in place
    rec = ctx.region_order_dev(ctx.stage(plane), plane.shape[0], plane.shape[1], None, len(contours))
    same_record(rec, _capi.host_region_order(plane, contours), name)
    assert sorted(rec["sorted_index"].tolist()) == list(range(len(contours)))
    with pytest.raises(RuntimeError, match="the handle holds"):
        ctx.contour_moments_dev(None, len(contours) + 1)


def test_moments_of_passed_lists_and_the_serial_fallback(ctx):
    from sbb_textline_detection_amd import _capi
    rng = np.random.default_rng(17)
    square = np.array([[32767, 0], [32767, 32767], [0, 32767], [0, 0]] * 300, np.int64)
    ring = lambda k: np.stack([np.rint(500 + 400 * np.cos(np.arange(k) * 2 * np.pi / k)), np.rint(500 + 400 * np.sin(np.arange(k) * 2 * np.pi / k))], 1).astype(np.int64)
    contours = [order_ref.random_contour(rng, 3000, 2000) for _ in range(40)]
    contours += [ring(k) for k in (63, 64, 65, 128, 129, 1000)]    # around the 64-point chunks of the wave scan
    contours += [square, square[:4], np.array([[40000, 5], [40010, 5], [40010, 30]]), np.array([[-3, -4], [10, -4], [10, 9]]),
                 np.array([[7, 9]]), np.array([[7, 9], [30, 9]]), np.zeros((0, 2), np.int64), square[::-1]]
    moments, centroids, serial = ctx.contour_moments_dev(contours)
    want = _capi.host_contour_moments(contours)
    assert np.array_equal(bits(moments), bits(want[0])) and np.array_equal(bits(centroids), bits(want[1]))
    flagged = [46, 48, 53]                                          # the 300-lap square both ways, and the coordinate beyond 32767
    assert np.flatnonzero(serial).tolist() == flagged and np.flatnonzero(want[2]).tolist() == flagged
    ref = order_ref.moments(square)
    assert np.array_equal(bits(moments[46]), bits([ref["m00"], ref["m10"], ref["m01"]]))
    assert ctx.contour_moments_dev([])[0].shape == (0, 3)


@pytest.mark.parametrize("n", [0, 1, 65, 1500])
def test_order_equals_the_host_twin(ctx, n):
    from sbb_textline_detection_amd import _capi
    rng = np.random.default_rng(100 + n)
    H, W = (2100, 67) if n == 1500 else (300, 260)
    plane = order_ref.random_plane(rng, H, W)
    contours = [order_ref.random_contour(rng, H, W) for _ in range(n)]
    launches = ctx.order_launches()
    rec = ctx.region_order(plane, contours)
    assert ctx.order_launches() == launches + (4 if n else 2)
    want = _capi.host_region_order(plane, contours)
    same_record(rec, want, n)
    assert sorted(rec["sorted_index"].tolist()) == list(range(n)) and (rec["band"] >= 0).all()
    if n == 1500:                                                   # ties in cx inside a band: broken by index on both sides
        keys = list(zip(rec["band"].tolist(), rec["centroids"][:, 0].tolist()))
        assert len(set(keys)) < n
    if n == 65:
        ref_sorted, ref_matrix, ref_edges, _ = order_ref.order_of_regions(plane, contours)
        assert rec["sorted_index"].tolist() == ref_sorted and rec["edges"].tolist() == ref_edges
        assert np.array_equal(bits(rec["centroids"]), bits(ref_matrix[:, 2:4]))


def test_plane_of_another_handle_and_argument_errors(ctx):
    from sbb_textline_detection_amd import _capi
    other = _model(1)
    try:
        rng = np.random.default_rng(9)
        plane = order_ref.random_plane(rng, 45, 17)
        contours = [order_ref.random_contour(rng, 45, 17) for _ in range(5)]
        rec = ctx.region_order_dev(other.ctx.stage(plane), 45, 17, contours)
        same_record(rec, _capi.host_region_order(plane, contours), "other handle")
    finally:
        other.release()
    with pytest.raises(RuntimeError, match="bad arguments"):
        ctx.region_order_dev(0, 45, 17, contours)
    edges, ne = np.zeros(4, np.int32), _capi.C.c_int(0)
    rc = ctx.lib.sbbseg_region_order_dev(ctx.h, _capi.C.c_void_p(ctx.stage(plane)), 45, 17, _capi._ptr(_capi.order_weights()), None, None, 0, None, None,
                                         None, None, _capi._ptr(edges), 4, _capi.C.byref(ne))
    assert rc != 0 and b"room for 4 edges" in ctx.lib.sbbseg_last_error()
