"""The device contour tracer (-m gpu; csrc/contours.hip) against the library's host twin and the host mirror.  The host twin runs the
same contour_walk.h and tests/test_contours_cpu.py holds it to tests/contours_ref.py, so a difference here is the device's: the bit map
in LDS, the ballot packing, the global form, the staged flush, the two-launch packing.  All tables are compared bit for bit."""
import time

import numpy as np
import pytest

import cc_planes
import contour_shapes

pytestmark = pytest.mark.gpu
T0 = time.time()
REGION = cc_planes.region_families()


@pytest.fixture(scope="module")
def ctx():
    from sbb_textline_detection_amd.model import SegModel
    from tools.synth_model import calibrated_model
    cfg, w = calibrated_model(2, 224, 224, seed=0)
    m = SegModel(cfg, w, device=0, max_batch=4)                  # any finalized handle: these calls do not touch the network
    yield m.ctx
    m.release()
    print(f"[test_gpu_contours] module wall time {time.time() - T0:.1f} s")


def _raw_planes():
    hand = contour_shapes.pack(list(contour_shapes.hand_shapes().values()), 128)
    assert hand.shape[0] <= 96
    hand = np.pad(hand, ((0, 96 - hand.shape[0]), (0, 0)))
    return {"hand_shapes": hand, "random_masks": contour_shapes.pack(contour_shapes.random_masks(200, seed=0), 300),
            "widths": contour_shapes.widths_plane(), "many_components": contour_shapes.many_components(),
            "staircase": contour_shapes.staircase(70)}


RAW = _raw_planes()
_HOST = {}


def _host_tables(name):
    from sbb_textline_detection_amd import _capi
    if name not in _HOST:
        _HOST[name] = _capi.mask_contours_host_tables(RAW[name])
    return _HOST[name]


def _device_tables(ctx, plane):
    import ctypes as C
    n, npts = C.c_int(0), C.c_int64(0)
    from sbb_textline_detection_amd._capi import check
    check(ctx.lib.sbbseg_debug_mask_contours_dev(ctx.h, C.c_void_p(ctx.stage(plane)), plane.shape[0], plane.shape[1], C.byref(n), C.byref(npts)))
    return ctx.contour_tables(n.value, npts.value)


def _same_tables(got, want, what):
    for g, w, table in zip(got, want, ("boxes", "area2", "point_off", "points")):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, table)


@pytest.mark.parametrize("lds_limit", [64 * 1024, 64])
@pytest.mark.parametrize("name", list(RAW))
def test_raw_masks_equal_the_host_twin(ctx, name, lds_limit):
    """sbbseg_debug_mask_contours_dev == sbbseg_mask_contours_host on every table; with the LDS limit at 64 bytes everything but the
    smallest specks takes the global form, and the tables must not change."""
    want = _host_tables(name)
    if name == "random_masks":
        assert RAW[name].shape == (84, 300) and len(want[0]) > 400          # 200 masks a pixel apart
    if name == "many_components":
        assert len(want[0]) > 1024                                 # more components than a tracer launch has blocks
    if name == "staircase":
        assert len(want[0]) == 1 and want[2][-1] > 128             # one contour, more than two full stages of kept points
    ctx.set_contour_lds_limit(lds_limit)
    try:
        _same_tables(_device_tables(ctx, RAW[name]), want, (name, lds_limit))
    finally:
        ctx.set_contour_lds_limit(64 * 1024)


def test_frame_beyond_the_lds_limit_equals_the_host_mirror(ctx):
    """A hollow 1024 x 640 frame: its bit map (33 words x 642 rows) is beyond kContourLdsBytes with no switch set, it survives OPEN and
    CLOSE, and its outer contour is the rectangle."""
    from sbb_textline_detection_amd import stages
    plane = contour_shapes.frame_plane()
    want = stages.host_text_region_contours(plane)
    assert want[0] == [[8, 8, 1024, 640]] and want[1][0].tolist() == [[8, 8], [8, 647], [1031, 647], [1031, 8]]
    boxes, contours = ctx.text_region_contours(plane)
    assert boxes == want[0] and len(contours) == 1 and np.array_equal(contours[0], want[1][0])
    assert ctx.contour_tables(1, 4)[1].tolist() == [2 * 1023 * 639]


_MIRROR = {}


def _mirror(name, lo, hi):
    from sbb_textline_detection_amd import stages
    key = (name, lo, hi)
    if key not in _MIRROR:
        _MIRROR[key] = stages.host_text_region_contours(cc_planes._region_plane(name), 1, lo, hi)
    return _MIRROR[key]


@pytest.mark.parametrize("family", list(REGION))
def test_region_planes_equal_the_host_mirror_and_the_boxes_call(ctx, family):
    """sbbseg_text_region_contours[_dev] on every cc_planes region plane at the three windows of tests/test_gpu_components.py: boxes ==
    sbbseg_text_region_boxes_dev, contours == the host mirror, no host tracing, and a second call gives identical tables."""
    longest = 0
    for name, plane in REGION[family].items():
        for lo, hi in ((0.0, 1.0), (1e-5, 1.0), cc_planes.interior_window(name)):
            want_boxes, want_contours = _mirror(name, lo, hi)
            H, W = plane.shape
            boxes_call = ctx.text_region_boxes_dev(ctx.stage(plane), H, W, 1, lo, hi)
            before = ctx.host_contour_calls()
            boxes, contours = ctx.text_region_contours(plane, 1, lo, hi)
            first = ctx.contour_tables(len(boxes), sum(len(c) for c in contours))
            assert boxes == boxes_call == want_boxes == cc_planes.oracle_region_boxes(name, lo, hi), (name, lo, hi)
            assert len(contours) == len(want_contours) and all(np.array_equal(a, b) for a, b in zip(contours, want_contours)), (name, lo, hi)
            boxes_dev, contours_dev = ctx.text_region_contours_dev(ctx.stage(plane), H, W, 1, lo, hi)
            assert ctx.host_contour_calls() == before, (name, lo, hi)
            _same_tables(ctx.contour_tables(len(boxes), sum(len(c) for c in contours)), first, (name, lo, hi, "second call"))
            assert boxes_dev == boxes and all(np.array_equal(a, b) for a, b in zip(contours_dev, contours))
            longest = max([longest] + [len(c) for c in contours])
    print(f"[contours:{family}] longest contour {longest} points")


def test_three_channels_and_the_fixture(ctx):
    """sbbseg_text_region_contours == tests/golden/contours_golden.npz: what the reference's own get_text_region_contours_and_boxes
    returned (boxes, list order, closed rings, dtype)."""
    from sbb_textline_detection_amd import stages
    kept = 0
    for regions, boxes, rings in contour_shapes.golden_cases():
        got_boxes, contours = ctx.text_region_contours(regions)
        got = stages.closed_rings(contours)
        assert got_boxes == boxes
        assert len(got) == len(rings) and all(g.dtype == np.uint and g.shape == r.shape and np.array_equal(g, r) for g, r in zip(got, rings))
        kept += len(rings)
    assert kept == 20


def test_read_with_too_little_room_writes_nothing(ctx):
    plane = RAW["hand_shapes"]
    want = _host_tables("hand_shapes")
    got = _device_tables(ctx, plane)
    n, npts = len(want[0]), len(want[3])
    from sbb_textline_detection_amd._capi import _ptr
    for cap_n, cap_p in ((n - 1, npts), (n, npts - 1), (0, 0)):
        boxes, area2 = np.full((n, 4), -7, np.int32), np.full(n, -7, np.int64)
        off, pts = np.full(n + 1, -7, np.int64), np.full((npts, 2), -7, np.int32)
        rc = ctx.lib.sbbseg_text_region_contours_read(ctx.h, _ptr(boxes), _ptr(area2), _ptr(off), cap_n, _ptr(pts), cap_p)
        assert rc != 0 and b"room for" in ctx.lib.sbbseg_last_error(), (cap_n, cap_p)
        assert (boxes == -7).all() and (area2 == -7).all() and (off == -7).all() and (pts == -7).all(), (cap_n, cap_p)
    _same_tables(ctx.contour_tables(n, npts), want, "after the failed reads")
    _same_tables(got, want, "before them")
    larger = ctx.contour_tables(n + 3, npts + 5)                    # more room than needed is fine: the rest stays as it was
    assert np.array_equal(larger[0][:n], want[0]) and np.array_equal(larger[3][:npts], want[3]) and (larger[3][npts:] == 0).all()


def test_an_empty_plane_gives_empty_tables(ctx):
    zero = np.zeros((40, 50), np.uint8)
    assert ctx.text_region_contours(zero) == ([], [])
    boxes, area2, off, pts = _device_tables(ctx, zero)
    assert len(boxes) == 0 and len(area2) == 0 and off.tolist() == [0] and len(pts) == 0
