"""The two device rotations against the numpy oracles on adversarial crops (-m gpu), bit for bit: the deskew sweep for all boxes
(``region_crop_erode_kernel``, ``region_deskew_profile_kernel``) and the one-region kernel it is modelled on (``deskew_profile_kernel``)
against oracle/deskew.py at EVERY angle of tests/rotation_cases.py; the deskewed line mask (``region_line_morph_kernel``,
``region_line_warp_kernel``, ``region_line_cols_kernel``) against tests/lines_ref.py on every crop x shape, bytes other than 0 / 1
included; the pooled calls on three planes with a run of tiny boxes that makes one wave of the crop kernel span many regions.  What
keeps these cases from being vacuous is asserted without a GPU in tests/test_rotation_cases_cpu.py.  Every case runs once."""
import ctypes as C
import time

import numpy as np
import pytest

from sbb_textline_detection_amd import _capi

import lines_ref
import rotation_cases as rc
import slopes_ref
from test_gpu_planes import Packed, _pooled

pytestmark = pytest.mark.gpu
T0 = time.time()


@pytest.fixture(scope="module")
def model():
    from sbb_textline_detection_amd.model import SegModel
    from tools.synth_model import calibrated_model
    cfg, w = calibrated_model(2, 224, 224, seed=0)
    m = SegModel(cfg, w, device=0, max_batch=4)                  # any finalized handle: these calls do not touch the network
    yield m
    m.release()
    print(f"[test_gpu_rotations] module wall time {time.time() - T0:.1f} s")


def _matrix(shape, angle):
    S = rc.side_of(*shape)
    return _capi.rotation_matrix(S // 2, S // 2, angle)


def _report(test, cases, boxes, angles, pixels, mismatches):
    print(f"[test_gpu_rotations] {test}: cases {cases}, boxes {boxes}, angles {angles}, pixels compared {pixels}, mismatches {mismatches}")


def _first_difference(got, want):
    a, y = np.argwhere(got != want)[0]
    return int(a), int(y), int(got[a, y]), int(want[a, y])


def _compare_profiles(got, c, k, angles=rc.ANGLES):
    """got: int32 [n_angles][S] of one case.  Returns the number of profile rows compared; reports box, angle, first row, both counts."""
    S = rc.side_of(*c.shape)
    assert got.dtype == np.int32 and got.shape == (len(angles), S) == (len(angles), _capi.deskew_side(*c.shape)), c
    want = np.stack([rc.sweep_reference(c, k, a, _matrix(c.shape, a)) for a in angles])
    if not np.array_equal(got, want):
        a, y, g, w = _first_difference(got, want)
        raise AssertionError(f"{c}, erode {k}: angle {angles[a]!r}, row {y}: device {g}, oracle {w} ({int((got != want).sum())} rows differ)")
    return got.size


@pytest.mark.parametrize("k", [0, 2])
@pytest.mark.parametrize("plane", [0, 1, 2])
def test_sweep_equals_the_oracle_at_every_angle(model, plane, k):
    """(a) every sweep case of one plane in one call, every angle of the list."""
    cases = rc.sweep_cases(plane)
    got = model.ctx.region_deskew_profiles(rc.planes()[plane], [c.box for c in cases], rc.ANGLES, erode_iterations=k)
    assert len(got) == len(cases)
    rows = sum(_compare_profiles(g, c, k) for g, c in zip(got, cases))
    _report(f"sweep[plane {plane}, erode {k}]", len(cases) * len(rc.ANGLES), len(cases), len(rc.ANGLES),
            sum(rc.side_of(*c.shape) ** 2 for c in cases) * len(rc.ANGLES), 0)
    assert rows == sum(rc.side_of(*c.shape) for c in cases) * len(rc.ANGLES)


def test_one_region_path_equals_the_oracle(model):
    """(b) a box per shape class through the older kernel, the same oracle values; and two maps that are no rotations.  The x scale
    decides by round-half-even: row 0 counts the single-column crop at x = 29 only through table index 31 (rotation_cases.x_scale_matrix)."""
    ctx = model.ctx
    picks = rc.one_per_shape_class()
    assert {name for name, shapes in rc.SHAPE_CLASSES.items() for c in picks if c.shape in shapes} == set(rc.SHAPE_CLASSES)
    pixels = 0
    for c in picks:
        for k in (0, 2):
            eroded = lines_ref.eroded_crop(rc.crop_of(c), k)
            _compare_profiles(ctx.deskew_profiles(eroded, rc.ANGLES), c, k)
            pixels += rc.side_of(*c.shape) ** 2 * len(rc.ANGLES)
    maps = [rc.shear_matrix(), rc.x_scale_matrix()]
    other = [rc.find("bytes", (43, 17)), rc.find("col", (43, 17)), rc.find("ones", (5, 6)), rc.find("wrap", (37, 90))]
    for c in other:
        crop = rc.crop_of(c)
        got = ctx.deskew_profiles(crop, matrices=np.stack(maps))
        want = np.stack([rc.sweep_profile(crop, M) for M in maps])
        assert want.sum(axis=1).all(), c
        if not np.array_equal(got, want):
            a, y, g, w = _first_difference(got, want)
            raise AssertionError(f"{c}: map {('shear', 'x scale')[a]}, row {y}: device {g}, oracle {w}")
        pixels += rc.side_of(*c.shape) ** 2 * len(maps)
    _report("one region", len(picks) * 2 * len(rc.ANGLES) + len(other) * len(maps), len(picks) * 2 + len(other), len(rc.ANGLES), pixels, 0)


def test_crop_erosion_alone(model):
    """(e) erode_iterations 0 .. 3 at angle 0 on the all-255 and random-byte crops up to 5 x 6: from 2 iterations on the window is wider
    than the crop and clipped on both sides at once.  At angle 0 the profile is the row sums of (eroded crop != 0) on the square."""
    ctx = model.ctx
    pixels = 0
    for plane in range(3):
        cases = [c for c in rc.line_cases(plane) if c.kind in ("full", "bytes") and c.shape in rc.TINY + rc.FIRST_CLIPPED]
        assert cases
        for k in range(4):
            got = ctx.region_deskew_profiles(rc.planes()[plane], [c.box for c in cases], [0.0], erode_iterations=k)
            for g, c in zip(got, cases):
                _compare_profiles(g, c, k, angles=[0.0])
                pixels += rc.side_of(*c.shape) ** 2
    _report("crop erosion", 12 * 4, 12 * 4, 1, pixels, 0)


_SLOPES = {}


def _oracle_slope(crop):
    """slopes_ref.oracle_slopes of one crop.  Its first statement is the two erosions, so crops with the same eroded bytes share it."""
    key = (crop.shape, slopes_ref.erode2(crop).tobytes())
    if key not in _SLOPES:
        _SLOPES[key] = slopes_ref.oracle_slopes(crop, [[0, 0, crop.shape[1], crop.shape[0]]])[0]
    return _SLOPES[key]


def test_pooled_calls_with_a_run_of_tiny_boxes(model):
    """(c) the three planes back to back in one allocation; 341 boxes, 210 consecutive ones of 1 x 1 .. 3 x 3 on alternating planes."""
    ctx = model.ctx
    host = rc.planes()
    boxes, box_plane = rc.pooled_case()
    crops = [slopes_ref.crop_of(host[k], b) for b, k in zip(boxes, box_plane)]
    packed = Packed(ctx, host)
    try:
        slopes, masks, _records = _pooled(ctx, packed.planes, boxes, box_plane, erode=2)
        upright = [a for a in rc.ANGLES if abs(a) <= 90]         # (the call also runs the line splitter, whose slopes are cleaned ones)
        given = [upright[r % len(upright)] for r in range(len(boxes))]
        _s, masks0, _r = _pooled(ctx, packed.planes, boxes, box_plane, erode=0, slopes=given)
    finally:
        packed.free()
    want = [_oracle_slope(c) for c in crops]
    assert slopes == want, [(r, boxes[r], box_plane[r], slopes[r], want[r]) for r in range(len(boxes)) if slopes[r] != want[r]][:6]
    assert any(s != 0 for s in slopes)
    pixels = 0
    for r, crop in enumerate(crops):
        for got, slope, it in ((masks[r], slopes[r], 2), (masks0[r], given[r], 0)):
            ref = lines_ref.line_mask(crop, slope, it)
            for g, w, name in zip(got, ref, ("mask", "rows", "cols")):
                assert g.shape == w.shape and np.array_equal(g, w), (r, boxes[r], box_plane[r], slope, it, name)
            pixels += crop.size
    assert sum(1 for m in masks0 if m[0].any()) >= 100 and sum(1 for m in masks0 if not m[0].all()) >= 100
    _report("pooled", 2 * len(boxes), len(boxes), len(set(given)), pixels, 0)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _raw(ctx, plane, boxes, slopes, erode, masks=True, dev=False):
    """The C call itself (tests/test_gpu_lines.py's, with the erode iterations as an argument)."""
    b = np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
    s = np.ascontiguousarray(slopes, np.float64)
    n = b.shape[0]
    m = np.full(int((b[:, 2].astype(np.int64) * b[:, 3]).sum()), 7, np.uint8) if masks else None
    rows, cols = np.full(int(b[:, 3].sum()), -1, np.int32), np.full(int(b[:, 2].sum()), -1, np.int32)
    mo, ro, co = (np.full(n + 1, -1, np.int64) for _ in range(3))
    if dev:
        src, fn = C.c_void_p(ctx.stage(plane)), ctx.lib.sbbseg_region_line_masks_dev
    else:
        src, fn = _p(plane), ctx.lib.sbbseg_region_line_masks
    _capi.check(fn(ctx.h, src, plane.shape[0], plane.shape[1], _p(b), n, int(erode), _p(s), _p(m), _p(rows), _p(cols), _p(mo), _p(ro), _p(co)),
                "sbbseg_region_line_masks")
    return m, rows, cols, mo, ro, co


@pytest.mark.parametrize("kind", rc.KINDS)
def test_line_masks_equal_the_restatement(model, kind):
    """(d) every shape of one kind of crop at every slope of the list, erode iterations 0 and 2: mask, rows, columns and the three
    offset arrays from both entry points; rows and columns are the sums of the mask; masks = NULL gives the same projections."""
    ctx = model.ctx
    n_boxes = pixels = 0
    for k, plane in enumerate(rc.planes()):
        cases = [c for c in rc.line_cases(k) if c.kind == kind]
        boxes = [c.box for c in cases for _s in rc.line_slopes(c.shape)]
        slopes = [s for c in cases for s in rc.line_slopes(c.shape)]
        w, h = np.array([b[2] for b in boxes], np.int64), np.array([b[3] for b in boxes], np.int64)
        for it in (0, 2):
            want = [ref for c in cases for ref in rc.line_masks_of(rc.crop_of(c), rc.line_slopes(c.shape), it)]
            m, rows, cols, mo, ro, co = _raw(ctx, plane, boxes, slopes, it)
            assert np.array_equal(mo, np.concatenate([[0], np.cumsum(w * h)])) and np.array_equal(ro, np.concatenate([[0], np.cumsum(h)]))
            assert np.array_equal(co, np.concatenate([[0], np.cumsum(w)]))
            for r, box in enumerate(boxes):
                dst = m[mo[r]:mo[r + 1]].reshape(box[3], box[2])
                tag = (kind, box, slopes[r], it)
                assert np.array_equal(dst, want[r][0]), (tag, "mask", int((dst != want[r][0]).sum()), np.argwhere(dst != want[r][0])[:3].tolist())
                assert np.array_equal(rows[ro[r]:ro[r + 1]], want[r][1]) and np.array_equal(cols[co[r]:co[r + 1]], want[r][2]), tag
                assert np.array_equal(rows[ro[r]:ro[r + 1]], dst.sum(axis=1)) and np.array_equal(cols[co[r]:co[r + 1]], dst.sum(axis=0)), tag
            for a, b in zip((m, rows, cols, mo, ro, co), _raw(ctx, plane, boxes, slopes, it, dev=True)):
                assert np.array_equal(a, b), (kind, k, it, "the _dev entry point")
            none, rows_only, cols_only, _mo, ro2, co2 = _raw(ctx, plane, boxes, slopes, it, masks=False)
            assert none is None and np.array_equal(rows_only, rows) and np.array_equal(cols_only, cols)
            assert np.array_equal(ro2, ro) and np.array_equal(co2, co)
            n_boxes += len(boxes)
            pixels += int((w * h).sum())
    _report(f"line masks[{kind}]", n_boxes, n_boxes, len(rc.ANGLES), pixels, 0)
