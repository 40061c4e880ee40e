"""The deskewed text-line masks without a GPU: the exported symbols, the fixed-point bicubic table, the host twin
(``sbbseg_region_line_masks_host``: the statements of csrc/line_mask.h on the CPU) against the numpy restatement (tests/lines_ref.py)
and against the fixture recorded from the reference's control flow, the shortcut morphology against the literal one, error statuses."""
import ctypes as C

import numpy as np
import pytest

from sbb_textline_detection_amd import _capi, stages

import lines_ref
import slopes_ref


def _same(got, want, what):
    for g, w, name in zip(got, want, ("dst", "rows", "cols")):
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, int((np.asarray(g, np.int64) != w).sum()))


def test_symbols_are_exported_and_the_abi_version_stays():
    lib = _capi.load_library()
    for name in ("sbbseg_region_line_masks_dev", "sbbseg_region_line_masks", "sbbseg_region_line_masks_host"):
        assert hasattr(lib, name), name
        assert name in _capi.EXPORTS
    assert lib.sbbseg_abi_version() == 5


def test_integer_table_sums_and_equals_the_restatement():
    tab = _capi.region_line_table()
    assert tab.dtype == np.int16 and tab.shape == (32, 32, 4, 4)
    assert (tab.astype(np.int64).sum(axis=(2, 3)) == 32768).all()
    assert np.array_equal(tab, lines_ref.integer_table())
    # the correction is exercised: some block's rounded entries do not sum to 32768 before it
    from oracle import deskew as dk
    t = dk.cubic_table()
    raw = np.rint((t[:, None, :, None] * t[None, :, None, :]).astype(np.float32) * np.float32(32768)).clip(-32768, 32767)
    assert (raw.sum(axis=(2, 3)) != 32768).any()


def test_host_twin_equals_the_restatement_on_the_fixture_crops():
    golden = lines_ref.load_golden()
    for k, ((_r, textlines, boxes, ref_slopes), (slopes, _m, _v)) in enumerate(zip(slopes_ref.load_pages(), golden)):
        assert slopes == ref_slopes, k                           # both fixtures record the same reference slopes
        for box, slope in zip(boxes, slopes):
            crop = slopes_ref.crop_of(textlines, box)
            _same(_capi.host_region_line_mask(crop, slope), lines_ref.line_mask(crop, slope), (k, box, slope))


def test_host_twin_equals_the_committed_fixture():
    golden = lines_ref.load_golden()
    non_empty = vertical = 0
    for k, ((_r, textlines, boxes, _s), (slopes, masks, routed)) in enumerate(zip(slopes_ref.load_pages(), golden)):
        assert len(masks) == len(boxes) == len(routed)
        for box, slope, want, v in zip(boxes, slopes, masks, routed):
            dst, rows, cols = _capi.host_region_line_mask(slopes_ref.crop_of(textlines, box), slope)
            assert np.array_equal(dst, want), (k, box, slope)
            assert np.array_equal(rows, want.sum(axis=1)) and np.array_equal(cols, want.sum(axis=0))
            assert v == int(abs(slope) > 45)                     # main.py:1514
            non_empty += bool(want.any())
            vertical += v
    assert non_empty >= 4 and vertical >= 1


def test_host_twin_equals_the_restatement_on_random_boxes_and_slopes():
    textlines, boxes = slopes_ref.random_page()
    for special in ([10, 10, 1, 1], [0, 0, 5, 5], [0, 0, textlines.shape[1], textlines.shape[0]]):
        assert special in boxes
    rng = np.random.RandomState(7)
    for r, box in enumerate(boxes):
        crop = slopes_ref.crop_of(textlines, box)
        if box[2] * box[3] == textlines.size:
            todo = [2.0, -70]                                    # (the whole plane: two slopes; the restatement takes seconds each)
        elif box[2] * box[3] <= 64:
            todo = lines_ref.SLOPES                              # the 1 x 1 and 5 x 5 boxes: all of them
        else:
            todo = [lines_ref.SLOPES[(r + j) % len(lines_ref.SLOPES)] for j in range(3)] + [float(rng.uniform(-90, 90))]
        for slope in todo:
            _same(_capi.host_region_line_mask(crop, slope), lines_ref.line_mask(crop, slope), (box, slope))
    # every listed slope on one mid-sized box with text in it, with and without the mask, and erode_iterations 0 and 1
    box = boxes[7]
    crop = slopes_ref.crop_of(textlines, box)
    assert lines_ref.eroded_crop(crop).any()
    for slope in lines_ref.SLOPES:
        want = lines_ref.line_mask(crop, slope)
        _same(_capi.host_region_line_mask(crop, slope), want, (box, slope))
        none, rows, cols = _capi.host_region_line_mask(crop, slope, mask=False)
        assert none is None and np.array_equal(rows, want[1]) and np.array_equal(cols, want[2])
    for it in (0, 1):
        _same(_capi.host_region_line_mask(crop, -9.5, erode_iterations=it), lines_ref.line_mask(crop, -9.5, erode_iterations=it), it)


def test_shortcut_morphology_equals_the_literal_one():
    rng = np.random.RandomState(3)
    textlines, boxes = slopes_ref.random_page()
    cases = [(rng.rand(h, w) < p).astype(np.uint8) * 255 for h, w, p in ((1, 1, 0.5), (3, 40, 0.7), (40, 3, 0.7), (5, 5, 0.9), (37, 53, 0.8),
                                                                        (64, 64, 0.97), (9, 9, 1.0))]
    cases += [lines_ref.eroded_crop(slopes_ref.crop_of(textlines, b)) * np.uint8(255) for b in boxes[1:10]]
    cases.append(slopes_ref.crop_of(textlines, boxes[3]) * np.uint8(255))      # not eroded: ragged edges
    changed = 0
    for m in cases:
        want = lines_ref.open_close(m)
        assert np.array_equal(lines_ref.open_close_shortcut(m), want), m.shape
        changed += not np.array_equal(want, m)
    assert changed >= 3
    # and the library's host twin runs the shortcut: slope 0 is the identity warp, so dst is the opened / closed crop itself
    for m in cases[:8]:
        dst = _capi.host_region_line_mask(m // 255, 0.0, erode_iterations=0)[0]
        assert np.array_equal(dst, lines_ref.open_close(m) // 255), m.shape


def test_bad_arguments_are_error_statuses():
    lib = _capi.load_library()
    crop = np.ones((6, 7), np.uint8)
    rows, cols = np.zeros(6, np.int32), np.zeros(7, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                   # noqa: E731
    for h, w in ((0, 7), (6, 0), (-1, 7), (6, -3)):
        assert lib.sbbseg_region_line_masks_host(p(crop), h, w, 2, 1.0, None, p(rows), p(cols)) != 0
        assert "crop" in lib.sbbseg_last_error().decode()
    assert lib.sbbseg_region_line_masks_host(None, 6, 7, 2, 1.0, None, p(rows), p(cols)) != 0
    assert lib.sbbseg_region_line_masks_host(p(crop), 6, 7, 2, 1.0, None, None, p(cols)) != 0
    assert lib.sbbseg_region_line_masks_host(p(crop), 6, 7, -1, 1.0, None, p(rows), p(cols)) != 0
    # the batched device entry point checks the boxes before it needs a handle: status + a message that names the box, never an abort
    # (the host-plane entry point stages the plane first, so without a handle it reports the handle)
    off = [np.zeros(3, np.int64) for _ in range(3)]
    slopes = np.zeros(2, np.float64)
    for bad, word in (([0, 0, 0, 5], "box 1"), ([0, 0, 5, 0], "box 1"), ([-1, 0, 5, 5], "box 1"), ([36, 0, 5, 5], "box 1"), ([0, 27, 5, 5], "box 1")):
        boxes = np.array([[2, 2, 8, 8], bad], np.int32)
        for fn in (lib.sbbseg_region_line_masks_dev, lib.sbbseg_region_line_masks):
            assert fn(None, None, 30, 40, p(boxes), 2, 2, p(slopes), None, p(rows), p(cols), p(off[0]), p(off[1]), p(off[2])) != 0
            assert fn is lib.sbbseg_region_line_masks or word in lib.sbbseg_last_error().decode()
    # good boxes, no handle: still a status; no boxes: success without a handle, offsets all zero
    boxes = np.array([[2, 2, 8, 8], [0, 0, 40, 30]], np.int32)
    assert lib.sbbseg_region_line_masks_dev(None, None, 30, 40, p(boxes), 2, 2, p(slopes), None, p(rows), p(cols), p(off[0]), p(off[1]), p(off[2])) != 0
    off[0][:] = 9
    assert lib.sbbseg_region_line_masks_dev(None, None, 30, 40, None, 0, 2, None, None, None, None, p(off[0]), p(off[1]), p(off[2])) == 0
    assert off[0][0] == 0


def test_stage_functions_need_a_handle():
    plane = np.zeros((30, 40), np.uint8)
    with pytest.raises(RuntimeError, match="library handle"):
        stages.get_line_masks(plane, [[2, 2, 8, 8]], [0.0])
    with pytest.raises(RuntimeError, match="library handle"):
        stages.get_slopes_and_line_masks(plane, [[2, 2, 8, 8]])
    assert hasattr(stages.InferenceStages, "get_line_masks") and hasattr(stages.InferenceStages, "run_with_lines")
