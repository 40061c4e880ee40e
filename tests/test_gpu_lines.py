"""The deskewed text-line masks on the device (-m gpu), through the C ABI: masks, row sums, column sums and offsets of
``sbbseg_region_line_masks(_dev)`` against the numpy restatement (tests/lines_ref.py), the fixture recorded from the reference's control
flow and the host twin; batching, ``masks=NULL``, the shared workspace; ``stages.get_line_masks`` and ``run_with_lines``."""
import ctypes as C
import time

import numpy as np
import pytest

from sbb_textline_detection_amd import _capi, stages

import lines_ref
import slopes_ref

pytestmark = pytest.mark.gpu
T0 = time.time()


def _small_model():
    from sbb_textline_detection_amd.model import SegModel
    from tools.synth_model import calibrated_model
    cfg, w = calibrated_model(2, 224, 224, seed=0)
    return SegModel(cfg, w, device=0, max_batch=4)               # any finalized handle: these calls do not touch the network


@pytest.fixture(scope="module")
def model():
    m = _small_model()
    yield m
    m.release()
    print(f"[test_gpu_lines] module wall time {time.time() - T0:.1f} s")


@pytest.fixture(scope="module")
def pages():
    return slopes_ref.load_pages()


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _raw(ctx, textlines, boxes, slopes, masks=True, dev=False):
    """The C call itself: (masks or None, rows, cols, mask_off, row_off, col_off) as the library packed them."""
    plane = np.ascontiguousarray(textlines, np.uint8)
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
    _capi.check(fn(ctx.h, src, plane.shape[0], plane.shape[1], _p(b), n, 2, _p(s), _p(m), _p(rows), _p(cols), _p(mo), _p(ro), _p(co)),
                "sbbseg_region_line_masks")
    return m, rows, cols, mo, ro, co


def _check_against(ctx, textlines, boxes, slopes, want):
    """want: per box (dst, rows, cols).  Checks the packing, the offsets, both entry points, and rows / cols against the mask."""
    m, rows, cols, mo, ro, co = _raw(ctx, textlines, boxes, slopes)
    w, h = np.array([b[2] for b in boxes], np.int64), np.array([b[3] for b in boxes], np.int64)
    assert np.array_equal(mo, np.concatenate([[0], np.cumsum(w * h)])) and np.array_equal(ro, np.concatenate([[0], np.cumsum(h)]))
    assert np.array_equal(co, np.concatenate([[0], np.cumsum(w)]))
    for r, box in enumerate(boxes):
        dst = m[mo[r]:mo[r + 1]].reshape(box[3], box[2])
        assert np.array_equal(dst, want[r][0]), (box, slopes[r], int((dst != want[r][0]).sum()))
        assert np.array_equal(rows[ro[r]:ro[r + 1]], want[r][1]) and np.array_equal(cols[co[r]:co[r + 1]], want[r][2]), (box, slopes[r])
        assert np.array_equal(rows[ro[r]:ro[r + 1]], dst.sum(axis=1)) and np.array_equal(cols[co[r]:co[r + 1]], dst.sum(axis=0))
    again = _raw(ctx, textlines, boxes, slopes, dev=True)
    for a, b in zip((m, rows, cols, mo, ro, co), again):
        assert np.array_equal(a, b)
    return m, rows, cols


def _random_case():
    textlines, boxes = slopes_ref.random_page()
    rng = np.random.RandomState(11)
    slopes = [float(lines_ref.SLOPES[r % len(lines_ref.SLOPES)]) if r < 2 * len(lines_ref.SLOPES) else float(rng.uniform(-90, 90)) for r in range(len(boxes))]
    slopes[0] = 2.0                                              # the whole plane
    return textlines, boxes, slopes


def test_fixture_pages_equal_the_restatement_the_fixture_and_the_host_twin(model, pages):
    ctx = model.ctx
    golden = lines_ref.load_golden()
    for k, ((_r, textlines, boxes, _s), (slopes, masks, _v)) in enumerate(zip(pages, golden)):
        want = [lines_ref.line_mask(slopes_ref.crop_of(textlines, b), s) for b, s in zip(boxes, slopes)]
        for r in range(len(boxes)):
            assert np.array_equal(want[r][0], masks[r]), (k, r)                      # restatement == committed fixture
        _check_against(ctx, textlines, boxes, slopes, want)
        host = [_capi.host_region_line_mask(slopes_ref.crop_of(textlines, b), s) for b, s in zip(boxes, slopes)]
        _check_against(ctx, textlines, boxes, slopes, host)
        # the slopes the device finds are the fixture's, so the chained call gives the fixture's masks
        got_slopes, got = stages.get_slopes_and_line_masks(textlines, boxes, ctx)
        assert got_slopes == slopes
        for r in range(len(boxes)):
            assert np.array_equal(got[r][0], masks[r]) and got[r][1].dtype == np.int64 and got[r][2].dtype == np.int64


def test_random_page_equals_the_restatement_and_the_host_twin(model):
    ctx = model.ctx
    textlines, boxes, slopes = _random_case()
    assert len(boxes) >= 24 and set(lines_ref.SLOPES) <= set(slopes) | {0.0}
    host = [_capi.host_region_line_mask(slopes_ref.crop_of(textlines, b), s) for b, s in zip(boxes, slopes)]
    m, rows, cols = _check_against(ctx, textlines, boxes, slopes, host)
    assert sum(1 for hst in host if hst[0].any()) >= 8
    for r in range(len(boxes)):                                  # and the numpy restatement, box by box
        want = lines_ref.line_mask(slopes_ref.crop_of(textlines, boxes[r]), slopes[r])
        for a, b in zip(host[r], want):
            assert np.array_equal(a, b), (boxes[r], slopes[r])
    # every listed slope on one box with text in it
    box = boxes[7]
    crop = slopes_ref.crop_of(textlines, box)
    _check_against(ctx, textlines, [box] * len(lines_ref.SLOPES), [float(s) for s in lines_ref.SLOPES], [lines_ref.line_mask(crop, s) for s in lines_ref.SLOPES])
    # all boxes in one call == one box per call; masks = NULL gives the same projections
    _m, rows_only, cols_only, _mo, ro, co = _raw(ctx, textlines, boxes, slopes, masks=False)
    assert np.array_equal(rows_only, rows) and np.array_equal(cols_only, cols)
    before = ctx.line_mask_launches()
    for r in range(len(boxes)):
        one = ctx.region_line_masks(textlines, [boxes[r]], [slopes[r]])
        assert np.array_equal(one[0][0], host[r][0]) and np.array_equal(one[0][1], host[r][1]) and np.array_equal(one[0][2], host[r][2])
    per_call = (ctx.line_mask_launches() - before) // len(boxes)
    before = ctx.line_mask_launches()
    ctx.region_line_masks(textlines, boxes, slopes, masks=False)
    assert ctx.line_mask_launches() - before == per_call == 10   # the number of launches does not depend on the number of boxes
    assert ctx.region_line_masks(textlines, [], []) == []


def test_bad_boxes_are_errors_and_the_handle_survives(model, pages):
    ctx = model.ctx
    _r, textlines, boxes, _s = pages[1]
    h, w = textlines.shape
    for bad in ([0, 0, 0, 5], [0, 0, 5, 0], [-1, 0, 5, 5], [w - 4, 0, 5, 5], [0, h - 4, 5, 5]):
        with pytest.raises(RuntimeError, match="box 1"):
            ctx.region_line_masks(textlines, [boxes[0], bad], [0.0, 0.0])
        with pytest.raises(RuntimeError, match="box 1"):
            ctx.region_line_masks_dev(ctx.stage(textlines), h, w, [boxes[0], bad], [0.0, 0.0])
    with pytest.raises(ValueError):
        ctx.region_line_masks(textlines, boxes, [])
    got = ctx.region_line_masks(textlines, boxes, [1.5])
    want = lines_ref.line_mask(slopes_ref.crop_of(textlines, boxes[0]), 1.5)
    assert all(np.array_equal(a, b) for a, b in zip(got[0], want))


def test_slopes_are_the_same_before_and_after_a_line_mask_call(model, pages):
    """The two steps share a workspace: neither may disturb the other."""
    ctx = model.ctx
    textlines, boxes, slopes = _random_case()
    boxes, slopes = boxes[1:], slopes[1:]
    first = stages.get_slopes(textlines, boxes, ctx)
    lines = stages.get_line_masks(textlines, boxes, slopes, ctx)
    assert stages.get_slopes(textlines, boxes, ctx) == first
    again = stages.get_line_masks(textlines, boxes, slopes, ctx)
    for a, b in zip(lines, again):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    _r, t4, b4, s4 = pages[4]
    assert stages.get_slopes(t4, b4, ctx) == s4
    no_masks = stages.get_line_masks(textlines, boxes, slopes, ctx, masks=False)
    for a, b in zip(lines, no_masks):
        assert b[0] is None and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert stages.get_line_masks(textlines, [], [], ctx) == [] and stages.get_slopes_and_line_masks(textlines, [], ctx) == ([], [])


def test_run_with_lines_at_full_size(tmp_path, monkeypatch):
    """The synthetic three-model pipeline of tests/test_gpu_slopes.py: run_with_lines' first six values are run_with_slopes', the seventh
    is get_line_masks applied to them; [] when the textline model does not run."""
    from sbb_textline_detection_amd import clear_session
    from sbb_textline_detection_amd.model import load_model
    from sbb_textline_detection_amd.synthetic import synthetic_page
    from sbb_textline_detection_amd.weights import save_sbbw
    from tools.synth_model import calibrated_model
    specs = {"model_page_mixed_best": (2, 21), "model_strukturerkennung": (4, 22), "model_textline_new": (2, 23)}      # main.py:58-60
    for name, (classes, seed) in specs.items():
        cfg, w = calibrated_model(classes, 448, 448, seed=seed)
        save_sbbw(str(tmp_path / (name + ".sbbw")), cfg, w)
    st = stages.InferenceStages(*[str(tmp_path / (n + ".h5")) for n in specs], model_kwargs={"max_batch": 108})
    page = synthetic_page(3500, 2500, seed=33)
    t = time.time()
    out = st.run_with_lines(page)
    t = time.time() - t
    ref = st.run_with_slopes(page)
    assert len(out) == 7 and out[3] == ref[3] and out[4] == ref[4] and out[5] == ref[5]
    for a, b in zip(out[:3], ref[:3]):
        assert (a is None) == (b is None) and (a is None or np.array_equal(a, b))
    textlines, boxes, slopes, lines = out[2], out[4], out[5], out[6]
    assert textlines is not None and len(boxes) >= 1, "this page and these nets are known to find text regions"
    ctx = load_model(str(tmp_path / "model_textline_new.h5"), max_batch=108).ctx
    want = stages.get_line_masks(textlines, boxes, slopes, ctx)
    assert len(lines) == len(want) == len(boxes) and lines is st.line_masks
    for box, slope, a, b in zip(boxes, slopes, lines, want):
        assert a[0].shape == (box[3], box[2]) and a[1].shape == (box[3],) and a[2].shape == (box[2],)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        if box[2] * box[3] <= 400 * 400:
            host = _capi.host_region_line_mask(slopes_ref.crop_of(textlines, box), slope)
            assert all(np.array_equal(x, y) for x, y in zip(a, host)), box
    print(f"[run_with_lines] 3500 x 2500: {len(boxes)} boxes, {sum(1 for a in lines if a[0].any())} non-empty masks, {t:.2f} s (first call)")
    monkeypatch.setenv("SBBSEG_STAGES_RESIDENT", "0")
    monkeypatch.setattr(stages.InferenceStages, "text_regions_present", lambda self, regions: False)
    out = st.run_with_lines(synthetic_page(520, 400, seed=9))
    assert out[2] is None and out[4] == [] and out[5] == [] and out[6] == [] and st.line_masks == []
    clear_session()
