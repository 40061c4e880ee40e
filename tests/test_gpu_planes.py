"""-m gpu: the per-box calls for boxes that lie on MANY device planes (``sbbseg_planes_deskew_slopes_dev``, ``sbbseg_planes_line_masks_dev``,
``sbbseg_planes_line_boxes_dev``) against their one-plane twins, bit for bit: on three tiny planes packed back to back in one allocation (a
wrong width or a read from the wrong plane returns a neighbour's bytes), on the five committed fixture pages pooled into one call (the
second sweep and the vertical splitter run on a subset that spans planes), the launch counters, and the host-side argument errors."""
import ctypes as C

import numpy as np
import pytest

from sbb_textline_detection_amd import _capi

import line_split_ref as lr
import lines_ref
import slopes_ref

pytestmark = pytest.mark.gpu
SIZES = [(23, 31), (19, 47), (64, 40)]                           # H x W


@pytest.fixture(scope="module")
def model():
    from sbb_textline_detection_amd.model import SegModel
    from tools.synth_model import calibrated_model
    cfg, w = calibrated_model(2, 224, 224, seed=0)
    m = SegModel(cfg, w, device=0, max_batch=4)                  # any finalized handle: these calls do not touch the network
    yield m
    m.release()


class Packed:
    """Host planes uploaded back to back into ONE device allocation: [(device pointer, H, W)]."""

    def __init__(self, ctx, arrays):
        self.ctx, self.arrays = ctx, [np.ascontiguousarray(a, np.uint8) for a in arrays]
        self.d = ctx.device_alloc(sum(a.size for a in self.arrays))
        ctx.upload(self.d, np.concatenate([a.ravel() for a in self.arrays]))
        at = np.concatenate([[0], np.cumsum([a.size for a in self.arrays])])
        self.planes = [(self.d + int(at[k]), a.shape[0], a.shape[1]) for k, a in enumerate(self.arrays)]

    def free(self):
        self.ctx.device_free(self.d)


def _plane_array(planes):
    arr = (_capi.Plane * len(planes))()
    for k, (d, h, w) in enumerate(planes):
        arr[k].d_hw, arr[k].H, arr[k].W = d or None, h, w
    return arr


def _pooled(ctx, planes, boxes, box_plane, erode=2, slopes=None):
    """The three pooled calls for boxes in ANY order (the binding's helpers with an explicit box_plane): (slopes, masks, records)."""
    arr, bp = _plane_array(planes), np.ascontiguousarray(box_plane, np.int32)
    if slopes is None:
        slopes = ctx._slopes_call(ctx.lib.sbbseg_planes_deskew_slopes_dev, arr, len(planes), 0, boxes, erode, None, bp)
    masks = ctx._line_masks_call(ctx.lib.sbbseg_planes_line_masks_dev, arr, len(planes), 0, boxes, slopes, erode, True, bp)
    records = ctx._line_boxes_call(ctx.lib.sbbseg_planes_line_boxes_dev, arr, lambda r: planes[int(bp[r])], len(planes), 0, boxes, slopes, erode,
                                   _capi.LINE_SIGMA_MAX, bp)
    return slopes, masks, records


def _one_plane(ctx, planes, boxes, box_plane, erode=2, slopes=None):
    """The same from the one-plane `_dev` calls, one call per plane with that plane's boxes, put back into box order."""
    n = len(boxes)
    out_s, out_m, out_r = [None] * n, [None] * n, [None] * n
    for k, (d, h, w) in enumerate(planes):
        mine = [r for r in range(n) if box_plane[r] == k]
        if not mine:
            continue
        bk = [boxes[r] for r in mine]
        sk = ctx.region_deskew_slopes_dev(d, h, w, bk, erode) if slopes is None else [slopes[r] for r in mine]
        mk = ctx.region_line_masks_dev(d, h, w, bk, sk, erode, True)
        rk = ctx.region_line_boxes_dev(d, h, w, bk, sk, erode)
        for q, r in enumerate(mine):
            out_s[r], out_m[r], out_r[r] = sk[q], mk[q], rk[q]
    return out_s, out_m, out_r


def _assert_same(got, want, tag):
    (gs, gm, gr), (ws, wm, wr) = got, want
    assert gs == ws, (tag, gs, ws)                               # floats, exactly
    assert len(gm) == len(wm) == len(gr) == len(wr) == len(gs)
    for r in range(len(gs)):
        for a, b in zip(gm[r], wm[r]):
            assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b), (tag, r)
        assert lr.same(gr[r], wr[r]), (tag, r)


def _tiny_boxes():
    """(boxes, box_plane) in shuffled plane order: each whole plane, a 1 x 1 box at a plane's last pixel, 5 x 5 boxes in the corners, boxes
    that touch the right and the bottom edge, plane 1 named by non-adjacent boxes."""
    per_plane = []
    for h, w in SIZES:
        per_plane.append([[0, 0, w, h], [w - 1, h - 1, 1, 1], [0, 0, 5, 5], [w - 5, 0, 5, 5], [0, h - 5, 5, 5], [w - 5, h - 5, 5, 5],
                          [w - 9, 2, 9, 11], [3, h - 7, 13, 7], [0, 0, 1, 1]])
    flat = [(k, b) for k, bs in enumerate(per_plane) for b in bs]
    order = np.random.RandomState(11).permutation(len(flat))
    boxes, box_plane = [flat[i][1] for i in order], [flat[i][0] for i in order]
    # plane 1 once more at both ends: one plane named by boxes that are not neighbours
    return [[2, 3, 30, 12]] + boxes + [[10, 1, 20, 17]], [1] + box_plane + [1]


def _tiny_planes(kind):
    rng = np.random.RandomState(3)
    dense = [(rng.rand(h, w) < 0.985).astype(np.uint8) for h, w in SIZES]      # mostly 1: the 9 x 9 erosion leaves a pattern, not zeros
    if kind == "random":
        return dense
    return [np.ones(SIZES[0], np.uint8), np.zeros(SIZES[1], np.uint8), dense[2]]


@pytest.mark.parametrize("kind", ["random", "ones_zeros_random"])
def test_tiny_planes_back_to_back_equal_the_one_plane_calls(model, kind):
    ctx = model.ctx
    host = _tiny_planes(kind)
    packed = Packed(ctx, host)
    try:
        boxes, box_plane = _tiny_boxes()
        assert sum(b[2] * b[3] for b in boxes) < 256 * 24 and set(box_plane) == {0, 1, 2} and box_plane[0] == box_plane[-1] == 1
        for erode in (2, 0):                                     # 0: the crops are the planes' own bytes
            want = _one_plane(ctx, packed.planes, boxes, box_plane, erode)
            got = _pooled(ctx, packed.planes, boxes, box_plane, erode)
            _assert_same(got, want, (kind, erode))
            # ... and with slopes that take the rotation and the vertical splitter (random planes have none of their own)
            given = [[0.0, 7.5, -21.0, 50.0, -88.0][r % 5] for r in range(len(boxes))]
            want_g = _one_plane(ctx, packed.planes, boxes, box_plane, erode, given)
            _assert_same(_pooled(ctx, packed.planes, boxes, box_plane, erode, given), want_g, (kind, erode, "given"))
            # the masks follow the numpy restatement of the crop of the box's OWN plane
            for r in (0, 1, len(boxes) - 1):
                dst, rows, cols = lines_ref.line_mask(slopes_ref.crop_of(host[box_plane[r]], boxes[r]), given[r], erode)
                assert np.array_equal(want_g[1][r][0], dst) and np.array_equal(want_g[1][r][1], rows) and np.array_equal(want_g[1][r][2], cols)
        # not vacuous: something survives the erosion, and the whole-plane masks of two planes differ
        whole = [r for r, b in enumerate(boxes) if b[:2] == [0, 0] and (b[3], b[2]) in SIZES]
        assert len(whole) == 3 and any(want[1][r][0].any() for r in whole)
        # a plane without a box, through the public binding (plane order): plane 1 is skipped and may even have no pointer
        per_plane = [[b for b, k in zip(boxes, box_plane) if k == q] for q in range(3)]
        some = [per_plane[0], [], per_plane[2]]
        planes = [packed.planes[0], (0, 19, 47), packed.planes[2]]
        slopes = ctx.planes_deskew_slopes_dev(planes, some)
        masks = ctx.planes_line_masks_dev(planes, some, slopes)
        records = ctx.planes_line_boxes_dev(planes, some, slopes)
        assert slopes[1] == [] and masks[1] == [] and records[1] == []
        for q in (0, 2):
            d, h, w = packed.planes[q]
            assert slopes[q] == ctx.region_deskew_slopes_dev(d, h, w, some[q])
            for a, b in zip(masks[q], ctx.region_line_masks_dev(d, h, w, some[q], slopes[q])):
                assert all(np.array_equal(x, y) for x, y in zip(a, b))
            assert all(lr.same(a, b) for a, b in zip(records[q], ctx.region_line_boxes_dev(d, h, w, some[q], slopes[q])))
        assert ctx.planes_deskew_slopes_dev(planes, [[], [], []]) == [[], [], []] and ctx.planes_line_boxes_dev([], [], []) == []
    finally:
        packed.free()


@pytest.fixture(scope="module")
def fixture_pages(model):
    """The five committed pages on the device (one allocation), their boxes and the per-box references, computed once."""
    pages = slopes_ref.load_pages()
    packed = Packed(model.ctx, [p[1] for p in pages])
    golden = lines_ref.load_golden()
    cases = {(c["page"], c["box"]): c for c in lr.load_golden()}
    ref_masks = [[lines_ref.line_mask(slopes_ref.crop_of(textlines, box), slope) for box, slope in zip(boxes, slopes)]
                 for (_r, textlines, boxes, _s), (slopes, _m, _v) in zip(pages, golden)]
    yield pages, packed, cases, ref_masks
    packed.free()


def test_fixture_pages_pooled_in_one_call(model, fixture_pages):
    ctx = model.ctx
    pages, packed, cases, ref_masks = fixture_pages
    boxes = [p[2] for p in pages]
    assert len(pages) == 5 and sum(len(b) for b in boxes) == 14
    before5, before2 = ctx.debug_counter(5), ctx.debug_counter(2)
    slopes = ctx.planes_deskew_slopes_dev(packed.planes, boxes)
    sweeps5 = ctx.debug_counter(5) - before5
    masks = ctx.planes_line_masks_dev(packed.planes, boxes, slopes)
    records = ctx.planes_line_boxes_dev(packed.planes, boxes, slopes)
    assert ctx.debug_counter(2) - before2 == 10 + 11             # masks; masks + split
    flat = [s for sl in slopes for s in sl]
    assert any(s <= -50 for s in flat) and any(abs(s) > 45 for s in flat) and any(0 < abs(s) <= 15 for s in flat)
    assert sum(1 for sl in slopes if any(abs(s) > 15 for s in sl)) >= 1
    per_page2 = ctx.debug_counter(2)
    for k, (_r, textlines, bk, recorded) in enumerate(pages):
        d, h, w = packed.planes[k]
        assert slopes[k] == recorded == ctx.region_deskew_slopes_dev(d, h, w, bk), k
        per_masks = ctx.region_line_masks_dev(d, h, w, bk, slopes[k])
        per_records = ctx.region_line_boxes_dev(d, h, w, bk, slopes[k])
        for r in range(len(bk)):
            for a, b, c in zip(masks[k][r], per_masks[r], ref_masks[k][r]):
                assert a.shape == b.shape == c.shape and np.array_equal(a, b) and np.array_equal(a, c), (k, r)
            assert lr.same(records[k][r], per_records[r]) and lr.same(records[k][r], cases[(k, r)]), (k, r)
    assert ctx.debug_counter(2) - per_page2 == 5 * (10 + 11)
    # (c) the pooled line-boxes call alone: 11 for five planes, the five per-page calls 55
    before2 = ctx.debug_counter(2)
    ctx.planes_line_boxes_dev(packed.planes, boxes, slopes)
    assert ctx.debug_counter(2) - before2 == 11
    before2 = ctx.debug_counter(2)
    for k in range(5):
        ctx.region_line_boxes_dev(*packed.planes[k], boxes[k], slopes[k])
    assert ctx.debug_counter(2) - before2 == 55
    # ... and the slope sweeps: a steep box makes two sweeps of 3 + 2 kernels each, for one plane as for five
    steep = [k for k in range(5) if any(abs(s) > 15 for s in slopes[k])]
    assert steep and sweeps5 == 10
    before5 = ctx.debug_counter(5)
    assert ctx.planes_deskew_slopes_dev([packed.planes[steep[0]]], [boxes[steep[0]]]) == [slopes[steep[0]]]
    assert ctx.debug_counter(5) - before5 == sweeps5
    assert ctx.slope_sweep_launches() == ctx.debug_counter(5)


def test_argument_errors_are_host_side_and_leave_the_handle_usable(model, fixture_pages):
    ctx = model.ctx
    pages, packed, _cases, _ref = fixture_pages
    planes, boxes = packed.planes[:2], [pages[0][2], pages[1][2]]
    good = ctx.planes_deskew_slopes_dev(planes, boxes)
    flat = [b for bs in boxes for b in bs]
    bp = [0] * len(boxes[0]) + [1] * len(boxes[1])
    flat_slopes = [s for sl in good for s in sl]
    (h0, w0), (h1, w1) = planes[0][1:], planes[1][1:]
    assert (h0, w0) != (h1, w1)
    own = [0, 0, max(w0, w1), 1] if w0 != w1 else [0, 0, 1, max(h0, h1)]      # fits the larger plane only
    small = (0 if w0 < w1 else 1) if w0 != w1 else (0 if h0 < h1 else 1)

    def calls(pl, b, plane_of, sl):
        arr, p_of = _plane_array(pl), np.ascontiguousarray(plane_of, np.int32)
        yield lambda: ctx._slopes_call(ctx.lib.sbbseg_planes_deskew_slopes_dev, arr, len(pl), 0, b, 2, None, p_of)
        yield lambda: ctx._line_masks_call(ctx.lib.sbbseg_planes_line_masks_dev, arr, len(pl), 0, b, sl, 2, True, p_of)
        yield lambda: ctx._line_boxes_call(ctx.lib.sbbseg_planes_line_boxes_dev, arr, None, len(pl), 0, b, sl, 2, _capi.LINE_SIGMA_MAX, p_of)

    cases = [
        (planes, flat, bp[:-1] + [2], flat_slopes, "box %d: plane 2 out of range" % (len(flat) - 1)),
        (planes, flat, [-1] + bp[1:], flat_slopes, "box 0: plane -1 out of range"),
        (planes, [flat[0], own], [0, small], flat_slopes[:2], r"box 1 \(.*\) leaves the %d x %d plane %d" % (planes[small][2], planes[small][1], small)),
        ([planes[0], (0, h1, w1)], flat, bp, flat_slopes, "box %d: plane 1 has no device pointer" % len(boxes[0])),
        (planes, [flat[0], [0, 0, 0, 3]], [0, 1], flat_slopes[:2], "box 1: width 0, height 3"),
    ]
    for pl, b, plane_of, sl, message in cases:
        for call in calls(pl, b, plane_of, sl):
            with pytest.raises(RuntimeError, match=message):
                call()
            assert ctx.planes_deskew_slopes_dev(planes, boxes) == good        # the handle works on
    b = np.ascontiguousarray(flat, np.int32)
    out = np.zeros(len(flat), np.float64)
    rc = ctx.lib.sbbseg_planes_deskew_slopes_dev(ctx.h, _plane_array(planes), 0, b.ctypes.data_as(C.c_void_p),
                                                 np.ascontiguousarray(bp, np.int32).ctypes.data_as(C.c_void_p), len(flat), 2, None, 0,
                                                 out.ctypes.data_as(C.c_void_p))
    assert rc != 0 and b"boxes but 0 planes" in ctx.lib.sbbseg_last_error()
    assert ctx.planes_deskew_slopes_dev(planes, boxes) == good
    assert ctx.planes_deskew_slopes_dev(planes, [[], []]) == [[], []]
    with pytest.raises(RuntimeError, match="unknown counter"):
        ctx.debug_counter(6)
