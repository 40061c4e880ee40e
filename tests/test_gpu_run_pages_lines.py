"""-m gpu: ``InferenceStages.run_pages_with_line_boxes`` -- one resident ``sbbseg_run_pages``, then boxes, slopes and text lines of all pages
from the planes that call leaves on the device -- against ``run_with_line_boxes`` page by page, and ``sbbseg_run_pages_planes`` itself.
Models and strips are those of tests/test_gpu_run_pages.py: 224 x 224 calibrated models, the first two strips reach the textline model,
the third cannot hold a model input."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from sbb_textline_detection_amd import _capi, clear_session, stages  # noqa: E402
from sbb_textline_detection_amd.model import load_model  # noqa: E402
from sbb_textline_detection_amd.stages import scaled_size  # noqa: E402
from sbb_textline_detection_amd.synthetic import synthetic_page  # noqa: E402
from sbb_textline_detection_amd.weights import save_sbbw  # noqa: E402
from tools.synth_model import calibrated_model  # noqa: E402

import line_split_ref as lr  # noqa: E402

SPECS = {"model_page_mixed_best": 2, "model_strukturerkennung": 4, "model_textline_new": 2}      # main.py:58-60


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    d = tmp_path_factory.mktemp("run_pages_lines")
    for name, classes in SPECS.items():
        cfg, w = calibrated_model(classes, 224, 224, seed=classes)
        save_sbbw(str(d / (name + ".sbbw")), cfg, w)
    paths = [str(d / (n + ".h5")) for n in SPECS]
    images = [np.ascontiguousarray(synthetic_page(h, 400, seed=s)[:, :w]) for h, w, s in ((600, 60, 6), (520, 75, 9), (600, 40, 1))]
    yield paths, images
    clear_session()


def _handles(paths):
    return [load_model(p, max_batch=16).ctx for p in paths]


def _pages(images):
    return [(img,) + scaled_size(*img.shape[:2]) for img in images]


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b))


def test_planes_fail_cleanly_without_a_run_and_return_what_run_pages_returned(setup):
    paths, images = setup
    border, layout, textline = _handles(paths)
    with pytest.raises(RuntimeError, match="no resident planes"):               # absent: these handles are fresh
        _capi.run_pages_planes(layout)
    got = _capi.run_pages(border, layout, textline, _pages(images), channels=3)
    regions, textlines = _capi.run_pages_planes(layout)
    assert len(regions) == len(textlines) == 3
    for k, (_mask, r, t, info, status) in enumerate(got):
        w, h = int(info.box_xywh[2]), int(info.box_xywh[3])
        assert status == 0 and regions[k][1:] == (h, w) and textlines[k][1:] == (h, w), k
        assert (regions[k][0] != 0) == (r is not None) and (textlines[k][0] != 0) == (t is not None), k
        if r is not None:
            assert np.array_equal(layout.download(regions[k][0], (h, w)), r[:, :, 0]), k
        if t is not None:                                         # read through ANOTHER handle: run_pages has synchronised all three streams
            assert np.array_equal(border.download(textlines[k][0], (h, w)), t), k
    assert [r[0] != 0 for r in regions] == [True, True, False] and [t[0] != 0 for t in textlines] == [True, True, False]
    # the wrong number of pages; then a failed call and a one-page call, which both leave nothing to return
    out = (_capi.Plane * 2)()
    assert layout.lib.sbbseg_run_pages_planes(layout.h, 2, out, out) != 0
    assert b"2 pages asked for, the last sbbseg_run_pages ran 3" in layout.lib.sbbseg_last_error()
    assert len(_capi.run_pages_planes(layout)[0]) == 3            # (the error changed nothing)
    with pytest.raises(RuntimeError, match="bad arguments"):
        _capi.run_pages(border, layout, textline, [], channels=3)
    with pytest.raises(RuntimeError, match="no resident planes"):
        _capi.run_pages_planes(layout)
    _capi.run_pages(border, layout, textline, _pages(images[:2]), channels=3)
    assert len(_capi.run_pages_planes(layout)[0]) == 2
    _capi.run_page(border, layout, textline, *_pages(images)[0])
    out3 = (_capi.Plane * 2)()
    assert layout.lib.sbbseg_run_pages_planes(layout.h, 2, out3, out3) != 0 and b"no resident planes" in layout.lib.sbbseg_last_error()
    assert C.sizeof(_capi.Plane) == 16


def test_run_pages_with_line_boxes_equals_the_page_loop(setup):
    paths, images = setup
    st = stages.InferenceStages(*paths, model_kwargs={"max_batch": 16})
    border, layout, textline = _handles(paths)
    border.set_ksplit(False)
    try:
        want = [st.run_with_line_boxes(img, masks=False) for img in images]
        want_masks = [st.run_with_line_boxes(img) for img in images]
        lines2, sweeps5, views = textline.debug_counter(2), textline.debug_counter(5), layout.views_launches()
        got = st.run_pages_with_line_boxes(images)
        pooled2, pooled5 = textline.debug_counter(2) - lines2, textline.debug_counter(5) - sweeps5
        assert layout.views_launches() > views                     # the pooled layout call ran
        got_masks = st.run_pages_with_line_boxes(images, masks=True)
    finally:
        border.set_ksplit(True)
    n_boxes = [len(w[4]) for w in want]
    print("[run_pages_with_line_boxes] boxes per page %s, slopes %s, line launches %d, sweep launches %d" % (n_boxes, [w[5] for w in want], pooled2, pooled5))
    assert sum(n_boxes) >= 1 and max(n_boxes[:2]) >= 1, n_boxes     # (else everything below passes vacuously: choose other seeds)
    # one masks call (10) and one line-boxes call (10 + the split: 1, or 2 with a profile beyond 2048 samples) for ALL pages; one or two
    # sweeps of 3 + 2 kernels (+ 1 with a deskew square beyond 2048): the strips are 2800 rows tall
    assert pooled2 in (21, 22) and pooled5 in (5, 6, 10, 12), (pooled2, pooled5)
    for g_all, w_all, with_masks in ((got, want, False), (got_masks, want_masks, True)):
        assert len(g_all) == len(w_all) == 3
        for k, (g, w) in enumerate(zip(g_all, w_all)):
            assert len(g) == len(w) == 8, k
            assert all(_same(a, b) for a, b in zip(g[:3], w[:3])), k
            assert g[3] == w[3] and g[4] == w[4] and g[5] == w[5], (k, g[3:6], w[3:6])      # page_coord, boxes, slopes: exactly
            assert all(isinstance(s, float) for s in g[5]) and len(g[6]) == len(w[6]) == len(g[7]) == len(w[7]) == len(g[4]), k
            for (gm, grows, gcols), (wm, wrows, wcols) in zip(g[6], w[6]):
                assert (gm is not None) == with_masks and _same(gm, wm) and _same(grows, wrows) and _same(gcols, wcols), k
            assert all(lr.same(a, b) for a, b in zip(g[7], w[7])), k
    # the third strip cannot hold a model input: no regions, no text lines, empty lists
    assert got[2][1] is None and got[2][2] is None and got[2][4:] == ([], [], [], [])
    assert got[0][2] is not None and got[1][2] is not None
    assert st.run_pages_with_line_boxes([]) == []
