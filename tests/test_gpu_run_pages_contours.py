"""-m gpu: ``InferenceStages.run_pages_with_contours`` -- ``run_pages_with_line_boxes`` with the per-page boxes call replaced by the device
contour tracer -- against ``run_with_line_boxes`` + ``get_text_region_contours`` page by page.  Models and strips are those of
tests/test_gpu_run_pages_lines.py: 224 x 224 calibrated models, the first two strips reach the textline model, the third cannot hold a
model input."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from sbb_textline_detection_amd import clear_session, stages  # noqa: E402
from sbb_textline_detection_amd.model import load_model  # noqa: E402
from sbb_textline_detection_amd.synthetic import synthetic_page  # noqa: E402
from sbb_textline_detection_amd.weights import save_sbbw  # noqa: E402
from tools.synth_model import calibrated_model  # noqa: E402

import line_split_ref as lr  # noqa: E402

SPECS = {"model_page_mixed_best": 2, "model_strukturerkennung": 4, "model_textline_new": 2}      # main.py:58-60


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    d = tmp_path_factory.mktemp("run_pages_contours")
    for name, classes in SPECS.items():
        cfg, w = calibrated_model(classes, 224, 224, seed=classes)
        save_sbbw(str(d / (name + ".sbbw")), cfg, w)
    paths = [str(d / (n + ".h5")) for n in SPECS]
    images = [np.ascontiguousarray(synthetic_page(h, 400, seed=s)[:, :w]) for h, w, s in ((600, 60, 6), (520, 75, 9), (600, 40, 1))]
    yield paths, images
    clear_session()


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b))


def test_run_pages_with_contours_equals_the_page_loop(setup):
    paths, images = setup
    st = stages.InferenceStages(*paths, model_kwargs={"max_batch": 16})
    border, layout = (load_model(p, max_batch=16).ctx for p in paths[:2])
    border.set_ksplit(False)
    try:
        want, want_rings = [], []
        for img in images:
            page = st.run_with_line_boxes(img, masks=False)
            want.append(page)
            want_rings.append(st.get_text_region_contours(page[1]) if page[2] is not None else [])
            assert page[2] is None or st.boxes == page[4]           # get_text_region_contours sets self.boxes: the boxes call's
        host_calls, launches = layout.host_contour_calls(), layout.contour_launches()
        got = st.run_pages_with_contours(images)
        assert layout.host_contour_calls() == host_calls            # no label plane left the device
        assert layout.contour_launches() > launches
    finally:
        border.set_ksplit(True)
    n_rings = [len(r) for r in want_rings]
    print("[run_pages_with_contours] contours per page %s, points %s" % (n_rings, [[len(c) for c in r] for r in want_rings]))
    assert sum(n_rings) >= 1 and max(n_rings[:2]) >= 1, n_rings     # (else everything below passes vacuously: choose other seeds)
    assert len(got) == 3
    for k, (g, w, rings) in enumerate(zip(got, want, want_rings)):
        assert len(g) == 9 and len(w) == 8, k
        assert all(_same(a, b) for a, b in zip(g[:3], w[:3])), k
        assert g[3] == w[3] and g[4] == w[4] and g[5] == w[5], (k, g[3:6], w[3:6])      # page_coord, boxes, slopes: exactly
        for (gm, grows, gcols), (wm, wrows, wcols) in zip(g[6], w[6]):
            assert gm is None and wm is None and _same(grows, wrows) and _same(gcols, wcols), k
        assert len(g[7]) == len(w[7]) and all(lr.same(a, b) for a, b in zip(g[7], w[7])), k
        assert len(g[8]) == len(rings) == len(g[4]), k
        for c, r, box in zip(g[8], rings, g[4]):
            assert c.dtype == np.uint and c.ndim == 3 and c.shape[1:] == (1, 2) and _same(c, r) and (c[0] == c[-1]).all(), k
            p = c.reshape(-1, 2).astype(np.int64)
            assert box == [p[:, 0].min(), p[:, 1].min(), p[:, 0].max() - p[:, 0].min() + 1, p[:, 1].max() - p[:, 1].min() + 1], k
    assert got[2][1] is None and got[2][2] is None and got[2][4:] == ([], [], [], [], [])
    assert st.run_pages_with_contours([]) == []
