"""-m gpu: ``InferenceStages.run_pages_with_reading_order`` -- ``run_pages_with_contours`` plus the reading order of every page's text
regions, computed on the resident textline plane and the resident contour table -- against the page loop (``run_with_line_boxes`` +
``get_text_region_contours`` + ``get_region_order``) and against the numpy / scipy restatement.  Models and strips are those of
tests/test_gpu_run_pages_contours.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from sbb_textline_detection_amd import clear_session, stages  # noqa: E402
from sbb_textline_detection_amd.model import load_model  # noqa: E402
from sbb_textline_detection_amd.synthetic import synthetic_page  # noqa: E402
from sbb_textline_detection_amd.weights import save_sbbw  # noqa: E402
from tools.synth_model import calibrated_model  # noqa: E402

import line_split_ref as lr  # noqa: E402
import order_ref  # noqa: E402

SPECS = {"model_page_mixed_best": 2, "model_strukturerkennung": 4, "model_textline_new": 2}      # main.py:58-60


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    d = tmp_path_factory.mktemp("run_pages_order")
    for name, classes in SPECS.items():
        cfg, w = calibrated_model(classes, 224, 224, seed=classes)
        save_sbbw(str(d / (name + ".sbbw")), cfg, w)
    paths = [str(d / (n + ".h5")) for n in SPECS]
    images = [np.ascontiguousarray(synthetic_page(h, 400, seed=s)[:, :w]) for h, w, s in ((600, 60, 6), (520, 75, 9), (600, 40, 1))]
    yield paths, images
    clear_session()


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b))


def test_run_pages_with_reading_order_equals_the_page_loop(setup):
    paths, images = setup
    st = stages.InferenceStages(*paths, model_kwargs={"max_batch": 16})
    border, layout = (load_model(p, max_batch=16).ctx for p in paths[:2])
    border.set_ksplit(False)
    try:
        want = []
        for img in images:
            page = st.run_with_line_boxes(img, masks=False)
            rings = st.get_text_region_contours(page[1]) if page[2] is not None else []
            want.append(page + (rings,) + (st.get_region_order(page[2], rings) if page[2] is not None else ([], [])))
        host_calls, launches = layout.host_contour_calls(), layout.order_launches()
        got = st.run_pages_with_reading_order(images)
        assert layout.host_contour_calls() == host_calls            # no label plane left the device
        with_lines = sum(1 for page in want if page[2] is not None)
        assert layout.order_launches() == launches + 4 * with_lines  # four launches a page, on the layout handle
    finally:
        border.set_ksplit(True)
    regions = [len(page[8]) for page in want]
    print("[run_pages_with_reading_order] regions per page %s, orders %s" % (regions, [page[9] for page in got]))
    assert max(regions) >= 2, regions                               # (else the order is trivially [0]: choose other strips)
    assert len(got) == 3
    for k, (g, w) in enumerate(zip(got, want)):
        assert len(g) == 11 and len(w) == 11, k
        assert all(_same(a, b) for a, b in zip(g[:3], w[:3])), k
        assert g[3] == w[3] and g[4] == w[4] and g[5] == w[5], k
        assert len(g[7]) == len(w[7]) and all(lr.same(a, b) for a, b in zip(g[7], w[7])), k
        assert len(g[8]) == len(w[8]) and all(_same(a, b) for a, b in zip(g[8], w[8])), k
        assert g[9] == w[9] and g[10] == w[10], (k, g[9:], w[9:])
        assert sorted(g[9]) == list(range(len(g[8]))) and g[10] == ["r%d" % m for m in range(len(g[8]))], k
        if g[2] is not None:                                        # and what scipy / numpy give for the same plane and rings
            ref_sorted, ref_matrix, _, _ = order_ref.order_of_regions(g[2], g[8])
            assert g[9] == order_ref.order_and_id_of_texts(g[8], ref_matrix, ref_sorted)[0], k
    assert got[2][2] is None and got[2][9:] == ([], [])
    assert st.run_pages_with_reading_order([]) == []
