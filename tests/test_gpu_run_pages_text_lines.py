"""-m gpu: ``InferenceStages.run_pages_with_text_lines`` -- ``run_pages_with_reading_order`` plus, per region, the reference's list of 4 x 2
line polygons, the lines of all pages' regions cut to their contours in one pooled call -- against ``run_pages_with_reading_order``
followed by the library's serial host twin region by region, and against ``stages.get_line_boxes(..., contours=...)`` page by page.
Models and strips are those of tests/test_gpu_run_pages_order.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from sbb_textline_detection_amd import _capi, clear_session, stages  # noqa: E402
from sbb_textline_detection_amd.model import load_model  # noqa: E402
from sbb_textline_detection_amd.synthetic import synthetic_page  # noqa: E402
from sbb_textline_detection_amd.weights import save_sbbw  # noqa: E402
from tools.synth_model import calibrated_model  # noqa: E402

SPECS = {"model_page_mixed_best": 2, "model_strukturerkennung": 4, "model_textline_new": 2}      # main.py:58-60
KEYS = ("status", "sigma", "raised", "branch", "peaks", "point_up", "point_down", "boxes", "boxes_rot", "extent")


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    d = tmp_path_factory.mktemp("run_pages_text_lines")
    for name, classes in SPECS.items():
        cfg, w = calibrated_model(classes, 224, 224, seed=classes)
        save_sbbw(str(d / (name + ".sbbw")), cfg, w)
    paths = [str(d / (n + ".h5")) for n in SPECS]
    images = [np.ascontiguousarray(synthetic_page(h, 400, seed=s)[:, :w]) for h, w, s in ((600, 60, 6), (520, 75, 9), (600, 40, 1))]
    yield paths, images
    clear_session()


def same_record(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in KEYS) and a["contour"] == b["contour"]


def test_run_pages_with_text_lines_equals_the_host_twin_region_by_region(setup):
    paths, images = setup
    st = stages.InferenceStages(*paths, model_kwargs={"max_batch": 16})
    textline = load_model(paths[2], max_batch=16).ctx
    base = st.run_pages_with_reading_order(images)
    launches = textline.extent_launches()
    got = st.run_pages_with_text_lines(images)
    with_boxes = sum(1 for page in base if page[4])
    assert with_boxes >= 1 and textline.extent_launches() - launches in (5, 7)      # ONE pooled call for all pages: the scan in one or both forms
    assert len(got) == len(base) == 3
    regions = 0
    for k, (g, b) in enumerate(zip(got, base)):
        assert len(g) == 12 and len(b) == 11, k
        assert g[4] == b[4] and g[5] == b[5] and g[9:11] == b[9:11], k
        want = stages.get_line_extents(b[4], b[5], b[7], b[8], None)                # the serial host twin on the uncut records
        assert len(g[7]) == len(want) and all(same_record(x, y) for x, y in zip(g[7], want)), k
        assert len(g[11]) == len(want), k
        for polygons, rec in zip(g[11], want):
            assert len(polygons) == (len(rec["boxes_rot"]) if rec["status"] == _capi.LINES_OK else 0)
            assert all(p.shape == (4, 2) and np.array_equal(p, q) for p, q in zip(polygons, rec["boxes_rot"]))
        if b[2] is not None and b[4]:                                               # and the one-page stage function with contours=
            page = stages.get_line_boxes(b[2], b[4], b[5], textline, contours=b[8])
            assert all(same_record(x, y) for x, y in zip(page, want)), k
            plain = stages.get_line_boxes(b[2], b[4], b[5], textline)               # the default is unchanged: the fallback extent 0 .. w
            assert all("extent" not in x and np.array_equal(x["boxes_rot"], y["boxes_rot"]) for x, y in zip(plain, b[7])), k
        regions += len(want)
    assert regions >= 2
    assert got[2][2] is None and got[2][11] == []
    assert st.run_pages_with_text_lines([]) == []
