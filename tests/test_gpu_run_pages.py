"""-m gpu: sbbseg_run_pages -- the three model stages for many pages in one resident, pooled call -- against one sbbseg_run_page call per
page on the same three handles, with split-K off on the border handle (from two pages on the batched border forward never splits).
Models and images are those of tests/test_gpu_views.py::test_run_pages_equals_run_page_by_page: the first two strips reach the textline
model, the third (2800 x 186 after the upscale) cannot hold the layout model's 224 x 224 input."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from sbb_textline_detection_amd import _capi, clear_session, stages  # noqa: E402
from sbb_textline_detection_amd.model import load_model  # noqa: E402
from sbb_textline_detection_amd.stages import scaled_size  # noqa: E402
from sbb_textline_detection_amd.synthetic import synthetic_page  # noqa: E402
from sbb_textline_detection_amd.weights import save_sbbw  # noqa: E402
from tools.synth_model import calibrated_model  # noqa: E402

SPECS = {"model_page_mixed_best": 2, "model_strukturerkennung": 4, "model_textline_new": 2}      # main.py:58-60
FILL = 9


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    d = tmp_path_factory.mktemp("run_pages")
    for name, classes in SPECS.items():
        cfg, w = calibrated_model(classes, 224, 224, seed=classes)
        save_sbbw(str(d / (name + ".sbbw")), cfg, w)
        if name == "model_page_mixed_best":                   # the same border model with a head bias that forces class 0: no page anywhere
            w0 = dict(w)
            last_bias = [k for k in w0 if k.endswith("/bias:0")][-1]
            w0[last_bias] = np.array([1.0e4, -1.0e4], w0[last_bias].dtype)
            save_sbbw(str(d / "model_page_empty.sbbw"), cfg, w0)
    paths = [str(d / (n + ".h5")) for n in SPECS]
    images = [np.ascontiguousarray(synthetic_page(h, 400, seed=s)[:, :w]) for h, w, s in ((600, 60, 6), (520, 75, 9), (600, 40, 1))]
    yield paths, str(d / "model_page_empty.h5"), images
    clear_session()


def _handles(paths):
    return [load_model(p, max_batch=16).ctx for p in paths]


def _pages(images):
    return [(img,) + scaled_size(*img.shape[:2]) for img in images]


def _info(info):
    return (tuple(int(v) for v in info.box_xywh), int(info.box_pixels), int(info.otsu_threshold), int(info.regions_ok), int(info.text_present),
            int(info.textlines_ok))


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b))


def test_run_pages_equals_run_page_per_page(setup):
    paths, _, images = setup
    border, layout, textline = _handles(paths)
    border.set_ksplit(False)
    try:
        want = [_capi.run_page(border, layout, textline, img, hs, ws) for img, hs, ws in _pages(images)]
        views, whole = layout.views_launches(), border.whole_launches()
        got = _capi.run_pages(border, layout, textline, _pages(images))
        assert layout.views_launches() > views                                 # the pooled layout call ran
        assert border.whole_launches() - whole == 2                            # three border forwards: one chunk, one ingest + one resize
    finally:
        border.set_ksplit(True)
    assert len(got) == len(want) == 3
    for k, ((mask, regions, lines, info, status), (wmask, wregions, wlines, winfo)) in enumerate(zip(got, want)):
        assert status == 0, k
        assert _info(info) == _info(winfo), (k, _info(info), _info(winfo))
        assert _same(mask, wmask) and _same(regions, wregions) and _same(lines, wlines), k
    # both outcomes are in the set (else the comparison above could pass vacuously)
    assert [int(g[3].textlines_ok) for g in got] == [1, 1, 0] and [int(g[3].regions_ok) for g in got] == [1, 1, 0]
    assert got[0][2] is not None and got[1][2] is not None and got[2][1] is None and got[2][2] is None
    # ... and with split-K left on only the border mask may differ from run_page's
    split = [_capi.run_page(border, layout, textline, img, hs, ws) for img, hs, ws in _pages(images)]
    for k, ((mask, regions, lines, info, status), (smask, sregions, slines, sinfo)) in enumerate(zip(got, split)):
        if np.array_equal(mask, smask):
            assert _info(info) == _info(sinfo) and _same(regions, sregions) and _same(lines, slines), k


def test_empty_border_masks_set_the_status_and_touch_nothing(setup):
    paths, empty_border, images = setup
    border, layout, textline = _handles([empty_border] + paths[1:])
    pages = _pages(images)
    io = (_capi.RunPageIO * len(pages))()
    keep = []
    for k, (img, hs, ws) in enumerate(pages):
        bufs = [np.full(hs * ws * 3, FILL, np.uint8), np.full(hs * ws * 3, FILL, np.uint8), np.full(hs * ws, FILL, np.uint8)]
        keep.append(bufs)
        io[k].page, io[k].Hp, io[k].Wp, io[k].Hs, io[k].Ws = img.ctypes.data, img.shape[0], img.shape[1], hs, ws
        io[k].page_mask_out, io[k].regions_out, io[k].textlines_out = (b.ctypes.data for b in bufs)
        io[k].status = -7
    views = layout.views_launches()
    rc = border.lib.sbbseg_run_pages(border.h, layout.h, textline.h, len(pages), io, 3)
    assert rc == 0, border.lib.sbbseg_last_error()
    for k in range(len(pages)):
        assert io[k].status == 1 and int(io[k].info.box_pixels) == 0 and list(io[k].info.box_xywh) == [0, 0, 0, 0], k
        assert int(io[k].info.regions_ok) == 0 and int(io[k].info.text_present) == 0 and int(io[k].info.textlines_ok) == 0
        assert all(bool((b == FILL).all()) for b in keep[k]), k
    assert layout.views_launches() == views                                    # no page reached the layout model
    assert all(g[4] == 1 and g[0] is None and g[1] is None and g[2] is None for g in _capi.run_pages(border, layout, textline, pages))
    st = stages.InferenceStages(empty_border, paths[1], paths[2], model_kwargs={"max_batch": 16})
    with pytest.raises(ValueError, match="argmax of an empty sequence") as loop:
        st.run(images[0])
    with pytest.raises(ValueError, match="argmax of an empty sequence") as resident:
        st.run_pages(images, resident=True)
    assert type(resident.value) is type(loop.value) and str(resident.value) == str(loop.value)


def test_stages_resident_equals_run_and_leaves_no_state(setup):
    paths, _, images = setup
    st = stages.InferenceStages(*paths, model_kwargs={"max_batch": 16})
    border, layout, _ = _handles(paths)
    before = st.run_pages(images)
    border.set_ksplit(False)
    try:
        want = [st.run(img) for img in images]
        views, whole = layout.views_launches(), border.whole_launches()
        got = st.run_pages(images, resident=True)
        assert layout.views_launches() > views and border.whole_launches() - whole == 2
    finally:
        border.set_ksplit(True)
    after = st.run_pages(images)
    assert len(got) == len(want) == len(before) == len(after) == 3
    for k in range(3):
        assert got[k][3] == want[k][3] and before[k][3] == after[k][3], k
        assert all(_same(a, b) for a, b in zip(got[k][:3], want[k][:3])), k
        assert all(_same(a, b) for a, b in zip(before[k][:3], after[k][:3])), k
    assert [g[1] is None for g in got] == [False, False, True] and [g[2] is None for g in got] == [False, False, True]
