"""The boxes + slopes step on the device (-m gpu): sbbseg_text_region_boxes against the fixture recorded from the reference's control
flow and against the host mirror; the batched per-region rotate-and-project, bit for bit, against the existing one-region path
(``ctx.deskew_profiles`` of the eroded crop: unchanged, the yardstick) and the CPU oracle; ``stages.get_slopes`` and ``run_with_slopes``."""
import os
import time

import numpy as np
import pytest

from sbb_textline_detection_amd import _capi, stages

import slopes_ref

pytestmark = pytest.mark.gpu
T0 = time.time()
GLUE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "glue_golden.npz")


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
    print(f"[test_gpu_slopes] module wall time {time.time() - T0:.1f} s")


@pytest.fixture(scope="module")
def pages():
    return slopes_ref.load_pages()


def test_boxes_equal_the_reference_and_the_host_mirror(model, pages):
    ctx = model.ctx
    for k, (regions, _t, boxes, _s) in enumerate(pages):
        assert ctx.text_region_boxes(regions) == boxes, k
        assert ctx.text_region_boxes(np.repeat(regions[:, :, None], 3, axis=2)) == boxes, k
        d = ctx.stage(regions)
        assert ctx.text_region_boxes_dev(d, *regions.shape) == boxes, k
    g = np.load(GLUE)
    seen = 0
    for k in range(int(g["regions_n"])):                         # the TEXT_REGION_CASES maps of make_glue_golden.py
        plane = g[f"regions_map{k}"]
        if not int(g[f"regions_ch1_{k}"]):
            continue                                             # (class 1 in one channel only: the plane alone does not say so)
        got = ctx.text_region_boxes(plane)
        assert got == stages.host_text_region_boxes(plane), k
        assert len(got) == len(g[f"regions_areas{k}"]), k        # as many boxes as the reference kept contours
        seen += len(got)
    assert seen >= 5
    # the exact host tracing of every candidate (test hook) decides the same
    ctx.set_conv_variant(1 << 21)
    try:
        for regions, _t, boxes, _s in pages[:3]:
            assert ctx.text_region_boxes(regions) == boxes
    finally:
        ctx.set_conv_variant(0)


def test_boxes_cap_and_area_bounds(model, pages):
    """n is the number found whatever cap is; a zero cap only counts; the area bounds hold on the device as on the host."""
    import ctypes as C
    ctx = model.ctx
    regions, boxes = pages[4][0], pages[4][2]
    n = C.c_int(-1)
    plane = np.ascontiguousarray(regions)
    _capi.check(ctx.lib.sbbseg_text_region_boxes(ctx.h, plane.ctypes.data_as(C.c_void_p), plane.shape[0], plane.shape[1], 1, 1e-5, 1.0, None, 0, C.byref(n)))
    assert n.value == len(boxes)
    two = np.full((3, 4), -7, np.int32)
    _capi.check(ctx.lib.sbbseg_text_region_boxes(ctx.h, plane.ctypes.data_as(C.c_void_p), plane.shape[0], plane.shape[1], 1, 1e-5, 1.0,
                                                 two.ctypes.data_as(C.c_void_p), 2, C.byref(n)))
    assert n.value == len(boxes) and two[:2].tolist() == boxes[:2] and (two[2] == -7).all()
    with pytest.raises(RuntimeError):
        _capi.check(ctx.lib.sbbseg_text_region_boxes(ctx.h, plane.ctypes.data_as(C.c_void_p), plane.shape[0], plane.shape[1], 1, 1e-5, 1.0, None, 2, C.byref(n)))
    r = np.zeros((1400, 1200), np.uint8)
    r[700:705, 600:605] = 1                                      # contour area 16 < 1e-5 x H x W = 16.8
    r[100:105, 100:106] = 1                                      # 20
    for kw in ({}, {"min_area": 0.0}, {"min_area": 0.0, "max_area": 17.0 / r.size}, {"min_area": 0.5}):
        assert ctx.text_region_boxes(r, 1, **kw) == stages.host_text_region_boxes(r, 1, **kw), kw
    assert ctx.text_region_boxes(r) == [[100, 100, 6, 5]]
    assert ctx.text_region_boxes(np.zeros((40, 50), np.uint8)) == []


def _old_path(ctx, textlines, box, angles):
    return ctx.deskew_profiles(slopes_ref.erode2(slopes_ref.crop_of(textlines, box)), angles)


def _check_profiles(ctx, textlines, boxes, oracle_below=0):
    out = []
    for angles in (slopes_ref.SWEEP1, slopes_ref.SWEEP2):
        got = ctx.region_deskew_profiles(textlines, boxes, angles)
        assert len(got) == len(boxes)
        for r, box in enumerate(boxes):
            ref = _old_path(ctx, textlines, box, angles)
            assert got[r].dtype == np.int32 and got[r].shape == ref.shape == (len(angles), _capi.deskew_side(box[3], box[2]))
            assert np.array_equal(got[r], ref), (box, len(angles), int(np.abs(got[r] - ref).max()), np.argwhere(got[r] != ref)[:4])
            if box[2] * box[3] <= oracle_below:                  # small ones: the CPU oracle too, with the library's own rotation matrices
                from oracle import deskew as dk
                side = ref.shape[1]
                sq = dk.padded_square(slopes_ref.erode2(slopes_ref.crop_of(textlines, box)))
                want = np.stack([(dk.warp_affine_cubic_replicate(sq, _capi.rotation_matrix(side // 2, side // 2, a)) != 0).sum(axis=1) for a in angles[::6]])
                assert np.array_equal(got[r][::6], want), box
        out.append(np.concatenate([g.reshape(-1) for g in got]).tobytes())
    return out


def test_batched_profiles_equal_the_one_region_path(model, pages):
    """(b) every fixture page and a page of 26 random boxes (5 x 5 ... 900 x 600, plane edges, the whole plane), both sweeps; (e) the
    same bytes from the first launches of a fresh handle."""
    ctx = model.ctx
    for _r, textlines, boxes, _s in pages:
        _check_profiles(ctx, textlines, boxes, oracle_below=130 * 100)
    textlines, boxes = slopes_ref.random_page()
    assert len(boxes) >= 24 and any(b[2] * b[3] == textlines.size for b in boxes)
    first = _check_profiles(ctx, textlines, boxes, oracle_below=3000)
    # erode_iterations: 0 = the plain crop, 1 = one 5 x 5 erosion
    from oracle import stage_glue as sg
    some = boxes[3:9]
    for it in (0, 1):
        got = ctx.region_deskew_profiles(textlines, some, slopes_ref.SWEEP1[::8], erode_iterations=it)
        for g, box in zip(got, some):
            crop = np.ascontiguousarray(slopes_ref.crop_of(textlines, box))
            assert np.array_equal(g, ctx.deskew_profiles(sg.morph(crop, "erode", 5, it) if it else crop, slopes_ref.SWEEP1[::8]))
    fresh = _small_model()
    try:
        again = [np.concatenate([g.reshape(-1) for g in fresh.ctx.region_deskew_profiles(textlines, boxes, a)]).tobytes()
                 for a in (slopes_ref.SWEEP1, slopes_ref.SWEEP2)]
    finally:
        fresh.release()
    assert again == first


def test_bad_boxes_are_errors_and_the_handle_survives(model, pages):
    ctx = model.ctx
    _r, textlines, boxes, _s = pages[1]
    h, w = textlines.shape
    for bad in ([0, 0, 0, 5], [-1, 0, 5, 5], [w - 4, 0, 5, 5], [0, h - 4, 5, 5]):
        with pytest.raises(RuntimeError, match="box 1"):
            ctx.region_deskew_profiles(textlines, [boxes[0], bad], slopes_ref.SWEEP2)
    assert ctx.region_deskew_profiles(textlines, [], slopes_ref.SWEEP2) == []
    assert np.array_equal(ctx.region_deskew_profiles(textlines, boxes, slopes_ref.SWEEP2)[0], _old_path(ctx, textlines, boxes[0], slopes_ref.SWEEP2))


def test_get_slopes_equals_the_reference_and_the_region_loop(model, pages):
    """(c) the fixture's slopes; and on the random page the loop that existed before: return_deskew_slope per eroded crop + clean-up."""
    ctx = model.ctx
    for k, (_r, textlines, boxes, slopes) in enumerate(pages):
        assert stages.get_slopes(textlines, boxes, ctx) == slopes, k
    assert stages.get_slopes(pages[0][1], [], ctx) == []
    textlines, boxes = slopes_ref.random_page()
    boxes = boxes[1:]                                            # (the whole plane is in the profile test; its host half alone takes seconds)
    want = [slopes_ref.cleaned(stages.return_deskew_slope(slopes_ref.erode2(slopes_ref.crop_of(textlines, b)), 2, ctx)) for b in boxes]
    got = stages.get_slopes(textlines, boxes, ctx)
    print(f"[get_slopes] random page: {len(boxes)} boxes, {sum(1 for s in got if s != 0)} non-zero slopes, {sum(1 for s in got if s <= -50)} from the second sweep")
    assert got == want


def test_run_with_slopes_at_full_size(tmp_path, monkeypatch):
    """(d) three 448 x 448 nets, a 3500 x 2500 page: run()'s four values, the boxes of its regions, the slopes of its text lines; and []
    for both when the textline model does not run."""
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
    mask, regions, textlines, page_coord, boxes, slopes = st.run_with_slopes(page)
    t = time.time() - t
    ref = st.run(page)
    assert page_coord == ref[3]
    for a, b in zip((mask, regions, textlines), ref[:3]):
        assert (a is None) == (b is None) and (a is None or np.array_equal(a, b))
    assert textlines is not None, "this page and these nets are known to find text regions"
    ctx = load_model(str(tmp_path / "model_textline_new.h5"), max_batch=108).ctx
    assert boxes == ctx.text_region_boxes(regions) == st.boxes and len(boxes) >= 1
    assert boxes == stages.host_text_region_boxes(regions)
    assert slopes == stages.get_slopes(textlines, boxes, ctx) == st.slopes and len(slopes) == len(boxes)
    print(f"[run_with_slopes] 3500 x 2500: {len(boxes)} boxes, {sum(1 for s in slopes if s != 0)} non-zero slopes, {t:.2f} s (first call)")
    # no text: the stage-by-stage run with the gate closed (main.py:2096) never runs the textline model
    monkeypatch.setenv("SBBSEG_STAGES_RESIDENT", "0")
    monkeypatch.setattr(stages.InferenceStages, "text_regions_present", lambda self, regions: False)
    out = st.run_with_slopes(synthetic_page(520, 400, seed=9))
    assert out[2] is None and out[4] == [] and out[5] == [] and st.boxes == [] and st.slopes == []
    clear_session()
