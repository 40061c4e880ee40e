"""The device's connected-component labelling (-m gpu) against scipy on the adversarial planes of tests/cc_planes.py: the three product
calls that rest on the lock-free union-find of csrc/page_glue.hip -- sbbseg_page_box_dev, sbbseg_text_regions_present_dev and
sbbseg_text_region_boxes[_dev] -- must give what ``slopes_ref.oracle_boxes`` (scipy.ndimage.label, the 4-connected background, the
oracle's contour area) and ``oracle.stage_glue.page_box`` give.  Every comparison is exact equality, box order included.
tests/test_cc_planes_cpu.py shows that the planes hold the structures they are named after and that the library's host mirror agrees
with the same oracle, so a failure here is the device's."""
import time

import numpy as np
import pytest

from oracle import stage_glue as sg

import cc_planes

pytestmark = pytest.mark.gpu
T0 = time.time()
REGION = cc_planes.region_families()
PAGE = cc_planes.page_families()
_REGION_STATS, _PAGE_STATS = {}, {}


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
    print(f"[test_gpu_components] module wall time {time.time() - T0:.1f} s")


def _windows(name):
    return ((0.0, 1.0), (1e-5, 1.0), cc_planes.interior_window(name))


def _region_answers(ctx, name, plane, lo, hi):
    """The three forms of the boxes call and the gate, each against the oracle; returns the oracle's boxes and how many of the three boxes
    calls traced contours on the host."""
    want = cc_planes.oracle_region_boxes(name, lo, hi)
    before = ctx.host_contour_calls()
    assert ctx.text_region_boxes(plane, 1, min_area=lo, max_area=hi) == want, (name, lo, hi)
    d = ctx.stage(plane)
    assert ctx.text_region_boxes_dev(d, plane.shape[0], plane.shape[1], 1, lo, hi) == want, (name, lo, hi, "dev")
    assert ctx.text_region_boxes(np.repeat(plane[:, :, None], 3, axis=2), 1, min_area=lo, max_area=hi) == want, (name, lo, hi, "three channels")
    traced = ctx.host_contour_calls() - before
    assert ctx.text_regions_present(plane, 1, lo) == (len(cc_planes.oracle_region_boxes(name, lo, 1.0)) > 0), (name, lo, "present")
    return want, traced


def _region_family(ctx, family):
    """Every plane of the family at the three windows, and with the host tracing forced; cached per family.  Returns the printed figures:
    (planes, components, kept boxes, boxes calls that traced on the host at the open window, at the interior windows)."""
    if family in _REGION_STATS:
        return _REGION_STATS[family]
    from scipy import ndimage
    components = kept = open_traced = interior_traced = 0
    for name, plane in REGION[family].items():
        components += ndimage.label(cc_planes.region_mask(plane) > 0, structure=np.ones((3, 3), int))[1]
        for k, (lo, hi) in enumerate(_windows(name)):
            want, traced = _region_answers(ctx, name, plane, lo, hi)
            if k == 0:
                kept += len(want)
                open_traced += traced
            elif k == 2:
                interior_traced += traced
        ctx.set_conv_variant(1 << 21)                            # test hook: every candidate is traced on the host
        try:
            before = ctx.host_contour_calls()
            assert ctx.text_region_boxes(plane, 1, min_area=0.0, max_area=1.0) == cc_planes.oracle_region_boxes(name, 0.0, 1.0), (name, "forced")
            assert ctx.host_contour_calls() > before or not cc_planes.oracle_region_boxes(name, 0.0, 1.0), (name, "the hook did not trace")
        finally:
            ctx.set_conv_variant(0)
    stats = (len(REGION[family]), components, kept, open_traced, interior_traced)
    print(f"[regions:{family}] {stats[0]} planes, {components} components, {kept} kept boxes, host tracings: {open_traced} at (0, 1), "
          f"{interior_traced} at the interior windows")
    _REGION_STATS[family] = stats
    return stats


def _page_family(ctx, family):
    if family in _PAGE_STATS:
        return _PAGE_STATS[family]
    from scipy import ndimage
    components = traced = 0
    for name, plane in PAGE[family].items():
        components += ndimage.label(cc_planes.page_mask(plane) > 0, structure=np.ones((3, 3), int))[1]
        before = ctx.host_contour_calls()
        got = ctx.page_box_dev(ctx.stage(plane), plane.shape[0], plane.shape[1])
        traced += ctx.host_contour_calls() - before
        assert got == sg.page_box(plane), (name, got, sg.page_box(plane))
    stats = (len(PAGE[family]), components, traced)
    print(f"[page box:{family}] {stats[0]} planes, {components} components, host tracings: {traced}")
    _PAGE_STATS[family] = stats
    return stats


@pytest.mark.parametrize("family", list(REGION))
def test_region_calls_equal_scipy(model, family):
    """sbbseg_text_region_boxes (one and three channels), sbbseg_text_region_boxes_dev and sbbseg_text_regions_present_dev on every plane of
    the family, for (min_area, max_area) = (0, 1), (1e-5, 1) and a window between the plane's own areas; (0, 1) again with host tracing."""
    _region_family(model.ctx, family)


@pytest.mark.parametrize("family", list(PAGE))
def test_page_box_equals_scipy(model, family):
    """sbbseg_page_box_dev: box and pixel count of oracle.stage_glue.page_box."""
    _page_family(model.ctx, family)


def test_empty_planes_give_zeros(model):
    ctx = model.ctx
    for plane in PAGE["empty"].values():
        assert ctx.page_box_dev(ctx.stage(plane), plane.shape[0], plane.shape[1]) == ((0, 0, 0, 0), 0)
    zero = REGION["narrow"]["all_zero"]
    assert ctx.text_region_boxes(zero, 1, min_area=0.0) == [] and ctx.text_regions_present(zero, 1, 0.0) is False


def test_both_the_device_decided_and_the_host_traced_path_ran(model):
    """sbbseg_debug_counter 0 counts the calls that traced contours on the host.  With the window (0, 1) every component's two bounds lie
    inside it, so nothing is traced; a window a quarter pixel wide around the spiral's area leaves it undecided.  For the page box: equal
    solid blobs are decided on the device (the cell count of a component without holes is exact and ties go to the later root), the
    notched lattice leaves all 288 others undecided."""
    ctx = model.ctx
    regions = {f: _region_family(ctx, f) for f in REGION}
    pages = {f: _page_family(ctx, f) for f in PAGE}
    assert all(s[3] == 0 for s in regions.values()), regions
    assert regions["paths"][4] > 0 and regions["rings"][4] > 0 and regions["rivals"][4] > 0, regions
    assert pages["diagonal"][2] == 0 and pages["chunks"][2] == 0 and pages["lattice"][2] >= 1, pages
    lattice = PAGE["lattice"]
    for name, traced in (("lattice_equal", 0), ("lattice_one_apart", 0), ("lattice_notched", 1)):
        before = ctx.host_contour_calls()
        ctx.page_box_dev(ctx.stage(lattice[name]), *lattice[name].shape)
        assert ctx.host_contour_calls() - before == traced, name


def test_the_winner_among_more_rivals_than_the_device_lists(model):
    """rivals_ring_last (tests/test_cc_planes_cpu.py checks the figures): the device's best is a block of contour area 182, 288 others
    stay undecided -- more than the 250 roots the device hands back, so the host must scan the label plane for every root -- and the true
    winner, a ring of area 196 with a lower bound of 162, is the last of them.  The gate at a threshold between the two areas is open only
    if that ring was traced."""
    ctx = model.ctx
    plane = REGION["rivals"]["rivals_ring_last"]
    total = float(plane.size)
    for need, want in ((150.0, True), (190.0, True), (196.0, True), (196.5, False)):
        assert (len(cc_planes.oracle_region_boxes("rivals_ring_last", need / total, 1.0)) > 0) is want
        before = ctx.host_contour_calls()
        assert ctx.text_regions_present(plane, 1, need / total) is want, need
        assert ctx.host_contour_calls() - before == 1, need                              # undecided rivals: traced whatever the threshold


def test_answers_repeat(model):
    """Three times each (the round-5 race ranked equal blobs differently from run to run): the same answer, the oracle's."""
    ctx = model.ctx
    for name in ("spiral", "comb"):
        plane = REGION["paths"][name]
        lo, hi = cc_planes.interior_window(name)
        for lo_hi in ((0.0, 1.0), (lo, hi)):
            want = cc_planes.oracle_region_boxes(name, *lo_hi)
            for it in range(3):
                assert ctx.text_region_boxes(plane, 1, min_area=lo_hi[0], max_area=lo_hi[1]) == want, (name, it)
    d = None
    for name in ("lattice_equal", "lattice_one_apart", "lattice_notched"):
        plane = PAGE["lattice"][name]
        want = sg.page_box(plane)
        d = ctx.stage(plane)
        for it in range(3):
            assert ctx.page_box_dev(d, *plane.shape) == want, (name, it)
    plane = REGION["rivals"]["rivals_ring_last"]
    for it in range(3):
        assert ctx.text_regions_present(plane, 1, 190.0 / plane.size) is True, it


def _large_small_large(ctx):
    """The entry points on a large plane, a small one and the large one again: the scratch planes are reused at the larger capacity."""
    out = []
    order = (("spiral", "lattice_notched"), ("narrow_3x40", "chunk_2x129_51_76"), ("rings_channel", "diag_down_left"), ("spiral", "lattice_notched"))
    for region_name, page_name in order:
        plane = cc_planes._region_plane(region_name)
        lo, hi = cc_planes.interior_window(region_name)
        page = next(p[page_name] for p in PAGE.values() if page_name in p)
        out.append((region_name, ctx.text_region_boxes(plane, 1, min_area=0.0), ctx.text_region_boxes(plane, 1, min_area=lo, max_area=hi),
                    ctx.text_regions_present(plane, 1, lo), page_name, ctx.page_box_dev(ctx.stage(page), *page.shape)))
    return out


def test_answers_do_not_depend_on_what_ran_before(model):
    first = _large_small_large(model.ctx)
    assert first[0] == first[3]
    for region_name, everything, inside, present, page_name, box in first:
        lo, hi = cc_planes.interior_window(region_name)
        assert everything == cc_planes.oracle_region_boxes(region_name, 0.0, 1.0), region_name
        assert inside == cc_planes.oracle_region_boxes(region_name, lo, hi), region_name
        assert present == (len(cc_planes.oracle_region_boxes(region_name, lo, 1.0)) > 0), region_name
        assert box == sg.page_box(next(p[page_name] for p in PAGE.values() if page_name in p)), page_name
    fresh = _small_model()
    try:
        assert _large_small_large(fresh.ctx) == first
    finally:
        fresh.release()
