"""The line splitters on the device (-m gpu), through the C ABI: ``sbbseg_line_split_dev`` against the host twin on every field, status
and packing offset, untouched sentinels beyond every count; ``sbbseg_region_line_boxes(_dev)`` and ``stages.get_line_boxes`` against the
numpy / scipy restatement (tests/line_split_ref.py) applied to tests/lines_ref.py's masks, and against the fixture recorded from the
reference's own functions; ``run_with_line_boxes``."""
import ctypes as C

import numpy as np
import pytest

from sbb_textline_detection_amd import _capi, stages

import line_split_ref as lr
import lines_ref
import slopes_ref

pytestmark = pytest.mark.gpu
SENTINEL = -77777


@pytest.fixture(scope="module")
def model():
    from sbb_textline_detection_amd.model import SegModel
    from tools.synth_model import calibrated_model
    cfg, w = calibrated_model(2, 224, 224, seed=0)
    m = SegModel(cfg, w, device=0, max_batch=4)                  # any finalized handle: these calls do not touch the network
    yield m
    m.release()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _regions():
    """37 regions: the lengths at which the kernel takes another path (1, 2, 3; around one wave; LDS; 2049 = the first beyond
    kProfileLdsSamples), both orientations, stripes of several periods, an empty and a constant profile."""
    rng = np.random.RandomState(17)
    lengths = [1, 2, 3, 63, 64, 65, 300, 2049] * 2 + [int(v) for v in rng.randint(4, 400, 21)]
    lengths[-2:] = [300, 400]
    out = []
    for k, n in enumerate(lengths):
        period, other = int(rng.randint(5, 90)), int(rng.randint(3, 200))
        y = (((np.arange(n) + rng.randint(0, period)) % period) < 0.5 * period) * rng.randint(1, other + 1)
        if k in (20, 21):
            y = np.full(n, 0 if k == 20 else other)
        if 30 <= k < 35:
            y = y * (rng.rand(n) < 0.8)
        if k >= 35:                                              # mass at both ends only: no peak left (main.py:1288)
            y = np.zeros(n, np.int64)
            y[:3] = y[-3:] = other
        slope = float([0.0, 3.0, -12.0, 44.0][k % 4]) if (k // 8) % 2 == 0 and k < 35 else float([90.0, -60.0, 46.0, -88.0][k % 4])
        vertical = abs(slope) > 45
        w, h = (n, other) if vertical else (other, n)
        out.append((y.astype(np.int32), other, vertical, _capi.line_rotation_terms(w, h, slope)))
    return out


def _dev_raw(ctx, regions, sigma_max=_capi.LINE_SIGMA_MAX):
    profiles = [r[0] for r in regions]
    n = len(regions)
    offsets = np.concatenate([[0], np.cumsum([len(y) for y in profiles])]).astype(np.int64)
    packed = np.ascontiguousarray(np.concatenate(profiles), np.int32)
    geom = np.ascontiguousarray([[len(r[0]), r[1], int(r[2])] for r in regions], np.int32)
    rots = np.ascontiguousarray([r[3] for r in regions], np.float64)
    w, w_off = _capi.line_weight_table(sigma_max)
    total = int(((geom[:, 0].astype(np.int64) + 40) // 2).sum())
    info, line_off = np.full((n, 5), SENTINEL, np.int32), np.full(n + 1, SENTINEL, np.int64)
    lines, corners, rot = np.full((total, 3), SENTINEL, np.int32), np.full((total, 4, 2), SENTINEL, np.int32), np.full((total, 4, 2), SENTINEL, np.int32)
    _capi.check(ctx.lib.sbbseg_line_split_dev(ctx.h, C.c_void_p(ctx.stage(packed)), _p(offsets), n, _p(geom), _p(rots), _p(w), _p(w_off), int(sigma_max),
                                              _p(info), _p(line_off), _p(lines), _p(corners), _p(rot)), "sbbseg_line_split_dev")
    return info, line_off, lines, corners, rot


def _assert_dev_equals_host(ctx, regions, sigma_max=_capi.LINE_SIGMA_MAX):
    got = _dev_raw(ctx, regions, sigma_max)
    want = _capi.line_split_host_raw([r[0] for r in regions], [r[1] for r in regions], [r[2] for r in regions], [r[3] for r in regions], sigma_max)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[1], np.concatenate([[0], np.cumsum([(len(r[0]) + 40) // 2 for r in regions])]))
    for r in range(len(regions)):
        at, end, n = int(got[1][r]), int(got[1][r + 1]), int(got[0][r, 4])
        assert 0 <= n <= end - at
        for a, b in zip(got[2:], want[2:]):
            assert np.array_equal(a[at:at + n], b[at:at + n]) and (a[at:at + n] != SENTINEL).all(), r      # (no coordinate is the sentinel)
            assert (a[at + n:end] == SENTINEL).all(), r                      # nothing beyond the count was touched
    return got


def test_dev_equals_the_host_twin_in_batches_of_1_2_and_37_and_permuted(model):
    ctx = model.ctx
    regions = _regions()
    assert len(regions) == 37 and {len(r[0]) for r in regions} >= {1, 2, 3, 63, 64, 65, 300, 2049}
    info = _assert_dev_equals_host(ctx, regions)[0]
    assert {0, 1, 2, 3, 4} <= set(info[:, 3].tolist()) and {0, 1} <= set(info[:, 0].tolist()) and info[:, 2].any() and (info[:, 1] > 3).any()
    for r in (0, 7, 15, 22):
        _assert_dev_equals_host(ctx, regions[r:r + 1])
    _assert_dev_equals_host(ctx, regions[6:8])
    order = np.random.RandomState(2).permutation(len(regions))
    permuted = _assert_dev_equals_host(ctx, [regions[k] for k in order])[0]
    assert np.array_equal(permuted, info[order])                    # a region's result does not depend on its neighbours
    # the Python layer gives the restatement's records
    got = ctx.line_split_dev(ctx.stage(np.concatenate([r[0] for r in regions])), np.concatenate([[0], np.cumsum([len(r[0]) for r in regions])]),
                             [r[1] for r in regions], [r[2] for r in regions], [r[3] for r in regions])
    for a, r in zip(got, regions):
        assert lr.same(a, lr.line_split(*r))


def _as_regions(profiles, others, slopes):
    """(y, other, vertical, rotation terms) per profile, as the CPU tests form them from (profiles, others, slopes)."""
    out = []
    for y, other, slope in zip(profiles, others, slopes):
        vertical = abs(slope) > 45
        w, h = (len(y), other) if vertical else (other, len(y))
        out.append((y, other, vertical, _capi.line_rotation_terms(w, h, slope)))
    return out


def test_dev_equals_the_host_twin_on_the_cpu_tests_seeded_sweep(model):
    """The 200 seeded profiles that hold the host twin to the restatement (test_line_split_cpu.py), in one batch."""
    regions = _as_regions(*lr._random_profiles())
    info = _assert_dev_equals_host(model.ctx, regions)[0]
    assert len(regions) == 200 and {0, 2, 3, 4} <= set(info[:, 3].tolist()) and info[:, 2].any() and {lr.OK, lr.NONE} <= set(info[:, 0].tolist())
    assert (info[:, 1] > 12).any()


def test_dev_equals_the_host_twin_on_the_cpu_tests_edge_profiles(model):
    """Mass at both ends only; a long, a zero, a constant and a one-sample profile."""
    ctx = model.ctx
    info = _assert_dev_equals_host(ctx, _as_regions(*lr.both_ends_profiles()))[0]
    for k in range(0, 6, 2):
        assert info[k, [0, 3, 4]].tolist() == [lr.OK, 1, 0] and info[k, 1] > 5 and info[k + 1, [0, 3]].tolist() == [lr.NONE, -1]
    info = _assert_dev_equals_host(ctx, _as_regions(*lr.long_zero_constant_profiles()))[0]
    assert info[0, 4] == 30 and info[1, 4] == 30 and info[2, 0] == lr.NONE and info[3, 2] == 1


def test_dev_equals_the_host_twin_beyond_64_lines(model):
    """More than 64 peaks in one profile and more than 64 lines in one region (the line kernel walks its lines 64 at a time), on the LDS form
    (1500, 2048) and on the global-workspace form (2049, 3000)."""
    ctx = model.ctx
    regions = _as_regions(*lr.striped_profiles())
    info = _assert_dev_equals_host(ctx, regions)[0]
    print("[test_gpu_line_split] striped profiles: lines per region", info[:, 4].tolist())
    assert (info[:, 0] == lr.OK).all() and (info[:, 4] > 64).all()
    assert info[:, 4].tolist() == list(lr.STRIPED_LINES)
    vertical = _as_regions(lr.striped_profiles()[0], [40] * 4, [80.0] * 4)
    assert (_assert_dev_equals_host(ctx, vertical)[0][:, 4] > 64).all()


def test_sigma_beyond_the_table_is_reported_by_the_device_and_finished_on_the_host(model):
    """SBBSEG_LINES_SIGMA_TOO_LARGE: info only, nothing else written; the Python layer finishes the region with the host twin."""
    ctx = model.ctx
    regions = _regions()
    # a table that ends at sigma 12: every region with a larger sigma_gaus stops after the first estimate, on device and host alike
    small = _assert_dev_equals_host(ctx, regions, sigma_max=12)[0]
    full = _assert_dev_equals_host(ctx, regions)[0]               # (and back: the handle takes the other table)
    big = full[:, 1] > 12
    assert big.sum() >= 3 and (~big).sum() >= 3 and (small[big, 0] == _capi.LINES_SIGMA_TOO_LARGE).all() and (small[big, 4] == 0).all()
    assert np.array_equal(small[big, 1:3], full[big, 1:3]) and (small[big, 3] == -1).all() and np.array_equal(small[~big], full[~big])
    packed = np.concatenate([r[0] for r in regions])
    offsets = np.concatenate([[0], np.cumsum([len(r[0]) for r in regions])])
    got = ctx.line_split_dev(ctx.stage(packed), offsets, [r[1] for r in regions], [r[2] for r in regions], [r[3] for r in regions], sigma_max=12)
    for a, r in zip(got, regions):
        assert lr.same(a, lr.line_split(*r))
    # a sigma beyond the device's own table (128): two stripes 1000 samples apart on the long form
    y = np.zeros(2049, np.int32)
    y[500:560] = y[1500:1560] = 30
    far = [(y, 30, False, _capi.line_rotation_terms(30, 2049, 1.0)), regions[6], (y, 30, True, _capi.line_rotation_terms(2049, 30, 70.0))]
    info = _assert_dev_equals_host(ctx, far)[0]
    assert info[0].tolist() == [_capi.LINES_SIGMA_TOO_LARGE, 175, 0, -1, 0] and info[2, 0] == _capi.LINES_SIGMA_TOO_LARGE and info[1, 0] == _capi.LINES_OK
    got = ctx.line_split_dev(ctx.stage(np.concatenate([r[0] for r in far])), np.cumsum([0] + [len(r[0]) for r in far]), [r[1] for r in far],
                             [r[2] for r in far], [r[3] for r in far])
    for a, r in zip(got, far):
        want = lr.line_split(*r)
        assert lr.same(a, want) and want["status"] == lr.OK and len(want["peaks"]) >= 1
    # the same through the box entry points: wide and narrow stripes, a table that ends at 12
    plane = np.zeros((460, 300), np.uint8)
    for top in range(10, 460, 110):
        plane[top:top + 40, 10:140] = 1
    for top in range(6, 460, 24):
        plane[top:top + 12, 160:290] = 1
    boxes, slopes = [[0, 0, 150, 460], [150, 0, 150, 460], [0, 0, 150, 460]], [0.0, 1.0, 60.0]
    want = ctx.region_line_boxes(plane, boxes, slopes)
    sigmas = [w["sigma"] for w in want]
    assert min(sigmas) <= 12 < max(sigmas), sigmas
    for got in (ctx.region_line_boxes(plane, boxes, slopes, sigma_max=12), ctx.region_line_boxes_dev(ctx.stage(plane), 460, 300, boxes, slopes, sigma_max=12)):
        for a, b, box, slope in zip(got, want, boxes, slopes):
            _dst, rows, cols = lines_ref.line_mask(slopes_ref.crop_of(plane, box), slope)
            vertical = abs(slope) > 45
            ref = lr.line_split(cols if vertical else rows, box[3] if vertical else box[2], vertical, _capi.line_rotation_terms(box[2], box[3], slope))
            assert lr.same(a, b) and lr.same(a, ref), (box, slope)


def test_fixture_pages_equal_the_restatement_and_the_fixture(model):
    ctx = model.ctx
    cases = {(c["page"], c["box"]): c for c in lr.load_golden()}
    golden = lines_ref.load_golden()
    for k, ((_r, textlines, boxes, _s), (slopes, _masks, _v)) in enumerate(zip(slopes_ref.load_pages(), golden)):
        want = []
        for box, slope in zip(boxes, slopes):
            dst, rows, cols = lines_ref.line_mask(slopes_ref.crop_of(textlines, box), slope)
            vertical = abs(slope) > 45
            want.append(lr.line_split(cols if vertical else rows, box[3] if vertical else box[2], vertical, _capi.line_rotation_terms(box[2], box[3], slope)))
        before = ctx.line_mask_launches()
        for got in (ctx.region_line_boxes(textlines, boxes, slopes), ctx.region_line_boxes_dev(ctx.stage(textlines), *textlines.shape, boxes, slopes),
                    stages.get_line_boxes(textlines, boxes, slopes, ctx), stages.get_slopes_and_line_boxes(textlines, boxes, ctx)[1]):
            assert len(got) == len(boxes)
            for r in range(len(boxes)):
                assert lr.same(got[r], want[r]) and lr.same(got[r], cases[(k, r)]), (k, r)
        assert ctx.line_mask_launches() - before == 4 * 11          # ten for the masks and one for the split, whatever the number of boxes
    assert ctx.region_line_boxes(textlines, [], []) == [] and stages.get_line_boxes(textlines, [], [], ctx) == []
    assert stages.get_slopes_and_line_boxes(textlines, [], ctx) == ([], [])
    with pytest.raises(RuntimeError, match="box 1"):
        ctx.region_line_boxes(textlines, [boxes[0], [0, 0, 0, 5]], [0.0, 0.0])


def test_run_with_line_boxes_keeps_run_with_lines_values(tmp_path):
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
    out = st.run_with_line_boxes(page)
    ref = st.run_with_lines(page)
    assert len(out) == 8 and out[3] == ref[3] and out[4] == ref[4] and out[5] == ref[5] and out[7] is st.line_boxes
    for a, b in zip(out[:3], ref[:3]):
        assert (a is None) == (b is None) and (a is None or np.array_equal(a, b))
    assert len(out[6]) == len(ref[6]) == len(out[4]) >= 1 and len(out[7]) == len(out[4])
    for a, b in zip(out[6], ref[6]):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for box, slope, (_m, rows, cols), rec in zip(out[4], out[5], out[6], out[7]):
        vertical = abs(slope) > 45
        want = lr.line_split(cols if vertical else rows, box[3] if vertical else box[2], vertical, _capi.line_rotation_terms(box[2], box[3], slope))
        assert lr.same(rec, want), (box, slope)
    clear_session()
