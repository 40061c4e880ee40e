"""The text-line x extents on the device (-m gpu; csrc/line_extent.hip) against the library's serial host twin, field by field.  The host
twin runs the same line_extent.h and tests/test_line_extent_cpu.py holds it to the literal restatement of the OpenCV text, so a difference
here is the device's: the row-parallel fill, the ballot-packed warp, the wave's word search in the border scan (in LDS and on the global
workspace), the staged winner points, the wave reduction over the samples.  Every shape runs with the LDS limit as it is and lowered to 0."""
import time

import numpy as np
import pytest

import line_extent_cases as cases

pytestmark = pytest.mark.gpu
T0 = time.time()
S = cases.SENTINEL
GRID = cases.grid_cases()
RAW = cases.raw_masks()


@pytest.fixture(scope="module")
def ctx():
    from sbb_textline_detection_amd.model import SegModel
    from tools.synth_model import calibrated_model
    cfg, w = calibrated_model(2, 224, 224, seed=0)
    m = SegModel(cfg, w, device=0, max_batch=4)                    # any finalized handle: these calls do not touch the network
    yield m.ctx
    m.ctx.set_extent_lds_limit(60 * 1024)
    m.release()
    print(f"[test_gpu_line_extent] module wall time {time.time() - T0:.1f} s")


@pytest.fixture(scope="module")
def host_grid():
    """The host twin's record of every grid case, computed once."""
    from sbb_textline_detection_amd import _capi
    return [_capi.host_region_line_extents(c["ring"], c["box"], c["slope"], c["record"], want_masks=True) for c in GRID]


def run_dev(ctx, group):
    return ctx.region_line_extents_raw([c["box"] for c in group], [c["slope"] for c in group], [c["record"] for c in group],
                                       [c["ring"] for c in group], fill=S)


def same_region(ctx, r, case, tables, want, read=True):
    """Region r of a device call against the host twin's record `want`: every field, and the sentinel beyond every count."""
    line_off, extent, corners, corners_rot, rec = tables
    wc, name = want["contour"], case["name"]
    got = dict(zip(("status", "borders", "points", "is_hole", "tie", "sx", "sy", "holes"), (int(v) for v in rec[r])))
    assert (got["status"], got["borders"], got["holes"]) == (wc["status"], wc["borders"], wc["holes"]), name
    at, cap, cnt = int(line_off[r]), int(line_off[r + 1] - line_off[r]), len(case["record"]["peaks"])
    assert (extent[at + cnt:at + cap] == S).all() and (corners[at + cnt:at + cap] == S).all() and (corners_rot[at + cnt:at + cap] == S).all(), name
    w, h = int(case["box"][2]), int(case["box"][3])
    if read:
        thr, winner = ctx.region_line_extents_read(r, w, h, got["points"])
        assert np.array_equal(thr, wc["threshrot"]), name
    if wc["status"] != 0:
        assert got["points"] == 0 and (extent[at:at + cnt] == [0, w]).all() and (corners[at:at + cnt] == S).all(), name
        return
    assert (got["points"], bool(got["is_hole"]), bool(got["tie"]), (got["sx"], got["sy"])) == (wc["points"], wc["is_hole"], wc["tie"], wc["start"]), name
    if read:
        assert np.array_equal(winner, wc["winner"]), name
    assert np.array_equal(extent[at:at + cnt], want["extent"]), name
    # (the host twin's record carries the sentinel corners where the step does not rewrite them)
    assert np.array_equal(corners[at:at + cnt], want["boxes"]) and np.array_equal(corners_rot[at:at + cnt], want["boxes_rot"]), name


@pytest.mark.parametrize("limit", [60 * 1024, 0], ids=["lds", "global"])
def test_device_equals_host_twin_on_every_shape(ctx, host_grid, limit):
    """Widths 1 .. 130 x heights 1 .. 40 x the eight slopes (rectangles and traced blobs) and the named rings (one point, two-point line,
    rectangle, L, U, one-pixel neck, diamond, blobs), all in ONE call."""
    ctx.set_extent_lds_limit(limit)
    before = ctx.extent_launches()
    tables = run_dev(ctx, GRID)
    assert ctx.extent_launches() - before == 5                     # fill, warp, two scan passes of the one form in use, extents
    kinds = set()
    for r, (case, want) in enumerate(zip(GRID, host_grid)):
        same_region(ctx, r, case, tables, want)
        rewritten = abs(case["slope"]) <= 45 and case["record"]["branch"] != 2 and want["contour"]["status"] == 0
        if rewritten and any(tuple(e) != (0, int(case["box"][2])) for e in want["extent"].tolist()):
            kinds.add("cut")
        if want["contour"]["holes"]:
            kinds.add("hole")
        if want["contour"]["is_hole"]:
            kinds.add("hole wins")
        if abs(case["slope"]) > 45:
            kinds.add("vertical")
    assert kinds >= {"cut", "hole", "vertical"}, kinds            # (the grid must not be trivial)


def test_both_forms_in_one_call(ctx, host_grid):
    """A limit between the shapes' sizes: small regions scan in LDS, large ones on the workspace, in the same call: 7 launches."""
    ctx.set_extent_lds_limit(1024)
    before = ctx.extent_launches()
    tables = run_dev(ctx, GRID)
    assert ctx.extent_launches() - before == 7
    for r, (case, want) in enumerate(zip(GRID, host_grid)):
        same_region(ctx, r, case, tables, want, read=False)


@pytest.mark.parametrize("limit", [60 * 1024, 0], ids=["lds", "global"])
def test_border_scan_on_raw_masks(ctx, limit):
    from sbb_textline_detection_amd import _capi
    ctx.set_extent_lds_limit(limit)
    names = sorted(RAW)
    got = ctx.debug_mask_border_winner([RAW[n] for n in names])
    for name, g in zip(names, got):
        want = _capi.host_mask_border_winner(RAW[name])
        assert {k: v for k, v in g.items() if k != "winner"} == {k: v for k, v in want.items() if k != "winner"}, name
        assert np.array_equal(g["winner"], want["winner"]), name
    by = dict(zip(names, got))
    assert by["empty"]["status"] == _capi.EXTENT_NONE and by["one_pixel"]["points"] == 1
    assert by["hollow_octagon"]["tie"] and by["hollow_octagon"]["is_hole"] and by["ragged_inside"]["is_hole"] and not by["ragged_inside"]["tie"]
    assert by["many_holes"]["holes"] == 6 * 22 and by["two_equal"]["tie"] and by["two_equal"]["start"] == (30, 4)


def test_one_region_alone_equals_the_same_region_among_37(ctx, host_grid):
    ctx.set_extent_lds_limit(60 * 1024)
    pick = next(k for k, c in enumerate(GRID) if c["name"].startswith("neck/12"))
    others = [k for k in range(0, len(GRID), 9) if k != pick][:36]
    group = others[:20] + [pick] + others[20:]
    assert len(group) == 37
    before = ctx.extent_launches()
    alone = run_dev(ctx, [GRID[pick]])
    mid = ctx.extent_launches()
    many = run_dev(ctx, [GRID[k] for k in group])
    assert mid - before == ctx.extent_launches() - mid == 5        # the launches do not grow with the regions
    a0, a1 = int(many[0][20]), int(many[0][21])
    assert np.array_equal(alone[1], many[1][a0:a1]) and np.array_equal(alone[2], many[2][a0:a1]) and np.array_equal(alone[3], many[3][a0:a1])
    assert np.array_equal(alone[4][0], many[4][20])
    for r, k in enumerate(group):
        same_region(ctx, r, GRID[k], many, host_grid[k], read=False)


def test_resident_contour_table_is_read_in_place(ctx):
    """Rings traced on the device and left resident (points_xy = NULL) give what the same rings give when they are passed in."""
    plane = np.zeros((90, 200), np.uint8)
    plane[5:40, 10:90] = 1
    plane[20:30, 30:60] = 0
    plane[50:85, 100:190] = 1
    plane[60, 150:199] = 0
    boxes, contours = ctx.debug_mask_contours_dev(ctx.stage(plane), 90, 200)
    assert len(contours) >= 2
    slopes = [3.0 * ((-1) ** k) for k in range(len(boxes))]
    records = [cases.record(b[3], 4) for b in boxes]
    resident = ctx.region_line_extents_raw(boxes, slopes, records, None, fill=S)
    passed = ctx.region_line_extents_raw(boxes, slopes, records, contours, fill=S)
    assert all(np.array_equal(a, b) for a, b in zip(resident, passed))
    with pytest.raises(RuntimeError, match="the handle holds"):
        ctx.region_line_extents_raw(boxes[:1], slopes[:1], records[:1], None)


def test_bad_rings_are_errors_that_name_the_region(ctx):
    good = GRID[0]
    for ring, what in (([[0, 0], [5, 2], [0, 4]], "not horizontal, vertical or an exact diagonal"), ([[0, 0], [12, 0], [12, 4], [0, 4]], "outside its box")):
        bad = {"ring": np.array(ring, np.int32), "box": np.array([0, 0, 10, 10], np.int32), "slope": 0.0, "record": cases.record(10, 4, 1)}
        with pytest.raises(RuntimeError, match="region 1.*" + what):
            run_dev(ctx, [good, bad, good])
    with pytest.raises(RuntimeError, match="no extents on this handle"):
        ctx.region_line_extents_read(0, 10, 10, 0)


def test_fixture_of_the_reference_on_the_device(ctx):
    """tests/golden/line_extent_golden.npz (the reference's own textline_contours_postprocessing on cv2 stubs; a self-consistency fixture):
    all its regions in one call give the polygons the reference returned."""
    from sbb_textline_detection_amd import _capi
    ctx.set_extent_lds_limit(60 * 1024)
    golden = cases.golden_cases()
    got = ctx.region_line_extents_dev([c["box"] for c in golden], [c["slope"] for c in golden], [c["record"] for c in golden], [c["ring"] for c in golden])
    for c, g in zip(golden, got):
        polygons = g["boxes_rot"] if g["status"] == _capi.LINES_OK else g["boxes_rot"][:0]
        assert g["contour"]["status"] == c["status"] and g["contour"]["holes"] == c["holes"] and np.array_equal(polygons, c["polygons"]), c["name"]
