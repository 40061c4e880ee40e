"""The adversarial rotation cases (tests/rotation_cases.py) without a GPU: the conditions that keep tests/test_gpu_rotations.py from
being vacuous, asserted on the numpy oracles and the library's host-only entry points, so that an edit of the case list that empties a
class fails here; and the line-mask host twin (csrc/line_mask.h on the CPU) against tests/lines_ref.py on every line-mask case."""
import numpy as np
import pytest

from oracle import deskew as dk
from sbb_textline_detection_amd import _capi

import lines_ref
import rotation_cases as rc
import slopes_ref


def _geometry(h, w):
    """S, top, left and the `clip` condition of region_sweep (csrc/stage_glue.hip), restated."""
    S = int(max(h, w) * 1.4)
    cp = int(S / 2.0)
    top, left = cp - int(h / 2.0), cp - int(w / 2.0)
    clip = top >= 1 and left >= 1 and top + h <= S - 1 and left + w <= S - 1
    return S, top, left, clip


def _matrix(shape, angle):
    S = rc.side_of(*shape)
    return _capi.rotation_matrix(S // 2, S // 2, angle)


def test_the_lists_hold_what_the_gpu_tests_rely_on():
    assert len(rc.KINDS) == 11 and len(set(rc.ANGLES)) == len(rc.ANGLES) == 31
    for a in (0, 90, -90, 180, 270, 360, 45, -45, 45.0001, 1e-9, -1e-9, 1e-4, 89.99999, 90.00001, -25, 25, -50):
        assert a in rc.ANGLES
    assert set(slopes_ref.SWEEP1[[0, -1]]) | set(slopes_ref.SWEEP2[[0, -1]]) <= set(rc.ANGLES) and 45.0001 in lines_ref.SLOPES
    assert all(-180 < a < 180 for a in rc.RANDOM_ANGLES) and len(rc.RANDOM_ANGLES) == 12
    assert sorted(s for ss in rc.SHAPE_CLASSES.values() for s in ss) == sorted(rc.SHAPES) == sorted(rc.PLANE_OF)
    assert max(max(s) for s in rc.SHAPES) <= 320
    cases = rc.line_cases()
    assert sorted((c.kind, c.shape) for c in cases) == sorted((k, s) for k in rc.KINDS for s in rc.SHAPES)
    sweep = rc.sweep_cases()
    assert {c.shape for c in sweep} == set(rc.SHAPES) and all(c in sweep for c in rc.one_per_shape_class())
    for shape in rc.SHAPES:                                      # every shape runs the sweep with an all-ones crop or with random bytes
        assert {c.kind for c in sweep if c.shape == shape} & {"ones", "bytes"}
    assert {rc.side_of(*c.shape) for c in sweep} >= {62, 64, 65, 127, 128, 130, 448}
    assert not any(int(m * 1.4) in (63, 129) for m in range(1, 321))                  # (no box has a square of side 63 or 129)
    assert {rc.side_of(*c.shape) % 8 for c in sweep} >= {0, 1, 4, 7}
    # a ragged last group of 8 rows on a square of more than one group, for each residue that has one
    assert {rc.side_of(*c.shape) % 8 for c in sweep if rc.side_of(*c.shape) > 8} >= {0, 1, 4, 7}
    clips = {shape: _geometry(*shape)[3] for shape in rc.SHAPES}
    assert [s for s in rc.SHAPES if not clips[s]] == rc.TINY and all(clips[s] for s in rc.FIRST_CLIPPED)
    for c in cases:                                              # the crops are what their names say
        crop = rc.crop_of(c)
        assert crop.shape == c.shape and crop.any(), c
    assert set(np.unique(np.concatenate([rc.crop_of(c).ravel() for c in cases if c.kind == "wrap"]))) == set(rc.WRAP_BYTES)
    assert len(np.unique(np.concatenate([rc.crop_of(c).ravel() for c in cases if c.kind == "bytes"]))) == 256
    assert all((rc.crop_of(c) == 255).all() for c in cases if c.kind == "full")


def test_the_planes_and_the_pooled_boxes():
    planes = rc.planes()
    assert len({p.shape[1] for p in planes}) == 3
    assert planes[0].shape[1] == max(c.box[2] for c in rc.line_cases(0)) + 1
    for k, p in enumerate(planes):
        H, W = p.shape
        boxes = [c.box for c in rc.line_cases(k)]
        assert all(x >= 0 and y >= 0 and x + w <= W and y + h <= H for x, y, w, h in boxes)
        assert any(b[0] == 0 for b in boxes) and any(b[1] == 0 for b in boxes)
        assert any(b[0] + b[2] == W for b in boxes) and any(b[1] + b[3] == H for b in boxes)
        areas = [b[2] * b[3] for b in boxes]                     # call order: small and large neighbours
        assert sum(1 for a, b in zip(areas, areas[1:]) if min(a, b) <= 36 and max(a, b) >= 1000) >= 20
    boxes, box_plane = rc.pooled_case()
    small = [b[2] <= 3 and b[3] <= 3 for b in boxes]
    run = best = 0
    for r, s in enumerate(small):
        run = run + 1 if s and (run == 0 or box_plane[r] != box_plane[r - 1]) else int(s)
        best = max(best, run)
    assert best >= 200                                           # consecutive tiny boxes, each on another plane than the one before
    assert sum(1 for s in small if not s) == len(rc.POOLED_LARGE) and not small[0] and not small[-26]
    assert {(b[3], b[2]) for b, s in zip(boxes, small) if s} == {(1, 1), (2, 2), (3, 3), (1, 3), (3, 1), (2, 3)}
    for k, p in enumerate(planes):
        mine = [b for b, q in zip(boxes, box_plane) if q == k]
        assert any(b[0] == 0 and b[1] == 0 for b in mine) and any(b[0] + b[2] == p.shape[1] and b[1] == 0 for b in mine)
    # the tiny crops differ from each other, and a crop read from the same place of another plane would differ
    crops = [slopes_ref.crop_of(planes[k], b) for b, k, s in zip(boxes, box_plane, small) if s]
    assert sum(1 for c in crops if c.any()) >= 100 and sum(1 for c in crops if not c.all()) >= 100
    other = [slopes_ref.crop_of(planes[(k + 1) % 3], b) for b, k, s in zip(boxes, box_plane, small) if s]
    assert sum(1 for a, b in zip(crops, other) if a.shape != b.shape or not np.array_equal(a, b)) >= 100


def test_the_inverse_maps_meet_every_branch_of_the_span():
    """|m0| < 1e-7 and |m3| < 1e-7 take clip_span's `all x or none` branch; 1e-7 <= |m3| < 2e-7 is its first division."""
    seen = set()
    for a in rc.ANGLES:
        m = dk.invert_affine(_matrix((37, 90), a)).reshape(-1)
        for name, hit in (("m0 ~ 0", abs(m[0]) < 1e-7), ("m3 ~ 0", abs(m[3]) < 1e-7), ("m3 just above", 1e-7 <= abs(m[3]) < 2e-7),
                          ("m3 ~ 1", abs(m[3]) > 0.99)):
            if hit:
                seen.add(name)
    assert seen == {"m0 ~ 0", "m3 ~ 0", "m3 just above", "m3 ~ 1"}
    below, above = (abs(dk.invert_affine(_matrix((37, 90), a))[1, 0]) for a in (5.72e-6, 5.74e-6))
    assert 0 < below < 1e-7 <= above < 2e-7
    # the x scale of the one-region test: the inverse the oracle computes is exactly 2049 / 2048, the row origin -15
    inv = dk.invert_affine(rc.x_scale_matrix())
    assert inv[0, 0] == 2049.0 / 2048.0 and inv[0, 1] == 0 and inv[1, 0] == 0 and inv[1, 1] == 1 and inv[1, 2] == 0
    assert np.rint(inv[0, 2] * 1024) == -31
    sx, _sy, ax, _ay = dk.source_coords(inv, 60, 60)
    assert (sx[0, 29], ax[0, 29]) == (28, 31) and (inv[0, 0] * 29 * 1024) % 1 == 0.5


@pytest.mark.parametrize("plane", [0, 1, 2])
def test_every_sweep_case_has_a_profile_and_the_ones_reach_their_edge(plane):
    """Every sweep case counts something at every angle.  All-ones crops with the analytic span on (squares up to 130): at every general
    angle up to 25 degrees some row's outermost counted pixel has a 4 x 4 window that holds exactly ONE column of the crop -- the pixel a
    span one too tight would lose."""
    general = [a for a in rc.ANGLES if 1e-3 < abs(a) <= 25]
    assert len(general) >= 3 and sum(1 for a in rc.ANGLES if abs(a) <= 25) >= 9
    edge_cases = 0
    for c in rc.sweep_cases(plane):
        h, w = c.shape
        S, top, left, clip = _geometry(h, w)
        crop = rc.crop_of(c)
        for a in rc.ANGLES:
            assert rc.sweep_reference(c, 0, a, _matrix(c.shape, a)).sum() > 0, (c, a)
        if c.kind != "ones" or not clip or S > 130:
            continue
        edge_cases += 1
        for a in general:
            M = _matrix(c.shape, a)
            counted = dk.warp_affine_cubic_replicate(dk.padded_square(crop), M) != 0
            sx = dk.source_coords(dk.invert_affine(M), S, S)[0]
            hit = False
            for y in np.nonzero(counted.any(axis=1))[0]:
                xs = np.nonzero(counted[y])[0]
                for x in (xs[0], xs[-1]):
                    cols = np.unique(np.clip(sx[y, x] - 1 + np.arange(4), 0, S - 1))
                    hit |= int(((cols >= left) & (cols < left + w)).sum()) == 1
            assert hit, (c, a)
    assert edge_cases >= 2


@pytest.mark.parametrize("kind", rc.KINDS)
def test_host_twin_equals_the_restatement_on_every_line_case(kind):
    compared = 0
    for c in rc.line_cases():
        if c.kind != kind:
            continue
        crop = rc.crop_of(c)
        slopes = rc.line_slopes(c.shape)
        for it in (0, 2):
            want = rc.line_masks_of(crop, slopes, it)
            literal = lines_ref.line_mask(crop, slopes[-1], it)                      # the hoisting changes nothing
            assert all(np.array_equal(a, b) for a, b in zip(want[-1], literal))
            for s, w in zip(slopes, want):
                got = _capi.host_region_line_mask(crop, s, erode_iterations=it)
                for g, ww, name in zip(got, w, ("dst", "rows", "cols")):
                    assert g.shape == ww.shape and np.array_equal(g, ww), (c, s, it, name)
                compared += w[0].size
    assert compared > 0


def test_shortcut_morphology_equals_the_literal_one_on_every_crop():
    changed = 0
    for c in rc.line_cases():
        for it in (0, 2):
            m = (lines_ref.eroded_crop(rc.crop_of(c), it) * np.uint8(255)).astype(np.uint8)
            want = lines_ref.open_close(m)
            assert np.array_equal(lines_ref.open_close_shortcut(m), want), (c, it)
            changed += not np.array_equal(want, m)
    assert changed >= 50
    masks = [(rc.crop_of(c) * np.uint8(255)).astype(np.uint8) for c in rc.line_cases() if c.kind in ("bytes", "wrap")]
    assert {int(v) for m in masks for v in np.unique(m)} >= {0, 1, 2, 128, 253, 254, 255}     # the product wraps in uint8
