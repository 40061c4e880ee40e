"""The text-line x extents from each region's filled, rotated contour, on the CPU: the library's serial host twin (csrc/line_extent.h through
sbbseg_region_line_extents_host) against the literal Python restatement of the OpenCV text (tests/line_extent_ref.py), field by field;
the arithmetic facts the header's integer predicates rest on, re-derived here and not taken from the header; and two independent holds on
the border scan: the library's own outer-border tracer, and scipy's count of enclosed background components."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import line_extent_cases as cases  # noqa: E402
import line_extent_ref as ref  # noqa: E402
from oracle import deskew as dk  # noqa: E402
from sbb_textline_detection_amd import _capi  # noqa: E402

REF_CASES = cases.ref_cases()


@pytest.mark.parametrize("case", REF_CASES, ids=[c["name"] for c in REF_CASES])
def test_host_twin_equals_the_restatement(case):
    w, h = int(case["box"][2]), int(case["box"][3])
    rot = _capi.line_rotation_terms(w, h, case["slope"])
    want = ref.region(case["ring"], case["box"], case["slope"], case["record"], rot)
    got = _capi.host_region_line_extents(case["ring"], case["box"], case["slope"], case["record"], want_masks=True)
    c = got["contour"]
    assert np.array_equal(c["threshrot"], want["threshrot"])
    assert (c["status"], c["borders"], c["holes"]) == (want["status"], want["borders"], want["holes"])
    if want["status"] != 0:
        assert got["status"] == _capi.LINES_NONE and len(got["peaks"]) == 0
        return
    assert (c["is_hole"], c["tie"], c["points"]) == (want["is_hole"], want["tie"], len(want["winner"]))
    assert np.array_equal(c["winner"], want["winner"]) and c["start"] == tuple(int(v) for v in want["winner"][0])
    assert np.array_equal(got["extent"], want["extent"])
    assert np.array_equal(got["boxes"], want["boxes"]) and np.array_equal(got["boxes_rot"], want["boxes_rot"])
    for key in ("peaks", "point_up", "point_down"):
        assert np.array_equal(got[key], case["record"][key])


def test_bicubic_products_are_multiples_of_2_to_minus_34():
    """R2: every float32 product tab[ay][r] * tab[ax][c] times 2^34 is an integer, the library's table holds exactly those integers, and
    255 * sum |weights| stays below 483: every partial sum of a 0 / 255 source is a multiple of 255 * 2^-34 below 2^9, exact in float64."""
    tab = dk.cubic_table()
    prod = (tab[:, None, :, None] * tab[None, :, None, :]).astype(np.float32)          # [ay][ax][r][c], float32 products
    scaled = [[Fraction(float(v)) * (1 << 34) for v in prod[ay, ax].reshape(-1)] for ay in range(32) for ax in range(32)]
    assert all(v.denominator == 1 for row in scaled for v in row)
    lib = _capi.region_line_extent_weights().reshape(1024, 16)
    assert [[int(v) for v in row] for row in scaled] == lib.tolist()
    worst = max(sum(abs(v) for v in row) for row in scaled)
    assert 255 * worst < 483 * (1 << 34)
    assert int(255 * worst).bit_length() <= 53                                         # ... as an integer numerator over 2^34


def test_numpy_cast_keeps_the_low_byte_of_the_truncated_value():
    """R3 on this machine's numpy: float64 -> uint8 truncates toward zero and keeps the low 8 bits on [-114, 369]."""
    v = np.arange(-114 * 64, 369 * 64 + 1, dtype=np.float64) / 64.0
    with np.errstate(invalid="ignore"):
        got = v.astype(np.uint8)
    want = np.array([int(x) & 255 for x in v], np.uint8)                                # int() truncates toward zero; & keeps the low byte
    assert np.array_equal(got, want)
    assert got[v == -1.0][0] == 255 and got[v == -0.984375][0] == 0 and got[v == 256.5][0] == 0 and got[v == 257.0][0] == 1


def test_signs_of_the_inside_test_survive_float64_rounding():
    """R5: with float32 inputs every product below is exact in float64, and rounding the sum of two exact products keeps its sign and its
    zero-ness -- checked against exact rationals on adversarial float32 operands (near-cancelling pairs included)."""
    rng = np.random.default_rng(3)
    vals = np.concatenate([rng.integers(-4000, 4000, 300).astype(np.float32), (rng.random(300) * 4000).astype(np.float32),
                           np.float32(1) + np.arange(1, 50, dtype=np.float32) * np.finfo(np.float32).eps])
    for _ in range(4000):
        a, b, c, d = (float(v) for v in rng.choice(vals, 4))
        if rng.random() < 0.3:
            c, d = b, a                                                                  # a * b - b * a: exactly zero
        for s, exact in ((a * b + c * d, Fraction(a) * Fraction(b) + Fraction(c) * Fraction(d)),
                         (a * b - c * d, Fraction(a) * Fraction(b) - Fraction(c) * Fraction(d))):
            assert Fraction(a * b) == Fraction(a) * Fraction(b)
            assert (s > 0) == (exact > 0) and (s == 0) == (exact == 0)
    # ... while the float32 subtraction that feeds them does round: the one place where the number format decides
    x, v = np.float32(1000.3), np.float32(0.1)
    assert Fraction(float(x - v)) != Fraction(float(x)) - Fraction(float(v))


def test_inside_samples_follow_the_float32_point():
    """The library's extent of a line equals the restatement's on a contour whose vertical edge sits where float32(xv[k]) and xv[k] fall on
    different sides of a sample."""
    ring = np.array([[0, 0], [100, 0], [100, 9], [0, 9]], np.int32)
    for w in (101, 130, 333):
        got = _capi.host_region_line_extents(ring, [0, 0, w, 10], 0.0, cases.record(10, 4, 1), want_masks=True)
        want = ref.line_extent(got["contour"]["winner"], w, int(got["peaks"][0]))
        assert tuple(int(v) for v in got["extent"][0]) == want


RAW = cases.raw_masks()


@pytest.mark.parametrize("name", sorted(RAW))
def test_border_scan_against_tracer_scipy_and_restatement(name):
    mask = RAW[name]
    got = _capi.host_mask_border_winner(mask)
    borders = ref.find_contours_tree(mask)
    k, tie = ref.winner(borders)
    assert got["borders"] == len(borders) and got["holes"] == sum(1 for b in borders if b[0])
    # outer borders: one per 8-connected component, each the library's own tracer's ring (same set of rings)
    outer = sorted(tuple(map(tuple, b[1].tolist())) for b in borders if not b[0])
    _boxes, traced = _capi.mask_contours_host(mask)
    assert outer == sorted(tuple(map(tuple, c.tolist())) for c in traced)
    # holes: the 4-connected background components that do not reach the frame
    lab, n = ndimage.label(np.pad(mask == 0, 1, constant_values=True))
    assert got["holes"] == n - 1
    if k is None:
        assert got["status"] == _capi.EXTENT_NONE and got["points"] == 0
        return
    assert got["status"] == _capi.EXTENT_OK and got["tie"] == tie and got["is_hole"] == bool(borders[k][0])
    assert np.array_equal(got["winner"], borders[k][1])


def test_named_raw_masks_are_what_their_names_say():
    assert _capi.host_mask_border_winner(RAW["empty"])["status"] == _capi.EXTENT_NONE
    hollow = _capi.host_mask_border_winner(RAW["hollow_square"])
    assert (hollow["borders"], hollow["points"], hollow["tie"], hollow["is_hole"]) == (2, 8, False, True)      # the hole border cuts the corners
    octagon = _capi.host_mask_border_winner(RAW["hollow_octagon"])
    assert (octagon["borders"], octagon["points"], octagon["tie"], octagon["is_hole"]) == (2, 8, True, True)     # 8 : 8, the last discovered wins
    ragged = _capi.host_mask_border_winner(RAW["ragged_inside"])
    assert ragged["is_hole"] and not ragged["tie"] and ragged["points"] > 4
    two = _capi.host_mask_border_winner(RAW["two_equal"])
    assert two["borders"] == 2 and two["tie"] and two["start"] == (30, 4)               # the last discovered of the maxima


def test_bad_rings_are_errors_that_name_the_region():
    rec = cases.record(10, 4, 1)
    with pytest.raises(RuntimeError, match="region 0.*not horizontal, vertical or an exact diagonal"):
        _capi.host_region_line_extents([[0, 0], [5, 2], [0, 4]], [0, 0, 10, 10], 0.0, rec)
    with pytest.raises(RuntimeError, match="region 0.*outside its box"):
        _capi.host_region_line_extents([[0, 0], [12, 0], [12, 4], [0, 4]], [0, 0, 10, 10], 0.0, rec)
