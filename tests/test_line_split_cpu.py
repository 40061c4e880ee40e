"""The line splitters after the projection, without a GPU: the numpy / scipy restatement (tests/line_split_ref.py) against the fixture
recorded from the reference's own ``seperate_lines`` / ``seperate_lines_vertical`` (tests/golden/make_line_split_golden.py), and the host
twin ``sbbseg_line_split_host`` (csrc/line_split.h on the CPU) against the restatement, exactly, on every field."""
import numpy as np
import pytest
from scipy.ndimage import gaussian_filter1d

from sbb_textline_detection_amd import _capi, stages

import line_split_ref as lr


def _terms(n, other, vertical, slope):
    w, h = (n, other) if vertical else (other, n)
    return _capi.line_rotation_terms(w, h, slope)


def _check(profiles, others, slopes):
    verticals = [abs(s) > 45 for s in slopes]
    rots = [_terms(len(y), o, v, s) for y, o, v, s in zip(profiles, others, verticals, slopes)]
    got = _capi.line_split_host(profiles, others, verticals, rots)
    want = [lr.line_split(y, o, v, r) for y, o, v, r in zip(profiles, others, verticals, rots)]
    for k, (a, b) in enumerate(zip(got, want)):
        assert lr.same(a, b), (k, len(profiles[k]), others[k], slopes[k], {f: (a[f], b[f]) for f in lr.FIELDS})
    return want


def test_the_fixture_covers_what_it_must_and_the_restatement_reproduces_it():
    cases = lr.load_golden()
    branches = {c["branch"] for c in cases}
    assert {0, 1, 2, 3, 4} <= branches
    assert any(c["branch"] == 1 and c["status"] == lr.OK and c["vertical"] and len(c["peaks"]) == 0 for c in cases)     # main.py:1288: `pass`
    assert any(c["vertical"] for c in cases) and any(c["raised"] and c["sigma"] == 12 for c in cases) and any(c["sigma"] > 3 for c in cases)
    assert any(c["clusters"] > 0 for c in cases) and any(c["status"] == lr.NONE for c in cases)
    assert sum(1 for c in cases if c["page"] >= 0) == 14 and any(c["vertical"] and len(c["peaks"]) for c in cases)
    clamped = 0
    for c in cases:
        mine = lr.line_split(c["y"], c["other"], c["vertical"], c["rot"])
        assert lr.same(mine, c) and mine["clusters"] == c["clusters"], (c["page"], c["box"])
        clamped += mine["clamped"]
        n = len(c["y"])
        assert c["rot"] == _terms(n, c["other"], c["vertical"], c["slope"])      # the library's getRotationMatrix2D gives the recorded terms
    assert clamped >= 1


def test_host_twin_equals_the_restatement_on_the_fixture():
    cases = lr.load_golden()
    got = _capi.line_split_host([c["y"] for c in cases], [c["other"] for c in cases], [c["vertical"] for c in cases], [c["rot"] for c in cases])
    for c, a in zip(cases, got):
        assert lr.same(a, c), (c["page"], c["box"], {f: (a[f], c[f]) for f in lr.FIELDS})


def test_host_twin_equals_the_restatement_on_a_seeded_sweep():
    want = _check(*lr._random_profiles())
    assert {0, 2, 3, 4} <= {w["branch"] for w in want} and any(w["raised"] for w in want) and any(w["clusters"] for w in want)
    assert any(w["status"] == lr.NONE for w in want) and any(w["sigma"] > 12 for w in want)


def test_host_twin_on_profiles_with_mass_at_both_ends_only():
    """No interior maximum after the second smoothing (its radius exceeds the pads and scipy reflects at the ends): the vertical splitter
    falls into ``len(peaks) < 1`` (main.py:1288), the horizontal one raises in main.py:646."""
    want = _check(*lr.both_ends_profiles())
    for k in range(0, 6, 2):
        assert (want[k]["status"], want[k]["branch"], len(want[k]["peaks"])) == (lr.OK, 1, 0) and want[k]["sigma"] > 5
        assert (want[k + 1]["status"], want[k + 1]["branch"]) == (lr.NONE, -1)


def test_host_twin_on_a_long_a_zero_and_a_constant_profile():
    want = _check(*lr.long_zero_constant_profiles())
    assert len(want[0]["peaks"]) == 30 and len(want[1]["peaks"]) == 30 and want[2]["status"] == lr.NONE and want[3]["raised"]


def test_weight_table_is_scipys_kernel():
    w, off = _capi.line_weight_table()
    assert off.shape == (_capi.LINE_SIGMA_MAX,) and off[-1] == w.shape[0] and w.nbytes < 300 * 1024
    for sigma in (2, 3, 12, 128):
        half = w[off[sigma - 2]:off[sigma - 1]]
        x = np.zeros(8 * sigma + 1)
        x[4 * sigma] = 1.0
        kernel = gaussian_filter1d(x, sigma, mode="constant")                    # an impulse gives the kernel itself
        assert half.shape == (4 * sigma + 1,) and np.array_equal(half, kernel[4 * sigma:]) and np.array_equal(half, kernel[4 * sigma::-1])


def test_sigma_beyond_the_table_is_reported_and_finished_on_the_host():
    y = ((np.arange(1500) % 500) < 200).astype(np.int32) * 40
    rot = _terms(1500, 50, False, 2.0)
    want = lr.line_split(y, 50, False, rot)
    assert want["sigma"] > 64 and want["status"] == lr.OK and len(want["peaks"]) >= 2
    info, line_off, lines, _c, _r = _capi.line_split_host_raw([y], [50], [False], [rot], sigma_max=64)
    assert info[0].tolist() == [_capi.LINES_SIGMA_TOO_LARGE, want["sigma"], 0, -1, 0] and line_off.tolist() == [0, 770] and not lines.any()
    assert lr.same(_capi.line_split_host([y], [50], [False], [rot], sigma_max=64)[0], want)
    assert lr.same(_capi.line_split_host([y], [50], [False], [rot])[0], want)


def test_bad_arguments_are_errors_and_the_stage_functions_exist():
    with pytest.raises(RuntimeError, match="region 0"):
        _capi.line_split_host([np.zeros(5, np.int32)], [0], [False], [[1, 0, 0, 1, 0, 0]])
    with pytest.raises(RuntimeError, match="sigma_max"):
        _capi.line_split_host_raw([np.zeros(5, np.int32)], [3], [False], [[1, 0, 0, 1, 0, 0]], sigma_max=11)
    assert _capi.line_split_host([], [], [], np.zeros((0, 6))) == []
    plane = np.zeros((20, 20), np.uint8)
    with pytest.raises(RuntimeError, match="library handle"):
        stages.get_line_boxes(plane, [[2, 2, 8, 8]], [0.0])
    with pytest.raises(RuntimeError, match="library handle"):
        stages.get_slopes_and_line_boxes(plane, [[2, 2, 8, 8]])
    assert hasattr(stages.InferenceStages, "get_line_boxes") and hasattr(stages.InferenceStages, "run_with_line_boxes")
