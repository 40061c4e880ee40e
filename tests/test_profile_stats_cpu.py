"""The 1-D statistic of the deskew search and the angle selection without a GPU: ``sbbseg_profile_statistics_host`` (the serial CPU entry
point that shares its arithmetic, csrc/profile_stat.h, with the kernels of profile_stats.hip) against the scipy path of
``stages._profile_statistics`` / ``stages._deskew_sweep`` -- float64 BIT PATTERNS, states and winners -- on synthetic and on real
profiles; the weights and angle tables; the new names of the C ABI and their argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy.ndimage import gaussian_filter1d

from sbb_textline_detection_amd import _capi, stages

import slopes_ref
from profile_cases import MULTIPLIER, bits, five_configurations, text_lines, yardstick_below, yardstick_profile, yardstick_sweep, yardstick_tops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["sbbseg_profile_statistics_host", "sbbseg_profile_statistics_dev", "sbbseg_deskew_sweep_angles", "sbbseg_region_deskew_slopes_dev",
               "sbbseg_region_deskew_slopes"]


def compare_sweeps(regions, n_angles, sigma, weights):
    """``regions``: a list of int32 [n_angles][S_r].  Returns the set of things seen."""
    offsets = np.concatenate([[0], np.cumsum([r.size for r in regions])]).astype(np.int64)
    counts = np.concatenate([r.reshape(-1) for r in regions]).astype(np.int32)
    spread, state, winner, smooth = _capi.profile_statistics_host(counts, offsets, n_angles, weights, MULTIPLIER, want_smooth=True)
    seen = set()
    angles = np.arange(n_angles, dtype=np.float64) + 1.0          # any distinct non-zero values: _deskew_sweep returns angles[winner]
    for r, prof in enumerate(regions):
        states, spreads, win, true_win, zs, facts = yardstick_sweep(prof, sigma)
        z_got = smooth[offsets[r]:offsets[r + 1]].reshape(n_angles, -1)
        assert np.array_equal(bits(z_got), bits(np.stack(zs))), (r, prof.shape)
        assert state[r].tolist() == states, (r, prof.shape)
        for k, st in enumerate(states):
            if st == 0:
                assert bits(spread[r, k]) == bits(np.float64(spreads[k])), (r, k, prof.shape, spread[r, k], spreads[k])
        assert int(winner[r]) == win, (r, prof.shape)
        assert stages._deskew_sweep(prof, angles, sigma) == (float(angles[win]) if win >= 0 else 0.0)
        seen |= {"state%d" % s for s in states} | {k for k, v in facts.items() if v}
        if win != true_win:
            seen.add("quirk")
        if win < 0:
            seen.add("nothing")
    return seen


def test_weight_and_angle_tables_equal_numpy_and_scipy():
    from scipy.ndimage._filters import _gaussian_kernel1d
    for sigma in (0.7, 1, 2, 3, 5.5):
        radius = int(4 * float(sigma) + 0.5)
        want = _gaussian_kernel1d(sigma, 0, radius)[radius:]
        got = _capi.gaussian_weights(sigma)
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), sigma
    # the built-in table (weights = NULL) is that of sigma = 2: a profile smoothed with it equals gaussian_filter1d(., 2) in every bit,
    # and a unit spike reads the table itself out
    rng = np.random.RandomState(5)
    y = rng.randint(0, 1000, (1, 300)).astype(np.int32)
    for w in (None, _capi.gaussian_weights(2)):
        smooth = _capi.profile_statistics_host(y, [0, 300], 1, w, want_smooth=True)[3]
        assert np.array_equal(bits(smooth), bits(gaussian_filter1d(y[0].astype(np.float64), 2)))
    spike = np.zeros((1, 41), np.int32)
    spike[0, 20] = 1
    table = _capi.profile_statistics_host(spike, [0, 41], 1, None, want_smooth=True)[3][20:29]
    assert np.array_equal(bits(table), bits(_gaussian_kernel1d(2, 0, 8)[8:]))
    assert np.array_equal(bits(_capi.deskew_sweep_angles(0)), bits(np.linspace(-25, 25, 80)))
    assert np.array_equal(bits(_capi.deskew_sweep_angles(1)), bits(np.linspace(-90, -50, 30)))
    assert np.array_equal(_capi.deskew_sweep_angles(0), slopes_ref.SWEEP1) and np.array_equal(_capi.deskew_sweep_angles(1), slopes_ref.SWEEP2)


def test_host_mirror_equals_scipy_on_synthetic_profiles():
    """Several hundred int32 profiles of 1 .. 2 100 samples in regions of 80 and of 30 angles: smoothed profile, state, spread and winner."""
    seen = set()
    n_profiles = 0
    for n_angles, sigma, weights, regions in five_configurations():
        n_profiles += n_angles * len(regions)
        seen |= compare_sweeps(regions, n_angles, sigma, weights)
    assert n_profiles >= 300
    missing = {"state0", "state1", "state2", "wrapped", "plateau", "quirk", "nothing"} - seen
    assert not missing, "the generators no longer produce: %s" % sorted(missing)


def test_host_mirror_equals_numpy_beyond_one_sum_buffer():
    """np.mean and np.std add stretches of 8192 elements (numpy's ufunc buffer) up one after the other, each summed pairwise: a profile or a
    list of maxima longer than that is not one pairwise sum.  Lengths around one and two stretches and the longest the tables admit; the
    second profile of each region has a maximum at every other sample, so the mean of the maxima crosses a stretch as well."""
    rng = np.random.RandomState(8)
    most = 0
    for n in (8191, 8192, 8193, 8200, 16383, 16384, 16385, 20000, 32767):
        prof = np.stack([text_lines(rng, n, 30, 12, 250, 7, 9), rng.randint(150, 400, n) * (np.arange(n) % 2)]).astype(np.int32)
        prof[:, :25] = 0
        prof[:, -25:] = 0
        assert "state0" in compare_sweeps([prof], 2, 0.1, np.array([1.0]))       # (radius 0: z = y)
        below = _capi.debug_profile_statistics(None, prof, [0, prof.size], 2, np.array([1.0]))[4]
        for k in range(2):
            tops = yardstick_tops(yardstick_profile(prof[k], 0.1)[2])
            assert bits(below[0, k]) == bits(yardstick_below(tops)), (n, k)
            most = max(most, tops.size)
    assert most > 2 * 8192 - 100


def test_multiplier_and_radius_zero():
    rng = np.random.RandomState(3)
    prof = np.stack([text_lines(rng, 400, 30, 12, 200, k, 5) for k in range(6)]).astype(np.int32)
    prof[:, :25] = 0
    prof[:, -25:] = 0
    for mult in (20.3, 3.8, 1.0, 0.5, -2.0):
        spread, state, winner = _capi.profile_statistics_host(prof, [0, prof.size], 6, None, mult)
        for k in range(6):
            st, sd, _z, _f = yardstick_profile(prof[k], 2, mult)
            assert state[0, k] == st and (st != 0 or bits(spread[0, k]) == bits(np.float64(sd))), (mult, k)
    # radius 0: one weight, z = y * w[0]
    spread, state, winner, smooth = _capi.profile_statistics_host(prof, [0, prof.size], 6, np.array([1.0]), want_smooth=True)
    assert np.array_equal(smooth.reshape(6, -1), prof.astype(np.float64))


def test_host_mirror_equals_scipy_on_real_profiles():
    """Row profiles of the eroded crops of the fixture pages by the ORACLE's rotate-and-project (angles subsampled to stay in seconds), and the
    full sweeps of the two smallest boxes: their winners reproduce the fixture's slopes."""
    from oracle import deskew as dk
    cases = [(t, b, s) for _r, t, boxes, slopes in slopes_ref.load_pages() for b, s in zip(boxes, slopes)]
    cases.sort(key=lambda c: c[1][2] * c[1][3])
    seen = set()
    for textlines, box, _slope in cases[:6]:
        crop = slopes_ref.erode2(slopes_ref.crop_of(textlines, box))
        for full, n in ((slopes_ref.SWEEP1, 8), (slopes_ref.SWEEP2, 5)):
            angles = full[::len(full) // n][:n]
            prof = np.ascontiguousarray(dk.row_profiles(crop, angles), np.int32)
            seen |= compare_sweeps([prof], len(angles), 2, None)
    assert "state0" in seen
    for textlines, box, slope in cases[:2]:
        crop = slopes_ref.erode2(slopes_ref.crop_of(textlines, box))
        prof = np.ascontiguousarray(dk.row_profiles(crop, slopes_ref.SWEEP1), np.int32)
        compare_sweeps([prof], 80, 2, None)
        winner = int(_capi.profile_statistics_host(prof, [0, prof.size], 80)[2][0])
        ang = float(_capi.deskew_sweep_angles(0)[winner]) if winner >= 0 else 0.0
        if abs(ang) > 15:
            prof = np.ascontiguousarray(dk.row_profiles(crop, slopes_ref.SWEEP2), np.int32)
            compare_sweeps([prof], 30, 2, None)
            winner = int(_capi.profile_statistics_host(prof, [0, prof.size], 30)[2][0])
            ang = float(_capi.deskew_sweep_angles(1)[winner]) if winner >= 0 else 0.0
        assert slopes_ref.cleaned(ang) == slope, (box, ang, slope)


def test_new_names_are_exported_declared_and_bound():
    lib = _capi.load_library()
    header = open(os.path.join(ROOT, "include", "sbbseg.h")).read()
    for name in NEW_EXPORTS:
        assert name in _capi.EXPORTS and hasattr(lib, name)
        assert re.search(r"\bint %s\(" % name, header)
    assert lib.sbbseg_abi_version() == 5
    for attr in ("profile_statistics_dev", "region_deskew_slopes", "region_deskew_slopes_dev"):
        assert callable(getattr(_capi.Context, attr))
    for attr in ("profile_statistics_host", "gaussian_weights", "deskew_sweep_angles"):
        assert callable(getattr(_capi, attr))
    assert os.path.exists(os.path.join(ROOT, "sbb_textline_detection_amd", "csrc", "profile_stats.hip"))


def test_bad_arguments_are_a_status_and_a_message():
    lib = _capi.load_library()
    counts, off = np.zeros(60, np.int32), np.array([0, 60], np.int64)
    spread, state, winner = np.zeros(6), np.zeros(6, np.uint8), np.zeros(1, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    host = lambda n_angles, radius, offsets=off: lib.sbbseg_profile_statistics_host(p(counts), p(offsets), 1, n_angles, None, radius, 20.3, p(spread), p(state),
                                                                                     p(winner), None)
    assert host(6, 0) == 0
    assert host(0, 0) != 0 and b"n_angles" in lib.sbbseg_last_error()
    assert host(6, -1) != 0 and b"radius" in lib.sbbseg_last_error()
    assert host(7, 0) != 0 and b"region 0" in lib.sbbseg_last_error()                       # 60 ints are not 7 profiles
    assert host(6, 0, np.array([0, 6 * 40000], np.int64)) != 0 and b"region 0" in lib.sbbseg_last_error()
    assert lib.sbbseg_profile_statistics_host(None, None, 0, 6, None, 0, 20.3, None, None, None, None) == 0          # no regions: success
    with pytest.raises(RuntimeError, match="n_angles"):
        _capi.profile_statistics_host(counts, off, 0)
    # a null handle
    assert lib.sbbseg_profile_statistics_dev(None, p(counts), p(off), 1, 6, None, 0, 20.3, p(spread), p(state), p(winner)) != 0
    assert b"null handle" in lib.sbbseg_last_error()
    plane, boxes, slopes = np.zeros((8, 8), np.uint8), np.array([[0, 0, 5, 5]], np.int32), np.zeros(1)
    for fn in (lib.sbbseg_region_deskew_slopes, lib.sbbseg_region_deskew_slopes_dev):
        assert fn(None, p(plane), 8, 8, p(boxes), 1, 2, None, 0, p(slopes)) != 0 and b"null handle" in lib.sbbseg_last_error()
    n = C.c_int(0)
    assert lib.sbbseg_deskew_sweep_angles(2, None, 0, C.byref(n)) != 0
    assert lib.sbbseg_deskew_sweep_angles(1, None, 0, C.byref(n)) == 0 and n.value == 30
    assert lib.sbbseg_deskew_sweep_angles(0, p(np.zeros(10)), 10, C.byref(n)) != 0 and b"80" in lib.sbbseg_last_error()


def test_debug_entry_points_without_a_handle():
    """sbbseg_debug_profile_statistics with a null handle is the host entry point plus `below`; sbbseg_debug_soft_arith checks its arguments."""
    lib = _capi.load_library()
    rng = np.random.RandomState(11)
    prof = np.stack([text_lines(rng, 300, 30, 12, 200, k, 5) for k in range(4)]).astype(np.int32)
    prof[2] = 0                                                  # no maximum: the level is NaN
    want = _capi.profile_statistics_host(prof, [0, prof.size], 4, None, want_smooth=True)
    got = _capi.debug_profile_statistics(None, prof, [0, prof.size], 4)
    assert all(np.array_equal(bits(a) if a.dtype == np.float64 else a, bits(b) if b.dtype == np.float64 else b) for a, b in zip(got[:4], want))
    for k in range(4):
        level = yardstick_below(yardstick_tops(yardstick_profile(prof[k], 2)[2]))
        assert np.isnan(level) == np.isnan(got[4][0, k]) == (k == 2) and (k == 2 or bits(got[4][0, k]) == bits(level))
    with pytest.raises(RuntimeError, match="n_angles"):
        _capi.debug_profile_statistics(None, prof, [0, prof.size], 0)
    assert _capi.debug_soft_arith(None, 0, [1.0, 0.0, 7.0], [3.0, 0.0, -0.0]).view(np.uint64).tolist() == [0x3fd5555555555555, 0x7ff8000000000000,
                                                                                                            0xfff0000000000000]
    assert _capi.debug_soft_arith(None, 1, [2.0, -1.0]).view(np.uint64).tolist() == [0x3ff6a09e667f3bcd, 0x7ff8000000000000]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    a, out = np.ones(2), np.zeros(2)
    assert lib.sbbseg_debug_soft_arith(None, 2, p(a), p(a), 2, p(out)) != 0 and b"bad arguments" in lib.sbbseg_last_error()
    assert lib.sbbseg_debug_soft_arith(None, 0, p(a), None, 2, p(out)) != 0 and lib.sbbseg_debug_soft_arith(None, 1, p(a), None, 2, p(out)) == 0
    assert lib.sbbseg_debug_soft_arith(None, 0, None, None, 0, None) == 0


def test_get_slopes_checks_its_keyword():
    plane = np.zeros((8, 8), np.uint8)
    with pytest.raises(ValueError, match="statistics"):
        stages.get_slopes(plane, [[0, 0, 5, 5]], None, statistics="nonsense")
    with pytest.raises(ValueError, match="statistics"):
        stages.get_slopes(plane, [[0, 0, 5, 5]], object(), statistics="nonsense")
    for st in ("device", "host"):
        with pytest.raises(RuntimeError, match="library handle"):
            stages.get_slopes(plane, [[0, 0, 5, 5]], None, statistics=st)
