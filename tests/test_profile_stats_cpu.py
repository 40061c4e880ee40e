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
from scipy.signal import find_peaks

from sbb_textline_detection_amd import _capi, stages

import slopes_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["sbbseg_profile_statistics_host", "sbbseg_profile_statistics_dev", "sbbseg_deskew_sweep_angles", "sbbseg_region_deskew_slopes_dev",
               "sbbseg_region_deskew_slopes"]
MULTIPLIER = 20.3                                                # main.py:1644


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def yardstick_profile(y, sigma, multiplier=MULTIPLIER):
    """stages._profile_statistics with its caller's bookkeeping (stages._deskew_sweep), statement for statement, plus what the tests want
    to know about the case: (state, spread, z, facts)."""
    y = np.asarray(y, np.float64)
    padded = np.zeros(len(y) + 20)
    padded[10:10 + len(y)] = y
    flipped = np.zeros(len(padded) + 20)
    flipped[10:10 + len(padded)] = padded.max() - padded
    z = gaussian_filter1d(y, sigma)
    minima = find_peaks(gaussian_filter1d(flipped, sigma), height=0)[0] - 20
    maxima, props = find_peaks(z, height=0, plateau_size=1)
    assert np.array_equal(maxima, find_peaks(z, height=0)[0])
    facts = {"wrapped": bool(((minima < 0) & (minima >= -len(y))).any()), "plateau": bool((props["plateau_sizes"] > 1).any())}
    tops = z[maxima]
    tops = tops[tops > 10]
    try:
        lows = z[minima]
    except IndexError:
        return 2, 0.0, z, facts
    with np.errstate(all="ignore"):
        level = np.mean(tops) if tops.size else np.float64("nan")
    if lows[lows < level - level / multiplier].size == 0:
        return 1, 0.0, z, facts
    return 0, np.std(z), z, facts


def yardstick_sweep(profiles, sigma):
    """(states, spreads, winner index or -1, the index of the maximum in the FULL list or -1, z per angle, facts)."""
    states, spreads, zs, facts = [], [], [], {"wrapped": False, "plateau": False}
    for y in profiles:
        st, sd, z, f = yardstick_profile(y, sigma)
        states.append(st); spreads.append(sd); zs.append(z)
        facts = {k: facts[k] or f[k] for k in facts}
    appended = [k for k, st in enumerate(states) if st != 1]
    if not appended:
        return states, spreads, -1, -1, zs, facts
    pos = int(np.argmax(np.array([spreads[k] for k in appended])))
    return states, spreads, pos, appended[pos], zs, facts


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


def text_lines(rng, n, period, thick, height, phase=0, noise=0):
    x = np.arange(n)
    y = np.where((x + phase) % period < thick, height, 0)
    if noise:
        y = y + rng.randint(0, noise + 1, n) * (y > 0)
    return y


def synthetic_regions(rng, n_angles, lengths):
    """One region per length; the kinds cycle so that every kind meets short and long profiles."""
    regions = []
    for q, n in enumerate(lengths):
        kind = q % 8
        if kind == 0:                                            # random counts
            p = rng.randint(0, 400, (n_angles, n))
        elif kind == 1:                                          # runs of equal values (plateaus survive the smoothing when they are long)
            run = int(rng.choice([7, 23, 40]))
            p = np.repeat(rng.randint(0, 60, (n_angles, n // run + 1)), run, axis=1)[:, :n]
        elif kind == 2:                                          # all zeros
            p = np.zeros((n_angles, n), np.int64)
        elif kind == 3:                                          # constants
            p = np.repeat(rng.randint(1, 900, (n_angles, 1)), n, axis=1)
        elif kind == 4:                                          # single spikes
            p = np.zeros((n_angles, n), np.int64)
            p[np.arange(n_angles), rng.randint(0, n, n_angles)] = rng.randint(1, 5000, n_angles)
        elif kind == 5:                                          # text-line-like: sharp at some angles, washed out (no deep minimum) at others
            p = np.stack([text_lines(rng, n, 30, 12, int(rng.randint(60, 300)), int(rng.randint(30)), 5) if rng.rand() < 0.6 else
                          np.full(n, int(rng.randint(20, 90))) + rng.randint(0, 3, n) for _ in range(n_angles)])
            p[:, :min(25, n // 4)] = 0
            p[:, n - min(25, n // 4):] = 0
        elif kind == 6:                                          # the mass at the right end: a minimum lands in the right-hand padding
            p = np.zeros((n_angles, n), np.int64)
            k = max(1, n // 8)
            p[:, n - k:] = rng.randint(20, 500, (n_angles, k))
        else:                                                    # the mass at the left end: a minimum before sample 0 wraps
            p = np.zeros((n_angles, n), np.int64)
            k = max(1, n // 8)
            p[:, :k] = rng.randint(20, 500, (n_angles, k))
            if n > 60:
                p[:, n // 2:n // 2 + 12] = 300                    # (and a line further in, so that there is a deep minimum as well)
        regions.append(np.ascontiguousarray(p, np.int32))
    return regions


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
    rng = np.random.RandomState(2024)
    lengths80 = [1, 2, 3, 7, 8, 9, 17, 19, 20, 21, 22, 39, 40, 41, 64, 100, 127, 128, 129, 130, 136, 255, 257, 300, 511, 700, 1031, 1300, 1500, 2100]
    lengths30 = [1, 5, 16, 18, 25, 33, 60, 90, 120, 131, 200, 260, 333, 512, 640, 801, 1024, 1111, 1600, 2049, 2100, 45, 77, 150]
    seen = set()
    n_profiles = 0
    for n_angles, lengths, sigma, weights in ((80, lengths80, 2, None), (30, lengths30, 2, _capi.gaussian_weights(2)),
                                              (30, lengths30[3::4], 0.7, _capi.gaussian_weights(0.7)), (30, lengths30[1::5], 5.5, _capi.gaussian_weights(5.5)),
                                              (30, [3, 12, 400], 3, _capi.gaussian_weights(3))):
        regions = synthetic_regions(rng, n_angles, lengths)
        n_profiles += n_angles * len(regions)
        seen |= compare_sweeps(regions, n_angles, sigma, weights)
    assert n_profiles >= 300
    missing = {"state0", "state1", "state2", "wrapped", "plateau", "quirk", "nothing"} - seen
    assert not missing, "the generators no longer produce: %s" % sorted(missing)


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


def test_get_slopes_checks_its_keyword():
    plane = np.zeros((8, 8), np.uint8)
    with pytest.raises(ValueError, match="statistics"):
        stages.get_slopes(plane, [[0, 0, 5, 5]], None, statistics="nonsense")
    with pytest.raises(ValueError, match="statistics"):
        stages.get_slopes(plane, [[0, 0, 5, 5]], object(), statistics="nonsense")
    for st in ("device", "host"):
        with pytest.raises(RuntimeError, match="library handle"):
            stages.get_slopes(plane, [[0, 0, 5, 5]], None, statistics=st)
