"""Cases and yardsticks of the deskew statistic that the CPU tests (test_profile_stats_cpu.py, test_soft_arith_cpu.py) and the device tests
(test_gpu_profile_cases.py) share: the scipy / numpy path of ``stages._profile_statistics`` / ``stages._deskew_sweep`` restated with what
the tests want to know about a case, the synthetic profile generators, and the operand sets of csrc/profile_stat.h's soft_div / soft_sqrt."""
import numpy as np
from scipy.ndimage import correlate1d, gaussian_filter1d
from scipy.signal import find_peaks

from sbb_textline_detection_amd import _capi

MULTIPLIER = 20.3                                                # main.py:1644
LENGTHS80 = [1, 2, 3, 7, 8, 9, 17, 19, 20, 21, 22, 39, 40, 41, 64, 100, 127, 128, 129, 130, 136, 255, 257, 300, 511, 700, 1031, 1300, 1500, 2100]
LENGTHS30 = [1, 5, 16, 18, 25, 33, 60, 90, 120, 131, 200, 260, 333, 512, 640, 801, 1024, 1111, 1600, 2049, 2100, 45, 77, 150]
CANONICAL_NAN = 0x7ff8000000000000


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def smoother(sigma):
    """``sigma``: a number -> gaussian_filter1d(., sigma); an array = half kernel weights[0 .. radius] of ANY values -> what gaussian_filter1d
    does with its own kernel (scipy's correlate1d over the symmetric kernel, mode "reflect")."""
    if np.ndim(sigma) == 0:
        return lambda v: gaussian_filter1d(v, sigma)
    half = np.asarray(sigma, np.float64)
    full = np.concatenate([half[:0:-1], half])
    return lambda v: correlate1d(v, full)


def yardstick_profile(y, sigma, multiplier=MULTIPLIER):
    """stages._profile_statistics with its caller's bookkeeping (stages._deskew_sweep), statement for statement, plus what the tests want
    to know about the case: (state, spread, z, facts)."""
    smooth = smoother(sigma)
    y = np.asarray(y, np.float64)
    padded = np.zeros(len(y) + 20)
    padded[10:10 + len(y)] = y
    flipped = np.zeros(len(padded) + 20)
    flipped[10:10 + len(padded)] = padded.max() - padded
    z = smooth(y)
    minima = find_peaks(smooth(flipped), height=0)[0] - 20
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


def yardstick_sweep(profiles, sigma, multiplier=MULTIPLIER):
    """(states, spreads, winner index or -1, the index of the maximum in the FULL list or -1, z per angle, facts)."""
    states, spreads, zs, facts = [], [], [], {"wrapped": False, "plateau": False}
    for y in profiles:
        st, sd, z, f = yardstick_profile(y, sigma, multiplier)
        states.append(st); spreads.append(sd); zs.append(z)
        facts = {k: facts[k] or f[k] for k in facts}
    appended = [k for k, st in enumerate(states) if st != 1]
    if not appended:
        return states, spreads, -1, -1, zs, facts
    pos = int(np.argmax(np.array([spreads[k] for k in appended])))
    return states, spreads, pos, appended[pos], zs, facts


def yardstick_tops(z):
    """The maxima above 10 of a smoothed profile, in order: what the statistic takes the mean of."""
    tops = z[find_peaks(z, height=0)[0]]
    return tops[tops > 10]


def yardstick_below(tops, multiplier=MULTIPLIER):
    """``level - level / multiplier`` of main.py:1576 with level = np.mean(tops); NaN without tops."""
    if tops.size == 0:
        return np.float64("nan")
    level = np.mean(tops)
    return level - level / np.float64(multiplier)


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


def five_configurations():
    """[(n_angles, sigma, weights, regions)]: regions of 80 and of 30 angles with profiles of 1 .. 2 100 samples under sigma 2 (built-in table and
    the binding's weights), 0.7, 5.5 (n = 5 at radius 22: the reflection wraps several times) and 3.  One seeded stream feeds all five."""
    rng = np.random.RandomState(2024)
    return [(n_angles, sigma, weights, synthetic_regions(rng, n_angles, lengths))
            for n_angles, lengths, sigma, weights in ((80, LENGTHS80, 2, None), (30, LENGTHS30, 2, _capi.gaussian_weights(2)),
                                                      (30, LENGTHS30[3::4], 0.7, _capi.gaussian_weights(0.7)),
                                                      (30, LENGTHS30[1::5], 5.5, _capi.gaussian_weights(5.5)), (30, [3, 12, 400], 3, _capi.gaussian_weights(3)))]


def pack(regions):
    """(counts int32, offsets int64) as sbbseg_region_deskew_profiles packs a list of int32 [n_angles][S_r]."""
    offsets = np.concatenate([[0], np.cumsum([r.size for r in regions])]).astype(np.int64)
    return np.concatenate([r.reshape(-1) for r in regions]).astype(np.int32), offsets


# ---- soft_div / soft_sqrt -------------------------------------------------------------------------------------------------------------

def _from_bits(u):
    return np.ascontiguousarray(u, np.uint64).view(np.float64)


def _scaled(rng, count, exponents):
    """random 52-bit mantissas under the given biased exponents (1 .. 2046), random signs"""
    mant = rng.randint(0, 1 << 52, count, dtype=np.int64).astype(np.uint64)
    sign = rng.randint(0, 2, count).astype(np.uint64) << np.uint64(63)
    return _from_bits(sign | (np.asarray(exponents, np.int64).astype(np.uint64) << np.uint64(52)) | mant)


def special_values():
    one = np.float64(1.0)
    base = [0.0, np.inf, np.nan, 5e-324, _from_bits([(1 << 52) - 1])[0], 2.2250738585072014e-308, np.finfo(np.float64).max, 1.0,
            np.nextafter(one, 2.0), np.nextafter(one, 0.0), 2.0, 3.0, 10.0, 20.3, 0.1]
    base += [np.ldexp(1.0, k) for k in (-1074, -1073, -1060, -1023, -1022, -1021, -538, -537, -512, -53, -52, -2, -1, 1, 2, 52, 53, 511, 512, 1021, 1022,
                                        1023)]
    v = np.array(base, np.float64)
    return np.concatenate([v, -v])


def soft_arith_operands(seed=77):
    """{family: (a, b)} for the divide and {family: a} for the square root, a fixed seed; a few hundred thousand sets in all."""
    rng = np.random.RandomState(seed)
    sp = special_values()
    rand_bits = lambda n: _from_bits(rng.randint(0, 1 << 32, n, dtype=np.int64).astype(np.uint64) << np.uint64(32)
                                     | rng.randint(0, 1 << 32, n, dtype=np.int64).astype(np.uint64))
    div = {"specials": (np.repeat(sp, sp.size), np.tile(sp, sp.size)), "random bits": (rand_bits(100000), rand_bits(100000))}
    eb = rng.randint(1, 2047, 50000)                             # quotients of 2^-1082 .. 2^-1018: subnormal results, every shift, and underflow
    ea = np.clip(eb + rng.randint(-1082, -1017, 50000), 1, 2046)
    div["subnormal quotients"] = (_scaled(rng, 50000, ea), _scaled(rng, 50000, eb))
    eb = rng.randint(1, 1030, 20000)                             # quotients of 2^1018 .. 2^1030: up to and beyond the largest finite
    ea = np.clip(eb + rng.randint(1018, 1031, 20000), 1, 2046)
    div["overflowing quotients"] = (_scaled(rng, 20000, ea), _scaled(rng, 20000, eb))
    ints = np.concatenate([rng.randint(0, 1 << 40, 50000, dtype=np.int64), rng.randint(0, 1 << 20, 50000, dtype=np.int64)])
    div["sums over counts"] = (ints.astype(np.float64), rng.randint(1, 4097, 100000).astype(np.float64))      # the product's own use
    x = np.concatenate([rng.randint(0, 1 << 30, 10000).astype(np.float64) * 0.1, rng.uniform(0, 5000, 10000)])
    div["x / 2"] = (x, np.full(x.size, 2.0))
    div["x / 20.3"] = (x, np.full(x.size, 20.3))
    root = rng.randint(1, (1 << 26) + 1, 30000, dtype=np.int64)
    root[:4] = [1, 2, 1 << 26, (1 << 26) - 1]
    sq = (root * root).astype(np.float64)                        # exact: at most 2^52
    sqrt = {"specials": sp, "random bits": rand_bits(100000), "squares": sq, "squares - 1 ulp": np.nextafter(sq, 0.0),
            "squares + 1 ulp": np.nextafter(sq, np.inf),
            "subnormals": _from_bits(rng.randint(1, 1 << 52, 20000, dtype=np.int64).astype(np.uint64))}
    e = rng.randint(1, 2046, 20000)
    mant = rng.randint(0, 1 << 52, 20000, dtype=np.int64).astype(np.uint64)
    sqrt["even and odd exponents"] = np.concatenate([_from_bits((np.asarray(e + k, np.int64).astype(np.uint64) << np.uint64(52)) | mant) for k in (0, 1)])
    return div, sqrt


def numpy_results(div, sqrt):
    """({family: a / b}, {family: np.sqrt(a)})"""
    with np.errstate(all="ignore"):
        return {k: a / b for k, (a, b) in div.items()}, {k: np.sqrt(a) for k, a in sqrt.items()}


def soft_arith_mismatches(got, want):
    """Elements of ``got`` that are not ``want`` bit for bit; a NaN must be a NaN with the canonical quiet pattern."""
    nan = np.isnan(want)
    g = bits(got)
    return int(np.count_nonzero(np.where(nan, g != np.uint64(CANONICAL_NAN), g != bits(want))))
