"""The deskew statistic's kernels (csrc/profile_stats.hip) on adversarial profiles (-m gpu): the cases that hold the serial host twin to scipy
(tests/profile_cases.py, test_profile_stats_cpu.py), and those at which only the DEVICE deals the work differently -- lengths around one
and two ballots of 64 lanes and around the LDS limit, maxima and plateaus on the lane boundaries, many maxima to compact in order, batches
that mix the LDS and the global-workspace form, ties and skipped angles in the selection, other multipliers.

``sbbseg_debug_profile_statistics`` runs the product's kernels through the product's launch and also returns the smoothed profile z and the
level ``below`` a deep minimum must lie below -- the one value in which a dropped, repeated or reordered maximum shows.  Every comparison is
on float64 BIT PATTERNS (NaN: both NaN), device against the host twin, and both against scipy / numpy.  csrc/profile_stat.h's soft_div and
soft_sqrt run on the device over the operand sets of test_soft_arith_cpu.py."""
import time

import numpy as np
import pytest

from sbb_textline_detection_amd import _capi

import profile_cases as pc
from profile_cases import bits

pytestmark = pytest.mark.gpu
T0 = time.time()
LDS_SAMPLES = 2048                                               # csrc/internal.h: kProfileLdsSamples
SEEN = set()                                                     # what the device runs of this module have met
COUNTS = {"profiles": 0, "batches": 0}
_YARD = {}


@pytest.fixture(scope="module")
def model():
    from sbb_textline_detection_amd.model import SegModel
    from tools.synth_model import calibrated_model
    cfg, w = calibrated_model(2, 224, 224, seed=0)
    m = SegModel(cfg, w, device=0, max_batch=4)                  # any finalized handle: these calls do not touch the network
    yield m
    m.release()
    print(f"[test_gpu_profile_cases] {COUNTS['profiles']} profiles in {COUNTS['batches']} device batches; seen on the device: {sorted(SEEN)}")
    print(f"[test_gpu_profile_cases] module wall time {time.time() - T0:.1f} s")


def same_bits(a, b):
    """float64 arrays equal bit for bit; a NaN equals any NaN."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def yardstick(regions, sigma, multiplier):
    """Per region (states, spreads, winner, true winner, z per angle, facts, tops per angle) by scipy / numpy."""
    out = []
    for prof in regions:
        sweep = pc.yardstick_sweep(prof, sigma, multiplier)
        out.append(sweep + ([pc.yardstick_tops(z) for z in sweep[4]],))
    return out


def check_batch(ctx, regions, n_angles, sigma, weights, multiplier=pc.MULTIPLIER, yard=None):
    """Device == host twin == scipy / numpy on spread, state, winner, smooth and below; the product call gives the debug call's spread, state
    and winner.  Returns (device results, yardstick, set of things seen)."""
    counts, offsets = pc.pack(regions)
    dev = _capi.debug_profile_statistics(ctx, counts, offsets, n_angles, weights, multiplier)
    host = _capi.debug_profile_statistics(None, counts, offsets, n_angles, weights, multiplier)
    for name, d, h in zip(("spread", "state", "winner", "smooth", "below"), dev, host):
        assert same_bits(d, h) if d.dtype == np.float64 else np.array_equal(d, h), (name, [r.shape for r in regions][:8])
    d_counts = ctx.device_alloc(counts.nbytes)
    try:
        ctx.upload(d_counts, counts)
        product = ctx.profile_statistics_dev(d_counts, offsets, n_angles, weights, multiplier)
    finally:
        ctx.device_free(d_counts)
    assert same_bits(product[0], dev[0]) and np.array_equal(product[1], dev[1]) and np.array_equal(product[2], dev[2])
    yard = yardstick(regions, sigma, multiplier) if yard is None else yard
    seen = set()
    with np.errstate(all="ignore"):
        for got, who in ((dev, "device"), (host, "host twin")):
            spread, state, winner, smooth, below = got
            for r, (prof, (states, spreads, win, true_win, zs, facts, tops)) in enumerate(zip(regions, yard)):
                at = (who, r, prof.shape)
                assert same_bits(smooth[offsets[r]:offsets[r + 1]].reshape(n_angles, -1), np.stack(zs)), at
                assert state[r].tolist() == states and int(winner[r]) == win, at
                assert same_bits(spread[r], np.array(spreads, np.float64)), at
                assert same_bits(below[r], np.array([pc.yardstick_below(t, multiplier) for t in tops])), at
    for prof, (states, _sp, win, true_win, _zs, facts, _tops) in zip(regions, yard):
        seen |= {"state%d" % s for s in states} | {k for k, v in facts.items() if v} | {"lds" if prof.shape[1] <= LDS_SAMPLES else "workspace"}
        if win != true_win:
            seen.add("quirk")
        if win < 0:
            seen.add("nothing")
    SEEN.update(seen)
    COUNTS["profiles"] += sum(r.shape[0] for r in regions)
    COUNTS["batches"] += 1
    return dev, yard, seen


# ---- a. the CPU test's five configurations ----

def _configuration_seen(ctx, k):
    if k not in _YARD:
        if "configurations" not in _YARD:
            _YARD["configurations"] = pc.five_configurations()
        n_angles, sigma, weights, regions = _YARD["configurations"][k]
        _YARD[k] = check_batch(ctx, regions, n_angles, sigma, weights)[2]
    return _YARD[k]


@pytest.mark.parametrize("k", range(5))
def test_cpu_configuration_on_the_device(model, k):
    """(80 angles, sigma 2, built-in table), (30, sigma 2, the binding's weights), sigma 0.7, sigma 5.5 (n = 5 at radius 22), sigma 3."""
    assert _configuration_seen(model.ctx, k)


def test_cpu_configurations_meet_every_state_and_quirk_on_the_device(model):
    seen = set().union(*[_configuration_seen(model.ctx, k) for k in range(5)])
    missing = {"state0", "state1", "state2", "wrapped", "plateau", "quirk", "nothing", "lds", "workspace"} - seen
    assert not missing, "the device run did not meet: %s" % sorted(missing)


# ---- b. lengths at which the deal changes ----

DEAL_LENGTHS = [1, 2, 3, 4] + list(range(62, 68)) + list(range(126, 132)) + [2047, 2048, 2049, 2050]


def test_lengths_around_one_and_two_ballots_and_the_lds_limit(model):
    """20 lengths twice over (20 = 4 mod 8: the second round meets each length with another kind), three angles each."""
    rng = np.random.RandomState(31)
    regions = pc.synthetic_regions(rng, 3, DEAL_LENGTHS * 2)
    seen = check_batch(model.ctx, regions, 3, 2, None)[2]
    assert {"lds", "workspace", "state0", "state1", "state2", "plateau"} <= seen, seen
    assert {r.shape[1] for r in regions} == set(DEAL_LENGTHS)


def test_the_longest_profile_the_tables_admit(model):
    """32 767 samples, one angle, every kind of synthetic profile."""
    rng = np.random.RandomState(32)
    regions = pc.synthetic_regions(rng, 1, [32767] * 8)
    dev, yard, seen = check_batch(model.ctx, regions, 1, 2, None)
    assert {"workspace", "state0", "state1"} <= seen and max(t[6][0].size for t in yard) > 1000, seen
    with pytest.raises(RuntimeError, match="region 0"):
        _capi.debug_profile_statistics(model.ctx, np.zeros(32768, np.int32), [0, 32768], 1)


BLOCKS = ((60, 70), (63, 66), (64, 65), (64, 66), (65, 66), (120, 135), (127, 130), (1, -1))


def _block_region(n):
    p = np.zeros((len(BLOCKS), n), np.int32)
    for a, (lo, hi) in enumerate(BLOCKS):
        p[a, lo:(hi if hi > 0 else n + hi)] = 200 + a
    return p


def test_maxima_and_plateaus_on_the_lane_boundaries(model):
    """Blocks on and across samples 64 / 65 and 128 / 129 (sample 64 is lane 63 of one ballot of the peak scan, sample 65 lane 0 of the next),
    under sigma 2 and unsmoothed (radius 0, weight 1: z = y, the plateau is the block itself)."""
    regions = [_block_region(140), _block_region(300)]
    for sigma, weights in ((2, None), (np.array([1.0]), np.array([1.0]))):
        dev, yard, seen = check_batch(model.ctx, regions, len(BLOCKS), sigma, weights)
        assert "plateau" in seen
        for _states, _sp, _w, _t, zs, _f, tops in yard:
            assert all(t.size == 1 for t in tops)                # one maximum per profile: the block
    assert np.array_equal(dev[3][:140 * 8].reshape(8, 140), regions[0].astype(np.float64))


# ---- c. compaction ----

KEPT = (0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 130, 257, 1000)


def _spikes(kept, lead=0):
    """Spikes one zero apart whose heights follow a fixed non-monotonic sequence over seven decades (so that a sum of them depends on its
    order) until `kept` of them exceed 100 (z = 0.1 y > 10); every fifth is at most 100 (filtered; 100 itself gives z = 10, not above), every seventh is two samples wide (a plateau); 12 trailing zeros."""
    y, j, n_kept = [0] * (lead + 1), 0, 0
    while n_kept < kept or (kept == 0 and j < 40):
        low = j % 5 == 4 or kept == 0
        h = (100 if j % 10 == 4 else 1 + (j * 31) % 100) if low else (101 + (j * 7919) % 3000) * (1, 1000, 600001)[j % 3]
        y += [h] * (2 if j % 7 == 3 else 1) + [0]
        n_kept += not low
        j += 1
    return np.array(y + [0] * 12, np.int32).reshape(1, -1)


def test_maxima_are_compacted_completely_and_in_order(model):
    """z = 0.1 y (radius 0): sums of such values depend on their order, so `below` tells a dropped, repeated or displaced maximum.  The numbers
    of kept maxima straddle numpy's pairwise block edges (8, 128) and one, two and four ballots; three cases run on the global-workspace form."""
    w = np.array([0.1])
    regions = [_spikes(k) for k in KEPT] + [_spikes(65, lead=2100), _spikes(129, lead=2050), _spikes(8200)]
    want = list(KEPT) + [65, 129, 8200]                          # (8200: numpy adds stretches of 8192 up one after the other)
    yard = yardstick(regions, w, pc.MULTIPLIER)
    assert [t[6][0].size for t in yard] == want
    assert all(t[5]["plateau"] for t, k in zip(yard, want) if k != 1) and {r.shape[1] > LDS_SAMPLES for r in regions} == {False, True}
    for (_st, _sp, _w, _t, _zs, _f, tops), k in zip(yard, want):  # the case is sensitive: without any one maximum `below` is another number
        full = pc.yardstick_below(tops[0])
        for drop in sorted({0, k // 2, k - 1} if k else ()):
            assert not same_bits(full, pc.yardstick_below(np.delete(tops[0], drop))), (k, drop)
        if 9 <= k <= 1000:                                       # and so is the order: some swap of two neighbours gives another number
            swapped = [np.concatenate([tops[0][:i], tops[0][i + 1:i + 2], tops[0][i:i + 1], tops[0][i + 2:]]) for i in range(k - 1)]
            assert any(not same_bits(full, pc.yardstick_below(t)) for t in swapped), k
    dev = check_batch(model.ctx, regions, 1, w, w, yard=yard)[0]
    assert np.isnan(dev[4][0, 0]) and not np.isnan(dev[4][1:]).any()


# ---- d. batch shape ----

def test_batch_shapes(model):
    ctx = model.ctx
    rng = np.random.RandomState(41)
    mixed = pc.synthetic_regions(rng, 3, [2100, 30, 2049, 64, 2500, 5, 2050, 300])      # the workspace offsets skip the short regions
    dev, yard, seen = check_batch(ctx, mixed, 3, 2, None)
    assert {"lds", "workspace"} <= seen
    order = [5, 2, 7, 0, 3, 6, 1, 4]
    permuted = check_batch(ctx, [mixed[k] for k in order], 3, 2, None, yard=[yard[k] for k in order])[0]
    assert same_bits(permuted[0], dev[0][order]) and np.array_equal(permuted[1], dev[1][order]) and np.array_equal(permuted[2], dev[2][order])
    assert same_bits(permuted[4], dev[4][order])
    assert check_batch(ctx, pc.synthetic_regions(rng, 2, [2049, 2100, 3000, 2051]), 2, 2, None)[2] >= {"workspace"}
    check_batch(ctx, pc.synthetic_regions(rng, 1, [100]), 1, 2, None)
    many = [np.ascontiguousarray(rng.randint(0, 400, (1, 5)), np.int32) for _ in range(70)]      # the selection kernel's second block
    check_batch(ctx, many, 1, 2, None)


# ---- e. winners ----

def _lines(rng, height, n=400):
    y = pc.text_lines(rng, n, 30, 12, height, 3, 5)
    y[:25] = 0
    y[-25:] = 0
    return y.astype(np.int32)


def test_ties_skipped_angles_and_exceptions_in_the_selection(model):
    rng = np.random.RandomState(51)
    t = [_lines(rng, h) for h in (90, 140, 260, 200)]
    zero, faint = np.zeros(400, np.int32), _lines(rng, 4)        # skipped: no minimum at all; no maximum above 10, so the level is NaN
    mirrored = np.stack(t + t[::-1])                             # an angle list that mirrors itself: every spread occurs twice
    quirk = np.stack([zero, faint] + t[:3] + t[2::-1])           # two skipped angles in front: the winner's position is not its index
    nothing = np.stack([zero, faint] * 4)
    exceptions = np.zeros((8, 400), np.int32)
    exceptions[:, 350:] = rng.randint(20, 500, (8, 50))          # the mass at the right end: a minimum lies in the padding (IndexError)
    dev, yard, seen = check_batch(model.ctx, [mirrored, quirk, nothing, exceptions], 8, 2, None)
    states, spreads, win, true_win = yard[0][:4]
    assert states == [0] * 8 and win == true_win == 2 and bits(spreads[2]) == bits(spreads[5]) and spreads[2] > spreads[3]      # the first of two
    assert yard[1][0] == [1, 1] + [0] * 6 and yard[1][2:4] == (2, 4)
    assert yard[2][0] == [1] * 8 and yard[2][2] == -1
    assert yard[3][0] == [2] * 8 and yard[3][2] == 0
    assert dev[2].tolist() == [2, 2, -1, 0] and not dev[0][2:].any()
    assert {"state0", "state1", "state2", "quirk", "nothing"} <= seen


# ---- f. multipliers ----

@pytest.mark.parametrize("multiplier", [20.3, 3.8, 1.0, 0.5, -2.0])
def test_other_multipliers(model, multiplier):
    rng = np.random.RandomState(3)
    prof = np.stack([pc.text_lines(rng, 400, 30, 12, 200, k, 5) for k in range(6)]).astype(np.int32)
    prof[:, :25] = 0
    prof[:, -25:] = 0
    regions = [prof] + pc.synthetic_regions(rng, 6, [64, 65, 2049, 130, 300, 77, 90, 257])
    dev, yard, seen = check_batch(model.ctx, regions, 6, 2, None, multiplier)
    assert "state0" in seen or multiplier <= 1.0


# ---- soft_div / soft_sqrt on the device ----

def test_soft_div_and_soft_sqrt_on_the_device_equal_the_host_and_numpy(model):
    ctx = model.ctx
    div, sqrt = pc.soft_arith_operands()
    want_div, want_sqrt = pc.numpy_results(div, sqrt)
    t, n_sets = time.time(), 0
    for op, families, want in ((0, div, want_div), (1, sqrt, want_sqrt)):
        for name, v in families.items():
            a, b = v if op == 0 else (v, None)
            dev, host = _capi.debug_soft_arith(ctx, op, a, b), _capi.debug_soft_arith(None, op, a, b)
            assert np.array_equal(bits(dev), bits(host)), (op, name, int(np.count_nonzero(bits(dev) != bits(host))))
            assert pc.soft_arith_mismatches(dev, want[name]) == 0 and pc.soft_arith_mismatches(host, want[name]) == 0, (op, name)
            n_sets += a.size
    print(f"[test_gpu_profile_cases] soft_div / soft_sqrt: {n_sets} operand sets on device and host, {time.time() - t:.2f} s")
    assert n_sets >= 200000
    SEEN.add("soft_arith")
