"""The deskew statistic and the slope selection on the device (-m gpu): ``sbbseg_profile_statistics_dev`` against the CPU entry point that
shares its arithmetic and against the scipy path, on the real row counts of every fixture page and of a random page;
``stages.get_slopes(statistics="device")`` against ``statistics="host"`` (today's path, unchanged: the yardstick) and the fixture."""
import time

import numpy as np
import pytest

from sbb_textline_detection_amd import _capi, stages

import slopes_ref

pytestmark = pytest.mark.gpu
T0 = time.time()


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
    print(f"[test_gpu_profile_stats] module wall time {time.time() - T0:.1f} s")


@pytest.fixture(scope="module")
def pages():
    return slopes_ref.load_pages()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _scipy_sweep(prof, sigma=2):
    """(states, spreads, winner) of one region by stages._profile_statistics with stages._deskew_sweep's bookkeeping."""
    states, spreads, appended = [], [], []
    for y in prof:
        try:
            lows, sd = stages._profile_statistics(y, sigma, 20.3)
            if lows.size == 0:
                states.append(1); spreads.append(0.0)
                continue
            states.append(0)
        except IndexError:
            sd = 0
            states.append(2)
        spreads.append(float(sd)); appended.append(sd)
    return states, spreads, (int(np.argmax(np.array(appended))) if appended else -1)


def _check_statistic(ctx, textlines, boxes, scipy_below):
    """Both sweeps: the device statistic on the counts the sweep produced == the CPU entry point on the same counts == scipy."""
    plane = np.ascontiguousarray(textlines, np.uint8)
    d_plane = ctx.stage(plane)
    seen = set()
    for angles in (slopes_ref.SWEEP1, slopes_ref.SWEEP2):
        na = len(angles)
        profiles = ctx.region_deskew_profiles_dev(d_plane, plane.shape[0], plane.shape[1], boxes, angles)
        offsets = _capi.region_deskew_offsets(boxes, na, *plane.shape)
        counts = np.concatenate([p.reshape(-1) for p in profiles]).astype(np.int32)
        d_counts = ctx.device_alloc(counts.nbytes)
        try:
            ctx.upload(d_counts, counts)
            for weights in (None, _capi.gaussian_weights(2)):
                spread, state, winner = ctx.profile_statistics_dev(d_counts, offsets, na, weights)
                h_spread, h_state, h_winner = _capi.profile_statistics_host(counts, offsets, na, weights)
                assert np.array_equal(state, h_state) and np.array_equal(winner, h_winner)
                assert np.array_equal(bits(spread), bits(h_spread)), np.argwhere(bits(spread) != bits(h_spread))[:4]
        finally:
            ctx.device_free(d_counts)
        for r, prof in enumerate(profiles):
            seen |= {"lds" if prof.shape[1] <= 2048 else "workspace"}
            if prof.shape[1] > scipy_below:
                continue
            states, spreads, win = _scipy_sweep(prof)
            assert state[r].tolist() == states and int(winner[r]) == win, (boxes[r], na)
            for k, st in enumerate(states):
                assert st != 0 or bits(spread[r, k]) == bits(np.float64(spreads[k])), (boxes[r], na, k)
            seen |= {"state%d" % s for s in states}
    return seen


def test_device_statistic_equals_the_cpu_entry_point_and_scipy(model, pages):
    ctx = model.ctx
    seen = set()
    for _r, textlines, boxes, _s in pages:
        seen |= _check_statistic(ctx, textlines, boxes, scipy_below=1 << 20)
    textlines, boxes = slopes_ref.random_page()
    seen |= _check_statistic(ctx, textlines, boxes + [[3, 0, 5, 1500]], scipy_below=700)       # (scipy on the long ones takes seconds per box)
    assert {"lds", "workspace", "state0", "state1"} <= seen, seen
    # another sigma: weights from the binding
    regions, textlines, boxes, _s = pages[-1]
    prof = ctx.region_deskew_profiles(textlines, boxes[:2], slopes_ref.SWEEP2)
    offsets = _capi.region_deskew_offsets(boxes[:2], 30, *textlines.shape)
    counts = np.concatenate([p.reshape(-1) for p in prof]).astype(np.int32)
    d_counts = ctx.device_alloc(counts.nbytes)
    try:
        ctx.upload(d_counts, counts)
        for sigma in (0.7, 5.5):
            w = _capi.gaussian_weights(sigma)
            spread, state, winner = ctx.profile_statistics_dev(d_counts, offsets, 30, w)
            for r, p in enumerate(prof):
                states, spreads, win = _scipy_sweep(p, sigma)
                assert state[r].tolist() == states and int(winner[r]) == win
                assert all(st != 0 or bits(spread[r, k]) == bits(np.float64(spreads[k])) for k, st in enumerate(states))
        with pytest.raises(RuntimeError, match="n_angles"):
            ctx.profile_statistics_dev(d_counts, offsets, 0)
        lengths = np.diff(offsets)
        n_bad = next(n for n in (7, 11, 13, 17, 19, 23) if (lengths % n).any())                  # some region does not hold n profiles
        with pytest.raises(RuntimeError, match="region %d:" % int(np.argmax(lengths % n_bad != 0))):
            ctx.profile_statistics_dev(d_counts, offsets, n_bad)
        assert ctx.profile_statistics_dev(d_counts, offsets, 30)[2].shape == (2,)                # the handle works afterwards
    finally:
        ctx.device_free(d_counts)


def test_device_slopes_equal_the_host_path_and_the_fixture(model, pages):
    ctx = model.ctx
    for k, (_r, textlines, boxes, slopes) in enumerate(pages):
        dev = stages.get_slopes(textlines, boxes, ctx, statistics="device")
        assert dev == stages.get_slopes(textlines, boxes, ctx, statistics="host") == slopes, k
        assert dev == stages.get_slopes(textlines, boxes, ctx) == ctx.region_deskew_slopes(textlines, boxes), k
        assert all(isinstance(s, float) for s in dev)
    assert stages.get_slopes(pages[0][1], [], ctx, statistics="device") == []
    assert ctx.region_deskew_slopes(pages[0][1], []) == []
    textlines, boxes = slopes_ref.random_page()
    boxes = boxes + [[3, 0, 5, 1500]]                            # S = 2100: the global-workspace form; boxes[0] is the whole plane
    t = time.time()
    dev = stages.get_slopes(textlines, boxes, ctx, statistics="device")
    t_dev = time.time() - t
    t = time.time()
    host = stages.get_slopes(textlines, boxes, ctx, statistics="host")
    t_host = time.time() - t
    print(f"[get_slopes] random page, {len(boxes)} boxes: device statistics {t_dev * 1e3:.1f} ms, host statistics {t_host * 1e3:.1f} ms; "
          f"{sum(1 for s in dev if s != 0)} non-zero slopes, {sum(1 for s in dev if s <= -50)} from the second sweep")
    assert dev == host
    assert any(s != 0 for s in dev)
    # another sigma goes through the binding's weights
    few = boxes[3:9]
    assert stages.get_slopes(textlines, few, ctx, sigma_des=3, statistics="device") == stages.get_slopes(textlines, few, ctx, sigma_des=3, statistics="host")


class HostStatisticCalled(BaseException):
    """Not an Exception: the host path catches those per angle and per region, as the reference does (main.py:1652, 1739)."""


def test_device_path_does_not_call_scipy(model, pages, monkeypatch):
    import scipy.ndimage
    import scipy.signal

    def boom(*a, **k):
        raise HostStatisticCalled()
    monkeypatch.setattr(scipy.signal, "find_peaks", boom)
    monkeypatch.setattr(scipy.ndimage, "gaussian_filter1d", boom)
    for name in ("gaussian_filter1d", "find_peaks"):             # (stages imports them inside _profile_statistics today)
        if hasattr(stages, name):
            monkeypatch.setattr(stages, name, boom)
    ctx = model.ctx
    for _r, textlines, boxes, slopes in pages:
        assert stages.get_slopes(textlines, boxes, ctx, statistics="device") == slopes
    _r, textlines, boxes, _s = pages[0]
    with pytest.raises(HostStatisticCalled):
        stages.get_slopes(textlines, boxes, ctx, statistics="host")
    assert stages.get_slopes(textlines, boxes, ctx) == pages[0][3]


def test_a_fresh_handle_gives_the_same_slopes(model, pages):
    textlines, boxes = slopes_ref.random_page()
    want = stages.get_slopes(textlines, boxes[1:], model.ctx)
    fresh = _small_model()
    try:
        assert stages.get_slopes(textlines, boxes[1:], fresh.ctx) == want         # the first call of a fresh handle
        assert stages.get_slopes(textlines, boxes[1:], fresh.ctx) == want
    finally:
        fresh.release()


def test_bad_boxes_are_errors_and_the_handle_survives(model, pages):
    ctx = model.ctx
    _r, textlines, boxes, slopes = pages[1]
    h, w = textlines.shape
    for bad in ([0, 0, 0, 5], [-1, 0, 5, 5], [w - 4, 0, 5, 5], [0, h - 4, 5, 5]):
        with pytest.raises(RuntimeError, match="box 1"):
            stages.get_slopes(textlines, [boxes[0], bad], ctx)
        with pytest.raises(RuntimeError, match="box 1"):
            ctx.region_deskew_slopes(textlines, [boxes[0], bad])
    with pytest.raises(RuntimeError, match="radius"):
        ctx.region_deskew_slopes(textlines, boxes, weights=np.zeros(0))                  # radius = -1
    assert stages.get_slopes(textlines, boxes, ctx) == slopes


def test_run_with_slopes_at_full_size_under_both_settings(tmp_path):
    """Three 448 x 448 nets, a 3500 x 2500 page (the set-up of test_gpu_slopes.test_run_with_slopes_at_full_size)."""
    from sbb_textline_detection_amd import clear_session
    from sbb_textline_detection_amd.synthetic import synthetic_page
    from sbb_textline_detection_amd.weights import save_sbbw
    from tools.synth_model import calibrated_model
    specs = {"model_page_mixed_best": (2, 21), "model_strukturerkennung": (4, 22), "model_textline_new": (2, 23)}      # main.py:58-60
    for name, (classes, seed) in specs.items():
        cfg, w = calibrated_model(classes, 448, 448, seed=seed)
        save_sbbw(str(tmp_path / (name + ".sbbw")), cfg, w)
    st = stages.InferenceStages(*[str(tmp_path / (n + ".h5")) for n in specs], model_kwargs={"max_batch": 108})
    page = synthetic_page(3500, 2500, seed=33)
    out_dev = st.run_with_slopes(page, statistics="device")
    out_host = st.run_with_slopes(page, statistics="host")
    out_default = st.run_with_slopes(page)
    assert out_dev[2] is not None and len(out_dev[4]) >= 1
    assert out_dev[4] == out_host[4] == out_default[4]
    assert out_dev[5] == out_host[5] == out_default[5] and len(out_dev[5]) == len(out_dev[4])
    assert st.get_slopes(out_dev[2], out_dev[4], statistics="host") == out_dev[5]
    print(f"[run_with_slopes] 3500 x 2500: {len(out_dev[4])} boxes, {sum(1 for s in out_dev[5] if s != 0)} non-zero slopes under both settings")
    clear_session()
