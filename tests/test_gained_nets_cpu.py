"""tests/gained_nets.py: the gained nets are exact, and the committed gains meet the coverage conditions -- no GPU.

(1) ``forward_torch`` in float64 on ``gained(cfg, weights, g)`` gives, for every node of the graph in front of the head conv, exactly g times
the calibrated net's tensor, and from the head conv on -- the softmax included -- exactly the calibrated net's, for every committed gain.
(2) The numpy stand-in of the device (tests/test_step_check_cpu.py ``StandIn``: it saturates and rounds like the formats) runs every hot and
cold variant of the two nets tests/test_gpu_steps_extremes.py runs -- 64 x 96 with n = 3 and 128 x 192 with n = 2, same weights, same
patches -- and the conditions of tests/gained_nets.py (``assert_coverage``) are checked on the float64 step reference of what the stand-in
stored.  The stand-in itself must stay inside the bound, with ``sat_bad == 0``, on every variant."""
import functools

import numpy as np
import pytest
import torch

import step_check as sc
from gained_nets import COLD_GAINS, HOT_GAINS, assert_coverage, gain_tag, gained, image_kernels, node_gains, patches, stores_fp16
from sbb_textline_detection_amd.keras_graph import parse_model_config
from sbb_textline_detection_amd.planner import build_plan
from test_step_check_cpu import StandIn, _fresh
from tools.synth_model import calibrated_model, forward_torch

SHAPES = {"64x96": (64, 96, 3), "128x192": (128, 192, 2)}             # name -> (H, W, n) of tests/test_gpu_steps_extremes.py


@functools.lru_cache(maxsize=None)
def net(shape):
    h, w, n = SHAPES[shape]
    cfg, weights = calibrated_model(2, h, w, seed=12, calib_hw=min(160, max(h, w)))            # tests/gpu_common.make_model(2, h, w, seed=12)
    return cfg, weights, patches(h, w, n)


@functools.lru_cache(maxsize=None)
def variant_reports(shape, precision, g):
    """(plan, {step name: report}) of the stand-in's run of the net gained by g."""
    cfg, weights, x = net(shape)
    plan = build_plan(parse_model_config(cfg), gained(cfg, weights, g), fuse_head=True, fuse_tail=True)
    dev = StandIn(precision, seed=11)
    vals, probs = _fresh(plan, precision, x)
    for s in plan.steps:
        dev.run_step(plan, s, vals, probs)
    return plan, {s.name: sc.check_step(plan, s, vals, precision, probs=probs) for s in plan.steps}


def _taps(graph, weights, x):
    taps = {}
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        out = forward_torch(graph, weights, x.astype(np.float64), torch.float64, taps=taps)
    finally:
        torch.set_num_threads(nt)
    return taps, out


def test_the_gains_are_few_powers_of_two_in_their_ranges():
    assert 1 <= len(HOT_GAINS) <= 4 and 1 <= len(COLD_GAINS) <= 2
    # "around 2^12 to 2^15": 2^16 is there because the conditions ask for it (tests/gained_nets.py) -- the window was not widened for 2^15
    assert all(2.0 ** 12 <= g <= 2.0 ** 16 for g in HOT_GAINS) and all(2.0 ** -19 <= g <= 2.0 ** -16 for g in COLD_GAINS)
    assert sorted({gain_tag(g) for g in HOT_GAINS + COLD_GAINS}) == sorted(gain_tag(g) for g in HOT_GAINS + COLD_GAINS)
    with pytest.raises(AssertionError):
        gain_tag(3.0)


@pytest.mark.parametrize("g", HOT_GAINS + COLD_GAINS, ids=gain_tag)
def test_every_tap_is_exactly_g_times_the_calibrated_tap(g):
    cfg, weights, x = net("64x96")
    graph = parse_model_config(cfg)
    base, p0 = _taps(graph, weights, x[:2])
    hot, p1 = _taps(graph, gained(cfg, weights, g), x[:2])
    head = [n for n in graph.nodes if n.op == "conv"][-1].name
    names = [n.name for n in graph.nodes]
    behind = names[names.index(head):]
    assert len(behind) == 3 and graph.output_name == behind[-1]
    gains = node_gains(graph, g)
    assert all(gains[name] == [(graph.by_name()[name].out_shape[2], 1.0)] for name in behind)
    plain = [name for name in names if name not in behind and all(k == 1.0 for _, k in gains[name])]
    assert plain == [graph.input_name, "zero_padding2d_1"], plain          # the image and its padded copy in front of the stem
    for name in names:
        k = np.concatenate([np.full(c, f) for c, f in gains[name]])          # per channel: a concat with the image is mixed
        assert np.array_equal(hot[name], base[name] * k[None, :, None, None]), name
        assert np.abs(base[name]).max() > 0
    assert np.array_equal(p0, p1)
    # the weights of the calibrated net are left alone, and only the kernels the module names change
    changed = {k for k in weights if k.endswith("kernel:0") and not np.array_equal(weights[k], gained(cfg, weights, g)[k])}
    assert changed == {f"{n}/kernel:0" for n, _ in image_kernels(cfg)} | {f"{head}/kernel:0"}


def test_the_image_kernels_stay_normal_fp16_numbers_on_the_hot_nets():
    cfg, weights, _ = net("64x96")
    found = image_kernels(cfg)
    assert [n for n, _ in found][0] == "conv1" and len(found) == 2
    for g in HOT_GAINS:
        w = gained(cfg, weights, g)
        for name, sl in found:
            k = np.abs(w[f"{name}/kernel:0"][:, :, sl])
            assert k.max() < sc.F16_MAX / 2 and np.median(k[k > 0]) > 2.0 ** -14, (name, gain_tag(g), k.max())


@pytest.mark.parametrize("precision", ["f16", "f16x3"])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("hot", [True, False], ids=["hot", "cold"])
def test_the_gains_meet_the_coverage_conditions_and_the_stand_in_is_clean(hot, shape, precision):
    by_gain = {}
    for g in (HOT_GAINS if hot else COLD_GAINS):
        plan, reps = variant_reports(shape, precision, g)
        by_gain[g] = reps
        for s in plan.steps:
            r = reps[s.name]
            assert not sc.failed(r) and r["sat_bad"] == 0, (gain_tag(g), s.name, r)
            if stores_fp16(s):
                print(f"[coverage {shape} {precision} {gain_tag(g)}] {s.name}: beyond {r['n_beyond']} (below -65504: {r['n_beyond_neg']}) sat {r['n_sat']} "
                      f"sub {r['n_sub']} held {r['n_sub_held']} nonzero {r['n_nonzero']} of {r['n_elem']}; worst err / bound {r['worst']:.3f}")
    assert_coverage(plan, by_gain, hot)


@pytest.mark.parametrize("precision", ["f16", "f16x3"])
def test_a_calibrated_net_has_nothing_at_the_extremes(precision):
    """What the issue says of the suite's nets, and the reason for this file: n_sat == 0, and no subnormal to speak of."""
    plan, reps = variant_reports("64x96", precision, 1.0)
    assert all(r["n_sat"] == 0 and r["sat_bad"] == 0 and r["n_beyond"] == 0 for r in reps.values())
    assert sum(r["n_sub"] for r in reps.values()) < 1e-3 * sum(r["n_nonzero"] for r in reps.values())
