"""The three small non-ResNet nets of the suite, with the weights and inputs of their end-to-end tests (test helper, no GPU):
tests/golden/keras23_model_config.json as test_handwritten_keras23_fixture_through_c_abi runs it and transpose_unet_config(3, 64, 96, k)
as test_conv2d_transpose_decoder_through_c_abi does.  Their plans hold what no ResNet-50-U-Net plan has (asserted by
``assert_odd_geometries``): non-square taps, a stride that differs between the axes, a second source at an offset, stride-2 convs
without top / left padding, a 3-class head in a conv's epilogue."""
import functools
import json
import os

import numpy as np

from sbb_textline_detection_amd.keras_graph import parse_model_config, transpose_unet_config
from sbb_textline_detection_amd.planner import build_plan
from sbb_textline_detection_amd.synthetic import synthetic_page
from sbb_textline_detection_amd.weights import synthetic_weights

SMALL_PLANS = ("keras23", "convT_k2", "convT_k3")


def _patches_from_page(h, w, n, seed):
    """tests/gpu_common.py patches_from_page (whose module needs the built library)."""
    page = synthetic_page(max(h * 2, 600), max(w * 3, 900), seed)
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        y0 = rng.randint(0, page.shape[0] - h)
        x0 = rng.randint(0, page.shape[1] - w)
        out.append(page[y0:y0 + h, x0:x0 + w])
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def small_net(name):
    """(model_config, {weight name: array}, x float32 [3, h, w, 3]) -- shared, leave unchanged."""
    if name == "keras23":
        cfg = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keras23_model_config.json")))
        w = synthetic_weights(parse_model_config(cfg), seed=5)
        rng = np.random.RandomState(2)
        for key in list(w):
            if key.endswith("moving_variance:0"):
                w[key] = rng.uniform(0.5, 2.0, w[key].shape).astype(np.float32)
        return cfg, w, rng.rand(3, 32, 48, 3).astype(np.float32)
    k = {"convT_k2": 2, "convT_k3": 3}[name]
    cfg = transpose_unet_config(3, 64, 96, k=k)
    w = synthetic_weights(parse_model_config(cfg), seed=4)
    return cfg, w, (_patches_from_page(64, 96, 3, seed=6) / 255.0).astype(np.float32)


def small_plan(name, precision):
    """The plan SegModel builds for `precision` with nothing set in the environment (model.py SegModel._plan_args)."""
    cfg, w, _ = small_net(name)
    return build_plan(parse_model_config(cfg), w, fuse_head=precision != "f32", fuse_tail=precision != "f32")


def assert_odd_geometries(name, plan, precision):
    """What makes the plan worth checking step by step."""
    convs = [s for s in plan.steps if s.kind == "conv"]
    srcs = [g for s in convs for g in s.srcs]
    if name == "keras23":
        assert any((g.kh, g.kw) == (7, 4) and (g.stride_y, g.stride_x) == (2, 1) for g in srcs)        # the stem's pair taps
        assert any(g.stride_y != g.stride_x for g in srcs)
        assert any(g.off_y > 0 and g.off_x > 0 for s in convs for g in s.srcs[1:])                     # second source at (1, 1)
        assert any((g.kh, g.kw, g.stride_y, g.stride_x) == (1, 1, 2, 2) for g in srcs)                 # stride-2 1 x 1 projection
        assert {8, 16, 24, 32} <= {s.cout for s in convs}
    else:
        assert any(g.stride_y == 2 and g.kh == 3 and g.pad_top == 0 and g.pad_left == 0 for g in srcs)
        taps = {(g.kh, g.kw) for s in convs if s.out_stride == (2, 2) for g in s.srcs}
        assert taps == ({(1, 1)} if name == "convT_k2" else {(1, 1), (2, 1), (1, 2), (2, 2)}), taps
    if name != "convT_k2":
        assert any(g.kh != g.kw for g in srcs)
    if precision != "f32":
        assert any(s.head is not None and s.head.classes == 3 and s.cout == 32 for s in convs)
    else:
        assert plan.steps[-1].kind == "head" and plan.steps[-1].classes == 3
