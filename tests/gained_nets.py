"""A calibrated net with every activation times a power of two -- exact by construction (test helper, no GPU).

Every net of the suite comes from ``tools/synth_model.calibrated_model``: activations of a few units, four orders of magnitude below the
65504 the fp16 formats saturate at and ten above their subnormals.  ``gained(cfg, weights, g)`` returns Keras-level weights of a net whose
every tensor behind the image is the calibrated net's tensor times ``g`` (a power of two) and whose logits -- the head conv's output, its
BatchNormalization, the softmax -- are the calibrated net's.  Gains: 1 for the image, 1 for everything from the head conv's output on, g for
every other tensor.  Add, concat, max-pool, upsampling, padding, cropping and ReLU commute with a positive gain and need nothing.  Per layer,
with gi the gain of its input and go of its output:

  * BatchNormalization: ``moving_mean`` x gi, ``gamma`` x go / gi, ``beta`` x go; variance and eps untouched;
  * conv: bias x go, and the kernel slice of the input channels that arrive with gain gi x go / gi.  For every conv that reads gained tensors
    only (gi = go = g) that is "bias x gi, kernel untouched"; for the head conv (gi = g, go = 1) it is "kernel x 1 / g, bias untouched".
    The image has gain 1 and cannot have another, so the three places where it enters change a kernel: ``conv1`` (the stem; its output is the
    skip f1, stored without ReLU, and has to be hot or cold like the rest) x g, and the three image channels of the last decoder conv's
    kernel x g.  No other kernel changes; in the 16-bit weight formats those slices stay far inside the normal range on the hot nets
    (asserted by the CPU test) and go through fp16 subnormals on the cold ones -- as MFMA B operands.

All factors are powers of two: in float64, and in fp32 short of over- and underflow, nothing is rounded, so ``forward_torch`` in float64
gives exactly g times every calibrated tap (tests/test_gained_nets_cpu.py).

HOT_GAINS / COLD_GAINS are fixed by conditions on the float64 step reference alone (``coverage``; tests/test_gained_nets_cpu.py checks them
on the numpy stand-in of the device, tests/test_gpu_steps_extremes.py again on what the device stored):
  hot   every plan step that stores an fp16 output has, in at least one hot variant, between 1 % and 60 % of its reference elements beyond
        65504 in magnitude before the clip AND at least 20 % strictly inside; every such step without ReLU has, in some hot variant, at
        least 16 elements below -65504;
  cold  every such step has, in some cold variant, at least half of its nonzero reference elements below 2^-14 in magnitude AND at least 16
        elements in [2^-24, 2^-14) -- subnormals fp16 can hold.
What the reference says of the candidates (64 x 96, n = 3 and 128 x 192, n = 2; both precisions alike): at 2^12 to 2^14 most steps have nothing
beyond the range; at 2^15 the stem (10.7 % beyond, 10794 elements below -65504), the pool and the block outputs meet the hot conditions but the
1x1 / 3x3 convs inside the blocks and the decoder convs stay at 0.0 to 0.8 %, under the 1 % the window asks for; at 2^16 every step lies
between 2.4 % and 41 %.  So 2^16 is added rather than the window widened, and 2^15 stays as the variant with more of each tensor in range.
At 2^-17 every step has 64 % to 100 % of its nonzero elements below 2^-14, thousands of them representable: one cold gain."""
import numpy as np

from sbb_textline_detection_amd.keras_graph import parse_model_config
from sbb_textline_detection_amd.synthetic import synthetic_page

HOT_GAINS = (2.0 ** 15, 2.0 ** 16)
COLD_GAINS = (2.0 ** -17,)

HOT_WINDOW = (0.01, 0.60)       # fraction of reference elements beyond 65504 before the clip
HOT_INSIDE = 0.20               # fraction strictly inside the range, same variant
MIN_NEGATIVE = 16               # elements below -65504, steps without ReLU
COLD_FRACTION = 0.5             # of the nonzero reference elements, below 2^-14
MIN_SUBNORMAL = 16              # elements in [2^-24, 2^-14)


def patches(h, w, n, seed=33):
    """n patches [n, h, w, 3] in [0, 1] cut from a synthetic page (the rule of tests/gpu_common.patches_from_page, importable without the library)."""
    page = synthetic_page(max(h * 2, 600), max(w * 3, 900), seed)
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        y0 = rng.randint(0, page.shape[0] - h)
        x0 = rng.randint(0, page.shape[1] - w)
        out.append(page[y0:y0 + h, x0:x0 + w])
    return (np.stack(out) / 255.0).astype(np.float32)


def gain_tag(g):
    """"gain15" / "gain-16": the k of g = 2^k, as the result files name a variant."""
    m, e = np.frexp(float(g))
    assert m == 0.5, f"{g} is no power of two"
    return f"gain{int(e) - 1}"


def node_gains(graph, g):
    """{node name: [(channels, gain)] runs of its output channels}."""
    last_conv = [n for n in graph.nodes if n.op in ("conv", "convT")][-1]
    behind_head = set()
    runs = {}
    for n in graph.nodes:
        c = n.out_shape[2]
        if n.op == "input":
            runs[n.name] = [(c, 1.0)]
        elif n.name == last_conv.name or any(i in behind_head for i in n.inputs):
            behind_head.add(n.name)
            runs[n.name] = [(c, 1.0)]
        elif n.op in ("conv", "convT", "bn"):
            runs[n.name] = [(c, g)]
        elif n.op == "concat":
            runs[n.name] = [r for i in n.inputs for r in runs[i]]
        elif n.op == "add":
            a, b = (runs[i] for i in n.inputs)
            assert a == b, (n.name, a, b)
            runs[n.name] = a
        else:                                                            # zeropad, act, maxpool, upsample, crop_last: channel-wise
            assert n.op != "act" or n.attrs["kind"] in ("relu", "linear"), n.name     # (positively homogeneous)
            runs[n.name] = runs[n.inputs[0]]
    return runs


def _per_channel(runs):
    return np.concatenate([np.full(c, k) for c, k in runs])


def gained(cfg, weights, g):
    """Keras-level weights (a new dict of new arrays) of the net whose every tensor is `g` times the net of `weights`, logits unchanged."""
    gain_tag(g)
    graph = parse_model_config(cfg)
    runs = node_gains(graph, float(g))
    out = {k: np.array(v, copy=True) for k, v in weights.items()}
    mul = lambda key, f: out.__setitem__(key, (out[key].astype(np.float64) * f).astype(out[key].dtype))
    for n in graph.nodes:
        if n.op in ("conv", "convT"):
            gi, (_, go) = _per_channel(runs[n.inputs[0]]), runs[n.name][0]
            f = go / gi                                                  # per input channel
            if not np.all(f == 1.0):
                mul(f"{n.name}/kernel:0", f[None, None, :, None] if n.op == "conv" else f[None, None, None, :])
            if n.attrs["use_bias"]:
                mul(f"{n.name}/bias:0", go)
        elif n.op == "bn":
            (gi_runs, (_, go)) = runs[n.inputs[0]], runs[n.name][0]
            assert len(set(k for _, k in gi_runs)) == 1, (n.name, gi_runs)
            gi = gi_runs[0][1]
            mul(f"{n.name}/moving_mean:0", gi)
            if n.attrs.get("scale", True):
                mul(f"{n.name}/gamma:0", go / gi)
            else:
                assert go == gi, n.name
            if n.attrs.get("center", True):
                mul(f"{n.name}/beta:0", go)
    for k in out:
        assert np.isfinite(out[k]).all(), k
    return out


def image_kernels(cfg):
    """[(conv name, slice of its input channels)] of the kernel slices that read the image: the only kernels a gain changes besides the head's."""
    graph = parse_model_config(cfg)
    runs = node_gains(graph, 2.0)
    found = []
    for n in graph.nodes:
        if n.op in ("conv", "convT") and runs[n.name][0][1] == 2.0:
            c0 = 0
            for c, k in runs[n.inputs[0]]:
                if k == 1.0:
                    found.append((n.name, slice(c0, c0 + c)))
                c0 += c
    return found


# ------------------------------------------------------------------------------------------------ coverage conditions
def stores_fp16(step):
    """A plan step that stores an output in the activation format (the tail and the head's own op keep logits only; a max-pool without
    pre-affine copies stored numbers)."""
    if step.kind == "conv":
        return step.out >= 0 or step.raw_out >= 0
    return step.kind == "maxpool" and step.pre_scale is not None


def has_unrectified_store(step):
    """The step stores an output no ReLU precedes: negative saturation can occur."""
    if step.kind == "conv":
        return step.raw_out >= 0 or (step.out >= 0 and not step.relu)
    return step.kind == "maxpool" and step.pre_scale is not None and not step.pre_relu


def coverage(rep):
    """(hot, negative, cold) of one report of step_check.check_step: which conditions of the module docstring the step meets in this variant."""
    n = max(rep["n_elem"], 1)
    beyond = rep["n_beyond"] / n
    hot = HOT_WINDOW[0] <= beyond <= HOT_WINDOW[1] and (rep["n_elem"] - rep["n_sat"]) / n >= HOT_INSIDE
    negative = rep["n_beyond_neg"] >= MIN_NEGATIVE
    cold = rep["n_nonzero"] > 0 and rep["n_sub"] >= COLD_FRACTION * rep["n_nonzero"] and rep["n_sub_held"] >= MIN_SUBNORMAL
    return hot, negative, cold


def assert_coverage(plan, reports_by_gain, hot, skip=()):
    """`reports_by_gain`: {gain: {step name: report}} over the hot (or the cold) variants of one plan and precision.  `skip`: names of steps
    that have no report (a fused kernel keeps one of their tensors in LDS)."""
    missing = []
    for s in plan.steps:
        if not stores_fp16(s) or s.name in skip:
            continue
        cov = [coverage(reps[s.name]) for reps in reports_by_gain.values()]
        if hot:
            if not any(c[0] for c in cov):
                missing.append((s.name, "saturated fraction", [(gain_tag(k), r[s.name]["n_beyond"], r[s.name]["n_sat"], r[s.name]["n_elem"]) for k, r in reports_by_gain.items()]))
            if has_unrectified_store(s) and not any(c[1] for c in cov):
                missing.append((s.name, "negative saturation", [(gain_tag(k), r[s.name]["n_beyond_neg"]) for k, r in reports_by_gain.items()]))
        elif not any(c[2] for c in cov):
            missing.append((s.name, "subnormals", [(gain_tag(k), r[s.name]["n_sub"], r[s.name]["n_sub_held"], r[s.name]["n_nonzero"]) for k, r in reports_by_gain.items()]))
    assert not missing, missing
