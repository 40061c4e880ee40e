"""One plan step against a float64 reference of THAT step, with a derived per-element error bound (test helper, no GPU).

Every other forward check of the suite compares a tensor with the oracle's tensor after the whole chain in front of it, in a
range-relative max norm.  Here nothing is carried over: the step's inputs are read as the device stored them
(``debug_read_tensor``: fp16 / bf16 widened, ``hi + lo`` in the split mode -- exact images of the stored numbers), the step is
evaluated in float64 with the weights quantised the way ``sbbseg_add_conv`` / ``sbbseg_add_tail`` quantise them, and every output
element is held to the largest error correct device arithmetic can make on it.  The data model and the geometry are those of
``tests/plan_interp.py`` (``source_conv``), evaluated with ``torch.nn.functional.conv2d`` in float64.

Weights (``quantise_weights``; csrc/wpack.h wins over any prose):
  * f32: unchanged.  f16 / bf16: one RNE rounding of the fp32 weight (``f32_to_f16_rne`` saturates at +-65504).
  * f16x3: one power of two ``pre`` per conv (``frexp``: the largest |w| of ALL the conv's sources lands in [256, 512)),
    ``hi = f16(w * pre)``, ``lo = f16(w * pre - hi)``; the kernels multiply with ``hi`` and ``lo`` and the epilogue multiplies
    ``scale`` by ``1 / pre`` (``wmul_cls``), both exact, so the effective weight is ``(hi + lo) / pre`` with the plan's own scale.
  * the fused tail pre-sums the taps of a 3x3 window that read the same stored pixel of the upsampled source IN FP32 (ky outer, kx
    inner, starting from 0.f) before it rounds; in the split mode ONE ``pre`` is taken over the four classes' pre-summed weights and
    the image taps together.  (The parity-split decoder convs arrive pre-summed from the planner, in float64 rounded once to fp32.)

Bound of one output element (``u32 = 2^-24``, the fp32 unit roundoff; S = sum_i |a_i| |w_i| from the same float64 convolution
on absolute values; K = sum over sources of kh * kw * channels, the number of products of one output element):
  * accumulation, ``n_add * 2^-23 * S``: the running sum of n_add terms is rounded at most n_add times, each time by at most one
    unit of a partial sum that never exceeds S in magnitude (to first order); 2^-23 instead of 2^-24 so that the bound holds
    whether the MFMA accumulator rounds to nearest or truncates.  The products themselves are exact in fp32 (11 x 11 or 8 x 8 bit
    significands); in the f32 mode every product is fused into its addition (``fmaf``).  n_add = K, and 3 K in the split mode,
    which issues hi*hi, hi*lo and lo*hi as three MFMAs per product.  Zero padding of K adds exact zeros.
    Split-K launch (the whole-image branch: ``conv_igemm_mfma<..KS>`` + ``splitk_finish``), ``extra_adds = splits - 1``: each of the
    `splits` blocks of a tile accumulates its own contiguous K-range in fp32 as above -- together the same K (3 K) roundings, every
    partial sum still bounded by S -- and stores it multiplied by the power-of-two ``wmul_cls`` (exact).  The finish adds the `splits`
    planes in split order starting from 0.f: the first addition to zero is exact, the other splits - 1 each round a partial sum
    bounded by S once more.  So n_add = K (3 K) + splits - 1; the epilogue behind it is the unsplit one.  No other term.
  * split mode only, ``2^-21 * S``: the dropped lo * lo products.  |lo| <= 2^-11 |hi| on both sides gives 2^-22 S; the stored
    operands ARE hi + lo (activations as read back, weights as quantised here), so no representation residue is left on top, and
    the term is kept at the 2^-21 S the format is held to elsewhere (a factor of two above what is derived, not below).
  * epilogue in fp32, carried as (value, error) pairs through ``_mul`` / ``_add``: a product with an fp32 constant scales the
    incoming error by |s| and adds u32 * |result|; a sum with an exactly known fp32 term (shift, stored residual) adds
    u32 * |result|; the magnitudes include the incoming error, so nothing is first-order only.  The device uses ``fmaf`` (one
    rounding) or a product and a sum (two): the two-rounding form is assumed everywhere.  In the split mode the residual is
    ``hi + lo`` added in fp32 first (exact: 22 significant bits), then to the value (``add_split8``): one rounding, as modelled.
  * ReLU and the saturation to +-65504 of the fp16 formats (``pack_f16x2`` / ``split_f32``) are 1-Lipschitz: the error passes
    through; the reference saturates too.  On top of the bound, at the extremes (tests/gained_nets.py): an element whose float64
    value in front of the clip lies beyond +-65504 by more than its own bound cannot have been inside the range in correct
    arithmetic, so its stored value must be exactly +-65504 with that sign -- in the split mode hi + lo, that is lo = 0
    (``sat_bad``, which ``failed`` counts; ``n_sat`` / ``n_sub`` say how much of a step sits at the clip / below 2^-14).
  * one output rounding, ``u * |v| + sub``: u = 2^-11 (f16), 2^-8 (bf16), 2^-21 (split: hi = f16(v), lo = f16(v - hi) leaves at
    most 2^-11 * 2^-11 |v|; 2^-21 is the figure ``test_ingest_forms`` holds the format to), 2^-24 (f32: the fp32 store is exact, the
    term covers nothing and costs nothing); sub = 2^-25, half the spacing of fp16 subnormals, for the fp16 formats (the rounding
    of a value, or of a lo half, below 2^-14 is absolute).
  * max-pool: the maximum is 1-Lipschitz in the sup norm, so the bound of an output is the largest bound in its window (the
    pre-affine ``fmaf`` + ReLU as above) plus the output rounding; without a pre-affine the step is exact (bound 0).
  * head (own op, fused into a conv's epilogue, or the tail's): logits = (sum_c z_c w_c) * scale + shift in fp32 on the UNROUNDED
    z of a fused producer (stored z for the own op), head weights in fp32.  Error: sum_c |w_c| e_c from z, plus
    ``cin * 2^-23 * sum_c (|z_c| + e_c) |w_c|`` for the fp32 fma chain and the lane reduction, then ``_mul`` / ``_add``.
    Labels must equal the float64 argmax wherever the float64 top-2 logit margin exceeds 2 d (d = the largest logit bound of the
    pixel).  The probabilities depend on the device's ``expf``: their tolerance is measured (tests/gpu_common.py), not derived.
No term is a fitted constant."""
import numpy as np
import torch
import torch.nn.functional as F

from sbb_textline_detection_amd.planner import ConvStep, Seg

U32 = 2.0 ** -24
U_OUT = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8, "f16x3": 2.0 ** -21, "f32": 2.0 ** -24}
SUBNORMAL = {"f16": 2.0 ** -25, "bf16": 0.0, "f16x3": 2.0 ** -25, "f32": 0.0}
F16_MAX = 65504.0
F16_MIN_NORMAL = 2.0 ** -14
F16_MIN_SUBNORMAL = 2.0 ** -24
SATURATING = ("f16", "f16x3")
_PARITY_TAPS = {(0, 0): (0, 0), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2, 2)}      # [parity][t] -> first, last tap summed (wpack.h `taps`)


# ------------------------------------------------------------------------------------------------ number formats
def _f16(a32):
    return np.clip(np.asarray(a32, np.float32), -F16_MAX, F16_MAX).astype(np.float16).astype(np.float32)


def _bf16(a32):
    t = torch.from_numpy(np.ascontiguousarray(a32, np.float32))
    return t.to(torch.bfloat16).to(torch.float32).numpy()


def split_halves(v32):
    """(hi, lo) fp16 halves of fp32 values, as fp32 arrays: hi = f16(v) saturating, lo = f16(v - hi) (device_prims.h split_f32)."""
    v32 = np.clip(np.asarray(v32, np.float32), -F16_MAX, F16_MAX)
    hi = v32.astype(np.float16).astype(np.float32)
    lo = (v32 - hi).astype(np.float16).astype(np.float32)
    return hi, lo


def round_storage(precision, v32):
    """fp32 values -> the fp32 image of what the activation format of `precision` stores."""
    v32 = np.asarray(v32, np.float32)
    if precision == "f32":
        return v32
    if precision == "f16":
        return _f16(v32)
    if precision == "bf16":
        return _bf16(v32)
    hi, lo = split_halves(v32)
    return hi + lo


def split_prescale(ws):
    """The power of two sbbseg_add_conv / sbbseg_add_tail scale a conv's weights by in the split mode (largest |w| -> [256, 512))."""
    wmax = max(float(np.abs(np.asarray(w, np.float32)).max()) for w in ws)
    if not wmax > 0:
        return 1.0
    _, ex = np.frexp(np.float32(wmax))
    return float(np.ldexp(1.0, int(np.clip(9 - int(ex), -60, 60))))


def split_weights(ws):
    """([(hi, lo) per array], pre): the two fp16 planes of the pre-scaled weights as fp32 arrays."""
    pre = split_prescale(ws)
    out = []
    for w in ws:
        sv = np.asarray(w, np.float32) * np.float32(pre)                 # exact (power of two)
        hi = _f16(sv)
        out.append((hi, _f16(sv - hi)))
    return out, pre


def quantise_weights(precision, w):
    """Effective weights the device multiplies with, float64.  `w`: one fp32 array, or the list of arrays of ONE conv (they share
    the split mode's pre-scale).  Split mode: (hi + lo) / pre -- the epilogue's `scale / pre` is folded back in, so callers keep
    the plan's own scale.  Differs from a per-array rule in exactly that: plan_build.hip takes `wmax` over all sources of the conv."""
    single = isinstance(w, np.ndarray)
    ws = [w] if single else list(w)
    if precision == "f32":
        out = [np.asarray(a, np.float32).astype(np.float64) for a in ws]
    elif precision == "f16":
        out = [_f16(a).astype(np.float64) for a in ws]
    elif precision == "bf16":
        out = [_bf16(a).astype(np.float64) for a in ws]
    elif precision == "f16x3":
        halves, pre = split_weights(ws)
        out = [(hi.astype(np.float64) + lo.astype(np.float64)) / pre for hi, lo in halves]
    else:
        raise ValueError(precision)
    return out[0] if single else out


def tail_class_weights(step):
    """The fused tail as its four output-parity classes: [(py, px, w2 [2][2][64][32] fp32 pre-summed as the host does, w_img)]."""
    out = []
    for py in (0, 1):
        for px in (0, 1):
            w2 = np.zeros((2, 2) + step.w_src0.shape[2:], np.float32)
            for ty in (0, 1):
                for tx in (0, 1):
                    v = np.zeros(step.w_src0.shape[2:], np.float32)
                    for ky in range(_PARITY_TAPS[(py, ty)][0], _PARITY_TAPS[(py, ty)][1] + 1):
                        for kx in range(_PARITY_TAPS[(px, tx)][0], _PARITY_TAPS[(px, tx)][1] + 1):
                            v = (v + np.asarray(step.w_src0[ky, kx], np.float32)).astype(np.float32)
                    w2[ty, tx] = v
            out.append((py, px, w2, np.asarray(step.w_img, np.float32)))
    return out


def tail_class_steps(step):
    """Pseudo ConvSteps (planner geometry of a parity-split decoder conv) of the tail's four classes, weights still fp32."""
    steps = []
    for py, px, w2, wi in tail_class_weights(step):
        srcs = [Seg(step.src0, 64, 0, 0, 0, 2, 2, 1, 1, 1 - py, 1 - px, w2), Seg(step.img, 3, 0, 0, 0, 3, 3, 2, 2, 1 - py, 1 - px, wi)]
        steps.append(ConvStep(f"{step.name}:p{py}{px}", srcs, cout=32, out_h=step.out_h // 2, out_w=step.out_w // 2,
                              scale=step.scale, shift=step.shift, out_stride=(2, 2), out_off=(py, px), relu=True, head=step.head))
    return steps


# ------------------------------------------------------------------------------------------------ float64 geometry
def source_input(vals, g, dtype=np.float64):
    a = np.asarray(vals[g.tensor][..., :g.channels], dtype)
    if g.shift:
        a = np.repeat(np.repeat(a, 2, axis=1), 2, axis=2)
    return a


def source_conv64(a, w, g, out_h, out_w):
    """plan_interp.source_conv in float64: a [n,h,w,c] (already upsampled), w [kh][kw][c][cout] -> [n,out_h,out_w,cout]."""
    n, h, wd, c = a.shape
    need_h = (out_h - 1) * g.stride_y - g.pad_top + g.kh
    need_w = (out_w - 1) * g.stride_x - g.pad_left + g.kw
    t = torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 1, 2)))
    # logical tensor: data at (off_y, off_x), zero elsewhere; the conv sees rows [-pad_top, need_h) of it (negative pad = crop)
    t = F.pad(t, (g.pad_left + g.off_x, need_w - (g.off_x + wd), g.pad_top + g.off_y, need_h - (g.off_y + h)))
    k = torch.from_numpy(np.ascontiguousarray(np.asarray(w, np.float64).transpose(3, 2, 0, 1)))
    y = F.conv2d(t, k, None, (g.stride_y, g.stride_x))
    assert y.shape[2] == out_h and y.shape[3] == out_w, (y.shape, out_h, out_w)
    return y.permute(0, 2, 3, 1).numpy()


def placed(arr, s):
    """The elements of a stored tensor that step `s` writes (strided output placement)."""
    (sy, sx), (oy, ox) = s.out_stride, s.out_off
    return arr[:, oy::sy, ox::sx][:, :s.out_h, :s.out_w]


def _mul(v, e, s):
    r = v * s
    e = e * np.abs(s)
    return r, e + U32 * (np.abs(r) + e)


def _add(v, e, b):
    r = v + b
    return r, e + U32 * (np.abs(r) + e)


def _store(precision, v, e):
    if precision in SATURATING:
        v = np.clip(v, -F16_MAX, F16_MAX)
    return v, e + U_OUT[precision] * (np.abs(v) + e) + SUBNORMAL[precision]


def step_K(step):
    if step.kind == "conv":
        return int(sum(g.kh * g.kw * g.channels for g in step.srcs))
    if step.kind == "tail":
        return 4 * 64 + 9 * 3
    if step.kind == "head":
        return int(step.cin)
    return 0


def _head(hd, z, e):
    """(logits, bound) of the 1x1 head on values z with error e, float64 [..., classes]."""
    w = np.asarray(hd.w, np.float64)
    lg = z @ w
    err = e @ np.abs(w) + hd.cin * 2.0 ** -23 * ((np.abs(z) + e) @ np.abs(w))
    lg, err = _mul(lg, err, np.asarray(hd.scale, np.float64))
    return _add(lg, err, np.asarray(hd.shift, np.float64))


def _conv_outputs(s, vals, precision, weff, extra_adds=0):
    split = precision == "f16x3"
    y = S = 0.0
    for g, w in zip(s.srcs, weff):
        a = source_input(vals, g)
        y = y + source_conv64(a, w, g, s.out_h, s.out_w)
        S = S + source_conv64(np.abs(a), np.abs(w), g, s.out_h, s.out_w)
    n_add = step_K(s) * (3 if split else 1) + extra_adds
    acc = n_add * 2.0 ** -23 * S + (2.0 ** -21 * S if split else 0.0)
    ref, bound, pre = {}, {}, {}
    if s.raw_out >= 0:
        v, e = _mul(y, acc, np.asarray(s.raw_scale, np.float64))
        v, e = _add(v, e, np.asarray(s.raw_shift, np.float64))
        pre["raw_out"] = v
        ref["raw_out"], bound["raw_out"] = _store(precision, v, e)
    v, e = _mul(y, acc, np.asarray(s.scale, np.float64))
    v, e = _add(v, e, np.asarray(s.shift, np.float64))
    if s.residual >= 0:
        v, e = _add(v, e, np.asarray(placed(vals[s.residual], s), np.float64))
    if s.relu:
        v = np.maximum(v, 0.0)
    if s.out >= 0:
        pre["out"] = v
        ref["out"], bound["out"] = _store(precision, v, e)
    if s.head is not None:
        ref["logits"], bound["logits"] = _head(s.head, v, e)
    return ref, bound, pre


def _maxpool64(x, k, stride):
    t = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2)))
    return F.max_pool2d(t, k, stride).permute(0, 2, 3, 1).numpy()


def step_reference(plan, step, vals, precision, extra_adds=0):
    """step_reference_pre without the values before the clip."""
    return step_reference_pre(plan, step, vals, precision, extra_adds)[:2]


def step_reference_pre(plan, step, vals, precision, extra_adds=0):
    """(ref, bound, pre): dicts of float64 arrays keyed by the outputs the step has -- "out", "raw_out" (on the step's own output grid,
    see `placed`) and "logits" ([n, out_h, out_w, classes] of a head, fused or not); `pre` holds, for the stored outputs, the float64 value in
    front of the saturation to +-65504 (equal to `ref` where nothing clips, and in the formats that do not saturate).  `extra_adds`: further fp32 additions of partial
    sums on top of the K (3 K) of the contraction -- ``splits - 1`` for a conv launched split-K (module docstring); convs only."""
    assert extra_adds == 0 or step.kind == "conv", (step.name, step.kind, extra_adds)
    if step.kind == "conv":
        return _conv_outputs(step, vals, precision, quantise_weights(precision, [g.w for g in step.srcs]), extra_adds)
    if step.kind == "tail":
        classes = tail_class_steps(step)
        flat = quantise_weights(precision, [c.srcs[0].w for c in classes] + [classes[0].srcs[1].w])      # one pre-scale for all
        n = vals[step.src0].shape[0]
        lg = np.zeros((n, step.out_h, step.out_w, step.head.classes))
        bd = np.zeros_like(lg)
        for q, c in enumerate(classes):
            r, b, _ = _conv_outputs(c, vals, precision, [flat[q], flat[4]])
            placed(lg, c)[...] = r["logits"]
            placed(bd, c)[...] = b["logits"]
        return {"logits": lg}, {"logits": bd}, {}
    if step.kind == "maxpool":
        x = np.asarray(vals[step.src], np.float64)
        e = np.zeros_like(x)
        if step.pre_scale is not None:
            x, e = _mul(x, e, np.asarray(step.pre_scale, np.float64))
            x, e = _add(x, e, np.asarray(step.pre_shift, np.float64))
            if step.pre_relu:
                x = np.maximum(x, 0.0)
            p, e = _maxpool64(x, step.k, step.stride), _maxpool64(e, step.k, step.stride)
            v, e = _store(precision, p, e)
        else:
            p = v = _maxpool64(x, step.k, step.stride)
            e = np.zeros_like(v)
        return {"out": v}, {"out": e}, {"out": p}
    if step.kind == "head":
        z = np.asarray(vals[step.src], np.float64)
        lg, e = _head(step, z, np.zeros_like(z))
        return {"logits": lg}, {"logits": e}, {}
    raise ValueError(step.kind)


def softmax64(lg):
    ex = np.exp(lg - lg.max(axis=-1, keepdims=True))
    return ex / ex.sum(axis=-1, keepdims=True)


def step_got(plan, step, vals):
    """The stored elements that `step` wrote, keyed like step_reference's outputs (no logits: the device keeps none)."""
    got = {}
    if step.kind == "conv":
        if step.out >= 0:
            got["out"] = placed(vals[step.out], step)
        if step.raw_out >= 0:
            got["raw_out"] = placed(vals[step.raw_out], step)
    elif step.kind == "maxpool":
        got["out"] = vals[step.dst]
    return got


def step_tensors(step):
    """(tensor ids the step reads, tensor ids it writes)."""
    if step.kind == "conv":
        return ([g.tensor for g in step.srcs] + ([step.residual] if step.residual >= 0 else []),
                [t for t in (step.out, step.raw_out) if t >= 0])
    if step.kind == "tail":
        return [step.src0, step.img], []
    if step.kind == "maxpool":
        return [step.src], [step.dst]
    return [step.src], []


def _mask_of(mask, key, shape):
    """bool array broadcastable to `shape` ([n, h, w, c]): the mask of output `key`, everything where there is none."""
    if mask is None or key not in mask:
        return np.ones((1,) * len(shape), bool)
    m = np.asarray(mask[key], bool)
    assert m.shape == tuple(shape[:3]), (key, m.shape, shape)
    return m[..., None]


def check_step(plan, step, vals, precision, probs=None, mask=None, extra_adds=0):
    """Compare what the device stored for `step` with its float64 reference.  `probs`: the device's softmax [n,H,W,classes], for a
    step that carries the head.  `mask`: dict keyed like the outputs ("out", "raw_out", "logits") of bool [n, out_h, out_w] on the
    step's own output grid -- elements outside it count nowhere (an owned-region launch writes, and is owed, only a part of the grid);
    an output without a key counts whole.  `extra_adds`: see step_reference (``splits - 1`` of a split-K launch).  Returns a report dict:
      worst     largest |got - ref| / bound over all elements of all stored outputs (inf where the bound is 0 and the error is not)
      index     (output key, patch, y, x, channel) of that element, on the step's own output grid
      n_over    elements with |got - ref| > bound;  n_nan / n_inf  non-finite stored elements where the reference is finite
      n_ref_bad non-finite reference elements (a poisoned source)
      rms       rms of err / bound;  ref_absmax  largest |ref| (0: the step proves nothing)
      abs_err, old_rel   max |err| and max |err| / max |ref| (the range-relative criterion of the per-layer tests)
      label_bad labels (argmax of probs) that differ from the float64 argmax where the top-2 logit margin exceeds 2 d; n_decided
      p_err     max |probs - softmax64(ref logits)|
    The extremes of the fp16 formats (f16, f16x3; all zero in the others), over the stored outputs:
      n_sat     reference elements at the clip (|value before the clip| >= 65504); n_beyond / n_beyond_neg: those strictly beyond it / below -65504
      sat_bad   elements whose value before the clip exceeds 65504 in magnitude by more than their own bound while the stored value is not
                exactly +-65504 with that sign (split mode: hi + lo, so lo must be 0) -- inf, a one-sided clamp, a lo half left over
      n_sub     nonzero reference elements below 2^-14 in magnitude; n_sub_held: those of them at or above 2^-24; n_nonzero"""
    ref, bound, pre = step_reference_pre(plan, step, vals, precision, extra_adds)
    got = step_got(plan, step, vals)
    rep = dict(name=step.name, kind=step.kind, K=step_K(step), worst=0.0, index=None, n_over=0, n_nan=0, n_inf=0, n_ref_bad=0,
               rms=0.0, ref_absmax=0.0, abs_err=0.0, old_rel=0.0, label_bad=0, n_decided=0, p_err=None, n_elem=0,
               n_sat=0, sat_bad=0, n_sub=0, n_beyond=0, n_beyond_neg=0, n_sub_held=0, n_nonzero=0)
    sq = 0.0
    for key, g in got.items():
        r, b = ref[key], bound[key]
        g = np.asarray(g, np.float64)
        assert g.shape == r.shape, (step.name, key, g.shape, r.shape)
        inside = _mask_of(mask, key, r.shape)
        ref_ok = np.isfinite(r) & np.isfinite(b)
        rep["n_ref_bad"] += int((~ref_ok & inside).sum())
        ref_ok &= inside
        rep["n_nan"] += int((np.isnan(g) & ref_ok).sum())
        rep["n_inf"] += int((np.isinf(g) & ref_ok).sum())
        ok = ref_ok & np.isfinite(g)
        err = np.where(ok, np.abs(g - r), 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err > 0, err / b, 0.0)                       # b == 0 < err -> inf
        rep["n_over"] += int((err > b).sum())
        rep["n_elem"] += int(ok.sum())
        if precision in SATURATING:
            p = np.where(ref_ok, pre[key], 0.0)
            rep["n_sat"] += int((np.abs(p) >= F16_MAX).sum())
            rep["n_beyond"] += int((np.abs(p) > F16_MAX).sum())
            rep["n_beyond_neg"] += int((p < -F16_MAX).sum())
            # beyond the range by more than the element's own bound: correct arithmetic cannot have kept it inside, so the store saturates
            rep["sat_bad"] += int(((np.abs(p) - F16_MAX > b) & ref_ok & (g != np.sign(p) * F16_MAX)).sum())
            a = np.abs(np.where(ref_ok, r, 0.0))
            rep["n_nonzero"] += int((a > 0).sum())
            rep["n_sub"] += int(((a > 0) & (a < F16_MIN_NORMAL)).sum())
            rep["n_sub_held"] += int(((a >= F16_MIN_SUBNORMAL) & (a < F16_MIN_NORMAL)).sum())
        sq += float(np.square(np.where(np.isfinite(ratio), ratio, 0.0)).sum())
        rmax = float(np.abs(np.where(ref_ok, r, 0.0)).max()) if r.size else 0.0
        rep["ref_absmax"] = max(rep["ref_absmax"], rmax)
        rep["abs_err"] = max(rep["abs_err"], float(err.max()) if err.size else 0.0)
        rep["old_rel"] = max(rep["old_rel"], float(err.max() / (rmax + 1e-6)) if err.size else 0.0)
        if ratio.size and float(ratio.max()) > rep["worst"]:
            rep["worst"] = float(ratio.max())
            rep["index"] = (key,) + tuple(int(i) for i in np.unravel_index(int(np.argmax(ratio)), ratio.shape))
    if "logits" in ref:
        lg, d = ref["logits"], bound["logits"]
        inside = _mask_of(mask, "logits", lg.shape)[..., 0]
        fin = np.isfinite(lg).all(-1) & np.isfinite(d).all(-1)
        rep["n_ref_bad"] += int((~fin & inside).sum())
        fin &= inside
        rep["ref_absmax"] = max(rep["ref_absmax"], float(np.abs(np.where(fin[..., None], lg, 0.0)).max()))
        if probs is not None:
            p = np.asarray(placed(probs, step) if step.kind == "conv" else probs, np.float64)
            assert p.shape == lg.shape, (step.name, p.shape, lg.shape)
            rep["n_nan"] += int((np.isnan(p).any(-1) & fin).sum())
            srt = np.sort(np.where(fin[..., None], lg, 0.0), axis=-1)
            decided = fin & ((srt[..., -1] - srt[..., -2]) > 2 * d.max(-1)) & np.isfinite(p).all(-1)
            rep["n_decided"] = int(decided.sum())
            rep["label_bad"] = int((decided & (p.argmax(-1) != lg.argmax(-1))).sum())
            pe = np.abs(p - softmax64(np.where(fin[..., None], lg, 0.0)))
            rep["p_err"] = float(np.where(fin[..., None] & np.isfinite(p), pe, 0.0).max())
    rep["rms"] = float(np.sqrt(sq / max(rep["n_elem"], 1)))
    return rep


def failed(rep):
    """True when a report breaks the per-step contract (over the bound, non-finite output, undecidable reference, wrong label, a value
    beyond the fp16 range not stored as +-65504)."""
    return bool(rep["n_over"] or rep["n_nan"] or rep["n_inf"] or rep["n_ref_bad"] or rep["label_bad"] or rep["sat_bad"] or not rep["ref_absmax"] > 0)
