"""-m gpu: every step of the plan ALONE against a float64 reference of that step on the inputs the device stored
(tests/step_check.py: derived per-element bound, nothing carried over from earlier layers).

"unfused": SBBSEG_FUSE_BLOCKS=0 and conv variant bits 22 | 23 | 24 | 25 -- every plan tensor reaches HBM, no step may be skipped.
"default": what the product runs; a step is checked when all its sources and its outputs were written (activation buffers are
filled with NaNs first).  The tensors that were not are exactly those a fused kernel keeps in LDS, re-derived here from the plan by
the library's own fusion rules (csrc/plan_build.hip fuse_bottlenecks / sbbseg_finalize) and tied to ``ctx.ops()`` by the block count.
One table per configuration goes to results/step_check_<precision>_<H>x<W>_<plan>.md (the directory the GPU scripts of tools/ write
their logs to, kept out of git; profiles/step_check.md keeps a copy).

The plans above are all the synthetic ResNet-50-U-Net.  test_every_step_of_the_small_plans_... runs the three small nets of
tests/small_plans.py the same way (default plan, n = 3, all four precisions): a 7 x 4 stem tap at stride (2, 1) on 8 channels, 8- to
32-channel convs (K padded inside one K-step), a stride-2 1 x 1 projection, second sources at offset (1, 1), stride-2 3 x 3 convs without
top / left padding, Conv2DTranspose classes of 1 x 1 to 2 x 2 taps placed at stride (2, 2), a 3-class head in a conv's epilogue.  Their
tables go to results/step_check_<precision>_<name>.md with the launch records."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import step_check as sc  # noqa: E402
from gpu_common import TOL_STEP_HEAD_PROB, make_model, patches_from_page  # noqa: E402
from small_plans import SMALL_PLANS, assert_odd_geometries, small_net  # noqa: E402

UNFUSED_BITS = (1 << 22) | (1 << 23) | (1 << 24) | (1 << 25)
OUT_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "results")

CONFIGS = [(p, 64, 96, 2, 3, "unfused") for p in ("f16", "f16x3", "bf16", "f32")]
CONFIGS += [(p, 224, 256, 4, 5, plan) for p in ("f16", "f16x3") for plan in ("unfused", "default")]
CONFIGS += [(p, 448, 448, 2, 2, plan) for p in ("f16", "f16x3") for plan in ("unfused", "default")]
CONFIGS += [(p, 320, 480, 2, 2, "default") for p in ("f16", "f16x3")]


def _is_conv(s, kh, cin, cout, n_src=1):
    if s.kind != "conv" or len(s.srcs) != n_src or s.cout != cout or s.raw_out >= 0 or s.head is not None or s.out < 0:
        return False
    g = s.srcs[0]
    pad = (kh - 1) // 2
    return ((g.kh, g.kw, g.stride_y, g.stride_x, g.pad_top, g.pad_left, g.shift, g.off_y, g.off_x) == (kh, kh, 1, 1, pad, pad, 0, 0, 0)
            and g.channels == cin and s.out_stride == (1, 1))


def fused_block_tensors(plan):
    """({plan tensor id: "a" | "b"}, number of blocks): the two 64-channel tensors of every stage-2 bottleneck block the library fuses
    (csrc/plan_build.hip fuse_bottlenecks)."""
    st = plan.steps
    keep = {}
    blocks = 0
    for i in range(len(st) - 2):
        a, b, c = st[i], st[i + 1], st[i + 2]
        if a.kind != "conv" or len(a.srcs) != 1:
            continue
        cin = a.srcs[0].channels
        if not (_is_conv(a, 1, cin, 64) and a.relu and a.residual < 0 and _is_conv(b, 3, 64, 64) and b.relu and b.residual < 0
                and b.srcs[0].tensor == a.out and c.kind == "conv" and c.cout == 256 and c.relu and c.out >= 0):
            continue
        x = a.srcs[0].tensor
        ident = len(c.srcs) == 1 and c.srcs[0].tensor == b.out and c.residual == x and cin == 256
        proj = len(c.srcs) == 2 and c.residual < 0 and cin == 64 and {g.tensor for g in c.srcs} == {b.out, x}
        if ident or proj:
            keep[a.out], keep[b.out] = "a", "b"
            blocks += 1
    return keep, blocks


def expected_unwritten(plan, precision, ops, dump_blocks=False):
    """{plan tensor id} the default plan keeps in LDS: the two 64-channel tensors of every fused stage-2 block and the 3x3 output b of
    every stage-3 identity block that runs as conv3_expand_reduce (128 channels, map sides multiples of 8).  `dump_blocks`: the form
    under conv variant bit 26, where bottleneck_fused* stores a and b too -- in the f16 / bf16 modes the block tensors leave the set; the
    split mode's block_x3 has no such form and keeps them."""
    st = plan.steps
    ab, blocks = fused_block_tensors(plan)
    assert blocks == sum(1 for o in ops if o["name"].startswith("block")), [o["name"] for o in ops]
    keep = set() if dump_blocks and precision in ("f16", "bf16") else set(ab)
    for i in range(1, len(st) - 1):
        k3, e, r = st[i - 1], st[i], st[i + 1]
        if not (_is_conv(k3, 3, 128, 128) and k3.relu and k3.residual < 0 and _is_conv(e, 1, 128, 512) and e.relu and e.residual >= 0
                and e.srcs[0].tensor == k3.out and _is_conv(r, 1, 512, 128) and r.relu and r.residual < 0 and r.srcs[0].tensor == e.out):
            continue
        t = plan.tensors[k3.out]
        if t.H % 8 == 0 and t.W % 8 == 0:
            keep.add(k3.out)
    return keep


def _kernel_name(step, ops):
    if step.kind == "conv":
        g = step.srcs[0]
        base = f"conv{g.kh}x{g.kw}_c{sum(q.channels for q in step.srcs)}to{step.cout}_{step.out_h}x{step.out_w}"
        names = {o["name"] for o in ops if base + "_" in o["name"] + "_"}
    else:
        names = {o["name"] for o in ops if o["name"].startswith({"maxpool": "maxpool", "tail": "tail_", "head": "head1x1"}[step.kind])}
    return names.pop() if len(names) == 1 else "-"


def check_steps(plan, vals, precision, probs, unwritten, ops, tag, extra_adds=None):
    """Every step of `plan` whose sources and outputs were all written, against its float64 reference on `vals` (tests/step_check.py).
    `extra_adds`: {step name: splits - 1} of the steps a split-K launch ran (tests/test_gpu_steps_whole.py).  Returns (rows [(step name, kernel name, report)], skipped step names, failures, max |p - p_ref64|, wrong labels, decided pixels)."""
    rows, skipped, bad = [], [], []
    p_err = label_bad = decided = 0
    for s in plan.steps:
        src, dst = sc.step_tensors(s)
        if unwritten & set(src + dst):
            skipped.append(s.name)
            continue
        rep = sc.check_step(plan, s, vals, precision, probs=probs, extra_adds=(extra_adds or {}).get(s.name, 0))
        print(f"[step {tag}] {s.name}: K {rep['K']} worst err/bound {rep['worst']:.4f} at {rep['index']} rms {rep['rms']:.4f} "
              f"over {rep['n_over']} nan {rep['n_nan']} inf {rep['n_inf']} refbad {rep['n_ref_bad']} |ref|max {rep['ref_absmax']:.4g}"
              + (f" p_err {rep['p_err']:.3e} label_bad {rep['label_bad']} / {rep['n_decided']} decided" if rep["p_err"] is not None else ""))
        rows.append((s.name, _kernel_name(s, ops), rep))
        if rep["p_err"] is not None:
            p_err, label_bad, decided = max(p_err, rep["p_err"]), label_bad + rep["label_bad"], decided + rep["n_decided"]
        if sc.failed(rep):
            bad.append((s.name, {k: rep[k] for k in ("worst", "index", "n_over", "n_nan", "n_inf", "n_ref_bad", "label_bad", "ref_absmax")}))
    return rows, skipped, bad, p_err, label_bad, decided


def write_table(f, title, rows, skipped, p_err, label_bad, decided, splits=None):
    """p_err None: the pass stored no probabilities (labels only).  `splits`: {step name: splits of its split-K launch} -> a column."""
    f.write(f"### {title}\n\n")
    head = f"max |p - p_ref64| {p_err:.3e}" if p_err is not None else "no probabilities stored, no p_err (the returned labels as one-hot planes)"
    f.write(f"worst err / bound {max(r['worst'] for _, _, r in rows):.4f}; head: {head}, "
            f"{label_bad} wrong labels among {decided} decided pixels; skipped steps: {', '.join(skipped) or 'none'}\n\n")
    more = ("| splits (bound: + splits - 1 additions) ", "|---") if splits is not None else ("", "")
    f.write(f"| step | kernel | K {more[0]}| worst err / bound | at (output, patch, y, x, channel) | rms err / bound |\n|---|---|---{more[1]}|---|---|---|\n")
    for name, kern, r in rows:
        col = f"| {splits.get(name, '-')} " if splits is not None else ""
        f.write(f"| {name} | {kern} | {r['K']} {col}| {r['worst']:.4f} | {r['index']} | {r['rms']:.4f} |\n")


@pytest.mark.parametrize("precision,h,w,classes,n,mode", CONFIGS, ids=[f"{c[0]}-{c[1]}x{c[2]}-{c[5]}" for c in CONFIGS])
def test_every_step_matches_its_float64_reference(precision, h, w, classes, n, mode, monkeypatch):
    if mode == "unfused":
        monkeypatch.setenv("SBBSEG_FUSE_BLOCKS", "0")
    cfg, wts, g, model = make_model(classes, h, w, seed=12, precision=precision, max_batch=n + 2, calib_hw=min(160, max(h, w)))
    try:
        ctx, plan = model.ctx, model.plan
        if mode == "unfused":
            ctx.set_conv_variant(UNFUSED_BITS)
        ops = ctx.ops()
        x = (patches_from_page(h, w, n, seed=33) / 255.0).astype(np.float32)
        ctx.poison_activations(0xFF)
        probs = model.predict(x)
        vals = {}
        for tid, t in enumerate(plan.tensors):
            if t.kind != "unused":
                vals[tid] = ctx.debug_read_tensor(tid, n, (t.H, t.W, t.C))
    finally:
        model.release()
    unwritten = {tid for tid, a in vals.items() if np.isnan(a).all()}
    expect = expected_unwritten(plan, precision, ops) if mode == "default" else set()
    names = lambda ids: sorted(plan.tensors[t].name for t in ids)
    assert unwritten == expect, (names(unwritten), names(expect))
    rows, skipped, bad, p_err, label_bad, decided = check_steps(plan, vals, precision, probs, unwritten, ops, f"{precision} {h}x{w} {mode}")
    want_skipped = [s.name for s in plan.steps if expect & set(sum(sc.step_tensors(s), []))]
    os.makedirs(OUT_DIR, exist_ok=True)
    with open(os.path.join(OUT_DIR, f"step_check_{precision}_{h}x{w}_{mode}.md"), "w") as f:
        write_table(f, f"{precision} {h} x {w}, {classes} classes, n = {n}, {mode} plan", rows, skipped, p_err, label_bad, decided)
    assert skipped == want_skipped, (skipped, want_skipped)
    assert mode == "default" or not skipped
    assert not bad, bad
    assert decided > 0 and label_bad == 0
    assert p_err < TOL_STEP_HEAD_PROB[precision], p_err


@pytest.mark.parametrize("precision", ["f16", "f16x3", "bf16", "f32"])
@pytest.mark.parametrize("name", SMALL_PLANS)
def test_every_step_of_the_small_plans_matches_its_float64_reference(name, precision):
    """The non-ResNet plans, step by step, with the assertions of the test above.  They fuse nothing: every plan tensor must be written and
    no step skipped.  Gather (from the launch records, asserted below): at these channel counts no conv of keras23 takes the fast gather in
    any mode, and the Conv2DTranspose nets take it only for the two 32- / 64-channel 3 x 3 convs of the split mode; every other conv -- the
    7 x 4 stem tap, the stride-2 convs without padding, every parity class -- runs conv_igemm_mfma's plain gather (conv_naive_f32 in the
    f32 mode), which no ResNet plan exercises on such geometries."""
    from sbb_textline_detection_amd.model import SegModel
    from test_gpu_steps_at_scale import launch_records, write_routes
    cfg, wts, x = small_net(name)
    n = x.shape[0]
    model = SegModel(cfg, wts, device=0, max_batch=n, precision=precision)
    try:
        ctx, plan = model.ctx, model.plan
        ops = ctx.ops()
        ctx.poison_activations(0xFF)
        probs = model.predict(x)
        recs = launch_records(ctx, ops)
        vals = {tid: ctx.debug_read_tensor(tid, n, (t.H, t.W, t.C)) for tid, t in enumerate(plan.tensors) if t.kind != "unused"}
    finally:
        model.release()
    assert_odd_geometries(name, plan, precision)
    unwritten = {tid for tid, a in vals.items() if np.isnan(a).all()}
    assert not unwritten, sorted(plan.tensors[t].name for t in unwritten)
    rows, skipped, bad, p_err, label_bad, decided = check_steps(plan, vals, precision, probs, unwritten, ops, f"{precision} {name}")
    os.makedirs(OUT_DIR, exist_ok=True)
    with open(os.path.join(OUT_DIR, f"step_check_{precision}_{name}.md"), "w") as f:
        write_table(f, f"{precision} {name} ({plan.in_h} x {plan.in_w}, {plan.classes} classes), n = {n}, default plan", rows, skipped, p_err, label_bad, decided)
        write_routes(f, n, recs)
    assert not skipped, skipped
    assert not bad, bad
    assert decided > 0 and label_bad == 0
    assert p_err < TOL_STEP_HEAD_PROB[precision], p_err
    convs = [r for r in recs if r["family"] in ("conv_igemm", "conv_naive_f32")]
    assert convs and len(convs) == sum(1 for r in recs if r["name"].startswith("conv")), [(r["name"], r["family"]) for r in recs]
    assert any(r["fast_gather"] == 0 for r in convs), [(r["name"], r["fast_gather"]) for r in convs]
