"""-m gpu: every kernel family at fp16 saturation and in fp16 subnormals (f16 and f16x3; bf16 and f32 have no 65504).

The nets are those of tests/gained_nets.py: the calibrated net with every activation times 2^15 or 2^16 (hot) or 2^-17 (cold), logits
unchanged where nothing clips.  The per-element bound of tests/step_check.py is the derived one, unchanged; the report's ``sat_bad`` -- a
value beyond +-65504 by more than its bound that was not stored as exactly +-65504 (split mode: hi + lo, so lo = 0) -- fails a step like an
element over the bound does.

  * every step alone (the loop and assertions of tests/test_gpu_steps.py on NaN-poisoned buffers): the unfused plan at 64 x 96, n = 3
    (SBBSEG_FUSE_BLOCKS=0, conv variant bits 22 | 23 | 24 | 25) and the default plan at 128 x 192, n = 2 -- the smallest shape at which
    every fused route is launched -- the stage-2 blocks, stem_pool in the split mode, conv3_expand_reduce, expand_reduce, dec_halo, the
    fused tail: asserted from the launch records (``FAMILIES``), so the 224 x 256 fallback was not needed.  direct64 is no launch of a
    default plan at any shape (it is the 3 x 3 conv inside the fused blocks); it runs, and is asserted, in the unfused plan;
  * coverage, from the float64 reference on what the device stored: the conditions tests/gained_nets.py fixes the gains by
    (``assert_coverage``) hold again here, so a green run is not vacuous;
  * the 16-bit bottleneck blocks: the f16 default plan once more per hot gain under conv variant bit 26, which stores the a and b a fused
    block keeps in LDS (tests/test_gpu_steps_blocks.py) -- the nine res2* steps at saturation, phase by phase;
  * fused equals unfused, bit for bit, on one hot and one cold net: block_x3 (bit 18), stem_pool (bit 22, SBBSEG_STEM_POOL_F16=1),
    dec_halo (23), expand_reduce (24 under 25), conv3_expand_reduce (24 | 25), each at the smallest shape its test in
    tests/test_gpu_parity.py uses; tensors only, and only after the tensors the fused kernel writes were seen to hold saturated
    (subnormal) elements;
  * split-K: one whole-image launch on a hot and one on a cold net per precision (``splitk_finish`` has its own epilogue), step-checked with
    the helpers of tests/test_gpu_steps_whole.py at that file's smallest fp16 shape, 224 x 256 with four classes.

One table per configuration goes to results/step_check_<precision>_<H>x<W>_<plan>_gain<k>.md with n_sat, n_sub and sat_bad per step;
profiles/step_check_extremes.md keeps a copy."""
import contextlib
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import step_check as sc  # noqa: E402
from gained_nets import COLD_GAINS, HOT_GAINS, assert_coverage, gain_tag, gained, patches, stores_fp16  # noqa: E402
from gpu_common import TOL_STEP_HEAD_PROB, patches_from_page  # noqa: E402
from sbb_textline_detection_amd.model import SegModel  # noqa: E402
from test_gpu_steps import OUT_DIR, UNFUSED_BITS, check_steps, expected_unwritten, fused_block_tensors  # noqa: E402
from test_gpu_steps_at_scale import launch_records  # noqa: E402
from test_gpu_steps_whole import page_for, split_counts, whole_pass  # noqa: E402
from tools.synth_model import calibrated_model  # noqa: E402

PRECISIONS = ("f16", "f16x3")
PLANS = {"unfused": (64, 96, 3), "default": (128, 192, 2)}                # plan -> (H, W, n); tests/test_gained_nets_cpu.py SHAPES
DUMP_BIT = 1 << 26
# launch families the default plan must have run at 128 x 192 (sbbseg_debug_op_launch); the plain mode fuses the stem's pool only on request.
# direct64 (conv3x3_c64_direct) is the 3 x 3 conv of a stage-2 block: the default plan runs it inside the fused blocks at every shape, so it
# is a launch of the unfused plan only and is asserted there.
FAMILIES = {"f16x3": {"block_x3", "stem_pool", "conv3_expand_reduce", "expand_reduce", "dec_halo", "tail"},
            "f16": {"bottleneck_pq", "conv3_expand_reduce", "expand_reduce", "dec_halo", "tail"}}
UNFUSED_FAMILIES = {"stem", "maxpool", "direct64", "conv_igemm", "tail"}
_RUNS = {}


@functools.lru_cache(maxsize=None)
def _net(classes, h, w, seed):
    return calibrated_model(classes, h, w, seed=seed, calib_hw=min(160, max(h, w)))


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _gained_model(classes, h, w, seed, precision, g, max_batch):
    cfg, weights = _net(classes, h, w, seed)
    return SegModel(cfg, gained(cfg, weights, g), device=0, max_batch=max_batch, precision=precision)


def write_extremes_table(f, title, rows, skipped, p_err, label_bad, decided, splits=None):
    f.write(f"### {title}\n\n")
    head = f"max |p - p_ref64| {p_err:.3e}" if p_err is not None else "no probabilities stored (the returned labels as one-hot planes)"
    f.write(f"worst err / bound {max(r['worst'] for _, _, r in rows):.4f}; sat_bad {sum(r['sat_bad'] for _, _, r in rows)}; head: {head}, "
            f"{label_bad} wrong labels among {decided} decided pixels; skipped steps: {', '.join(skipped) or 'none'}\n\n")
    more = ("| splits ", "|---") if splits is not None else ("", "")
    f.write(f"| step | kernel | K {more[0]}| stored elements | n_sat | below -65504 | n_sub | sat_bad | worst err / bound | at (output, patch, y, x, channel) |\n"
            f"|---|---|---{more[1]}|---|---|---|---|---|---|---|\n")
    for name, kern, r in rows:
        col = f"| {splits.get(name, '-')} " if splits is not None else ""
        f.write(f"| {name} | {kern} | {r['K']} {col}| {r['n_elem']} | {r['n_sat']} | {r['n_beyond_neg']} | {r['n_sub']} | {r['sat_bad']} | {r['worst']:.4f} | {r['index']} |\n")


def run_steps(precision, mode, g, variant=0):
    """One predict of the net gained by g on poisoned buffers, every checkable step against its float64 reference (cached per configuration)."""
    key = (precision, mode, g, variant)
    if key in _RUNS:
        return _RUNS[key]
    h, w, n = PLANS[mode]
    with _env(**({"SBBSEG_FUSE_BLOCKS": "0"} if mode == "unfused" else {})):
        model = _gained_model(2, h, w, 12, precision, g, n + 2)
        try:
            ctx, plan = model.ctx, model.plan
            bits = (UNFUSED_BITS if mode == "unfused" else 0) | variant
            if bits:
                ctx.set_conv_variant(bits)
            ops = ctx.ops()
            ctx.poison_activations(0xFF)
            probs = model.predict(patches(h, w, n))
            recs = launch_records(ctx, ops)
            vals = {tid: ctx.debug_read_tensor(tid, n, (t.H, t.W, t.C)) for tid, t in enumerate(plan.tensors) if t.kind != "unused"}
        finally:
            model.release()
    unwritten = {tid for tid, a in vals.items() if np.isnan(a).all()}
    expect = expected_unwritten(plan, precision, ops, dump_blocks=bool(variant & DUMP_BIT)) if mode == "default" else set()
    names = lambda ids: sorted(plan.tensors[t].name for t in ids)
    assert unwritten == expect, (names(unwritten), names(expect))
    form = mode + ("_dump" if variant & DUMP_BIT else "")
    tag = f"{precision} {h}x{w} {form} {gain_tag(g)}"
    rows, skipped, bad, p_err, label_bad, decided = check_steps(plan, vals, precision, probs, unwritten, ops, tag)
    for name, _, r in rows:
        print(f"[extremes {tag}] {name}: n_sat {r['n_sat']} beyond {r['n_beyond']} below -65504 {r['n_beyond_neg']} n_sub {r['n_sub']} held {r['n_sub_held']} "
              f"nonzero {r['n_nonzero']} of {r['n_elem']} sat_bad {r['sat_bad']}")
    os.makedirs(OUT_DIR, exist_ok=True)
    with open(os.path.join(OUT_DIR, f"step_check_{precision}_{h}x{w}_{form}_{gain_tag(g)}.md"), "w") as f:
        write_extremes_table(f, f"{precision} {h} x {w}, 2 classes, n = {n}, {form} plan, every activation x 2^{gain_tag(g)[4:]}", rows, skipped, p_err, label_bad, decided)
    want_skipped = [s.name for s in plan.steps if expect & set(sum(sc.step_tensors(s), []))]
    out = dict(plan=plan, ops=ops, recs=recs, rows=rows, reports={name: r for name, _, r in rows}, skipped=skipped, want_skipped=want_skipped, bad=bad,
               p_err=p_err, label_bad=label_bad, decided=decided)
    _RUNS[key] = out
    return out


def _assert_steps(run, precision, mode):
    assert run["skipped"] == run["want_skipped"], (run["skipped"], run["want_skipped"])
    assert mode == "default" or not run["skipped"]
    assert not run["bad"], run["bad"]
    assert all(r["sat_bad"] == 0 for r in run["reports"].values())
    assert run["decided"] > 0 and run["label_bad"] == 0
    assert run["p_err"] < TOL_STEP_HEAD_PROB[precision], run["p_err"]


@pytest.mark.parametrize("g", HOT_GAINS + COLD_GAINS, ids=gain_tag)
@pytest.mark.parametrize("mode", list(PLANS))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_step_alone_at_the_extremes(precision, mode, g):
    run = run_steps(precision, mode, g)
    _assert_steps(run, precision, mode)
    stored = [run["reports"][s.name] for s in run["plan"].steps if stores_fp16(s) and s.name in run["reports"]]
    # (which step has how much of it is the coverage test's business: at 2^15 the convs inside the blocks may have nothing beyond the range)
    assert stored and sum((r["n_sat"] if g > 1 else r["n_sub"]) > 0 for r in stored) > len(stored) // 4, [(r["name"], r["n_sat"], r["n_sub"]) for r in stored]
    if mode == "default":
        ran = {r["family"] for r in run["recs"]}
        assert FAMILIES[precision] <= ran, (sorted(FAMILIES[precision] - ran), sorted(ran))
    else:
        assert UNFUSED_FAMILIES <= {r["family"] for r in run["recs"]}, sorted({r["family"] for r in run["recs"]})
        assert not {r["family"] for r in run["recs"]} & {"block_x3", "bottleneck", "bottleneck_pq", "stem_pool", "conv3_expand_reduce", "expand_reduce", "dec_halo"}


@pytest.mark.parametrize("hot", [True, False], ids=["hot", "cold"])
@pytest.mark.parametrize("mode", list(PLANS))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_device_runs_meet_the_coverage_conditions(precision, mode, hot):
    """The conditions the gains were fixed by, on the float64 reference of what the device stored.  A step of the default plan behind a tensor
    that stays in LDS has no report there: the unfused plan holds it, and the dump form below the blocks of the plain mode."""
    runs = {g: run_steps(precision, mode, g) for g in (HOT_GAINS if hot else COLD_GAINS)}
    first = next(iter(runs.values()))
    assert_coverage(first["plan"], {g: r["reports"] for g, r in runs.items()}, hot, skip=set(first["skipped"]))


@pytest.mark.parametrize("g", HOT_GAINS, ids=gain_tag)
def test_fused_16_bit_blocks_phase_by_phase_at_saturation(g):
    run = run_steps("f16", "default", g, variant=DUMP_BIT)
    _assert_steps(run, "f16", "default")
    ab, n_blocks = fused_block_tensors(run["plan"])
    block_steps = [s for s in run["plan"].steps if set(ab) & set(sum(sc.step_tensors(s), []))]
    assert n_blocks == 3 and len(block_steps) == 9 and not [s for s in run["skipped"] if s.startswith("res2")]
    blk = [r for r in run["recs"] if r["name"].startswith("block")]
    assert len(blk) == 3 and all(r["family"] == "bottleneck_pq" for r in blk), [(r["name"], r["family"]) for r in blk]
    for s in block_steps:
        r = run["reports"][s.name]
        assert not sc.failed(r) and r["n_sat"] > 0 and r["n_elem"] > r["n_sat"], (s.name, r)
    product = run_steps("f16", "default", g)
    assert {name: r for name, r in run["reports"].items() if name in product["reports"]} == product["reports"]       # (the dump form changes nothing else)


# ------------------------------------------------------------------------------------------------ fused equals unfused, bit for bit
# family -> (precisions, (H, W), patches, net seed, page seed, variant of the fused run, variant of the launches it replaces, environment
# at model build, (channels, H divisor, H offset) of the tensors the fused kernel writes): the smallest case of the family's test in
# tests/test_gpu_parity.py
PARITY = {
    "block_x3": (("f16x3",), (64, 96), 3, 5, 8, 0, 1 << 18, {}, [(256, 4, -1)]),
    "stem_pool": (PRECISIONS, (64, 96), 3, 6, 18, 0, 1 << 22, {"SBBSEG_STEM_POOL_F16": "1"}, [(64, 2, 0), (64, 4, -1)]),
    "dec_halo": (PRECISIONS, (64, 96), 3, 8, 28, 0, 1 << 23, {}, [(64, 2, 0)]),
    "expand_reduce": (PRECISIONS, (64, 96), 3, 9, 29, 1 << 25, (1 << 24) | (1 << 25), {}, [(512, 8, 0), (1024, 16, 0)]),
    "conv3_expand_reduce": (PRECISIONS, (64, 64), 5, 11, 31, 0, (1 << 24) | (1 << 25), {}, [(512, 8, 0)]),
}
_PARITY_CASES = [(fam, p, g) for fam, c in PARITY.items() for p in c[0] for g in (max(HOT_GAINS), min(COLD_GAINS))]


@pytest.mark.parametrize("family,precision,g", _PARITY_CASES, ids=[f"{f}-{p}-{gain_tag(g)}" for f, p, g in _PARITY_CASES])
def test_fused_kernels_equal_the_launches_they_replace_at_the_extremes(family, precision, g):
    _, (h, w), nb, seed, page_seed, fused_bits, parts_bits, env, written = PARITY[family]
    with _env(**env):
        model = _gained_model(2, h, w, seed, precision, g, nb + 2)
    try:
        ctx, plan = model.ctx, model.plan
        x = (patches_from_page(h, w, nb, seed=page_seed) / 255.0).astype(np.float32)

        def run(bits):
            ctx.set_conv_variant(bits)
            ctx.poison_activations(0xFF)
            probs = model.predict(x)
            recs = launch_records(ctx, ctx.ops())
            return probs, recs, {name: ctx.debug_read_tensor(tid, nb, (plan.tensors[tid].H, plan.tensors[tid].W, plan.tensors[tid].C))
                                 for name, tid in plan.layer_tensor.items()}
        p_fused, recs_fused, t_fused = run(fused_bits)
        p_parts, recs_parts, t_parts = run(parts_bits)
        ctx.set_conv_variant(0)
    finally:
        model.release()
    assert family in {r["family"] for r in recs_fused} and family not in {r["family"] for r in recs_parts}, sorted({r["family"] for r in recs_fused})
    own = [name for name, tid in plan.layer_tensor.items()
           if any((plan.tensors[tid].C, plan.tensors[tid].H) == (c, h // div + off) for c, div, off in written) and not np.isnan(t_fused[name]).all()]
    assert len(own) >= len(written), (own, list(plan.layer_tensor))                 # (a and b of a fused stage-2 block share the pool's shape: in LDS, all NaN)
    for name in own:
        a = np.abs(t_fused[name])
        assert not np.isnan(a).any(), name
        if g > 1:
            assert (a == sc.F16_MAX).any() and (a < sc.F16_MAX).any(), (name, float(a.max()))
        else:
            assert ((a > 0) & (a < sc.F16_MIN_NORMAL)).any(), (name, float(a.max()))
    compared = 0
    for name in t_fused:
        if np.isnan(t_fused[name]).all():                               # the fused form keeps it in LDS
            continue
        assert np.array_equal(t_fused[name], t_parts[name], equal_nan=True), (name, float(np.nanmax(np.abs(t_fused[name] - t_parts[name]))))
        compared += 1
    assert compared > len(own) and np.isfinite(p_fused).all()
    assert np.array_equal(p_fused, p_parts)


# ------------------------------------------------------------------------------------------------ split-K
@pytest.mark.parametrize("g", [max(HOT_GAINS), min(COLD_GAINS)], ids=gain_tag)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_split_k_whole_image_launch_at_the_extremes(precision, g):
    h, w, classes = 224, 256, 4
    page = page_for(h, w)
    model = _gained_model(classes, h, w, 12, precision, g, 2)
    try:
        model.ctx.set_lanes(1)
        plan, ops = model.plan, model.ctx.ops()
        labels, recs, vals = whole_pass(model, page, h, w)
    finally:
        model.release()
    recs, splits = split_counts(plan, ops, recs)
    assert splits, "no op of the whole-image launch took the split-K route"
    unwritten = {tid for tid, a in vals.items() if np.isnan(a).all()}
    expect = expected_unwritten(plan, precision, ops)
    assert unwritten == expect, (sorted(plan.tensors[t].name for t in unwritten), sorted(plan.tensors[t].name for t in expect))
    onehot = np.zeros((1, h, w, classes), np.float32)
    np.put_along_axis(onehot[0], labels[..., None].astype(np.int64), 1.0, axis=-1)
    tag = f"{precision} {h}x{w} whole {gain_tag(g)}"
    rows, skipped, bad, _, label_bad, decided = check_steps(plan, vals, precision, onehot, unwritten, ops, tag, extra_adds={k: v - 1 for k, v in splits.items()})
    os.makedirs(OUT_DIR, exist_ok=True)
    with open(os.path.join(OUT_DIR, f"step_check_{precision}_{h}x{w}_whole_{gain_tag(g)}.md"), "w") as f:
        write_extremes_table(f, f"{precision} {h} x {w}, {classes} classes, whole-image launch (one patch), split-K on, every activation x 2^{gain_tag(g)[4:]}",
                             rows, skipped, None, label_bad, decided, splits=splits)
    reports = {name: r for name, _, r in rows}
    assert set(splits) <= set(reports), sorted(set(splits) - set(reports))
    assert not bad, bad
    assert all(r["sat_bad"] == 0 for r in reports.values())
    assert decided > 0 and label_bad == 0
    split_reports = [reports[name] for name in splits]
    assert all((r["n_sat"] if g > 1 else r["n_sub"]) > 0 for r in split_reports), [(r["name"], r["n_sat"], r["n_sub"]) for r in split_reports]
    assert any(r["residual"] == 1 for r in recs if r["family"] == "conv_splitk") and any(r.get("par4") == 1 for r in recs if r["family"] == "conv_splitk")
