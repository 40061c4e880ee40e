"""-m gpu: the per-step float64 check of tests/test_gpu_steps.py on the whole-image launch (``sbbseg_segment_whole*``, the border model
of ``run_page``), the only caller of the split-K route.

With one patch, ``launch_op`` (csrc/forward.hip, the last ``else`` of the conv branch) sends every long-K generic conv of the 128-channel tile
through ``conv_igemm_mfma<..KS>`` -- 2^ks blocks per tile, each writing its K-range's fp32 partial sums x ``wmul_cls`` to a workspace -- and
``splitk_finish<MODE>``, which adds the planes in split order and runs its own copy of the epilogue.  Recipe of one configuration (one lane,
max_batch 2): a page whose sides are no multiples of the model's, so that the whole-image gather of ``ingest_u8_kernel`` really resamples;
one ``segment_whole`` so that the workspace has its final size; ``poison_activations(0xFF)``, which fills the activation buffers AND that
workspace with NaNs; the pass under test; the launch records; every plan tensor read back.  Because the pass follows the poison, a partial
sum that is never written (a split dropped on a ragged tile, say) arrives as NaN in its op's output instead of as the previous pass's --
equal -- value: ``n_nan`` of that step fails the check.

Asserted per configuration: the unwritten tensors are exactly the fused ones (``expected_unwritten``); some op reports ``conv_splitk`` and the
split count derived from its plan step and its record, n_tiles / (n_cls * ceil(out_h * out_w / 128) * ceil(cout / 128)), is 2, 4, 8 or 16;
every checkable step is inside its derived bound, a split one with ``extra_adds = splits - 1`` (tests/step_check.py) and nothing else new;
the returned labels go through the float64 margin rule as one-hot planes (the branch stores no probabilities: no ``p_err`` for this pass).
An unsplit twin (``set_ksplit(False)``) reports no ``conv_splitk``, leaves every tensor byte-identical to ``predict`` of the same resampled
patch -- the input forms first, with their own message: a difference there is ``ingest_u8_kernel`` / ``ingest_f32_kernel``'s, not a conv's --
and that one-patch ``predict`` (n = 1, which test_gpu_steps.py never runs) passes the step check with its probabilities.  Between the two
handles every step that did not split and whose stored sources are byte-identical must have byte-identical outputs: the split touched only
what it was meant to.

What splits where (measured, in the tables of profiles/step_check.md): at 224 x 256 and 256 x 256 every generic conv from stage 3 on splits
except the expand convs that run as expand_reduce / conv3_expand_reduce and the last expand conv of stage 3 (K = 128: fewer than the 8
K-steps two splits need); single-class ops with 2 to 16 splits, the three long decoder convs as four-class (``_par4``) ops with 4 to 16, the
last expand conv of stages 4 and 5 with a stored residual.  The count is set by the K-steps far more than by the tile count (512 blocks
are never reached at these sizes), which is why it barely moves with the image size.  All four forms -- single class, four classes, with
and without a residual -- occur at every listed size, bf16 at 64 x 96 included (its ``splitk_finish<2>``), so no form had to be argued
away.  256 x 256 is there because its stage-3 maps are multiples of 8: ``conv3_expand_reduce`` then runs at n = 1 beside the split ops.

test_whole_image_routes_of_the_product_...: the routes -- ``ROUTE_FIELDS`` plus, for ``conv_splitk``, the split count -- of one whole-image
launch of the 448 x 448 two-class model must all be among those of the configurations above.  They are (measured): the 448 launch splits
the same ops 2- to 16-fold, each count with the masked and with the pointwise gather as above; so neither 320 x 480 nor 448 x 448 had to
join the list, and no float64 reference is computed at those sizes.  (The route says nothing of the class count: the split mode's 448 launch runs one four-class op with 4 splits,
which among its checked sizes only single-class ops have -- the plain mode's 224 x 256 table holds that op.)

One table per configuration goes to results/step_check_<precision>_<H>x<W>_whole.md; profiles/step_check.md keeps a copy."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import step_check as sc  # noqa: E402
from gpu_common import TOL_STEP_HEAD_PROB, make_model  # noqa: E402
from oracle import tiling  # noqa: E402
from sbb_textline_detection_amd.model import SegModel  # noqa: E402
from sbb_textline_detection_amd.synthetic import synthetic_page  # noqa: E402
from test_gpu_steps import OUT_DIR, check_steps, expected_unwritten, write_table  # noqa: E402
from test_gpu_steps_at_scale import launch_records, route_of, write_routes  # noqa: E402

WHOLE_CONFIGS = [("f16x3", 224, 256, 4), ("f16", 224, 256, 4), ("f16x3", 256, 256, 4), ("f16", 256, 256, 4), ("bf16", 64, 96, 2)]
SPLIT_COUNTS = (2, 4, 8, 16)
_RECORDS = {}                             # configuration -> launch records of its split pass (with "splits", "par4"), for the coverage tests


def page_for(h, w):
    return synthetic_page(2 * h + 37, 3 * w // 2 + 51, seed=h + w)


def ops_of_steps(plan, ops):
    """[op index per plan step]: the ops follow the plan's order; a fused block holds three steps, a ``_par4`` op the four classes."""
    out, i = [], 0
    for o in ops:
        take = 3 if o["name"].startswith("block") else 4 if "_par4" in o["name"] else 1
        for s in plan.steps[i:i + take]:
            if s.kind == "conv" and not o["name"].startswith("block"):
                g = s.srcs[0]
                base = f"conv{g.kh}x{g.kw}_c{sum(q.channels for q in s.srcs)}to{s.cout}_{s.out_h}x{s.out_w}_"
                assert base in o["name"] + "_", (s.name, base, o["name"])
            else:
                assert o["name"].startswith({"conv": "block", "maxpool": "maxpool", "tail": "tail_", "head": "head1x1"}[s.kind]), (s.name, o["name"])
            out.append(o["index"])
        i += take
    assert i == len(plan.steps) == len(out), (i, len(plan.steps))
    return out


def split_counts(plan, ops, recs):
    """The records with "splits" (conv_splitk ops only) and "par4" added, and {step name: splits} of the steps those ops ran."""
    by_op, per_step = {}, {}
    for s, oi in zip(plan.steps, ops_of_steps(plan, ops)):
        by_op.setdefault(oi, []).append(s)
    for o, r in zip(ops, recs):
        if r["family"] != "conv_splitk":
            continue
        steps = by_op[o["index"]]
        r["par4"] = int("_par4" in o["name"])
        assert len(steps) == (4 if r["par4"] else 1) and all(s.kind == "conv" for s in steps), (o["name"], [s.name for s in steps])
        s = steps[0]
        tiles = len(steps) * -(-s.out_h * s.out_w // 128) * -(-s.cout // 128)
        assert r["n_tiles"] % tiles == 0 and r["n_tiles"] // tiles in SPLIT_COUNTS, (o["name"], r["n_tiles"], tiles)
        assert r["residual"] == int(s.residual >= 0), (o["name"], r["residual"], s.residual)
        r["splits"] = r["n_tiles"] // tiles
        for q in steps:
            per_step[q.name] = r["splits"]
    return recs, per_step


def whole_pass(model, page, h, w):
    """Steps 3 to 7 of the recipe on a one-lane handle -> (labels, launch records, {plan tensor: values of patch 0})."""
    ctx, plan = model.ctx, model.plan
    ctx.segment_whole(page, h, w)
    ctx.poison_activations(0xFF)
    labels = ctx.segment_whole(page, h, w)
    recs = launch_records(ctx, ctx.ops())
    vals = {tid: ctx.debug_read_tensor(tid, 1, (t.H, t.W, t.C)) for tid, t in enumerate(plan.tensors) if t.kind != "unused"}
    return labels, recs, vals


def records_of(cfg):
    """The split pass's records of a configuration (run without a reference when its test has not run)."""
    if cfg not in _RECORDS:
        precision, h, w, classes = cfg
        _, _, _, model = make_model(classes, h, w, seed=12, precision=precision, max_batch=2, calib_hw=min(160, max(h, w)))
        try:
            model.ctx.set_lanes(1)
            model.ctx.segment_whole(page_for(h, w), h, w)
            recs, _ = split_counts(model.plan, model.ctx.ops(), launch_records(model.ctx, model.ctx.ops()))
        finally:
            model.release()
        _RECORDS[cfg] = recs
    return _RECORDS[cfg]


def whole_route(r):
    return route_of(r) + ((r["splits"],) if r["family"] == "conv_splitk" else ())


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("precision,h,w,classes", WHOLE_CONFIGS, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in WHOLE_CONFIGS])
def test_every_step_of_the_whole_image_launch_matches_its_float64_reference(precision, h, w, classes):
    page = page_for(h, w)
    assert page.shape[0] % h and page.shape[1] % w
    tag = f"{precision} {h}x{w} whole"
    names = lambda plan, ids: sorted(plan.tensors[t].name for t in ids)
    # ---- the pass under test: split-K on
    cfg, wts, _, model = make_model(classes, h, w, seed=12, precision=precision, max_batch=2, calib_hw=min(160, max(h, w)))
    try:
        model.ctx.set_lanes(1)
        plan, ops = model.plan, model.ctx.ops()
        labels, recs, vals = whole_pass(model, page, h, w)
    finally:
        model.release()
    assert labels.shape == (h, w) and int(labels.max()) < classes
    recs, splits = split_counts(plan, ops, recs)
    _RECORDS[(precision, h, w, classes)] = recs
    assert splits, "no op of the whole-image launch took the split-K route"
    unwritten = {tid for tid, a in vals.items() if np.isnan(a).all()}
    expect = expected_unwritten(plan, precision, ops)
    assert unwritten == expect, (names(plan, unwritten), names(plan, expect))
    onehot = np.zeros((1, h, w, classes), np.float32)
    np.put_along_axis(onehot[0], labels[..., None].astype(np.int64), 1.0, axis=-1)
    rows, skipped, bad, _, label_bad, decided = check_steps(plan, vals, precision, onehot, unwritten, ops, tag,
                                                            extra_adds={k: v - 1 for k, v in splits.items()})
    os.makedirs(OUT_DIR, exist_ok=True)
    with open(os.path.join(OUT_DIR, f"step_check_{precision}_{h}x{w}_whole.md"), "w") as f:
        write_table(f, f"{precision} {h} x {w}, {classes} classes, whole-image launch (one patch, page {page.shape[0]} x {page.shape[1]} resampled), split-K on",
                    rows, skipped, None, label_bad, decided, splits=splits)
        write_routes(f, 1, recs)
    assert skipped == [s.name for s in plan.steps if expect & set(sum(sc.step_tensors(s), []))], skipped
    checked = {name for name, _, _ in rows}
    assert set(splits) <= checked, sorted(set(splits) - checked)              # (no split step sits behind a fused tensor)
    assert not bad, bad
    assert decided > 0 and label_bad == 0

    # ---- the unsplit twin, and predict() of the same resampled patch on it
    x = tiling.resize_nearest(page / 255.0, h, w)[None].astype(np.float32)
    twin = SegModel(cfg, wts, device=0, max_batch=2, precision=precision)             # (the same calibrated net: make_model's handle)
    try:
        twin.ctx.set_lanes(1)
        twin.ctx.set_ksplit(False)
        labels_u, recs_u, vals_u = whole_pass(twin, page, h, w)
        twin.ctx.poison_activations(0xFF)
        probs = twin.predict(x)
        recs_p = launch_records(twin.ctx, ops)
        vals_p = {tid: twin.ctx.debug_read_tensor(tid, 1, vals[tid].shape[1:]) for tid in vals}
    finally:
        twin.release()
    assert not [r["name"] for r in recs_u + recs_p if r["family"] == "conv_splitk"]
    forms = [tid for tid in vals if plan.tensors[tid].kind.startswith("input")]
    assert forms
    for tid in forms:
        assert _same_bits(vals_u[tid], vals_p[tid]), (f"input form {plan.tensors[tid].name}: the whole-image gather of the u8 page and predict's f32 patch "
                                                      f"store different forms (ingest_u8_kernel / ingest_f32_kernel)")
        assert _same_bits(vals[tid], vals_u[tid]), plan.tensors[tid].name
    unwritten_u = {tid for tid, a in vals_u.items() if np.isnan(a).all()}
    assert unwritten_u == {tid for tid, a in vals_p.items() if np.isnan(a).all()} == expect, (names(plan, unwritten_u), names(plan, expect))
    differ = [plan.tensors[tid].name for tid in vals if tid not in expect and not _same_bits(vals_u[tid], vals_p[tid])]
    assert not differ, f"the unsplit whole-image pass and predict() of the same patch differ in {differ}"
    rows_p, skipped_p, bad_p, p_err, label_bad_p, decided_p = check_steps(plan, vals_p, precision, probs, expect, ops, f"{precision} {h}x{w} predict n=1")
    with open(os.path.join(OUT_DIR, f"step_check_{precision}_{h}x{w}_whole.md"), "a") as f:
        f.write("\n")
        write_table(f, f"{precision} {h} x {w}, {classes} classes, predict of the same patch (n = 1) on a handle with split-K off; its tensors are byte-identical "
                       f"to that handle's whole-image pass", rows_p, skipped_p, p_err, label_bad_p, decided_p)
    assert skipped_p == skipped
    assert not bad_p, bad_p
    assert decided_p > 0 and label_bad_p == 0
    assert p_err < TOL_STEP_HEAD_PROB[precision], p_err

    # ---- split against unsplit: a step that did not split and read the same bytes wrote the same bytes
    same = 0
    for s in plan.steps:
        src, dst = sc.step_tensors(s)
        if s.name in splits or not dst or expect & set(src + dst):
            continue
        if all(_same_bits(vals[t], vals_u[t]) for t in src):
            assert all(_same_bits(vals[t], vals_u[t]) for t in dst), f"{s.name} did not split and read identical sources, but differs between the handles"
            same += 1
    first_split = min(i for i, s in enumerate(plan.steps) if s.name in splits)
    assert same >= sum(1 for s in plan.steps[:first_split] if sc.step_tensors(s)[1] and not expect & set(sum(sc.step_tensors(s), []))) > 0


@pytest.mark.parametrize("precision", ["f16x3", "f16", "bf16"])
def test_split_ops_take_every_form(precision):
    """Over the configurations of one precision: a single-class and a four-class split op, one with a stored residual and one without."""
    recs = [r for cfg in WHOLE_CONFIGS if cfg[0] == precision for r in records_of(cfg) if r["family"] == "conv_splitk"]
    assert any(r["par4"] == 0 for r in recs) and any(r["par4"] == 1 for r in recs), sorted({(r["name"], r["par4"]) for r in recs})
    assert any(r["residual"] == 1 for r in recs) and any(r["residual"] == 0 for r in recs), sorted({(r["name"], r["residual"]) for r in recs})
    assert all(r["res_epilogue"] == 0 and r["tile_map"] == 0 and r["cls_minor"] == 0 and (r["BP"], r["BC"]) == (128, 128) for r in recs)


@pytest.mark.parametrize("precision", ["f16x3", "f16"])
def test_whole_image_routes_of_the_product_are_among_the_checked_ones(precision):
    """Records only (module docstring): one whole-image launch of the 448 x 448 two-class model, the size the stages run."""
    checked = {}
    for cfg in WHOLE_CONFIGS:
        if cfg[0] == precision:
            for r in records_of(cfg):
                if r["family"] != "none":
                    checked.setdefault(whole_route(r), r["name"])
    _, _, _, model = make_model(2, 448, 448, seed=12, precision=precision, max_batch=2, calib_hw=160)
    try:
        model.ctx.set_lanes(1)
        model.ctx.segment_whole(page_for(448, 448), 448, 448)
        recs, splits = split_counts(model.plan, model.ctx.ops(), launch_records(model.ctx, model.ctx.ops()))
    finally:
        model.release()
    assert splits
    print(f"[whole-image product {precision}] split counts {sorted({r['splits'] for r in recs if 'splits' in r})}")
    missing = {}
    for r in recs:
        if r["family"] != "none" and whole_route(r) not in checked:
            missing.setdefault(whole_route(r), []).append(r["name"])
    assert not missing, f"routes (family, BP, BC, fast_gather, tile_map, cls_minor, res_epilogue[, splits]) of the product's whole-image launch that no checked one takes: {missing}"
