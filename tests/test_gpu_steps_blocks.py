"""-m gpu: the fused 16-bit bottleneck blocks (csrc/bottleneck.hip: bottleneck_fused_pq and, under conv variant bit 20, bottleneck_fused)
phase by phase against the float64 reference of each phase (tests/step_check.py, bound unchanged).

The product keeps a and b of a stage-2 block in LDS, so the default-plan tables of test_gpu_steps*.py skip the nine res2* steps, and the
blocks are not bit-identical to the three launches they replace.  Conv variant bit 26 selects the DUMP instantiation of the two kernels:
the same code, which also stores what phase A packs for a lane's two inner pixels and what phase B packs to the plan tensors of a and b
(bottleneck_fused_pq, short of registers, stores these groups where they are read back from LDS: a at phase B's centre tap, b where the Q
waves read it).  Per configuration:

  * dump run (buffers poisoned, bit 26 set): the unwritten tensors are ``expected_unwritten`` minus the blocks' a / b tensors, no res2* step
    is skipped, and each of the nine block steps -- a on the device's x, b on the DUMPED a, c on the dumped b and x -- passes ``sc.failed``
    with ``ref_absmax > 0``.  Only inner pixels of a are dumped: a tile whose halo copy of a disagrees with the neighbour tile's inner a
    puts b over its bound, because b's reference is built from the dumped tensor;
  * product run (poisoned again, bit 26 clear): the a / b tensors read all-NaN, and every other tensor and the returned probabilities are
    byte-identical to the dump run's -- which ties the instantiation the product launches to the checked one.

Shapes: 64 x 96 (stage-2 map 15 x 23: 2 x 2 tiles of 8 x 16 per patch, the bottom and right tiles ragged) in f16 and bf16, whole plan; f16 at
224 x 256 (55 x 63: 28 tiles per patch) with n taken from the launch record's grid so that some block walks two tiles (the next-tile prefetch
and the hand-over of the prefetched x), where only the nine block steps get a reference.  Tables go to
results/step_check_<precision>_<H>x<W>_blocks.md; profiles/step_check.md keeps a copy."""
import copy
import io
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import step_check as sc  # noqa: E402
from gpu_common import TOL_STEP_HEAD_PROB, make_model, patches_from_page  # noqa: E402
from test_gpu_steps import OUT_DIR, check_steps, expected_unwritten, fused_block_tensors, write_table  # noqa: E402
from test_gpu_steps_at_scale import launch_records  # noqa: E402

DUMP_BIT = 1 << 26
ONE_GROUP_BIT = 1 << 20
FORMS = {"pq": 0, "one_group": ONE_GROUP_BIT}
CONFIGS = [("f16", 64, 96, 3), ("bf16", 64, 96, 3), ("f16", 224, 256, None)]       # n None: from the launch record (below)
PROBE_N = 15            # (from 16 patches on a predict is dealt to two lanes: ctx.h kMinLaneTiles)
_TABLES = {}            # (precision, h, w) -> {form: table text}; the file is rewritten with every form that has run


def _read_all(ctx, plan, n):
    return {tid: ctx.debug_read_tensor(tid, n, (t.H, t.W, t.C)) for tid, t in enumerate(plan.tensors) if t.kind != "unused"}


def _same_bytes(a, b):
    """debug_read_tensor widens the stored 16-bit numbers to fp32 exactly: equal fp32 bit patterns <=> equal stored bytes."""
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _run(model, x, variant):
    ctx = model.ctx
    ctx.set_conv_variant(variant)
    ctx.poison_activations(0xFF)
    probs = model.predict(x)
    recs = launch_records(ctx, ctx.ops())
    return probs, recs, _read_all(ctx, model.plan, x.shape[0])


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("precision,h,w,n", CONFIGS, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in CONFIGS])
def test_fused_block_phases_match_their_float64_references(precision, h, w, n, form):
    whole_plan = n is not None
    cfg, wts, g, model = make_model(2, h, w, seed=12, precision=precision, max_batch=n or PROBE_N, calib_hw=min(160, max(h, w)))
    try:
        ctx, plan = model.ctx, model.plan
        ops = ctx.ops()
        block_ops = [o for o in ops if o["name"].startswith("block")]
        if n is None:
            # the grid of a launch that fills the device = the blocks resident at once; one patch more than they can take one tile each
            ctx.set_conv_variant(FORMS[form])
            model.predict((patches_from_page(h, w, PROBE_N, seed=33) / 255.0).astype(np.float32))
            rec = launch_records(ctx, block_ops)[0]
            per_patch = rec["n_tiles"] // PROBE_N
            assert rec["n_tiles"] == per_patch * PROBE_N and rec["n_tiles"] > rec["grid"], rec
            n = rec["grid"] // per_patch + 1
            assert n <= PROBE_N, (n, rec)
        x = (patches_from_page(h, w, n, seed=33) / 255.0).astype(np.float32)
        probs_d, recs_d, vals_d = _run(model, x, FORMS[form] | DUMP_BIT)
        probs_p, recs_p, vals_p = _run(model, x, FORMS[form])
    finally:
        model.release()
    tag = f"{precision} {h}x{w} blocks {form}"
    names = lambda ids: sorted(plan.tensors[t].name for t in ids)
    ab, n_blocks = fused_block_tensors(plan)
    assert n_blocks == len(block_ops) == 3 and len(ab) == 6, (n_blocks, [o["name"] for o in ops])
    family = "bottleneck_pq" if form == "pq" else "bottleneck"
    for recs in (recs_d, recs_p):
        blk = [r for r in recs if r["name"].startswith("block")]
        assert len(blk) == 3 and all(r["family"] == family for r in blk), [(r["name"], r["family"]) for r in blk]
        if not whole_plan:
            # some block walks two tiles: XCD x's grid / 8 blocks share its ceil(n_tiles / 8) tiles (csrc/tile_walk.h)
            assert all((r["n_tiles"] + 7) // 8 > r["grid"] // 8 for r in blk), [(r["n_tiles"], r["grid"]) for r in blk]
    if not whole_plan:
        print(f"[{tag}] n = {n}: {blk[0]['n_tiles']} tiles on {blk[0]['grid']} blocks")

    # ---- dump run: a and b are written, nothing else changes in what is written, every block step holds its bound
    unwritten = {tid for tid, a in vals_d.items() if np.isnan(a).all()}
    product_expect = expected_unwritten(plan, precision, ops)
    expect = expected_unwritten(plan, precision, ops, dump_blocks=True)
    assert expect == product_expect - set(ab) and set(ab) <= product_expect
    assert unwritten == expect, (names(unwritten), names(expect))
    block_steps = [s for s in plan.steps if set(ab) & set(sum(sc.step_tensors(s), []))]
    assert len(block_steps) == 9 and all(s.name.startswith("res2") for s in block_steps), [s.name for s in block_steps]
    checked_plan = plan
    if not whole_plan:
        checked_plan = copy.copy(plan)
        checked_plan.steps = block_steps
    rows, skipped, bad, p_err, label_bad, decided = check_steps(checked_plan, vals_d, precision, probs_d if whole_plan else None, unwritten, ops, tag)
    assert not [s for s in skipped if s.startswith("res2")], skipped
    want_skipped = [s.name for s in checked_plan.steps if expect & set(sum(sc.step_tensors(s), []))]
    assert skipped == want_skipped, (skipped, want_skipped)
    phase = {s.name: f"{block_ops[i // 3]['name']} (phase {'ABC'[i % 3]}, {family})" for i, s in enumerate(block_steps)}
    rows = [(name, phase.get(name, kern), rep) for name, kern, rep in rows]
    block_rows = [r for r in rows if r[0] in phase]
    assert len(block_rows) == 9
    kinds = {(bool(s.residual >= 0), len(s.srcs)) for s in block_steps[2::3]}
    assert kinds == {(True, 1), (False, 2)}, kinds                      # identity blocks (residual) and the projection block ([b, x])
    os.makedirs(OUT_DIR, exist_ok=True)
    blk0 = next(r for r in recs_d if r["name"] == block_ops[0]["name"])
    buf = io.StringIO()
    write_table(buf, f"{precision} {h} x {w}, 2 classes, n = {n}, default plan with conv variant bit 26 (a and b of the fused blocks stored), "
                     f"{'bottleneck_fused_pq' if form == 'pq' else 'bottleneck_fused (bit 20)'}, {blk0['n_tiles']} tiles on {blk0['grid']} blocks"
                     + ("" if whole_plan else "; the nine block steps only"),
                rows, skipped, p_err if whole_plan else None, label_bad, decided)
    _TABLES.setdefault((precision, h, w), {})[form] = buf.getvalue()
    with open(os.path.join(OUT_DIR, f"step_check_{precision}_{h}x{w}_blocks.md"), "w") as f:
        f.write("\n".join(_TABLES[(precision, h, w)][k] for k in FORMS if k in _TABLES[(precision, h, w)]))
    for name, _, rep in block_rows:
        assert not sc.failed(rep) and rep["ref_absmax"] > 0, (name, rep)
    assert not bad, bad
    if whole_plan:
        assert decided > 0 and label_bad == 0
        assert p_err < TOL_STEP_HEAD_PROB[precision], p_err

    # ---- product run: a and b stay in LDS, everything else is the dump run's, byte for byte
    unwritten_p = {tid for tid, a in vals_p.items() if np.isnan(a).all()}
    assert unwritten_p == product_expect, (names(unwritten_p), names(product_expect))
    differ = [plan.tensors[tid].name for tid in vals_p if tid not in ab and not _same_bytes(vals_p[tid], vals_d[tid])]
    assert not differ, differ
    assert _same_bytes(probs_p, probs_d)
