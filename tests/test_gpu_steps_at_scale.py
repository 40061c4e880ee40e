"""-m gpu: the per-step float64 check of tests/test_gpu_steps.py on launches of the size the product runs.

test_gpu_steps.py runs 2 to 5 patches per launch; at that size conv_igemm_mfma stays on its 128 x 128 tile with the class-major walk, and its
encoder launches give a persistent block at most one tile (the CU-sized grids of the direct kernels do loop there: the tail walks 6272 tiles
on 256 blocks at two 448 x 448 patches; the records below assert the loop either way).  Here one ``predict`` runs N patches in ONE launch per
op (lane 0, max_batch = N):

  * the batch is K = 5 distinct patches repeated cyclically, x[i] = x[i % K];
  * patches [0, K) of the big launch are read back and held to the derived float64 bounds, step by step, with the helpers and the
    tolerances of test_gpu_steps.py unchanged (``check_steps``, ``expected_unwritten``, ``sc.failed``, ``TOL_STEP_HEAD_PROB``);
  * every written plan tensor must be periodic with period K over all N patches, byte for byte over the whole patch stride (compared on the
    device: ``tensor_period_mismatches``), and so must the returned probabilities.  Within one launch the arithmetic of an element does not
    depend on the tile that computes it, so every element of the big launch inherits the bound of its image among the first K patches;
  * the launch records (``op_launch``: filled by the host where each launch is sized) say which kernel route every op took, and the test
    FAILS if the routes it is there for are not taken.

N.  N = 587, a prime (no multiple of K, of 8 or of a tile size).  A conv of stage 4 (224 output pixels a patch at 224 x 256, one or four
channel tiles of 256) gets ceil(224 N / 256) >= 2 * 256 + 1 pixel tiles from N = 586 on: the smallest N at which every ROUTE seen -- the tuple
(family, BP, BC, fast_gather, tile_map, cls_minor, residual in the epilogue) -- has an op with two full trips and a ragged last round
(n_tiles >= 2 * grid + 1), which is what is asserted.  N = 563 would reproduce the pixel count of the product's chunk (160 x 448 x 448) exactly,
but leaves the 3 x 3 convs of stages 4 / 5 on the 256 x 256 tile without such an op (493 and 248 tiles on 256 blocks).  Two full trips for every
OP is out of reach: the 512-channel convs of stage 5 (56 pixels a patch, two channel tiles) need N >= 1171, where the split mode's largest
stored tensor (3 670 016 bytes a patch) passes 4 GiB, beyond the kernels' 32-bit byte offsets -- the product's own chunk runs them at 246 tiles
on 246 blocks.  The tables list n_tiles / grid of every op.

Tile map 2 (every block walks a contiguous run of its XCD's tiles) is opt-in -- conv variant bits 8-15 set the K limit, the default is 0 -- so
no default plan takes it; the unfused split-mode configuration sets the limit to K = 512 on top of its unfuse bits so that the walk is checked
too (tile map 1 stays on the longer-K layers).  conv3_expand_reduce needs stage-3 maps whose sides are multiples of 8 (28 x 32 at 224 x 256
is not): the 256 x 256 configurations are there for it, since the product's 448 x 448 plan runs it.

One table per configuration goes to results/step_check_<precision>_<H>x<W>_<plan>_n<N>.md; profiles/step_check.md keeps a copy."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import step_check as sc  # noqa: E402
from gpu_common import TOL_STEP_HEAD_PROB, make_model, patches_from_page  # noqa: E402
from test_gpu_steps import OUT_DIR, UNFUSED_BITS, check_steps, expected_unwritten, write_table  # noqa: E402

K = 5
N = 587
CONTIG_K512 = 8 << 8                      # conv variant bits 8-15: tile map 2 up to K = 8 * 64
SCALE_CONFIGS = [("f16x3", 224, 256, "default"), ("f16x3", 224, 256, "unfused"), ("f16", 224, 256, "default"),
                 ("f16x3", 256, 256, "default"), ("f16", 256, 256, "default")]
NOT_PERSISTENT = {"maxpool", "head", "conv_naive_f32"}      # one block per slice of the output: no loop carries state to a second work item
ROUTE_FIELDS = ("family", "BP", "BC", "fast_gather", "tile_map", "cls_minor", "res_epilogue")
_ROUTES = {}                              # (precision, h, w, mode) -> {route: [op names]} of the big launch, for the subset test


def route_of(rec):
    return tuple(rec[k] for k in ROUTE_FIELDS)


def cyclic_batch(h, w, n, k, seed=33):
    base = (patches_from_page(h, w, k, seed=seed) / 255.0).astype(np.float32)
    return base[np.arange(n) % k]


def launch_records(ctx, ops):
    return [dict(ctx.op_launch(o["index"]), name=o["name"]) for o in ops]


def routes_by_name(recs):
    out = {}
    for r in recs:
        if r["family"] != "none":
            out.setdefault(route_of(r), []).append(r["name"])
    return out


def assert_periodic(ctx, plan, n, k, probs, written):
    """0 differing bytes at period k over all n patches in every written plan tensor and in the probabilities."""
    bad = {}
    for tid in sorted(written):
        cnt, first = ctx.tensor_period_mismatches(tid, n, k)
        if cnt:
            bad[plan.tensors[tid].name] = (cnt, first)
    assert not bad, f"(differing bytes, first byte offset past patch {k}) per tensor: {bad}"
    bits = probs.view(np.uint32)
    diff = bits[k:] != bits[:-k]
    assert not diff.any(), ("probs", int(diff.sum()), tuple(int(i) for i in np.argwhere(diff)[0]))


def write_routes(f, n, recs):
    f.write(f"\nlaunch records at n = {n} (route = family, BP x BC, LDS stages, fast gather, tile map, class-minor, residual in the epilogue)\n\n")
    ks = any("splits" in r for r in recs)                     # (tests/test_gpu_steps_whole.py adds the split count of a conv_splitk launch)
    f.write("| op | family | BP x BC | stages | fast gather | tile map | class-minor | residual (epilogue) | n_tiles / grid |" + (" splits |" if ks else "")
            + "\n|---|---|---|---|---|---|---|---|---|" + ("---|" if ks else "") + "\n")
    for r in recs:
        if r["family"] == "none":
            f.write(f"| {r['name']} | none (in another op's launch) | | | | | | | |" + (" |" if ks else "") + "\n")
        else:
            f.write(f"| {r['name']} | {r['family']} | {r['BP']} x {r['BC']} | {r['stages']} | {r['fast_gather']} | {r['tile_map']} | {r['cls_minor']} | "
                    f"{r['residual']} ({r['res_epilogue']}) | {r['n_tiles']} / {r['grid']} = {r['n_tiles'] / r['grid']:.2f} |"
                    + (f" {r.get('splits', '-')} |" if ks else "") + "\n")


def big_launch(model, plan, n, k, h, w, variant=0, reference=True):
    """One predict of n cyclic patches on poisoned buffers -> (launch records, values of patches [0, k) per plan tensor, probs of [0, k),
    ids of the tensors no launch wrote); periodicity is asserted on the way.  reference=False: records only."""
    ctx = model.ctx
    if variant:
        ctx.set_conv_variant(variant)
    ops = ctx.ops()
    x = cyclic_batch(h, w, n, k)
    ctx.poison_activations(0xFF)
    probs = model.predict(x)
    recs = launch_records(ctx, ops)
    if not reference:
        return recs, None, None, None
    vals = {tid: ctx.debug_read_tensor(tid, k, (t.H, t.W, t.C)) for tid, t in enumerate(plan.tensors) if t.kind != "unused"}
    unwritten = {tid for tid, a in vals.items() if np.isnan(a).all()}
    assert_periodic(ctx, plan, n, k, probs, set(vals) - unwritten)
    return recs, vals, np.ascontiguousarray(probs[:k]), unwritten


def check_against_float64(plan, precision, mode, ops, vals, probs, unwritten, tag):
    """test_every_step_matches_its_float64_reference's assertions on the first patches of the big launch."""
    expect = expected_unwritten(plan, precision, ops) if mode == "default" else set()
    names = lambda ids: sorted(plan.tensors[t].name for t in ids)
    assert unwritten == expect, (names(unwritten), names(expect))
    rows, skipped, bad, p_err, label_bad, decided = check_steps(plan, vals, precision, probs, unwritten, ops, tag)
    want_skipped = [s.name for s in plan.steps if expect & set(sum(sc.step_tensors(s), []))]
    assert skipped == want_skipped, (skipped, want_skipped)
    assert mode == "default" or not skipped
    return rows, skipped, bad, p_err, label_bad, decided


def assert_checked(precision, bad, p_err, label_bad, decided):
    assert not bad, bad
    assert decided > 0 and label_bad == 0
    assert p_err < TOL_STEP_HEAD_PROB[precision], p_err


def scale_variant(precision, mode):
    if mode != "unfused":
        return 0
    return UNFUSED_BITS | (CONTIG_K512 if precision == "f16x3" else 0)


def run_scale_config(precision, h, w, mode, monkeypatch, reference=True):
    if mode == "unfused":
        monkeypatch.setenv("SBBSEG_FUSE_BLOCKS", "0")
    cfg, wts, g, model = make_model(4, h, w, seed=12, precision=precision, max_batch=N, calib_hw=min(160, max(h, w)))
    try:
        plan, ops = model.plan, model.ctx.ops()
        recs, vals, probs, unwritten = big_launch(model, plan, N, K, h, w, scale_variant(precision, mode), reference)
    finally:
        model.release()
    _ROUTES[(precision, h, w, mode)] = routes_by_name(recs)
    return plan, ops, recs, vals, probs, unwritten


@pytest.mark.parametrize("precision,h,w,mode", SCALE_CONFIGS, ids=[f"{c[0]}-{c[1]}x{c[2]}-{c[3]}" for c in SCALE_CONFIGS])
def test_steps_of_a_product_sized_launch(precision, h, w, mode, monkeypatch):
    plan, ops, recs, vals, probs, unwritten = run_scale_config(precision, h, w, mode, monkeypatch)
    tag = f"{precision} {h}x{w} {mode} n={N}"
    rows, skipped, bad, p_err, label_bad, decided = check_against_float64(plan, precision, mode, ops, vals, probs, unwritten, tag)
    os.makedirs(OUT_DIR, exist_ok=True)
    with open(os.path.join(OUT_DIR, f"step_check_{precision}_{h}x{w}_{mode}_n{N}.md"), "w") as f:
        write_table(f, f"{precision} {h} x {w}, 4 classes, one launch of N = {N} patches ({K} distinct, cyclic; patches [0, {K}) checked, "
                       f"all {N} periodic byte for byte), {mode} plan", rows, skipped, p_err, label_bad, decided)
        write_routes(f, N, recs)
    assert_checked(precision, bad, p_err, label_bad, decided)
    # coverage: what this configuration is there for must have been launched, and launched big enough
    launched = [r for r in recs if r["family"] != "none"]
    for r in launched:
        print(f"[launch {tag}] {r['name']}: {route_of(r)} n_tiles {r['n_tiles']} grid {r['grid']}")
        assert r["table"] == 0, r                                # (no owned-region launches here: test_gpu_region_steps.py owns those)
        assert r["persistent"] == (r["family"] not in NOT_PERSISTENT), r
    two_trips = {}
    for r in launched:
        if r["persistent"]:
            two_trips[route_of(r)] = two_trips.get(route_of(r), False) or r["n_tiles"] >= 2 * r["grid"] + 1
    assert all(two_trips.values()), f"routes without an op of two full trips and a ragged round: {[k for k, v in two_trips.items() if not v]}"
    seen = set(two_trips)
    big = {s for s in seen if s[0] == "conv_igemm" and s[1:3] == (256, 256)}
    assert any(s[6] == 1 for s in big), f"no 256 x 256 tile with the residual in its epilogue: {sorted(seen)}"
    assert any(s[6] == 0 for s in big), f"no 256 x 256 tile without a residual: {sorted(seen)}"
    assert any(s[5] == 1 for s in seen), f"no class-minor walk: {sorted(seen)}"
    if precision == "f16x3":                                     # (the plain modes keep single-class layers on tile map 0: launch_op)
        assert any(s[4] == 1 and s[5] == 0 for s in seen), f"no single-class launch on tile map 1: {sorted(seen)}"
    if precision == "f16x3" and mode == "unfused":
        assert any(s[4] == 2 for s in seen), f"no tile map 2: {sorted(seen)}"
    if (h, w) == (256, 256):
        assert any(s[0] == "conv3_expand_reduce" for s in seen), sorted(seen)


@pytest.mark.parametrize("precision", ["f16x3", "f16"])
def test_product_routes_are_among_the_checked_ones(precision, monkeypatch):
    """The routes of one 160-patch launch at 448 x 448 (what bench.py and a page take run per chunk) must all be routes of the checked launches
    above, so that the step check follows the product when tile heuristics move.  No reference work here."""
    checked = {}
    for cfg in SCALE_CONFIGS:
        if cfg[0] != precision:
            continue
        if cfg not in _ROUTES:                                   # (this test selected alone: records only)
            run_scale_config(*cfg, monkeypatch, reference=False)
            monkeypatch.delenv("SBBSEG_FUSE_BLOCKS", raising=False)
        for route, names in _ROUTES[cfg].items():
            checked.setdefault(route, names)
    cfg, wts, g, model = make_model(2, 448, 448, seed=12, precision=precision, max_batch=160, calib_hw=160)
    try:
        recs, _, _, _ = big_launch(model, model.plan, 160, K, 448, 448, reference=False)
    finally:
        model.release()
    product = routes_by_name(recs)
    missing = {route: names for route, names in product.items() if route not in checked}
    assert not missing, f"routes {ROUTE_FIELDS} of the product's launch that no checked launch takes, with their ops: {missing}"


def test_steps_across_the_2gib_gather_switch(monkeypatch):
    """launch_op takes a conv off the fast gather when a source's bytes in use reach 2^31 (bit 31 of a lane offset marks an out-of-bounds tap).
    At 448 x 448 in the split mode the largest tensors store 12 845 056 bytes a patch: 167 patches stay below 2^31 (2 145 124 352 bytes), 168
    pass it, and 173 is the first prime past the switch.  One lane, so that the second lane's buffers are not allocated."""
    import torch
    precision, h, w, k, n = "f16x3", 448, 448, 2, 173
    monkeypatch.setenv("SBBSEG_LANES", "1")
    cfg, wts, g, model = make_model(2, h, w, seed=12, precision=precision, max_batch=1, calib_hw=160)
    try:
        per_patch = model.ctx.device_bytes()
    finally:
        model.release()
    need = per_patch * n
    free, total = torch.cuda.mem_get_info()
    if free < 1.1 * need:
        pytest.skip(f"needs {need / 2**30:.1f} GiB (+10 %) of device memory for one lane of {n} patches, {free / 2**30:.1f} GiB of {total / 2**30:.1f} GiB are free")
    cfg, wts, g, model = make_model(2, h, w, seed=12, precision=precision, max_batch=n, calib_hw=160)
    try:
        plan, ops = model.plan, model.ctx.ops()
        small, _, _, _ = big_launch(model, plan, k, k, h, w, reference=False)
        recs, vals, probs, unwritten = big_launch(model, plan, n, k, h, w)
    finally:
        model.release()
    switched = [b["name"] for a, b in zip(small, recs) if a["fast_gather"] >= 1 and b["fast_gather"] == 0 and b["family"] == "conv_igemm"]
    print(f"[2 GiB switch] off the fast gather at n = {n}: {switched}")
    assert switched, "no op left the fast gather"
    tag = f"{precision} {h}x{w} default n={n}"
    rows, skipped, bad, p_err, label_bad, decided = check_against_float64(plan, precision, "default", ops, vals, probs, unwritten, tag)
    os.makedirs(OUT_DIR, exist_ok=True)
    with open(os.path.join(OUT_DIR, f"step_check_{precision}_{h}x{w}_default_n{n}.md"), "w") as f:
        write_table(f, f"{precision} {h} x {w}, 2 classes, one launch of N = {n} patches on one lane ({k} distinct, cyclic; patches [0, {k}) checked, "
                       f"all {n} periodic byte for byte), default plan; off the fast gather: {', '.join(switched)}", rows, skipped, p_err, label_bad, decided)
        write_routes(f, n, recs)
    assert_checked(precision, bad, p_err, label_bad, decided)
