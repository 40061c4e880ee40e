"""-m gpu: what the owned-region decoder launches (csrc/region.h, region.hip, sbbseg_set_owned_regions) WRITE, level by level.

tests/test_gpu_regions.py compares stitched label maps only.  Here the activations of every decoder level are read back
(``debug_read_tensor``) after a whole-tile run and after owned-region runs over poisoned buffers, and held to tests/regions_ref.py,
a loop-by-loop restatement of region.h (pinned on the CPU by tests/test_regions_ref_cpu.py):

  (a) executed work: ``exec_patches * Rh * Rw / 256`` (16 x 16 tiles, kind 0) or ``/ 4`` (class-grid pixels, kind 1) is the number of
      table entries of the restatement, for one of the two kinds -- which also tells the kind the library chose (the handle does not
      export it); under conv variant 1 every level below the tail is kind 1, at variant 0 one level takes the tile kernel.
  (b) exact footprint: with the finite poison byte 0x3C, the pixels that differ from the poison pattern (read off the handle before
      its first launch) are exactly ``footprint()`` of the restatement, per patch and level -- a table that covers more would leave the
      labels alone and make ``exec_patches`` (and every roofline fraction priced on it) wrong; one that covers less shows here at its
      level and pixel.  A tile that owns nothing (the repeated clamped tile, dedupe off) writes nothing at any level.
  (c) level 0 has no stored tensor: ``set_owned_regions(2)`` + ``segment_tile_range_dev`` into a buffer filled with a value no class
      uses; the touched pixels of every tile are the kind-0 footprint of level 0, and on the owned box they are the whole-tile labels.
  (d) with NaN poison, on ``needed_box`` of every patch and level the owned-region tensors are finite and bit-identical to the
      whole-tile image, and the stitched maps are equal.  Pixels inside the footprint but outside the needed box (the rounding of a
      box to tiles / to an even class grid) may hold anything: their taps need not have been written below, nothing reads them.
  (e) 224 x 224 model: each decoder class step and the tail of the owned-region run (NaN poison) against the float64 reference of
      THAT step on the stored inputs (tests/step_check.py), masked to the step's part of the needed box: ``n_ref_bad == 0`` says that
      every tap a needed pixel reads was written by the level below.  Four patches (corner, interior, short, clamped) keep the
      float64 convolutions short.  The page entry points store no probabilities, so the tail's ``p_err`` is taken from ``predict`` on
      the same tile pixels -- after checking that it left bit-identical tail inputs on the needed box -- and the labels of the
      owned-region run itself (cut from the stitched map) go through the same float64 margin rule.

Recipe: one lane and max_batch >= the page's tile count, so one chunk holds the page and patch p is tile p of the grid
(g -> (i, j) = (g // ny, g % ny), x outer).  Pages: 583 x 700 on the 224 model (rows 0 / 180 / 359, the fourth row repeats the third
and is dropped by dedupe; columns first / interior / short penultimate / clamped last) and 404 x 405 (a repeated clamped row, a
column that keeps one pixel), dedupe on and off; 1000 x 1234 on the 448 model, the product's size."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import regions_ref as rr  # noqa: E402
import step_check as sc  # noqa: E402
from gpu_common import TOL_STEP_HEAD_PROB, make_model  # noqa: E402
from sbb_textline_detection_amd.synthetic import synthetic_page  # noqa: E402

FINITE_POISON, NAN_POISON = 0x3C, 0xFF
UNUSED_LABEL = 0xEE
# (model side, classes, max_batch, [(page rows, page columns, dedupe)])
MODELS = {224: (4, 16, [(583, 700, True), (404, 405, True), (404, 405, False)]), 448: (2, 12, [(1000, 1234, True)])}
PRECISIONS = ("f16x3", "f16")
VARIANTS = (0, 1)                 # conv variant 1: every decoder conv on the generic kernel (pixel tables)
# the model (fixture `net`, parametrised indirectly: one handle per size and precision for the whole module) x page x variant
CASES = [pytest.param((side, p), hp, wp, dd, v, id=f"{side}-{p}-{hp}x{wp}-{'dedupe' if dd else 'all'}-variant{v}")
         for side, (_, _, pages) in MODELS.items() for p in PRECISIONS for hp, wp, dd in pages for v in VARIANTS]
TILE_CASES = [pytest.param((side, p), hp, wp, v, id=f"{side}-{p}-{hp}x{wp}-variant{v}")
              for side, (_, _, pages) in MODELS.items() for p in PRECISIONS for hp, wp in sorted({q[:2] for q in pages}) for v in VARIANTS]
REF_CASES = [pytest.param((224, p), v, id=f"224-{p}-variant{v}") for p in PRECISIONS for v in VARIANTS]


class Level:
    def __init__(self, steps, tensor, H, W, C):
        self.steps, self.tensor, self.H, self.W, self.C = steps, tensor, H, W, C


def find_chain(plan):
    """The plan's side of find_region_chain (csrc/plan_build.hip): the tail, then down through source 0 of the parity-split decoder convs."""
    tail = plan.steps[-1]
    assert tail.kind == "tail"
    chain = [Level([tail], -1, tail.out_h, tail.out_w, 0)]
    below = tail.src0
    while True:
        st = [s for s in plan.steps if s.kind == "conv" and s.out == below]
        t = plan.tensors[below]
        readers = sum(1 for s in plan.steps for tid in sc.step_tensors(s)[0] if tid == below)
        ok = (len(st) == 4 and {s.out_off for s in st} == {(0, 0), (0, 1), (1, 0), (1, 1)} and readers == (1 if len(chain) == 1 else 4)
              and all(s.out_stride == (2, 2) and len(s.srcs) == 2 and s.residual < 0 and s.raw_out < 0 and s.head is None
                      and (s.srcs[0].kh, s.srcs[0].kw, s.srcs[0].stride_y, s.srcs[0].shift) == (2, 2, 1, 0)
                      and (2 * s.out_h, 2 * s.out_w) == (t.H, t.W) and plan.tensors[s.srcs[0].tensor].H == s.out_h for s in st))
        if not ok:
            return chain
        chain.append(Level(sorted(st, key=lambda s: s.out_off), below, t.H, t.W, t.C))
        below = st[0].srcs[0].tensor


def _level_op(ops, lv):
    if lv.tensor < 0:
        hit = [o for o in ops if o["name"].startswith("tail_")]
    else:
        s = lv.steps[0]
        base = f"conv{s.srcs[0].kh}x{s.srcs[0].kw}_c{sum(g.channels for g in s.srcs)}to{s.cout}_{s.out_h}x{s.out_w}_"
        hit = [o for o in ops if o["name"].startswith(base) and "_par4" in o["name"]]
    assert len(hit) == 1, (lv.tensor, [o["name"] for o in ops])
    return hit[0]


_NETS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_nets():
    yield
    for model in _NETS.values():
        model.release()
    _NETS.clear()


@pytest.fixture
def net(request):
    """One handle per (model side, precision), made on first use and shared by every case of the module (the cases of a handle are not
    adjacent in the run order, and a handle with its calibrated net takes longer to make than all its cases take to run)."""
    side, precision = request.param
    if (side, precision) in _NETS:
        return _NETS[(side, precision)]
    classes, max_batch, _ = MODELS[side]
    cfg, w, g, model = make_model(classes, side, side, seed=9, precision=precision, max_batch=max_batch, calib_hw=160)
    _NETS[(side, precision)] = model
    model.side, model.test_precision, model.chain = side, precision, find_chain(model.plan)
    ctx = model.ctx
    ctx.set_lanes(1)
    # the poison pattern as debug_read_tensor returns it, off the handle BEFORE its first launch (one value per channel)
    ctx.poison_activations(FINITE_POISON)
    model.pattern = {}
    for L, lv in enumerate(model.chain):
        if L >= 1:
            a = ctx.debug_read_tensor(lv.tensor, 1, (lv.H, lv.W, lv.C))[0]
            assert np.isfinite(a).all() and (a == a[0, 0]).all(), (L, "the poison pattern is not one finite value per channel")
            model.pattern[L] = a[0, 0].copy()
    model.captures = {}
    return model


def _geom(model, hp, wp, dedupe):
    return rr.make_geom(hp, wp, model.side, model.side, [(lv.H, lv.W) for lv in model.chain], dedupe)


def _page(hp, wp):
    return synthetic_page(hp, wp, seed=hp * 7 + wp)


def _read_levels(model, n):
    return {L: model.ctx.debug_read_tensor(lv.tensor, n, (lv.H, lv.W, lv.C)) for L, lv in enumerate(model.chain) if L >= 1}


def capture(model, hp, wp, dedupe, variant, keep_vals=False):
    """Whole-tile run, then owned-region runs over 0x3C and NaN poison.  Returns small per-pixel maps (the tensors are dropped):
    written[L] bool [n, H, W] (finite poison), same[L] bool [n, H, W] (NaN poison: finite and bit-identical to the whole-tile image),
    exec[L] (exec_patches of the level's op), labels of the three runs."""
    key = (hp, wp, dedupe, variant)
    if key in model.captures and not keep_vals:
        return model.captures[key]
    t0 = time.time()
    ctx, chain = model.ctx, model.chain
    geom = _geom(model, hp, wp, dedupe)
    n = geom.tpp
    page = _page(hp, wp)
    cap = dict(geom=geom, n=n)
    ctx.set_dedupe(dedupe)
    ctx.set_conv_variant(variant)
    try:
        ctx.poison_activations(NAN_POISON)
        ctx.set_owned_regions(0)
        cap["labels_whole"] = ctx.segment_page(page)
        whole = _read_levels(model, n)
        for poison in (FINITE_POISON, NAN_POISON):
            ctx.poison_activations(poison)
            ctx.set_owned_regions(1)
            ctx.profile_reset()
            labels = ctx.segment_page(page)
            got = _read_levels(model, n)
            if poison == FINITE_POISON:
                cap["labels_finite"] = labels
                cap["written"] = {L: (a != model.pattern[L]).any(-1) for L, a in got.items()}
            else:
                cap["labels_nan"] = labels
                ops = ctx.profile()
                cap["exec"] = {L: float(_level_op(ops, lv)["exec_patches"]) for L, lv in enumerate(chain)}
                cap["same"] = {L: (a.view(np.uint32) == whole[L].view(np.uint32)).all(-1) & np.isfinite(a).all(-1) for L, a in got.items()}
                cap["whole_finite"] = {L: bool(np.isfinite(w).all()) for L, w in whole.items()}
                if keep_vals:
                    cap["owned_vals"] = got
    finally:
        ctx.set_conv_variant(0)
        ctx.set_dedupe(True)
    cap["seconds"] = time.time() - t0
    print(f"[region steps {model.side} {model.test_precision} {hp}x{wp} dedupe {dedupe} variant {variant}] {n} tiles, capture {cap['seconds']:.2f} s")
    if not keep_vals:
        model.captures[key] = cap
    return cap


def _counts(geom, L, R_h, R_w):
    """{kind: entries of the whole page} for the kinds a launch of this level can take."""
    kinds = [0] if L == 0 else ([0, 1] if min(R_h, R_w) >= 16 else [1])
    return {k: sum(len(rr.entries(geom, g, L, k)) for g in range(geom.tpp)) for k in kinds}


def kinds_from_executed_work(model, cap):
    """(a): ({level: kinds whose table size is what the launch reports}, [a message per level where that is neither kind])."""
    out, errors = {}, []
    for L, lv in enumerate(model.chain):
        counts = _counts(cap["geom"], L, lv.H, lv.W)
        work = {k: cap["exec"][L] * lv.H * lv.W / (4 if k else 256) for k in counts}
        print(f"    level {L} ({lv.H} x {lv.W}): exec_patches {cap['exec'][L]:.6f} of {cap['n']} -> tiles / class pixels {work}, tables {counts}")
        out[L] = [k for k in counts if abs(work[k] - round(work[k])) < 1e-6 and round(work[k]) == counts[k]]
        if not out[L]:
            errors.append(f"level {L}: exec_patches {cap['exec'][L]!r} = {work} tiles (kind 0) / class pixels (kind 1), the tables have {counts}")
    return out, errors


def _where(diff):
    p, y, x = (int(v[0]) for v in np.nonzero(diff))
    return f"first at patch {p} (y {y}, x {x}), {int(diff.sum())} pixels in {sorted(set(np.nonzero(diff)[0].tolist()))}"


@pytest.mark.parametrize("net,hp,wp,dedupe,variant", CASES, indirect=["net"])
def test_chain_and_executed_work(net, hp, wp, dedupe, variant):
    """(a), and the plan's chain against the library's."""
    assert len(net.chain) == net.ctx.owned_region_levels() == 5          # tail and four decoder convs, down to 28 x 28 (14 x 14 on the 224 model)
    cap = capture(net, hp, wp, dedupe, variant)
    kinds, errors = kinds_from_executed_work(net, cap)
    assert not errors, errors
    assert kinds[0] == [0]
    for L in range(1, len(net.chain)):
        if variant & 3:
            assert 1 in kinds[L], (L, kinds[L])                  # the generic kernel reads the pixel table
        assert cap["exec"][L] < cap["n"]                         # (none of these pages has a tile that keeps everything at every level)
    if variant == 0:
        assert any(0 in kinds[L] and 1 not in kinds[L] for L in range(1, len(net.chain))), kinds       # the LDS-halo tile kernel's level


@pytest.mark.parametrize("net,hp,wp,dedupe,variant", CASES, indirect=["net"])
def test_written_pixels_are_exactly_the_footprint(net, hp, wp, dedupe, variant):
    """(b)"""
    cap = capture(net, hp, wp, dedupe, variant)
    geom, n = cap["geom"], cap["n"]
    kinds, _ = kinds_from_executed_work(net, cap)
    empty = [g for g in range(n) if rr.needed_box(geom, g, 0) == (0, 0, 0, 0)]
    assert bool(empty) == (not dedupe and (hp, wp) == (404, 405))
    errs = []
    for L in range(1, len(net.chain)):
        written = cap["written"][L]
        lv_errs = []
        # the kind (a) found; where the executed work is no table at all, either footprint is accepted
        for kind in kinds[L] or list(_counts(geom, L, net.chain[L].H, net.chain[L].W)):
            want = np.stack([rr.footprint(geom, g, L, kind) for g in range(n)])
            extra, missing = written & ~want, want & ~written
            if not extra.any() and not missing.any():
                lv_errs = []
                break
            lv_errs.append(f"level {L} kind {kind}: " + (f"written outside the footprint, {_where(extra)}; " if extra.any() else "")
                           + (f"footprint not written, {_where(missing)}" if missing.any() else ""))
        errs += lv_errs
        errs += [f"level {L}: tile {g} owns nothing and wrote {int(written[g].sum())} pixels" for g in empty if written[g].any()]
    assert not errs, errs
    assert np.array_equal(cap["labels_finite"], cap["labels_whole"])


@pytest.mark.parametrize("net,hp,wp,dedupe,variant", CASES, indirect=["net"])
def test_needed_box_is_bit_identical_to_the_whole_tile_run(net, hp, wp, dedupe, variant):
    """(d)"""
    cap = capture(net, hp, wp, dedupe, variant)
    geom, n = cap["geom"], cap["n"]
    errs = []
    for L in range(len(net.chain) - 1, 0, -1):                               # the deepest level first: what is wrong there is wrong above
        assert cap["whole_finite"][L], L
        need = np.stack([rr.needed_mask(geom, g, L) for g in range(n)])
        assert need.any()
        bad = need & ~cap["same"][L]
        if bad.any():
            errs.append(f"level {L}: needed pixels that are not finite / not the whole-tile bits, {_where(bad)}")
    assert not errs, errs
    assert np.array_equal(cap["labels_nan"], cap["labels_whole"]), int((cap["labels_nan"] != cap["labels_whole"]).sum())
    assert 0.01 < float((cap["labels_whole"] > 0).mean()) < 0.99


@pytest.mark.parametrize("net,hp,wp,variant", TILE_CASES, indirect=["net"])
def test_level0_touches_exactly_its_tiles(net, hp, wp, variant):
    """(c): the tile-range entry point computes the reference's whole call list (no dedupe)."""
    import torch
    ctx, side = net.ctx, net.side
    geom = _geom(net, hp, wp, False)
    n = geom.tpp
    assert n <= MODELS[side][1]
    d_page = torch.from_numpy(_page(hp, wp)).cuda()
    tiles = {}
    ctx.set_conv_variant(variant)
    try:
        for mode in (1, 2):
            ctx.set_owned_regions(mode)
            ctx.poison_activations(NAN_POISON)
            d_tiles = torch.full((n, side, side), UNUSED_LABEL, dtype=torch.uint8, device="cuda")
            ctx.segment_tile_range_dev(d_page.data_ptr(), hp, wp, 0, n, d_tiles.data_ptr())
            ctx.synchronize()
            tiles[mode] = d_tiles.cpu().numpy()
    finally:
        ctx.set_conv_variant(0)
        ctx.set_owned_regions(1)
    assert (tiles[1] < MODELS[side][0]).all()                                 # mode 1: whole tiles
    touched = tiles[2] != UNUSED_LABEL
    want = np.stack([rr.footprint(geom, g, 0, 0) for g in range(n)])
    extra, missing = touched & ~want, want & ~touched
    assert not extra.any(), f"level 0: labels written outside the footprint, {_where(extra)}"
    assert not missing.any(), f"level 0: footprint not written, {_where(missing)}"
    need = np.stack([rr.needed_mask(geom, g, 0) for g in range(n)])
    bad = need & (tiles[2] != tiles[1])
    assert not bad.any(), f"level 0: owned labels differ from the whole-tile labels, {_where(bad)}"


@pytest.mark.parametrize("net,variant", REF_CASES, indirect=["net"])
def test_each_level_matches_its_float64_reference_on_the_needed_box(net, variant):
    """(e) -- the 224 x 224 model only: the 448 x 448 case would cost a minute of CPU convolution."""
    hp, wp, dedupe = 583, 700, True
    precision, plan, chain, ctx = net.test_precision, net.plan, net.chain, net.ctx
    cap = capture(net, hp, wp, dedupe, variant, keep_vals=True)             # (the handle's buffers now hold the NaN-poison owned run)
    geom, n = cap["geom"], cap["n"]
    sel = [i * geom.ny + j for i, j in ((0, 0), (1, 1), (2, 1), (3, 2))]     # corner, interior, short penultimate column, clamped last
    t0 = time.time()
    need_ids = {tid for lv in chain for s in lv.steps for tid in sum(sc.step_tensors(s), [])}
    vals = {}
    ctx.set_conv_variant(variant)
    try:
        for tid in need_ids:
            L = next((k for k, lv in enumerate(chain) if lv.tensor == tid), None)
            t = plan.tensors[tid]
            vals[tid] = (cap["owned_vals"][L] if L is not None else ctx.debug_read_tensor(tid, n, (t.H, t.W, t.C)))[sel]
        # probabilities: predict() on the same tile pixels (whole-tile launches); the tail inputs it left are compared below
        page = _page(hp, wp)
        x = np.stack([page[rr.origin(geom.ay, j):rr.origin(geom.ay, j) + 224, rr.origin(geom.ax, i):rr.origin(geom.ax, i) + 224]
                      for i, j in (rr.grid_ij(geom, g) for g in sel)])
        probs = net.predict((x / 255.0).astype(np.float32))
        tail = chain[0].steps[0]
        after_predict = {tid: ctx.debug_read_tensor(tid, len(sel), (plan.tensors[tid].H, plan.tensors[tid].W, plan.tensors[tid].C))
                         for tid in (tail.src0, tail.img)}
    finally:
        ctx.set_conv_variant(0)
    bad = []
    for L in range(len(chain) - 1, 0, -1):
        need = np.stack([rr.needed_mask(geom, g, L) for g in sel])
        for s in chain[L].steps:
            rep = sc.check_step(plan, s, vals, precision, mask={"out": sc.placed(need, s)})
            print(f"[region step {precision} variant {variant}] level {L} {s.name}: worst err/bound {rep['worst']:.4f} at {rep['index']} over {rep['n_over']} "
                  f"nan {rep['n_nan']} refbad {rep['n_ref_bad']} elements {rep['n_elem']} |ref|max {rep['ref_absmax']:.4g}")
            assert rep["n_elem"] == int(sc.placed(need, s).sum()) * s.cout or rep["n_nan"] or rep["n_ref_bad"]
            if sc.failed(rep):
                bad.append((L, s.name, {k: rep[k] for k in ("worst", "index", "n_over", "n_nan", "n_inf", "n_ref_bad", "ref_absmax")}))
    assert not bad, bad
    for tid, again in after_predict.items():                                # predict()'s probabilities stand for the owned run's only on the same inputs
        m = np.stack([rr.needed_mask(geom, g, 1) for g in sel]) if tid == tail.src0 else np.ones(again.shape[:3], bool)
        assert np.array_equal(again.view(np.uint32)[m], vals[tid].view(np.uint32)[m]), ("predict() left other tail inputs on the needed box", tid)
    need0 = np.stack([rr.needed_mask(geom, g, 0) for g in sel])
    rep = sc.check_step(plan, tail, vals, precision, probs=probs, mask={"logits": need0})
    print(f"[region step {precision} variant {variant}] level 0 {tail.name}: refbad {rep['n_ref_bad']} nan {rep['n_nan']} p_err {rep['p_err']:.3e} "
          f"label_bad {rep['label_bad']} / {rep['n_decided']} decided")
    if sc.failed(rep):
        bad.append((0, tail.name, {k: rep[k] for k in ("n_nan", "n_ref_bad", "label_bad", "ref_absmax")}))
    # the labels of the owned-region run itself: what the stitch took from each tile, as one-hot "probabilities" through the same rule
    onehot = np.zeros_like(probs)
    for k, g in enumerate(sel):
        i, j = rr.grid_ij(geom, g)
        ylo, yhi, xlo, xhi = rr.needed_box(geom, g, 0)
        y0, x0 = rr.origin(geom.ay, j), rr.origin(geom.ax, i)
        lab = cap["labels_nan"][y0 + ylo:y0 + yhi, x0 + xlo:x0 + xhi]
        np.put_along_axis(onehot[k, ylo:yhi, xlo:xhi], lab[..., None].astype(np.int64), 1.0, axis=-1)
    rep1 = sc.check_step(plan, tail, vals, precision, probs=onehot, mask={"logits": need0})
    print(f"[region step {precision} variant {variant}] level 0 labels of the owned run: label_bad {rep1['label_bad']} / {rep1['n_decided']} decided; "
          f"float64 part {time.time() - t0:.2f} s")
    assert not bad, bad
    assert rep["n_ref_bad"] == 0 and rep["n_decided"] > 0 and rep["label_bad"] == 0
    assert rep1["n_decided"] == rep["n_decided"] and rep1["label_bad"] == 0
    assert rep["p_err"] < TOL_STEP_HEAD_PROB[precision], rep["p_err"]
