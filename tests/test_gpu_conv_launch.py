"""-m gpu: the launch records of the generic conv (conv_igemm_mfma, its split-K form) under the tile-family knobs, held to a recording.

csrc/conv_choice.h states once which tile form, gather, walk and table a launch of conv_igemm_mfma takes, and launch_conv (csrc/kernels.hip)
maps the chosen form to a template instantiation.  A wrong tile computes right answers, so only the records (``op_launch``: filled by the host
where each launch is sized) can catch a mis-mapped switch.  tests/golden/conv_launch_golden.json holds the records of the commit before that
header existed (9dd1a7e: the ladders of launch_conv_16 / launch_conv_x3 / launch_conv_t and launch_generic_conv's own conditions), written by
this module's recorder -- ``python tests/test_gpu_conv_launch.py`` on a checkout of that commit; it uses nothing that commit's Context lacks.

The shapes are the smallest at which the dispatch can still go wrong, all on the 224 x 256 four-class ResNet plan that
tests/test_gpu_steps_at_scale.py builds, one handle per precision (f16, f16x3):

  * n = 2, records only, for the forced forms (they do not look at tile counts): variants 1, 2, 3, bit 4 (half-K-step stages), bit 16 with
    variant 3 (the 8-phase 256 x 256 tile), bit 17 (plain gather);
  * n = 587 for variant 0, bit 4 and bit 16: the auto rules and the 256 x 256 half-stage and 8-phase tiles need 200 tiles of 256 x 256
    (test_gpu_steps_at_scale.py derives 587);
  * one whole-image forward (one patch, split-K), with the split count of every conv_splitk op;
  * one owned-region chunk -- the smallest page of tests/test_gpu_region_steps.py, 404 x 405, one lane -- at variants 0 and 1 and at bit 4:
    the table column, and the executed share of every op (bit 4 withholds the pixel table: the level runs whole and counts as whole).

Compared per op: family, BP, BC, stages, fast gather, tile map, class-minor, table, n_tiles, grid, residual, res_epilogue, the split count of
a split-K launch and, in the owned-region cases, exec_patches."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

if __name__ == "__main__":                # the recorder: tests/ is on the path already, the repository root is not
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_launch_golden.json")
H, W, CLASSES, N_BIG, K = 224, 256, 4, 587, 5
PRECISIONS = ("f16", "f16x3")
FIELDS = ("family", "BP", "BC", "stages", "fast_gather", "tile_map", "cls_minor", "table", "n_tiles", "grid", "residual", "res_epilogue")
BIT4, BIT16, BIT17 = 1 << 4, 1 << 16, 1 << 17
REGION_PAGE = (404, 405)
# (kind, conv variant)
CASES = ([("n2", v) for v in (1, 2, 3, BIT4, BIT16 | 3, BIT17)] + [("big", v) for v in (0, BIT4, BIT16)] + [("whole", 0)]
         + [("region", v) for v in (0, 1, BIT4)])


def case_id(kind, variant):
    return f"{kind}-variant{variant:#x}"


_NETS = {}


def net(precision):
    if precision not in _NETS:
        from gpu_common import make_model
        _, _, _, model = make_model(CLASSES, H, W, seed=12, precision=precision, max_batch=N_BIG, calib_hw=160)
        model.ctx.set_lanes(1)
        _NETS[precision] = model
    return _NETS[precision]


def release_nets():
    for model in _NETS.values():
        model.release()
    _NETS.clear()


@pytest.fixture(scope="module", autouse=True)
def _release_nets():
    yield
    release_nets()


def run_case(model, kind, variant):
    """One forward of the case -> [[op name, the FIELDS..., split count or 0, exec_patches or None] per plan op]."""
    from sbb_textline_detection_amd.synthetic import synthetic_page
    from test_gpu_steps_at_scale import cyclic_batch, launch_records
    from test_gpu_steps_whole import page_for, split_counts
    ctx = model.ctx
    ops = ctx.ops()
    executed = None
    ctx.set_conv_variant(variant)
    try:
        if kind in ("n2", "big"):
            n = 2 if kind == "n2" else N_BIG
            model.predict(cyclic_batch(H, W, n, min(n, K)))
        elif kind == "whole":
            ctx.segment_whole(page_for(H, W), H, W)
        else:
            hp, wp = REGION_PAGE
            ctx.set_owned_regions(1)
            ctx.profile_reset()
            ctx.segment_page(synthetic_page(hp, wp, seed=hp * 7 + wp))
            executed = [float(o["exec_patches"]) for o in ctx.profile()]
        recs = launch_records(ctx, ops)
    finally:
        ctx.set_conv_variant(0)
    if kind == "whole":
        recs, _ = split_counts(model.plan, ops, recs)
    return [[r["name"]] + [r[f] for f in FIELDS] + [r.get("splits", 0), executed[i] if executed else None] for i, r in enumerate(recs)]


def check_coverage(precision, kind, variant, rows):
    """What each case is there for must have been launched (asserted when recording and when comparing)."""
    col = {f: i + 1 for i, f in enumerate(FIELDS)}
    conv = [r for r in rows if r[col["family"]] == "conv_igemm"]
    tiles = {(r[col["BP"]], r[col["BC"]], r[col["stages"]]) for r in conv}
    if kind == "whole":
        assert any(r[col["family"]] == "conv_splitk" and r[-2] >= 2 for r in rows), "no split-K launch"
    if kind == "region":
        tabled = [r for r in conv if r[col["table"]]]
        assert bool(tabled) == (variant != BIT4), (variant, [r[0] for r in tabled])
        n = max(r[-1] for r in rows)
        assert all(r[-1] < n for r in tabled)                    # a table walks less than the whole grid
        if variant == BIT4:                                      # withheld: the decoder convs on the generic kernel run whole and count as whole
            assert all(r[-1] == n for r in conv), [(r[0], r[-1]) for r in conv if r[-1] != n]
    plain = precision != "f16x3"                                 # (the split mode has neither half-stage, 3-stage nor forced 8-wave tiles)
    if kind == "big" and variant == BIT4 and plain:
        assert (256, 256, 4) in tiles and (128, 128, 4) in tiles, sorted(tiles)
    if kind == "big" and variant in (0, BIT16):
        assert (256, 256, 2) in tiles, sorted(tiles)
    if kind == "n2" and variant == 2 and plain:
        assert {t for t in tiles if t[2] == 3}, sorted(tiles)
    if kind == "n2" and (variant & 3) == 3 and plain:
        assert (256, 256, 2) in tiles and (512, 128, 2) in tiles, sorted(tiles)
    if kind == "n2" and variant == BIT17:
        assert conv and all(r[col["fast_gather"]] == 0 for r in conv)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert tuple(g["fields"]) == FIELDS + ("splits", "exec_patches") and g["shape"] == [H, W, CLASSES, N_BIG]
    return g["records"]


@pytest.mark.parametrize("kind,variant", CASES, ids=[case_id(*c) for c in CASES])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_launch_records_are_the_recorded_ones(precision, kind, variant, golden):
    want = golden[precision][case_id(kind, variant)]
    got = run_case(net(precision), kind, variant)
    check_coverage(precision, kind, variant, got)
    assert [r[0] for r in got] == [r[0] for r in want]
    names = ("op",) + FIELDS + ("splits", "exec_patches")
    bad = [(g[0], {names[i]: (g[i], w[i]) for i in range(1, len(names)) if g[i] != w[i]}) for g, w in zip(got, want) if g != w]
    assert not bad, f"(got, recorded) per differing field: {bad[:8]} ({len(bad)} ops)"


def record():
    out = {"fields": list(FIELDS) + ["splits", "exec_patches"], "shape": [H, W, CLASSES, N_BIG], "records": {}}
    for precision in PRECISIONS:
        out["records"][precision] = {}
        for kind, variant in CASES:
            rows = run_case(net(precision), kind, variant)
            try:
                check_coverage(precision, kind, variant, rows)
            except AssertionError as e:                          # (recorded all the same: the message says what the case failed to launch)
                print(f"[record {precision} {case_id(kind, variant)}] COVERAGE: {e!r}")
            out["records"][precision][case_id(kind, variant)] = rows
            print(f"[record {precision} {case_id(kind, variant)}] {sum(1 for r in rows if r[1] != 'none')} launches")
    release_nets()
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    record()
