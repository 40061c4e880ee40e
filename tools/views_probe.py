#!/usr/bin/env python3
"""Time the crops of 16 differently sized pages through a 448 x 448 f16x3 model, three ways, alternating in one process:

  (a) 16 ``segment_crop_dev`` calls, one view each -- what the product's two patch stages do today;
  (b) one ``segment_views_dev`` call over the same 16 views -- their tiles pooled into shared launches;
  (c) ``segment_pages_dev`` on 16 equal 3500 x 2500 pages -- the pooled rate of the benchmark's input, for scale.

The stored pages differ by a few pixels (scans of one document), each is upscaled by the ``scaled_size`` rule, and every view is a crop of
about 3300-3500 x 2300-2500 of the upscaled page with its own size and offset (fixed seed); every other view is binarised.  Each
measurement ends with a stream synchronise; median and min-max of ``--repeats`` rounds after ``--warmup`` rounds.  The one condition: the
median of (b) is not above the median of (a) by more than the spread (max - min) of (a) in the same run; the exit status says so.
Prints one JSON line; ``--write FILE.md`` also writes the table.  Not part of bench.py.

    python tools/views_probe.py [--views 16] [--repeats 7] [--write profiles/mixed_views.md]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-batch", type=int, default=70)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--write", default=None)
    a = ap.parse_args()
    import torch
    from sbb_textline_detection_amd import _capi
    from sbb_textline_detection_amd.model import SegModel
    from sbb_textline_detection_amd.stages import scaled_size
    from sbb_textline_detection_amd.synthetic import synthetic_page
    from tools.synth_model import calibrated_model
    model = SegModel(*calibrated_model(2, 448, 448, seed=0), device=0, max_batch=a.max_batch, precision="f16x3")
    ctx = model.ctx
    rng = np.random.RandomState(a.seed)
    base = synthetic_page(3500, 2500, seed=33)
    views, keep, sizes = [], [], set()
    while len(views) < a.views:
        hs, ws = 3500 - int(rng.randint(0, 9)), 2500 - int(rng.randint(0, 9))
        hp, wp = scaled_size(hs, ws)
        ch, cw = int(rng.randint(3300, 3501)), int(rng.randint(2300, 2501))
        if (ch, cw) in sizes:
            continue
        sizes.add((ch, cw))
        box = (int(rng.randint(0, wp - cw + 1)), int(rng.randint(0, hp - ch + 1)), cw, ch)
        page = torch.from_numpy(np.ascontiguousarray(np.roll(base, 37 * len(views), axis=0)[:hs, :ws])).cuda()
        out = torch.zeros((ch, cw), dtype=torch.uint8, device="cuda")
        thr = torch.zeros((1,), dtype=torch.int32, device="cuda")
        keep.append((page, out, thr))
        views.append((page.data_ptr(), hs, ws, hp, wp, box, len(views) % 2 == 0, out.data_ptr(), thr.data_ptr()))
    equal = [torch.from_numpy(np.ascontiguousarray(np.roll(base, 37 * k, axis=0))).cuda() for k in range(a.views)]
    equal_out = [torch.zeros((3500, 2500), dtype=torch.uint8, device="cuda") for _ in equal]

    def tiles(h, w):
        xy, _, _ = _capi.tile_grid(h, w, 448, 448)
        return len(set(xy[:, 0].tolist())) * len(set(xy[:, 1].tolist()))       # (the dedupe rule is on)
    n_tiles = {"a": sum(tiles(v[5][3], v[5][2]) for v in views), "c": a.views * tiles(3500, 2500)}
    n_tiles["b"] = n_tiles["a"]

    def one_by_one():
        for v in views:
            ctx.segment_crop_dev(*v)

    def pooled():
        ctx.segment_views_dev(views)

    def equal_pages():
        ctx.segment_pages_dev([t.data_ptr() for t in equal], 3500, 2500, [t.data_ptr() for t in equal_out])
    paths = {"a": one_by_one, "b": pooled, "c": equal_pages}
    ms = {k: [] for k in paths}
    first = {}
    for rnd in range(a.warmup + a.repeats):
        for k, fn in paths.items():                        # alternating: a, b, c, a, b, c, ...
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            if rnd >= a.warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
            if k in ("a", "b") and rnd == 0:
                first[k] = [(o.cpu().numpy().copy(), int(t.item())) for _, o, t in keep]
    same = all(np.array_equal(x[0], y[0]) and x[1] == y[1] for x, y in zip(first["a"], first["b"]))
    med = {k: statistics.median(v) for k, v in ms.items()}
    lo, hi = {k: min(v) for k, v in ms.items()}, {k: max(v) for k, v in ms.items()}
    spread_a = hi["a"] - lo["a"]
    met = med["b"] <= med["a"] + spread_a
    per_tile = {k: med[k] / n_tiles[k] for k in med}
    res = {"views": a.views, "repeats": a.repeats, "max_batch": a.max_batch, "tiles": n_tiles, "median_ms": med, "min_ms": lo, "max_ms": hi,
           "spread_a_ms": spread_a, "b_minus_a_ms": med["b"] - med["a"], "condition_met": bool(met), "b_over_a": med["b"] / med["a"],
           "b_over_c_per_tile": per_tile["b"] / per_tile["c"], "planes_equal": bool(same)}
    print(json.dumps(res))
    if a.write:
        names = {"a": "%d `segment_crop_dev` calls" % a.views, "b": "one `segment_views_dev` call", "c": "`segment_pages_dev`, %d equal 3500 x 2500 pages" % a.views}
        with open(a.write, "w") as f:
            f.write("# Mixed views: one pooled call against one call per view\n\n")
            f.write("`tools/views_probe.py` on one MI355X: %d views of a 448 x 448 f16x3 model (max_batch %d), crops of pairwise different size "
                    "(3300-3500 x 2300-2500, seed %d) of pages that differ by a few pixels and are upscaled x1.2; every other view binarised.  "
                    "The three paths alternate in one process, every measurement ends with a stream synchronise; median and min-max of %d "
                    "rounds after %d warm-up rounds.\n\n" % (a.views, a.max_batch, a.seed, a.repeats, a.warmup))
            f.write("| path | tiles | median ms | min - max ms | us per tile |\n|---|---|---|---|---|\n")
            for k in ("a", "b", "c"):
                f.write("| (%s) %s | %d | %.2f | %.2f - %.2f | %.1f |\n" % (k, names[k], n_tiles[k], med[k], lo[k], hi[k], 1e3 * per_tile[k]))
            f.write("\n* Condition: median (b) <= median (a) + spread of (a).  (b) - (a) = %+.2f ms beside a spread of (a) of %.2f ms: %s.\n"
                    % (med["b"] - med["a"], spread_a, "met" if met else "NOT met"))
            f.write("* (b) / (a) = %.3f.\n" % (med["b"] / med["a"]))
            f.write("* (b) / (c) per tile = %.3f (reported, not gated).\n" % (per_tile["b"] / per_tile["c"]))
            f.write("* Label planes and thresholds of (a) and (b) equal byte for byte: %s.\n" % ("yes" if same else "NO"))
    model.release()
    return 0 if met and same else 1


if __name__ == "__main__":
    sys.exit(main())
