#!/usr/bin/env python3
"""Time the model-running part of run() for 16 stored pages of pairwise different size through the three 448 x 448 models, three ways,
alternating in one process, host arrays in and host arrays out:

  (a) ``InferenceStages.run_pages(images)`` -- the default: layout and textline stages pooled, border stage and glue page by page;
  (b) ``InferenceStages.run_pages(images, resident=True)`` -- one ``sbbseg_run_pages`` call: pages uploaded once, border forwards at
      batch width, region maps resident between model, cleaning and gate;
  (c) ``[run(img) for img in images]`` -- one ``sbbseg_run_page`` call per page.

Beside them the border stage alone, on pages already on the device: 16 ``extract_page_box_dev`` calls against one
``extract_page_boxes_dev`` call.  Every measurement ends with a synchronise of the three handles; median and min-max of ``--repeats``
rounds after ``--warmup`` rounds.  The one condition: the median of (b) is not above the median of (a) by more than the spread
(max - min) of (a) in the same run; the exit status says so.  Byte equality of (b) and (c) is checked once with split-K off on the border
handle (from two pages on the batched border forward never splits).  Prints one JSON line; ``--write FILE.md`` also writes the table.
Not part of bench.py.

    python tools/run_pages_probe.py [--pages 16] [--repeats 7] [--only a|b] [--write profiles/run_pages.md]"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def same(x, y):
    return (x is None and y is None) or (x is not None and y is not None and np.array_equal(x, y))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None, choices=["a", "b"], help="run one path alone (for a kernel trace); nothing is compared")
    ap.add_argument("--write", default=None)
    a = ap.parse_args()
    import torch
    from sbb_textline_detection_amd import clear_session, stages
    from sbb_textline_detection_amd.model import load_model
    from sbb_textline_detection_amd.synthetic import synthetic_page
    from sbb_textline_detection_amd.weights import save_sbbw
    from tools.synth_model import calibrated_model
    specs = {"model_page_mixed_best": 2, "model_strukturerkennung": 4, "model_textline_new": 2}      # main.py:58-60
    tmp = tempfile.mkdtemp(prefix="run_pages_probe_")
    for name, classes in specs.items():
        cfg, w = calibrated_model(classes, 448, 448, seed=classes)
        save_sbbw(os.path.join(tmp, name + ".sbbw"), cfg, w)
    paths = [os.path.join(tmp, n + ".h5") for n in specs]
    st = stages.InferenceStages(*paths)
    border, layout, textline = (load_model(p).ctx for p in paths)
    base = synthetic_page(2900, 2080, seed=33)
    images = [np.ascontiguousarray(np.roll(base, 37 * k, axis=0)[:2900 - k, :2080 - (5 * k) % 16]) for k in range(a.pages)]
    assert len({img.shape for img in images}) == len(images)
    scaled = [stages.scaled_size(*img.shape[:2]) for img in images]

    def sync():
        for c in (border, layout, textline):
            c.synchronize()

    fns = {"a": lambda: st.run_pages(images), "b": lambda: st.run_pages(images, resident=True), "c": lambda: [st.run(img) for img in images]}
    if a.only:
        for _ in range(a.warmup + 1):
            fns[a.only]()
            sync()
        clear_session()
        shutil.rmtree(tmp, ignore_errors=True)
        return 0
    # byte equality of (b) and (c), split-K off on the border handle
    border.set_ksplit(False)
    try:
        rb, rc = fns["b"](), fns["c"]()
    finally:
        border.set_ksplit(True)
    equal = len(rb) == len(rc) and all(x[3] == y[3] and all(same(p, q) for p, q in zip(x[:3], y[:3])) for x, y in zip(rb, rc))
    reached = sum(1 for x in rb if x[2] is not None)
    del rb, rc
    # the border stage alone, pages on the device
    d_pages = [torch.from_numpy(img).cuda() for img in images]
    views = [(t.data_ptr(), img.shape[0], img.shape[1], hs, ws, hs, ws, 0) for t, img, (hs, ws) in zip(d_pages, images, scaled)]

    def border_one_by_one():
        return [border.extract_page_box_dev(v[0], v[1], v[2], v[3], v[4]) for v in views]

    def border_batched():
        return border.extract_page_boxes_dev(views)
    fns.update({"border_1": border_one_by_one, "border_n": border_batched})
    ms = {k: [] for k in fns}
    for rnd in range(a.warmup + a.repeats):
        for k, fn in fns.items():                          # alternating: a, b, c, border_1, border_n, a, ...
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            if rnd >= a.warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    lo, hi = {k: min(v) for k, v in ms.items()}, {k: max(v) for k, v in ms.items()}
    spread_a = hi["a"] - lo["a"]
    met = med["b"] <= med["a"] + spread_a
    res = {"pages": a.pages, "repeats": a.repeats, "median_ms": med, "min_ms": lo, "max_ms": hi, "spread_a_ms": spread_a,
           "b_minus_a_ms": med["b"] - med["a"], "condition_met": bool(met), "b_over_a": med["b"] / med["a"], "b_over_c": med["b"] / med["c"],
           "border_n_over_1": med["border_n"] / med["border_1"], "b_equals_c": bool(equal), "pages_with_textlines": reached}
    print(json.dumps(res))
    if a.write:
        names = {"a": "`run_pages(images)`", "b": "`run_pages(images, resident=True)`", "c": "`[run(img) for img in images]`",
                 "border_1": "border stage: %d `extract_page_box_dev` calls" % a.pages, "border_n": "border stage: one `extract_page_boxes_dev` call"}
        with open(a.write, "w") as f:
            f.write("# run() for many pages: the resident pooled call against the pooled stages and the page loop\n\n")
            f.write("`tools/run_pages_probe.py` on one MI355X: the three 448 x 448 models (f16x3, max_batch 70), %d stored pages of pairwise "
                    "different size near 2900 x 2080 (upscaled x1.2 to about 3480 x 2496), host arrays in, host arrays out; %d of them reach "
                    "the textline model.  The paths alternate in one process, every measurement ends with a synchronise of the three handles; "
                    "median and min-max of %d rounds after %d warm-up rounds.  The border-stage rows take pages that are already on the "
                    "device and leave the masks there.\n\n" % (a.pages, reached, a.repeats, a.warmup))
            f.write("| path | median ms | min - max ms | ms per page |\n|---|---|---|---|\n")
            for k in ("a", "b", "c", "border_1", "border_n"):
                f.write("| %s%s | %.2f | %.2f - %.2f | %.2f |\n" % ("(%s) " % k if len(k) == 1 else "", names[k], med[k], lo[k], hi[k], med[k] / a.pages))
            f.write("\n* Condition: median (b) <= median (a) + spread of (a).  (b) - (a) = %+.2f ms beside a spread of (a) of %.2f ms: %s.\n"
                    % (med["b"] - med["a"], spread_a, "met" if met else "NOT met"))
            f.write("* (b) / (a) = %.3f.\n* (b) / (c) = %.3f.\n" % (med["b"] / med["a"], med["b"] / med["c"]))
            f.write("* Border stage, batched / page by page = %.3f.\n" % (med["border_n"] / med["border_1"]))
            f.write("* Outputs of (b) and (c) with split-K off on the border handle equal byte for byte: %s.\n" % ("yes" if equal else "NO"))
    clear_session()
    shutil.rmtree(tmp, ignore_errors=True)
    return 0 if met and equal else 1


if __name__ == "__main__":
    sys.exit(main())
