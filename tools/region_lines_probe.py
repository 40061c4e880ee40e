#!/usr/bin/env python3
"""Time the deskewed text-line masks of one synthetic page (the page of ``tools/region_slopes_probe.py``) next to the slopes step, in
one process:

  (i)   ``stages.get_slopes`` alone (statistic on the device);
  (ii)  ``stages.get_slopes_and_line_masks``: the same, then the masks and projections of every box with the slopes found, the
        textline map staged once, masks copied back;
  (iii) the same with ``masks=False``: only the row and column sums come back.

Also the number of kernels one line-mask call queues for 1 box and for all boxes (they must be equal).  Median of ``--repeats`` runs
after ``--warmup`` runs; every run sits under its own alarm (``--step-timeout`` seconds).  Prints one JSON line; ``--write FILE.md``
also writes the rows as a Markdown table.  Not part of bench.py.

    python tools/region_lines_probe.py [--boxes 28] [--repeats 7] [--write profiles/region_lines.md]"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.region_slopes_probe import synthetic_textline_page  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=3600)
    ap.add_argument("--width", type=int, default=2600)
    ap.add_argument("--boxes", type=int, default=28)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--write", default=None)
    args = ap.parse_args()

    from sbb_textline_detection_amd import _capi, stages
    from sbb_textline_detection_amd.model import SegModel
    from tools.synth_model import calibrated_model
    cfg, wts = calibrated_model(2, 224, 224, seed=0)
    model = SegModel(cfg, wts, device=0, max_batch=4)            # any finalized handle: these calls do not touch the network
    ctx = model.ctx
    textlines, boxes = synthetic_textline_page(args.height, args.width, args.boxes, args.seed)

    def on_alarm(_sig, _frame):
        raise TimeoutError("step timed out")
    signal.signal(signal.SIGALRM, on_alarm)

    def measure(fn):
        total, result = [], None
        for k in range(args.warmup + args.repeats):
            signal.alarm(args.step_timeout)
            try:
                t0 = time.perf_counter()
                result = fn()
                dt = time.perf_counter() - t0
            finally:
                signal.alarm(0)
            if k >= args.warmup:
                total.append(dt * 1e3)
        return {"total_ms": round(statistics.median(total), 2), "min_ms": round(min(total), 2), "max_ms": round(max(total), 2)}, result
    row_slopes, slopes = measure(lambda: stages.get_slopes(textlines, boxes, ctx))
    row_both, both = measure(lambda: stages.get_slopes_and_line_masks(textlines, boxes, ctx))
    row_sums, sums = measure(lambda: stages.get_slopes_and_line_masks(textlines, boxes, ctx, masks=False))
    row_lines, lines = measure(lambda: stages.get_line_masks(textlines, boxes, slopes, ctx))
    launches = []
    for some in (boxes[:1], boxes):
        before = ctx.line_mask_launches()
        stages.get_line_masks(textlines, some, slopes[:len(some)], ctx, masks=False)
        launches.append(ctx.line_mask_launches() - before)
    # the smallest box on the host twin: the A/B path says the same
    r = min(range(len(boxes)), key=lambda k: boxes[k][2] * boxes[k][3])
    x, y, w, h = boxes[r]
    host = _capi.host_region_line_mask(textlines[y:y + h, x:x + w], slopes[r])
    same = (both[0] == slopes == sums[0] and all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) for a, b in zip(both[1], lines))
            and all(b[0] is None and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) for a, b in zip(both[1], sums[1]))
            and all(np.array_equal(a, b) for a, b in zip(lines[r], host)))
    model.release()
    res = {"probe": "region_lines", "page": [args.height, args.width], "boxes": len(boxes), "repeats": args.repeats, "warmup": args.warmup,
           "crop_pixels": int(sum(b[2] * b[3] for b in boxes)), "non_empty_masks": sum(1 for a in lines if a[0].any()),
           "vertical_boxes": sum(1 for s in slopes if abs(s) > 45), "consistent": bool(same),
           "get_slopes": row_slopes, "get_slopes_and_line_masks": row_both, "get_slopes_and_line_masks_no_mask_download": row_sums,
           "get_line_masks": row_lines, "launches_1_box": launches[0], "launches_all_boxes": launches[1]}
    print(json.dumps(res))
    if args.write:
        with open(args.write, "w") as f:
            f.write("# Deskewed text-line masks and line profiles of all text regions of a page\n\n")
            f.write(f"`tools/region_lines_probe.py`: one synthetic textline map of {args.height} x {args.width} with {len(boxes)} boxes "
                    f"({res['crop_pixels']} crop pixels in all), MI355X, median of {args.repeats} runs after {args.warmup} warm-up runs in one "
                    f"process.  {res['non_empty_masks']} masks are non-empty, {res['vertical_boxes']} boxes have |slope| > 45.  The paths agree with "
                    f"each other and with the host twin on the smallest box: {res['consistent']}.\n\n")
            f.write("| call | total ms | min .. max ms |\n|---|---|---|\n")
            for label, row in (("`get_slopes` alone", row_slopes), ("`get_slopes_and_line_masks` (masks copied back)", row_both),
                               ("`get_slopes_and_line_masks(masks=False)` (projections only)", row_sums),
                               ("`get_line_masks` alone (its own upload of the plane, masks copied back)", row_lines)):
                f.write(f"| {label} | {row['total_ms']} | {row['min_ms']} .. {row['max_ms']} |\n")
            f.write(f"\nKernels queued by one line-mask call: {launches[0]} for 1 box, {launches[1]} for {len(boxes)} boxes.\n")
    return 0 if same and launches[0] == launches[1] else 1


if __name__ == "__main__":
    sys.exit(main())
