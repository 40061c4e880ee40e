#!/usr/bin/env python3
"""Time the text lines of every box of one synthetic page (the page of ``tools/region_slopes_probe.py``), in one process:

  (i)   the host path, the only one before the device splitter: ``stages.get_line_masks(masks=False)`` (row and column sums copied
        back), then scipy's ``gaussian_filter1d`` / ``find_peaks`` and numpy per box (``tests/line_split_ref.py``);
  (ii)  ``stages.get_line_boxes``: the same masks, then the splitter on the device, the sums never leaving it.

Also the number of kernels one ``get_line_boxes`` call queues for 1 box and for all boxes (they must be equal).  Median of ``--repeats``
runs after ``--warmup`` runs; every run sits under its own alarm (``--step-timeout`` seconds).  Prints one JSON line; ``--write FILE.md``
also writes the rows as a Markdown table.  Not part of bench.py.

    python tools/region_line_split_probe.py [--boxes 28] [--repeats 11] [--write profiles/region_line_split.md]"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

from tools.region_slopes_probe import synthetic_textline_page  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=3600)
    ap.add_argument("--width", type=int, default=2600)
    ap.add_argument("--boxes", type=int, default=28)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--write", default=None)
    args = ap.parse_args()

    import line_split_ref as lr
    from sbb_textline_detection_amd import _capi, stages
    from sbb_textline_detection_amd.model import SegModel
    from tools.synth_model import calibrated_model
    cfg, wts = calibrated_model(2, 224, 224, seed=0)
    model = SegModel(cfg, wts, device=0, max_batch=4)            # any finalized handle: these calls do not touch the network
    ctx = model.ctx
    textlines, boxes = synthetic_textline_page(args.height, args.width, args.boxes, args.seed)
    slopes = stages.get_slopes(textlines, boxes, ctx)

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

    def host_path():
        out = []
        for box, slope, (_m, rows, cols) in zip(boxes, slopes, stages.get_line_masks(textlines, boxes, slopes, ctx, masks=False)):
            vertical = abs(slope) > 45
            out.append(lr.line_split(cols if vertical else rows, box[3] if vertical else box[2], vertical, _capi.line_rotation_terms(box[2], box[3], slope)))
        return out
    row_host, host = measure(host_path)
    row_dev, dev = measure(lambda: stages.get_line_boxes(textlines, boxes, slopes, ctx))
    launches = []
    for some in (boxes[:1], boxes):
        before = ctx.line_mask_launches()
        stages.get_line_boxes(textlines, some, slopes[:len(some)], ctx)
        launches.append(ctx.line_mask_launches() - before)
    same = len(host) == len(dev) and all(lr.same(a, b) for a, b in zip(dev, host))
    model.release()
    res = {"probe": "region_line_split", "page": [args.height, args.width], "boxes": len(boxes), "repeats": args.repeats, "warmup": args.warmup,
           "lines": int(sum(len(r["peaks"]) for r in dev)), "regions_without_lines": sum(1 for r in dev if r["status"] != 0),
           "vertical_boxes": sum(1 for s in slopes if abs(s) > 45), "max_sigma": max(r["sigma"] for r in dev), "consistent": bool(same),
           "host_path": row_host, "get_line_boxes": row_dev, "launches_1_box": launches[0], "launches_all_boxes": launches[1]}
    print(json.dumps(res))
    if args.write:
        with open(args.write, "w") as f:
            f.write("# Text-line peaks and line boxes of all text regions of a page\n\n")
            f.write(f"`tools/region_line_split_probe.py`: one synthetic textline map of {args.height} x {args.width} with {len(boxes)} boxes, MI355X, "
                    f"median of {args.repeats} runs after {args.warmup} warm-up runs in one process.  {res['lines']} lines in all, "
                    f"{res['regions_without_lines']} regions without lines, {res['vertical_boxes']} boxes with |slope| > 45, largest sigma_gaus "
                    f"{res['max_sigma']}.  Both paths give the same records: {res['consistent']}.\n\n")
            f.write("| call | total ms | min .. max ms |\n|---|---|---|\n")
            for label, row in (("`get_line_masks(masks=False)`, then scipy / numpy per box on the host", row_host),
                               ("`get_line_boxes` (masks and splitter on the device)", row_dev)):
                f.write(f"| {label} | {row['total_ms']} | {row['min_ms']} .. {row['max_ms']} |\n")
            f.write(f"\nKernels queued by one `get_line_boxes` call: {launches[0]} for 1 box, {launches[1]} for {len(boxes)} boxes.\n")
    return 0 if same and launches[0] == launches[1] else 1


if __name__ == "__main__":
    sys.exit(main())
