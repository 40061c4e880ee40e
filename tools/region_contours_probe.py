#!/usr/bin/env python3
"""Time the text-region contours of one synthetic layout plane, in one process:

  (a) ``text_region_boxes_dev`` alone -- what the library did before it traced contours;
  (b) ``text_region_contours_dev`` (the device tracer, which reads the tables back through ``sbbseg_text_region_contours_read``);
  (c) the host route on the same build: the boxes call, a download of the plane, then ``mask_contours_host`` on it.  The plane is built
      from blocks of rows at least 26 high and 40 wide, which OPEN and CLOSE leave as they are, so the host traces the plane itself;
      the probe fails if (b) and (c) disagree.

The page is the 28-box 3600 x 2600 page of tools/region_slopes_probe.py with every box turned into a paragraph with a ragged right
edge (one step per text line).  Also reported: the tracer and packing kernels queued for 1 box and for all of them, and the longest
contour.  Median of ``--repeats`` runs after ``--warmup`` runs; every run sits under its own alarm.  Prints one JSON line; ``--write
FILE.md`` also writes a Markdown table.  Not part of bench.py.

    python tools/region_contours_probe.py [--boxes 28] [--repeats 7] [--write profiles/region_contours.md]"""
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


def ragged_regions(h, w, boxes, seed):
    """A 0 / 1 layout plane: every box a paragraph whose lines (26 .. 43 rows each) end at their own column."""
    rng = np.random.RandomState(seed)
    r = np.zeros((h, w), np.uint8)
    for x, y, bw, bh in boxes:
        yy = y
        while yy < y + bh:
            step = min(int(rng.randint(26, 44)), y + bh - yy)
            if y + bh - (yy + step) < 26:
                step = y + bh - yy
            r[yy:yy + step, x:x + int(rng.randint(max(40, bw // 2), bw + 1))] = 1
            yy += step
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=3600)
    ap.add_argument("--width", type=int, default=2600)
    ap.add_argument("--boxes", type=int, default=28)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=60)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--write", default=None)
    args = ap.parse_args()

    from sbb_textline_detection_amd import _capi
    from sbb_textline_detection_amd.model import SegModel
    from tools.region_slopes_probe import synthetic_textline_page
    from tools.synth_model import calibrated_model
    cfg, wts = calibrated_model(2, 224, 224, seed=0)
    model = SegModel(cfg, wts, device=0, max_batch=4)            # any finalized handle: these calls do not touch the network
    ctx = model.ctx
    _, boxes = synthetic_textline_page(args.height, args.width, args.boxes, args.seed)
    regions = ragged_regions(args.height, args.width, boxes, args.seed)
    H, W = regions.shape
    d_plane = ctx.device_alloc(regions.nbytes)
    ctx.upload(d_plane, regions)

    def boxes_only():
        return ctx.text_region_boxes_dev(d_plane, H, W, 1, 0.00001, 1.0)

    def device_route():
        return ctx.text_region_contours_dev(d_plane, H, W, 1, 0.00001, 1.0)

    def host_route():
        found = ctx.text_region_boxes_dev(d_plane, H, W, 1, 0.00001, 1.0)
        return found, _capi.mask_contours_host(ctx.download(d_plane, (H, W)))[1]

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
        return {"total_ms": round(statistics.median(total), 3), "min_ms": round(min(total), 3), "max_ms": round(max(total), 3)}, result
    row_boxes, got_boxes = measure(boxes_only)
    row_device, (dev_boxes, dev_contours) = measure(device_route)
    row_host, (host_boxes, host_contours) = measure(host_route)
    same = (got_boxes == dev_boxes == host_boxes and len(dev_contours) == len(host_contours)
            and all(np.array_equal(a, b) for a, b in zip(dev_contours, host_contours)))
    before = ctx.contour_launches()
    device_route()
    launches_all = ctx.contour_launches() - before
    one = np.zeros_like(regions)
    x, y, bw, bh = boxes[0]
    one[y:y + bh, x:x + bw] = regions[y:y + bh, x:x + bw]
    ctx.upload(d_plane, one)
    before = ctx.contour_launches()
    one_boxes, _ = device_route()
    launches_one = ctx.contour_launches() - before
    ctx.device_free(d_plane)
    model.release()
    res = {"probe": "region_contours", "page": [H, W], "boxes": len(dev_boxes), "repeats": args.repeats, "same_contours": bool(same),
           "points": int(sum(len(c) for c in dev_contours)), "longest_contour_points": int(max(len(c) for c in dev_contours)),
           "largest_box": max(dev_boxes, key=lambda b: b[2] * b[3])[2:], "boxes_only": row_boxes, "device_contours_and_read": row_device,
           "host_route": row_host, "contour_kernels_queued": {"1_box": launches_one, "%d_boxes" % len(dev_boxes): launches_all},
           "boxes_in_one_box_plane": len(one_boxes), "plane_download_bytes": int(regions.nbytes)}
    print(json.dumps(res))
    if args.write:
        with open(args.write, "w") as f:
            f.write("# Text-region contours of a page: boxes alone, traced on the device, traced on the host\n\n")
            f.write(f"`tools/region_contours_probe.py`: one synthetic layout plane of {H} x {W} with {res['boxes']} ragged paragraphs (largest box "
                    f"{res['largest_box'][0]} x {res['largest_box'][1]}; {res['points']} contour points in all, the longest contour "
                    f"{res['longest_contour_points']}), MI355X, median of {args.repeats} runs after {args.warmup} warm-up runs in one process.  "
                    f"The device and the host route return the same boxes and contours: {res['same_contours']}.\n\n")
            f.write("| path | total ms | min .. max ms |\n|---|---|---|\n")
            for label, r in (("(a) `text_region_boxes_dev` alone", row_boxes),
                             ("(b) `text_region_contours_dev` + `sbbseg_text_region_contours_read`", row_device),
                             (f"(c) host route: the boxes call, a download of the plane ({regions.nbytes} bytes), `mask_contours_host`", row_host)):
                f.write(f"| {label} | {r['total_ms']} | {r['min_ms']} .. {r['max_ms']} |\n")
            f.write(f"\nTracer and packing kernels queued by one contours call: {launches_one} for 1 box, {launches_all} for {res['boxes']} "
                    "(a counting launch, the packing launch, a writing launch; one more of each tracer launch when a box is beyond the LDS "
                    "limit).\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
