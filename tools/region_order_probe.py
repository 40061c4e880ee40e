#!/usr/bin/env python3
"""Time the reading order of the text regions of ``--pages`` synthetic pages (the 28-box page of ``tools/region_slopes_probe.py``, one
copy per page in device memory, as ``run_pages`` leaves them), in one process:

  (i)   the only route before the device order: download each page's textline plane (H x W bytes), then scipy's ``gaussian_filter1d`` /
        ``find_peaks`` and numpy on the host (``tests/order_ref.py``, the serial Python moment loop included);
  (ii)  ``Context.region_order_dev`` per page on the resident plane, the contours being the resident result of one
        ``text_region_contours_dev`` call on the pages' region map (the boxes, class 1).

Both end in a stream synchronise inside the library call.  Median of ``--repeats`` runs after ``--warmup`` runs, the two routes
alternating; every run sits under its own alarm (``--step-timeout`` seconds).  Also the kernels one order call queues and the bytes route
(i) downloads per page.  Prints one JSON line; ``--write FILE.md`` also writes a Markdown table.  Not part of bench.py.

    python tools/region_order_probe.py [--pages 16] [--repeats 11] [--write profiles/region_order.md]"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

import numpy as np

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
    ap.add_argument("--pages", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--write", default=None)
    args = ap.parse_args()

    import order_ref
    from sbb_textline_detection_amd import stages
    from sbb_textline_detection_amd.model import SegModel
    from tools.synth_model import calibrated_model
    cfg, wts = calibrated_model(2, 224, 224, seed=0)
    model = SegModel(cfg, wts, device=0, max_batch=4)            # any finalized handle: these calls do not touch the network
    ctx = model.ctx
    textlines, boxes = synthetic_textline_page(args.height, args.width, args.boxes, args.seed)
    H, W = textlines.shape
    regions = np.zeros((H, W), np.uint8)
    for x, y, w, h in boxes:
        regions[y:y + h, x:x + w] = 1
    planes = []
    for _ in range(args.pages):
        d = ctx.device_alloc(H * W)
        ctx.upload(d, textlines)
        planes.append(d)
    d_regions = ctx.device_alloc(H * W)
    ctx.upload(d_regions, regions)
    _, contours = ctx.text_region_contours_dev(d_regions, H, W, 1, 0.00001, 1.0)      # stays resident: no other contour call follows
    rings = stages.closed_rings(contours)
    n = len(contours)

    def on_alarm(_sig, _frame):
        raise TimeoutError("step timed out")
    signal.signal(signal.SIGALRM, on_alarm)

    def host_route():
        out = []
        for d in planes:
            plane = ctx.download(d, (H, W))
            indexes_sorted, matrix, _, _ = order_ref.order_of_regions(plane, rings)
            out.append(order_ref.order_and_id_of_texts(rings, matrix, indexes_sorted)[0])
        return out

    def device_route():
        out = []
        for d in planes:
            indexes_sorted, matrix = stages._order_result(ctx.region_order_dev(d, H, W, None, n))
            out.append(stages.order_and_id_of_texts(rings, matrix, indexes_sorted)[0])
        return out

    times, results = {"host": [], "device": []}, {}
    for k in range(args.warmup + args.repeats):
        for name, fn in (("host", host_route), ("device", device_route)):
            signal.alarm(args.step_timeout)
            try:
                t0 = time.perf_counter()
                results[name] = fn()
                dt = time.perf_counter() - t0
            finally:
                signal.alarm(0)
            if k >= args.warmup:
                times[name].append(dt * 1e3)
    before = ctx.order_launches()
    ctx.region_order_dev(planes[0], H, W, None, n)
    launches = ctx.order_launches() - before
    for d in planes + [d_regions]:
        ctx.device_free(d)
    model.release()

    def row(v):
        return {"total_ms": round(statistics.median(v), 2), "min_ms": round(min(v), 2), "max_ms": round(max(v), 2)}
    out = {"pages": args.pages, "regions": n, "plane": [H, W], "host": row(times["host"]), "device": row(times["device"]),
           "same": results["host"] == results["device"], "bytes_per_page": H * W, "launches_per_page": launches,
           "order_page0": results["device"][0]}
    print(json.dumps(out))
    if args.write:
        with open(args.write, "w") as f:
            f.write("# Reading order of the text regions of %d pages\n\n" % args.pages)
            f.write("`tools/region_order_probe.py`: %d copies of one synthetic textline map of %d x %d with %d regions resident in device memory, "
                    "MI355X, median of %d runs after %d warm-up runs in one process, the two routes alternating; both end in a stream "
                    "synchronise.  Both routes give the same orders: %s.\n\n" % (args.pages, H, W, n, args.repeats, args.warmup, out["same"]))
            f.write("| route, all %d pages | total ms | min .. max ms |\n|---|---|---|\n" % args.pages)
            f.write("| download each plane, then scipy / numpy on the host (the only route before) | %s | %s .. %s |\n"
                    % (out["host"]["total_ms"], out["host"]["min_ms"], out["host"]["max_ms"]))
            f.write("| `region_order_dev` on the resident plane and the resident contour table | %s | %s .. %s |\n\n"
                    % (out["device"]["total_ms"], out["device"]["min_ms"], out["device"]["max_ms"]))
            f.write("Bytes no longer downloaded per page: %d (the plane); the device call returns %d int32 and %d float64 per page plus the "
                    "band edges.\n\nKernels queued by one order call: %d (row sums, band edges, moments, rank), whatever the number of regions.\n"
                    % (H * W, 3 * n, 2 * n, launches))


if __name__ == "__main__":
    main()
