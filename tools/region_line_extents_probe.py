#!/usr/bin/env python3
"""Time the text-line x extents of the regions of one synthetic page (the 28-box page of ``tools/region_slopes_probe.py``), in one process:

  (i)   the library's serial host twin, region by region (``_capi.host_region_line_extents``: fill, float64 rotation, cast, border scan,
        the 1000 samples of every line) -- there is no earlier route to compare with: the step did not exist;
  (ii)  ``Context.region_line_extents_dev``: all regions in one call, the rings being the resident result of one
        ``text_region_contours_dev`` call on the page's region map (the boxes, class 1), read in place.

Slopes and line records come from the device steps before it (``region_deskew_slopes_dev``, ``region_line_boxes_dev``).  Both routes end
on the host with the same records.  Median of ``--repeats`` runs after ``--warmup`` runs, the two routes alternating; every run sits under
its own alarm (``--step-timeout`` seconds).  Prints one JSON line; ``--write FILE.md`` also writes a Markdown table.  Not part of bench.py.

    python tools/region_line_extents_probe.py [--repeats 7] [--write profiles/region_line_extents.md]"""
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

    from sbb_textline_detection_amd import _capi
    from sbb_textline_detection_amd.model import SegModel
    from tools.synth_model import calibrated_model
    cfg, wts = calibrated_model(2, 224, 224, seed=0)
    model = SegModel(cfg, wts, device=0, max_batch=4)            # any finalized handle: these calls do not touch the network
    ctx = model.ctx
    textlines, page_boxes = synthetic_textline_page(args.height, args.width, args.boxes, args.seed)
    H, W = textlines.shape
    regions = np.zeros((H, W), np.uint8)
    for x, y, w, h in page_boxes:
        regions[y:y + h, x:x + w] = 1
    d_text, d_regions = ctx.device_alloc(H * W), ctx.device_alloc(H * W)
    ctx.upload(d_text, textlines)
    ctx.upload(d_regions, regions)
    boxes, contours = ctx.text_region_contours_dev(d_regions, H, W, 1, 0.00001, 1.0)      # stays resident: no other contour call follows
    slopes = ctx.region_deskew_slopes_dev(d_text, H, W, boxes, 2)
    records = ctx.region_line_boxes_dev(d_text, H, W, boxes, slopes, 2)
    n = len(boxes)

    def on_alarm(_sig, _frame):
        raise TimeoutError("step timed out")
    signal.signal(signal.SIGALRM, on_alarm)

    def host_route():
        return [_capi.host_region_line_extents(c, b, s, r) for c, b, s, r in zip(contours, boxes, slopes, records)]

    def device_route():
        return ctx.region_line_extents_dev(boxes, slopes, records, None)

    def same(a, b):
        return all(np.array_equal(x[k], y[k]) for x, y in zip(a, b) for k in ("extent", "boxes", "boxes_rot")) and \
            all(x["contour"] == y["contour"] for x, y in zip(a, b))

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
    before = ctx.extent_launches()
    device_route()
    launches = ctx.extent_launches() - before
    for d in (d_text, d_regions):
        ctx.device_free(d)
    model.release()

    def row(v):
        return {"total_ms": round(statistics.median(v), 2), "min_ms": round(min(v), 2), "max_ms": round(max(v), 2)}
    dev = results["device"]
    lines = sum(len(r["peaks"]) for r in dev)
    cut = sum(1 for r, b in zip(dev, boxes) for e in r["extent"].tolist() if tuple(e) != (0, int(b[2])))
    out = {"regions": n, "plane": [H, W], "lines": lines, "lines_cut": cut, "host": row(times["host"]), "device": row(times["device"]),
           "same": same(results["host"], dev), "launches": launches, "ties": sum(1 for r in dev if r["contour"]["tie"]),
           "hole_winners": sum(1 for r in dev if r["contour"]["is_hole"]), "borders": sum(r["contour"]["borders"] for r in dev),
           "winner_points": sum(r["contour"]["points"] for r in dev)}
    print(json.dumps(out))
    if args.write:
        with open(args.write, "w") as f:
            f.write("# Text-line x extents of the %d regions of one page\n\n" % n)
            f.write("`tools/region_line_extents_probe.py`: one synthetic textline map of %d x %d with %d regions and %d lines (%d of them cut "
                    "narrower than 0 .. w), MI355X, median of %d runs after %d warm-up runs in one process, the two routes alternating; both end "
                    "with the records on the host.  Both routes give the same records: %s.\n\n"
                    % (H, W, n, lines, cut, args.repeats, args.warmup, out["same"]))
            f.write("| route, all %d regions | total ms | min .. max ms |\n|---|---|---|\n" % n)
            f.write("| serial host twin, region by region (`sbbseg_region_line_extents_host`) | %s | %s .. %s |\n"
                    % (out["host"]["total_ms"], out["host"]["min_ms"], out["host"]["max_ms"]))
            f.write("| `region_line_extents_dev`, one call, rings read from the resident contour table | %s | %s .. %s |\n\n"
                    % (out["device"]["total_ms"], out["device"]["min_ms"], out["device"]["max_ms"]))
            f.write("Kernels queued by the device call: %d, whatever the number of regions.  Borders found in the rotated contour images: %d; "
                    "points of the winners: %d; regions whose winner is a hole border: %d; regions with a tie for the most points: %d.\n\n"
                    "No threshold: the step has no earlier counterpart, and nobody had measured it.  The LDS limit of the border scan "
                    "(60 KB for the three bit maps) and one wave per region are chosen, not measured.\n"
                    % (launches, out["borders"], out["winner_points"], out["hole_winners"], out["ties"]))


if __name__ == "__main__":
    main()
