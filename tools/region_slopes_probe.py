#!/usr/bin/env python3
"""Time the per-region deskew slopes of one synthetic page, three ways, in one process:

  (i)  the per-region loop: for every box, crop, erode x 2 (``ctx.morph``) and ``stages.return_deskew_slope`` -- one upload, one blocking
       launch per sweep and one copy back PER REGION;
  (ii) ``stages.get_slopes(statistics="host")``: one upload of the textline map, one batched sweep over all boxes (and one over the steep
       ones), the row counts copied back and the scipy peak logic per region on the host;
  (iii) ``stages.get_slopes(statistics="device")`` (the default): the same sweeps, the peak logic and the angle selection on the device
       (``sbbseg_region_deskew_slopes_dev``), only the winners copied back.

The statistic call alone (``sbbseg_profile_statistics_dev`` on the first sweep's counts, already in device memory: its launches, the copy of
the small tables in and of spread / state / winner out, one synchronisation) is timed the same way.

Each path is split into device + copy time (the time spent inside the library calls) and host time (the scipy peak logic and the rest).
Median of ``--repeats`` runs after ``--warmup`` runs; every run sits under its own alarm (``--step-timeout`` seconds).  Prints one JSON
line; ``--write FILE.md`` also writes the three rows and the ratios as a Markdown table.  Not part of bench.py.

    python tools/region_slopes_probe.py [--boxes 28] [--repeats 7] [--write profiles/region_slopes.md]"""
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


def synthetic_textline_page(h, w, n_boxes, seed):
    """A 0 / 1 textline plane with n_boxes non-overlapping text blocks on a grid (each with its own size, line pitch and skew of up to
    about 8 degrees, a few steeper) and their boxes [x, y, w, h]."""
    rng = np.random.RandomState(seed)
    cols = 4
    rows = (n_boxes + cols - 1) // cols
    ch, cw = h // rows, w // cols
    t = np.zeros((h, w), np.uint8)
    boxes = []
    for k in range(n_boxes):
        gy, gx = divmod(k, cols)
        bh, bw = int(rng.randint(ch // 3, ch - 8)), int(rng.randint(cw // 3, cw - 8))
        y0, x0 = gy * ch + int(rng.randint(0, ch - bh - 4)), gx * cw + int(rng.randint(0, cw - bw - 4))
        pitch, thick = int(rng.randint(26, 44)), int(rng.randint(11, 17))
        slant = np.tan(np.deg2rad(rng.uniform(-8, 8) if k % 9 else 20.0))
        xs = np.arange(bw)
        for y in range(-bh, 2 * bh, pitch):
            ys = y + np.round(slant * (xs - bw / 2)).astype(int)
            for d in range(thick):
                yy = ys + d
                ok = (yy >= 4) & (yy < bh - 4) & (xs >= 4) & (xs < bw - 4)
                t[y0 + yy[ok], x0 + xs[ok]] = 1
        boxes.append([x0, y0, bw, bh])
    return t, boxes


class Clock:
    """Accumulates the wall time spent inside wrapped library calls."""

    def __init__(self):
        self.t = 0.0

    def wrap(self, fn):
        def timed(*a, **k):
            t0 = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                self.t += time.perf_counter() - t0
        return timed


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
    if args.boxes < 24 or args.repeats < 5:
        ap.error("at least 24 boxes and 5 repeats")

    from sbb_textline_detection_amd import stages
    from sbb_textline_detection_amd.model import SegModel
    from tools.synth_model import calibrated_model
    cfg, wts = calibrated_model(2, 224, 224, seed=0)
    model = SegModel(cfg, wts, device=0, max_batch=4)            # any finalized handle: the deskew calls do not touch the network
    ctx = model.ctx
    textlines, boxes = synthetic_textline_page(args.height, args.width, args.boxes, args.seed)
    clock = Clock()
    for name in ("morph", "deskew_profiles", "stage", "region_deskew_profiles_dev", "region_deskew_slopes_dev"):
        setattr(ctx, name, clock.wrap(getattr(ctx, name)))

    def clean(s):
        return 0 if (s == 999 or abs(s) > 120.5) else s

    def loop():
        out = []
        for x, y, w, h in boxes:
            crop = np.ascontiguousarray(textlines[y:y + h, x:x + w])
            out.append(clean(stages.return_deskew_slope(ctx.morph(crop, 0, 5, 2), 2, ctx)))
        return out

    def batched():
        return stages.get_slopes(textlines, boxes, ctx, statistics="host")

    def on_device():
        return stages.get_slopes(textlines, boxes, ctx, statistics="device")

    from sbb_textline_detection_amd import _capi
    sweep1 = np.linspace(-25, 25, 80)
    first = ctx.region_deskew_profiles(textlines, boxes, sweep1)
    stat_offsets = _capi.region_deskew_offsets(boxes, len(sweep1), *textlines.shape)
    stat_counts = np.concatenate([p.reshape(-1) for p in first]).astype(np.int32)
    d_stat_counts = ctx.device_alloc(stat_counts.nbytes)
    ctx.upload(d_stat_counts, stat_counts)

    def statistic_only():
        return ctx.profile_statistics_dev(d_stat_counts, stat_offsets, len(sweep1))[2].tolist()

    def on_alarm(_sig, _frame):
        raise TimeoutError("step timed out")
    signal.signal(signal.SIGALRM, on_alarm)

    def measure(fn):
        total, device, result = [], [], None
        for k in range(args.warmup + args.repeats):
            signal.alarm(args.step_timeout)
            try:
                clock.t = 0.0
                t0 = time.perf_counter()
                result = fn()
                dt = time.perf_counter() - t0
            finally:
                signal.alarm(0)
            if k >= args.warmup:
                total.append(dt * 1e3)
                device.append(clock.t * 1e3)
        med, dev = statistics.median(total), statistics.median(device)
        return {"total_ms": round(med, 2), "device_and_copies_ms": round(dev, 2), "host_ms": round(med - dev, 2),
                "min_ms": round(min(total), 2), "max_ms": round(max(total), 2)}, result
    row_loop, slopes_loop = measure(loop)
    row_batched, slopes_batched = measure(batched)
    row_device, slopes_device = measure(on_device)
    row_stat, _winners = measure(statistic_only)
    ctx.device_free(d_stat_counts)
    model.release()
    res = {"probe": "region_slopes", "page": [args.height, args.width], "boxes": len(boxes), "repeats": args.repeats,
           "largest_box": max(boxes, key=lambda b: b[2] * b[3])[2:], "same_slopes": slopes_loop == slopes_batched == slopes_device,
           "nonzero_slopes": sum(1 for s in slopes_batched if s != 0), "second_sweep_boxes": sum(1 for s in slopes_batched if s <= -50),
           "per_region_loop": row_loop, "get_slopes": row_batched, "get_slopes_device": row_device,
           "statistic_call_80_angles": {k: row_stat[k] for k in ("total_ms", "min_ms", "max_ms")}, "profiles_first_sweep": len(boxes) * len(sweep1),
           "ratio_total": round(row_loop["total_ms"] / row_batched["total_ms"], 2),
           "ratio_host_to_device_statistics": round(row_batched["total_ms"] / row_device["total_ms"], 2),
           "ratio_device": round(row_loop["device_and_copies_ms"] / max(row_batched["device_and_copies_ms"], 1e-9), 2)}
    print(json.dumps(res))
    if args.write:
        with open(args.write, "w") as f:
            f.write("# Deskew slopes of all text regions of a page: per-region loop, batched sweep, statistic on the device\n\n")
            f.write(f"`tools/region_slopes_probe.py`: one synthetic textline map of {args.height} x {args.width} with {len(boxes)} boxes "
                    f"(largest {res['largest_box'][0]} x {res['largest_box'][1]}), MI355X, median of {args.repeats} runs after {args.warmup} "
                    f"warm-up runs in one process.  All three paths return the same slopes: {res['same_slopes']} "
                    f"({res['nonzero_slopes']} non-zero, {res['second_sweep_boxes']} from the second sweep).\n\n")
            f.write("| path | total ms | device + copies ms | host (scipy) ms | min .. max ms |\n|---|---|---|---|---|\n")
            for label, r in (("(i) per-region loop: `ctx.morph` + `return_deskew_slope` per box", row_loop), ("(ii) `get_slopes(statistics=\"host\")`: batched sweeps, scipy peak logic", row_batched),
                             ("(iii) `get_slopes(statistics=\"device\")`: batched sweeps, statistic and selection on the device", row_device)):
                f.write(f"| {label} | {r['total_ms']} | {r['device_and_copies_ms']} | {r['host_ms']} | {r['min_ms']} .. {r['max_ms']} |\n")
            f.write(f"\nRatio (i) / (ii): {res['ratio_total']} on the total, {res['ratio_device']} on device + copies.  "
                    f"Ratio (ii) / (iii): {res['ratio_host_to_device_statistics']} on the total.\n\n")
            f.write(f"The statistic call alone (`sbbseg_profile_statistics_dev` on the {res['profiles_first_sweep']} profiles of the first sweep, counts already in "
                    f"device memory; wall time of the call: the copy of the tables in, the launches, the copy of spread / state / winner out, one "
                    f"synchronisation): {row_stat['total_ms']} ms (min .. max {row_stat['min_ms']} .. {row_stat['max_ms']}).\n")
    return 0 if res["same_slopes"] else 1


if __name__ == "__main__":
    sys.exit(main())
