#!/usr/bin/env python3
"""Time boxes, slopes and text lines for 16 stored pages of pairwise different size through the three 448 x 448 models (the setup of
tools/run_pages_probe.py), host arrays in and host arrays out:

  (a)  ``[run_with_line_boxes(img, masks=False) for img in images]`` on a build of the PARENT commit: ``--rows a --package-root DIR`` runs
       this script against the package in DIR (a checkout of the parent with its library built) in a process of its own;
  (a') the same loop on this build (its one-plane calls go through the plane table of one plane);
  (b)  ``run_pages_with_line_boxes(images)``: one ``sbbseg_run_pages``, boxes per page on the resident plane, three pooled calls;
  (c)  ``run_pages(images, resident=True)`` alone: what the lines add.

Rows of one process alternate; every measurement ends with a synchronise of the three handles; median and min-max of ``--repeats`` rounds
after ``--warmup`` rounds.  Per row: kernels queued by the line calls and by the slope sweeps (``sbbseg_debug_counter`` 2 and 5, summed
over the three handles; 5 does not exist in the parent), label-map bytes uploaded per page (counted from the calls' arguments: the loop
stages the cleaned region map once and the textline map three times, the pooled path none), and a digest of every output with split-K
off on the border handle.  ``--json FILE`` keeps the result; ``--combine A.json B.json --write FILE.md`` writes the table from the parent's
and this build's results.  The one condition: median (b) <= median (a) + the min-max spread of (a).  Not part of bench.py.

    python tools/run_pages_lines_probe.py --rows a --package-root PARENT --json a.json
    python tools/run_pages_lines_probe.py --rows a,b,c --json bc.json
    python tools/run_pages_lines_probe.py --combine a.json bc.json --write profiles/run_pages_lines.md"""
import argparse
import hashlib
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def digest(results):
    """sha256 over every array, box, slope and line record of a list of 8-tuples (page order)."""
    h = hashlib.sha256()

    def feed(x):
        if x is None:
            h.update(b"<none>")
        elif isinstance(x, dict):
            for k in sorted(x):
                h.update(k.encode())
                feed(x[k])
        elif isinstance(x, (list, tuple)):
            h.update(b"[%d]" % len(x))
            for v in x:
                feed(v)
        else:
            a = np.ascontiguousarray(x)
            h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    feed(results)
    return h.hexdigest()


def measure(a):
    root = os.path.abspath(a.package_root) if a.package_root else ROOT
    for p in (ROOT, root):                                          # tools/ and the synthetic models from here, the package from `root`
        if p in sys.path:
            sys.path.remove(p)
        sys.path.insert(0, p)
    from sbb_textline_detection_amd import _capi, clear_session, stages
    from sbb_textline_detection_amd.model import load_model
    from sbb_textline_detection_amd.synthetic import synthetic_page
    from sbb_textline_detection_amd.weights import save_sbbw
    from tools.synth_model import calibrated_model
    assert os.path.abspath(_capi.__file__).startswith(root + os.sep), _capi.__file__
    specs = {"model_page_mixed_best": 2, "model_strukturerkennung": 4, "model_textline_new": 2}      # main.py:58-60
    tmp = tempfile.mkdtemp(prefix="run_pages_lines_probe_")
    for name, classes in specs.items():
        cfg, w = calibrated_model(classes, 448, 448, seed=classes)
        save_sbbw(os.path.join(tmp, name + ".sbbw"), cfg, w)
    paths = [os.path.join(tmp, n + ".h5") for n in specs]
    st = stages.InferenceStages(*paths)
    handles = [load_model(p).ctx for p in paths]
    border = handles[0]
    base = synthetic_page(2900, 2080, seed=33)
    images = [np.ascontiguousarray(np.roll(base, 37 * k, axis=0)[:2900 - k, :2080 - (5 * k) % 16]) for k in range(a.pages)]
    pooled = hasattr(st, "run_pages_with_line_boxes")
    fns = {"a": lambda: [st.run_with_line_boxes(img, masks=False) for img in images]}
    if pooled:
        fns["b"] = lambda: st.run_pages_with_line_boxes(images)
        fns["c"] = lambda: st.run_pages(images, resident=True)
    rows = [r for r in a.rows.split(",") if r in fns]

    def sync():
        for c in handles:
            c.synchronize()

    def counter(which):
        try:
            return sum(c.debug_counter(which) for c in handles)
        except RuntimeError:                                        # the parent has no counter 5
            return None

    # one round with split-K off on the border handle: digests, launches, uploads
    out = {"pages": a.pages, "repeats": a.repeats, "warmup": a.warmup, "package_root": root, "rows": {}}
    border.set_ksplit(False)
    try:
        for r in rows:
            before = (counter(2), counter(5))
            res = fns[r]()
            sync()
            after = (counter(2), counter(5))
            info = {"line_launches": after[0] - before[0], "sweep_launches": None if after[1] is None else after[1] - before[1]}
            if r != "c":
                info["digest"] = digest(res)
                info["boxes"] = sum(len(x[4]) for x in res)
                info["pages_with_lines"] = sum(1 for x in res if x[2] is not None)
                maps = [x[2].size for x in res if x[2] is not None]                   # the page box: region map and textline map have its size
                # the loop: text_region_boxes stages the region plane, get_slopes / get_line_masks / get_line_boxes the textline plane
                info["label_map_upload_bytes_per_page"] = (4 * sum(maps) / len(res)) if r == "a" else 0.0
                info["page_upload_bytes_per_page"] = sum(img.nbytes for img in images) / len(images)
            out["rows"][r] = info
            del res
    finally:
        border.set_ksplit(True)
    ms = {r: [] for r in rows}
    for rnd in range(a.warmup + a.repeats):
        for r in rows:                                              # alternating
            sync()
            t0 = time.perf_counter()
            fns[r]()
            sync()
            if rnd >= a.warmup:
                ms[r].append((time.perf_counter() - t0) * 1e3)
    for r in rows:
        out["rows"][r].update(median_ms=statistics.median(ms[r]), min_ms=min(ms[r]), max_ms=max(ms[r]))
    clear_session()
    shutil.rmtree(tmp, ignore_errors=True)
    return out


def combine(parent_json, this_json, write):
    pa, th = json.load(open(parent_json)), json.load(open(this_json))
    a, a2, b, c = pa["rows"]["a"], th["rows"]["a"], th["rows"]["b"], th["rows"]["c"]
    n = th["pages"]
    spread = a["max_ms"] - a["min_ms"]
    met = b["median_ms"] <= a["median_ms"] + spread
    equal = a["digest"] == b["digest"]
    res = {"condition_met": bool(met), "b_over_a": b["median_ms"] / a["median_ms"], "b_minus_a_ms": b["median_ms"] - a["median_ms"], "spread_a_ms": spread,
           "a_equals_b": bool(equal), "a_parent_equals_a_this_build": a["digest"] == a2["digest"], "lines_add_ms": b["median_ms"] - c["median_ms"]}
    print(json.dumps(res))
    if write:
        names = [("(a) `[run_with_line_boxes(img, masks=False) for img in images]`, build of the parent commit", a),
                 ("(a') the same loop, this build", a2), ("(b) `run_pages_with_line_boxes(images)`", b), ("(c) `run_pages(images, resident=True)` alone", c)]

        def cnt(v):
            return "n/a" if v is None else "%d" % v
        with open(write, "w") as f:
            f.write("# Boxes, slopes and text lines for many pages: the resident pooled path against the page loop\n\n")
            f.write("`tools/run_pages_lines_probe.py` on one MI355X: the three 448 x 448 models (f16x3, max_batch 70), %d stored pages of pairwise "
                    "different size near 2900 x 2080 (upscaled x1.2 to about 3480 x 2496), host arrays in, host arrays out; %d of them reach the "
                    "textline model, %d text-region boxes in all.  Row (a) is a process of its own on a build of the parent commit, the other "
                    "rows alternate in a second process of the same session on the same box; every measurement ends with a synchronise of the "
                    "three handles; median and min-max of %d rounds after %d warm-up rounds.  Launches: `sbbseg_debug_counter` 2 (line calls) and "
                    "5 (slope sweeps; not in the parent) over one pass of all pages.  Uploads: bytes of label maps staged per page besides the "
                    "stored page itself (%.1f MB per page on every path), counted from the calls' arguments.\n\n"
                    % (n, b["pages_with_lines"], b["boxes"], th["repeats"], th["warmup"], b["page_upload_bytes_per_page"] / 1e6))
            f.write("| path | median ms | min - max ms | ms per page | line launches | sweep launches | label maps uploaded per page |\n|---|---|---|---|---|---|---|\n")
            for name, r in names:
                up = "%.1f MB" % (r["label_map_upload_bytes_per_page"] / 1e6) if "label_map_upload_bytes_per_page" in r else "0.0 MB"
                f.write("| %s | %.2f | %.2f - %.2f | %.2f | %s | %s | %s |\n" % (name, r["median_ms"], r["min_ms"], r["max_ms"], r["median_ms"] / n,
                                                                        cnt(r["line_launches"]), cnt(r["sweep_launches"]), up))
            f.write("\n* Condition: median (b) <= median (a) + spread of (a).  (b) - (a) = %+.2f ms beside a spread of (a) of %.2f ms: %s.\n"
                    % (res["b_minus_a_ms"], spread, "met" if met else "NOT met"))
            f.write("* (b) / (a) = %.3f.\n* (b) / (a') = %.3f.\n* (a') / (a) = %.3f: the same loop in two processes of one session (this build's one-plane calls read their plane through a table of one "
                    "record; nothing else on that path changed).\n"
                    % (res["b_over_a"], b["median_ms"] / a2["median_ms"], a2["median_ms"] / a["median_ms"]))
            f.write("* (b) - (c) = %.2f ms: what boxes, slopes, line sums and line boxes add to the three models for %d pages.\n" % (res["lines_add_ms"], n))
            f.write("* Outputs of (a) and (b) with split-K off on the border handle equal byte for byte (sha256 over every array, box, slope and "
                    "line record): %s; (a) and (a'): %s.\n" % ("yes" if equal else "NO", "yes" if res["a_parent_equals_a_this_build"] else "NO"))
    return 0 if met and equal else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", default="a,b,c")
    ap.add_argument("--package-root", default=None, help="import sbb_textline_detection_amd from this checkout (a build of the parent commit)")
    ap.add_argument("--json", default=None)
    ap.add_argument("--combine", nargs=2, default=None, metavar=("PARENT.json", "THIS.json"))
    ap.add_argument("--write", default=None)
    a = ap.parse_args()
    if a.combine:
        return combine(a.combine[0], a.combine[1], a.write)
    out = measure(a)
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f)
    return 0


if __name__ == "__main__":
    sys.exit(main())
