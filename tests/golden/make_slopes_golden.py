#!/usr/bin/env python3
"""Generate tests/golden/slopes_golden.npz by running the REFERENCE's OWN control flow for the step after the three models:
``get_text_region_contours_and_boxes`` (main.py:456-480, sets ``boxes``) and ``do_work_of_slopes`` (main.py:1721-1758: crop, erode x 2,
``return_deskew_slope`` in its try / except, the 999 / 120.5 rules).

Runs only where the reference is available (the build container); never on the GPU box.  The reference is imported exactly as
``make_glue_golden.py`` imports it, with that generator's cv2 stubs (the oracle's restatements of the OpenCV arithmetic, [EXT]) plus
``cv2.erode`` -> ``oracle.stage_glue.morph``.  ``textline_contours_postprocessing`` (out of scope) is replaced by a no-op and a plain
object with ``put`` stands in for the multiprocessing queue.  The fixture holds arrays only: the synthetic maps, the reference's boxes
and slopes.
    python tests/golden/make_slopes_golden.py [out.npz]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from make_glue_golden import install_contour_tree_stubs, install_cv2_stubs  # noqa: E402
from make_tiling_golden import load_reference  # noqa: E402
from oracle import deskew as dk  # noqa: E402
from oracle import stage_glue as sg  # noqa: E402


def lines(h, w, period=24, thick=13, margin=6):
    """Horizontal text lines (0 / 1), thick enough to survive the 9 x 9 minimum of two 5 x 5 erosions."""
    m = np.zeros((h, w), np.uint8)
    for y in range(margin, h - thick - margin + 1, period):
        m[y:y + thick, margin:w - margin] = 1
    return m


def skewed(h, w, angle, **kw):
    """Those lines rotated by ``angle`` degrees about the centre of their padded square (the oracle's warp): uint8 0 / 1, square."""
    return (dk.rotate_image(dk.padded_square(lines(h, w, **kw)), angle) != 0).astype(np.uint8)


def put(regions, textlines, y, x, patch, label=1, pad=8):
    """A text region of class ``label`` (the patch's rectangle, grown by ``pad``) with the patch as its text lines."""
    h, w = patch.shape
    regions[y - pad:y + h + pad, x - pad:x + w + pad] = label
    textlines[y:y + h, x:x + w] = patch


def page(kind):
    """(regions uint8 [H, W] of classes 0..3, textlines uint8 [H, W] of 0 / 1)"""
    if kind == 0:        # a ring with an island inside its hole (the island has a parent: no box) and a separate block, lines skewed by 4 degrees
        r, t = np.zeros((420, 520), np.uint8), np.zeros((420, 520), np.uint8)
        r[20:220, 20:260] = 1
        r[50:190, 50:230] = 0
        r[100:140, 110:170] = 1                                  # the island
        t[24:44, 30:250] = 1                                     # a line in the ring's upper bar
        t[108:132, 118:162] = 1                                  # lines on the island: never looked at
        put(r, t, 200, 290, skewed(100, 150, 4.0))
        return r, t
    if kind == 1:        # two blocks three pixels apart (CLOSE joins them), another class below, specks that die in the opening
        r, t = np.zeros((300, 400), np.uint8), np.zeros((300, 400), np.uint8)
        r[30:170, 30:150] = 1
        r[30:170, 153:300] = 1
        r[200:280, 30:300] = 3
        r[10:13, 350:354] = 1
        t[30:170, 30:300] = lines(140, 270, period=30, thick=15)
        return r, t
    if kind == 2:        # lines at -70 degrees: the first sweep answers beyond 15 degrees, the second sweep runs; and a mild -9.5 degrees
        r, t = np.zeros((620, 420), np.uint8), np.zeros((620, 420), np.uint8)
        put(r, t, 20, 30, skewed(100, 170, -70.0, period=26, thick=15))
        put(r, t, 300, 60, skewed(90, 150, -9.5))
        return r, t
    if kind == 3:        # crops that are empty after the erosion: lines 4 px thick, and a region without any text line
        r, t = np.zeros((260, 340), np.uint8), np.zeros((260, 340), np.uint8)
        r[20:120, 20:200] = 1
        for y in range(30, 110, 12):
            t[y:y + 4, 30:190] = 1
        r[150:240, 40:160] = 1
        r[150:240, 200:320] = 1
        t[160:230, 210:310] = lines(70, 100, period=22, thick=12, margin=4)
        return r, t
    if kind == 4:        # a page of 1400 x 1200 with regions of several sizes and skews, one at the page's corner
        r, t = np.zeros((1400, 1200), np.uint8), np.zeros((1400, 1200), np.uint8)
        put(r, t, 0, 0, skewed(110, 160, 2.0), pad=0)
        put(r, t, 40, 400, skewed(140, 200, -3.0))
        put(r, t, 520, 60, skewed(110, 170, 7.0))
        put(r, t, 560, 600, lines(180, 280, period=28))
        put(r, t, 960, 100, skewed(90, 120, 21.0))
        r[1300:1400, 900:1200] = 1                               # touches the bottom right corner
        t[1300:1400, 900:1200] = lines(100, 300, period=26)
        r[900:1000, 800:1000] = 2                                # other classes are not text
        return r, t
    raise ValueError(kind)


N_PAGES = 5


class Sink:
    def put(self, item):
        self.item = item


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "slopes_golden.npz")
    ref = load_reference()
    import cv2
    install_cv2_stubs(cv2, {})
    install_contour_tree_stubs(cv2, ref)
    cv2.erode = lambda src, kernel, iterations=1: sg.morph(src, "erode", kernel.shape[0], iterations)
    swept = []                                                   # every angle the reference rotates by
    rotation = cv2.getRotationMatrix2D

    def recording_rotation(center, angle, scale):
        swept.append(float(angle))
        return rotation(center, angle, scale)
    cv2.getRotationMatrix2D = recording_rotation
    det = ref.textline_detector.__new__(ref.textline_detector)
    det.kernel = np.ones((5, 5), np.uint8)                       # main.py:57
    det.textline_contours_postprocessing = lambda *a, **k: None  # out of scope
    out = {"n": np.int64(N_PAGES)}
    second_sweeps = nonzero = empty_crops = 0
    for k in range(N_PAGES):
        regions, textlines = page(k)
        contours = det.get_text_region_contours_and_boxes(np.repeat(regions[:, :, None], 3, axis=2))
        boxes = [list(b) for b in det.boxes]
        assert len(boxes) == len(contours)
        del swept[:]
        sink = Sink()
        det.do_work_of_slopes(sink, boxes, textlines, contours)  # all boxes in one call, as get_slopes_and_deskew hands them over
        slopes = [float(s) for s in sink.item[0]]
        assert [list(b) for b in sink.item[2]] == boxes and len(swept) % 80 % 30 == 0
        second_sweeps += sum(1 for a in swept if a < -49.0) // 30
        for box in boxes:
            crop = textlines[box[1]:box[1] + box[3], box[0]:box[0] + box[2]]
            empty_crops += not sg.morph(crop, "erode", 5, 2).any()
        nonzero += sum(1 for s in slopes if s != 0)
        out[f"regions{k}"] = regions
        out[f"textlines{k}"] = np.packbits(textlines)
        out[f"shape{k}"] = np.array(regions.shape, np.int64)
        out[f"boxes{k}"] = np.array(boxes, np.int64).reshape(-1, 4)
        out[f"slopes{k}"] = np.array(slopes, np.float64)
        print("page", k, regions.shape, "boxes", boxes, "slopes", slopes)
    # a fixture in which every slope is 0 proves nothing
    assert second_sweeps >= 2 and nonzero >= 4 and empty_crops >= 2, (second_sweeps, nonzero, empty_crops)
    assert len(out["boxes0"]) == 2, "the island inside the ring must not get a box"
    assert len(out["boxes1"]) == 1, "CLOSE must join the two blocks"
    np.savez_compressed(out_path, **out)
    print("wrote", out_path, os.path.getsize(out_path), "bytes;", second_sweeps, "second sweeps,", nonzero, "non-zero slopes,", empty_crops, "empty crops")


if __name__ == "__main__":
    main()
