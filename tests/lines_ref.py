"""numpy restatement of the deskewed text-line mask of one text region (tests/test_lines_cpu.py, tests/test_gpu_lines.py,
tests/golden/make_lines_golden.py): ``textline_contours_postprocessing`` up to ``dst`` (main.py:1472-1487) as ``do_work_of_slopes`` calls
it (main.py:1750), and the two projections the line splitters open on (main.py:539, 1020).  Built from the oracle's own functions and
an integer table of its own: nothing here is product code, and nothing here touches the GPU.

The rotation of a uint8 image is OpenCV's fixed-point bicubic path [EXT, unpinned: OpenCV 4.5.1 initInterTab2D / remapBicubic restated]:
per (ay, ax) sixteen int16 weights i[r][c] = saturate_cast<short>(float32(tab[ay][r] * tab[ax][c]) * 32768) (to nearest even), the
difference of their sum to 32768 removed from one entry of the 2 x 2 block at rows / columns {2, 3} (row-major scan from (2, 2): a
strictly smaller entry becomes the minimum candidate, otherwise a strictly larger one the maximum candidate; a negative difference
raises the maximum, a positive one lowers the minimum); v = clamp((sum of 16 taps src * i + 16384) >> 15, 0, 255)."""
import os

import numpy as np

from oracle import deskew as dk
from oracle import stage_glue as sg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lines_golden.npz")
SLOPES = [0, 2.0, -9.5, 21, 45, 45.0001, -70, 90, -90]

_TABLE = None


def integer_table() -> np.ndarray:
    """int16 [32][32][4][4], indexed [ay][ax][row][column]."""
    global _TABLE
    if _TABLE is None:
        tab = dk.cubic_table()
        out = np.zeros((32, 32, 4, 4), np.int64)
        for ay in range(32):
            for ax in range(32):
                v = (tab[ay][:, None] * tab[ax][None, :]).astype(np.float32) * np.float32(32768)
                i = np.clip(np.rint(v), -32768, 32767).astype(np.int64)
                diff = int(i.sum()) - 32768
                if diff != 0:
                    lo = hi = (2, 2)
                    for r in (2, 3):
                        for c in (2, 3):
                            if i[r, c] < i[lo]:
                                lo = (r, c)
                            elif i[r, c] > i[hi]:
                                hi = (r, c)
                    if diff < 0:
                        i[hi] -= diff
                    else:
                        i[lo] -= diff
                    i = i.astype(np.int16).astype(np.int64)      # the (short) cast of the corrected entry
                out[ay, ax] = i
        _TABLE = out.astype(np.int16)
    return _TABLE


def warp_affine_cubic_replicate_u8(src: np.ndarray, M: np.ndarray) -> np.ndarray:
    """cv2.warpAffine(src, M, (w, h), flags=INTER_CUBIC, borderMode=BORDER_REPLICATE) for a uint8 single-channel image."""
    src = np.ascontiguousarray(src, np.uint8)
    h, w = src.shape
    sx, sy, ax, ay = dk.source_coords(dk.invert_affine(M), h, w)
    flat = integer_table().reshape(32 * 32, 16).astype(np.int64)
    which = ay * 32 + ax
    s = src.astype(np.int64)
    acc = np.zeros((h, w), np.int64)
    for r in range(4):
        yy = np.clip(sy - 1 + r, 0, h - 1)
        for c in range(4):
            xx = np.clip(sx - 1 + c, 0, w - 1)
            acc = acc + s[yy, xx] * flat[which, r * 4 + c]
    assert np.abs(acc).max(initial=0) < 2 ** 31 - 16384
    return np.clip((acc + 16384) >> 15, 0, 255).astype(np.uint8)


def rotate_image_u8(img: np.ndarray, slope: float) -> np.ndarray:
    """main.py:159-163 on a uint8 plane."""
    h, w = img.shape[:2]
    return warp_affine_cubic_replicate_u8(img, dk.rotation_matrix((w // 2, h // 2), slope))


def open_close(mask255: np.ndarray) -> np.ndarray:
    """main.py:1478-1479, literally: erode, dilate, dilate, erode with the 5 x 5 kernel, one iteration each."""
    m = sg.morph(sg.morph(mask255, "erode", 5, 1), "dilate", 5, 1)
    return sg.morph(sg.morph(m, "dilate", 5, 1), "erode", 5, 1)


def open_close_shortcut(mask255: np.ndarray) -> np.ndarray:
    """The allowed shortcut: one clipped separable min(5) / max(9) / min(5)."""
    def sep(a, radius, is_max):
        f = np.maximum if is_max else np.minimum
        fill = 0 if is_max else 255
        for axis in (1, 0):
            p = np.pad(a, [(radius, radius) if k == axis else (0, 0) for k in (0, 1)], constant_values=fill)
            out = np.full_like(a, fill)
            for d in range(2 * radius + 1):
                out = f(out, p[:, d:d + a.shape[1]] if axis == 1 else p[d:d + a.shape[0], :])
            a = out
        return a
    return sep(sep(sep(np.ascontiguousarray(mask255, np.uint8), 2, False), 4, True), 2, False)


def eroded_crop(crop: np.ndarray, erode_iterations: int = 2) -> np.ndarray:
    """main.py:1734."""
    crop = np.ascontiguousarray(crop, np.uint8)
    return sg.morph(crop, "erode", 5, erode_iterations) if erode_iterations else crop


def line_mask(crop: np.ndarray, slope: float, erode_iterations: int = 2):
    """(dst uint8 [h, w] of 0 / 1, rows int64 [h], cols int64 [w]) for the textline plane cut to one box."""
    mask = (eroded_crop(crop, erode_iterations) * np.uint8(255)).astype(np.uint8)             # main.py:1475-1476 (uint8 arithmetic)
    dst = (rotate_image_u8(open_close(mask), slope) != 0).astype(np.uint8)
    return dst, dst.sum(axis=1).astype(np.int64), dst.sum(axis=0).astype(np.int64)


def load_golden():
    """Per page: (slopes [float], [dst uint8 [h, w]] per box, [1 = seperate_lines_vertical was called, 0 = seperate_lines])."""
    import slopes_ref
    g = np.load(GOLDEN)
    out = []
    for k, (_r, _t, boxes, _s) in enumerate(slopes_ref.load_pages()):
        masks = []
        for r, box in enumerate(boxes):
            w, h = box[2], box[3]
            masks.append(np.unpackbits(g[f"dst{k}_{r}"])[:h * w].reshape(h, w))
        out.append(([float(s) for s in g[f"slopes{k}"]], masks, [int(v) for v in g[f"vertical{k}"]]))
    return out
