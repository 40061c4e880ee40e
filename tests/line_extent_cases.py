"""Shapes for the text-line x extent tests (tests/test_line_extent_cpu.py, tests/test_gpu_line_extent.py): rings that are CHAIN_APPROX_SIMPLE
lists (written out, or traced by the library's host tracer from a mask), boxes with a non-zero origin, slopes on both sides of every
branch, and line records as ``sbbseg_region_line_boxes_dev`` packs them.  The step reads only peak / point_up / point_down / branch of a
record and overwrites its corners, so the records are made up: peaks on rows of the box, corners filled with a sentinel."""
import numpy as np

from sbb_textline_detection_amd import _capi

WIDTHS = (1, 2, 3, 31, 32, 33, 63, 64, 65, 130)
HEIGHTS = (1, 2, 5, 40)
SLOPES = (0.0, 0.5, -3.0, 12.0, -30.0, 44.9, -45.0, 45.1)
SENTINEL = -777


def record(h, branch, n_lines=None):
    """A line record of an h-row dst: distinct peaks on rows of the box, point_up above row 0 for the first line (the `< 0` clamps)."""
    peaks = sorted({min(h - 1, max(0, v)) for v in (h // 5, h // 2, (4 * h) // 5)})
    if branch == 2:
        peaks = peaks[:1]
    if n_lines is not None:
        peaks = peaks[:n_lines]
    peaks = np.array(peaks, np.int32)
    n = len(peaks)
    up, down = (peaks - 2).astype(np.int32), (peaks + 3).astype(np.int32)
    return {"status": _capi.LINES_OK, "sigma": 3, "raised": False, "branch": int(branch), "peaks": peaks, "point_up": up, "point_down": down,
            "boxes": np.full((n, 4, 2), SENTINEL, np.int32), "boxes_rot": np.full((n, 4, 2), SENTINEL, np.int32)}


def traced(mask):
    """The host tracer's ring of the component of ``mask`` with the most points."""
    _boxes, contours = _capi.mask_contours_host(np.ascontiguousarray(mask, np.uint8))
    return max(contours, key=len).astype(np.int32)


def blob(w, h, seed):
    rng = np.random.default_rng(seed)
    m = (rng.random((h, w)) < 0.62).astype(np.uint8)
    m[h // 2, :] = 1                                  # one component spans the box
    return traced(m)


def named_rings():
    """name -> (ring in box coordinates, w, h)."""
    out = {}
    out["one_point"] = (np.array([[3, 2]], np.int32), 9, 6)
    out["two_point_line"] = (np.array([[1, 1], [7, 7]], np.int32), 10, 9)
    out["rectangle"] = (np.array([[2, 1], [30, 1], [30, 17], [2, 17]], np.int32), 33, 20)
    out["rectangle_closed"] = (np.array([[2, 1], [30, 1], [30, 17], [2, 17], [2, 1]], np.int32), 33, 20)
    out["L"] = (np.array([[1, 1], [9, 1], [9, 20], [28, 20], [28, 28], [1, 28]], np.int32), 31, 30)
    out["U"] = (np.array([[0, 0], [8, 0], [8, 25], [24, 25], [24, 0], [31, 0], [31, 31], [0, 31]], np.int32), 32, 32)
    neck = np.zeros((24, 40), np.uint8)
    neck[2:20, 2:14] = 1
    neck[4:22, 26:38] = 1
    neck[11, 14:26] = 1                               # a one-pixel neck: the ring runs along it twice
    out["neck"] = (traced(neck), 40, 24)
    out["diamond"] = (np.array([[16, 0], [32, 16], [16, 32], [0, 16]], np.int32), 33, 33)
    for k, (w, h) in enumerate(((65, 40), (33, 21), (64, 17))):
        out["blob%d" % k] = (blob(w, h, 11 + k), w, h)
    return out


def case(name, ring, w, h, slope, branch, origin=(37, 11), n_lines=None):
    ring = np.asarray(ring, np.int32).reshape(-1, 2) + np.array(origin, np.int32)
    return {"name": "%s/%g/b%d" % (name, slope, branch), "ring": ring, "box": np.array([origin[0], origin[1], w, h], np.int32), "slope": float(slope),
            "record": record(w if abs(slope) > 45 else h, branch, n_lines)}


def ref_cases():
    """The cases small enough for the literal Python restatement: every named ring at two slopes, every slope once, every branch."""
    rings = named_rings()
    out = []
    for k, (name, (ring, w, h)) in enumerate(sorted(rings.items())):
        out.append(case(name, ring, w, h, SLOPES[k % len(SLOPES)], (0, 3, 4, 2)[k % 4], n_lines=2))
        out.append(case(name, ring, w, h, SLOPES[(k + 3) % len(SLOPES)], (3, 4, 0, 0)[k % 4], n_lines=1))
    for w, h in ((1, 1), (2, 1), (1, 5), (3, 2)):
        out.append(case("full%dx%d" % (w, h), [[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]], w, h, 12.0, 4, n_lines=1))
    return out


def grid_cases():
    """Every width x height x slope: the full-box rectangle, and a traced blob where the box has room for one."""
    out = []
    k = 0
    for w in WIDTHS:
        for h in HEIGHTS:
            for slope in SLOPES:
                k += 1
                branch = (0, 3, 4, 2)[k % 4]
                if w >= 3 and h >= 5 and k % 2:
                    out.append(case("blob%dx%d" % (w, h), blob(w, h, k), w, h, slope, branch, origin=(k, 2 * k)))
                else:
                    out.append(case("full%dx%d" % (w, h), [[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]], w, h, slope, branch, origin=(k, 2 * k)))
    for name, (ring, w, h) in sorted(named_rings().items()):
        for slope in SLOPES:
            out.append(case(name, ring, w, h, slope, 0))
    return out


def raw_masks():
    """name -> mask for the border scan alone."""
    out = {}
    out["empty"] = np.zeros((5, 7), np.uint8)
    one = np.zeros((4, 6), np.uint8)
    one[2, 3] = 1
    out["one_pixel"] = one
    hollow = np.zeros((9, 9), np.uint8)
    hollow[2:7, 2:7] = 1
    hollow[3:6, 3:6] = 0
    out["hollow_square"] = hollow                     # outer border 4 points; the hole border cuts the corners: 8 points, the hole wins
    octagon = hollow.copy()
    octagon[3:6, 3:6] = 0
    octagon[2:7, 2:7] = 0
    octagon[2, 3:6] = octagon[6, 3:6] = octagon[3:6, 2] = octagon[3:6, 6] = 1
    out["hollow_octagon"] = octagon                   # the same ring of pixels from outside and from inside: 8 points each, a tie
    ragged = np.zeros((16, 20), np.uint8)
    ragged[1:15, 1:19] = 1
    ragged[4:12, 4:16] = 0
    ragged[4:12:2, 4] = 1                             # teeth on the inside: the hole border has the most points
    ragged[5:12:2, 15] = 1
    out["ragged_inside"] = ragged
    holes = np.ones((21, 67), np.uint8)
    holes[2:20:3, 2:66:3] = 0
    out["many_holes"] = holes
    out["touches_all_sides"] = np.ones((6, 33), np.uint8)
    two = np.zeros((8, 40), np.uint8)
    two[1:4, 2:9] = 1
    two[4:7, 30:37] = 1
    out["two_equal"] = two
    rng = np.random.default_rng(5)
    out["noise"] = (rng.random((40, 130)) < 0.55).astype(np.uint8)
    out["noise_tall"] = (rng.random((70, 31)) < 0.7).astype(np.uint8)
    return out


def golden_cases():
    """The cases of tests/golden/line_extent_golden.npz (recorded from the reference's own textline_contours_postprocessing on cv2 stubs, see
    tests/golden/make_line_extent_golden.py): ring, box, slope, the library's own line record of the recorded ``dst``, and what the
    reference returned."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "line_extent_golden.npz"))
    out = []
    for k in range(len(g["slope"])):
        box, slope = g["box"][k].astype(np.int32), float(g["slope"][k])
        w, h = int(box[2]), int(box[3])
        dst = np.unpackbits(g["dst"][g["dst_off"][k]:g["dst_off"][k + 1]])[:w * h].reshape(h, w)
        vertical = abs(slope) > 45
        profile = dst.sum(axis=0 if vertical else 1).astype(np.int32)
        rec = _capi.line_split_host([profile], [h if vertical else w], [vertical], [_capi.line_rotation_terms(w, h, slope)])[0]
        out.append({"name": "golden%d" % k, "ring": g["ring"][g["ring_off"][k]:g["ring_off"][k + 1]].astype(np.int32), "box": box, "slope": slope,
                    "record": rec, "status": int(g["status"][k]), "holes": int(g["holes"][k]), "is_hole": bool(g["is_hole"][k]), "tie": bool(g["tie"][k]),
                    "polygons": g["polygons"][g["polygon_off"][k]:g["polygon_off"][k + 1]], "page": int(g["page"][k])})
    return out
