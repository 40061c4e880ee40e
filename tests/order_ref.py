"""The reading order of text regions, restated with numpy and scipy: what order_of_regions / order_and_id_of_texts (main.py:1802-1906)
compute, with the real ``gaussian_filter1d`` and ``find_peaks``, and cv2.moments / cv2.contourArea for integer contours as a serial Python
loop ([EXT]: OpenCV's contourMoments restated; cv2 is not installable).  Python floats are IEEE binary64 and every operation below is
one rounding, so the loop is the float64 arithmetic of the C++ it restates."""
import numpy as np
from scipy.ndimage import gaussian_filter1d
from scipy.signal import find_peaks

FLT_EPSILON = 1.1920928955078125e-07


def _points(contour):
    return [(int(x), int(y)) for x, y in np.asarray(contour).reshape(-1, 2).tolist()]


def contour_sums(contour):
    """(a00, a10, a01) of contourMoments: serial, float64, starting from the last point."""
    pts = _points(contour)
    a00 = a10 = a01 = 0.0
    if not pts:
        return a00, a10, a01
    xp, yp = float(pts[-1][0]), float(pts[-1][1])
    for x, y in pts:
        x, y = float(x), float(y)
        dxy = xp * y - x * yp
        a00 = a00 + dxy
        a10 = a10 + dxy * (xp + x)
        a01 = a01 + dxy * (yp + y)
        xp, yp = x, y
    return a00, a10, a01


def moments(contour):
    """cv2.moments(contour)'s m00, m10, m01 (the keys order_of_regions reads)."""
    a00, a10, a01 = contour_sums(contour)
    m00 = m10 = m01 = 0.0
    if abs(a00) > FLT_EPSILON:
        half, sixth = (0.5, 0.16666666666666666) if a00 > 0 else (-0.5, -0.16666666666666666)
        m00, m10, m01 = a00 * half, a10 * sixth, a01 * sixth
    return {"m00": m00, "m10": m10, "m01": m01}


def contour_area(contour):
    """cv2.contourArea(contour) (computed by the reference, read by nothing)."""
    return abs(contour_sums(contour)[0]) * 0.5


def centroid(contour):
    m = moments(contour)
    return m["m10"] / (m["m00"] + 1e-32), m["m01"] / (m["m00"] + 1e-32)


def exact_sums(contour):
    """The three sums as exact integers, and whether every prefix stays below 2^53 in magnitude with coordinates below 32768."""
    pts = _points(contour)
    s00 = s10 = s01 = 0
    small = all(abs(v) < 32768 for p in pts for v in p)
    for (xp, yp), (x, y) in zip(pts[-1:] + pts[:-1], pts):
        dxy = xp * y - x * yp
        s00, s10, s01 = s00 + dxy, s10 + dxy * (xp + x), s01 + dxy * (yp + y)
        small = small and max(abs(s00), abs(s10), abs(s01)) < 2 ** 53
    return (s00, s10, s01), small


def band_edges(textline_mask):
    """[0] + peaks_neg + [H] of main.py:1803-1827, 1868-1872: unclamped."""
    y = np.asarray(textline_mask).sum(axis=1)
    y_padded = np.zeros(len(y) + 40)
    y_padded[20:len(y) + 20] = y
    zneg_rev = -y_padded + np.max(y_padded)
    zneg = np.zeros(len(zneg_rev) + 40)
    zneg[20:len(zneg_rev) + 20] = zneg_rev
    zneg = gaussian_filter1d(zneg, 8)
    peaks_neg, _ = find_peaks(zneg, height=0)
    return [0] + [int(p) - 40 for p in peaks_neg] + [int(np.asarray(textline_mask).shape[0])]


def order_of_regions(textline_mask, contours):
    """(indexes_sorted, matrix_of_orders, edges, bands): the reference's two values, the band edges, and per region the band it landed in
    (-1: none).  Ties in cx [EXT]: ascending region index (a stable sort)."""
    n = len(contours)
    cs = [centroid(c) for c in contours]
    matrix = np.zeros((n, 5))
    matrix[:, 0] = np.arange(n)
    matrix[:, 1] = 1
    matrix[:, 2] = [c[0] for c in cs]
    matrix[:, 3] = [c[1] for c in cs]
    matrix[:, 4] = np.arange(n)
    edges = band_edges(textline_mask)
    final, bands = [], [-1] * n
    for i in range(len(edges) - 1):
        top, down = edges[i], edges[i + 1]
        inside = (matrix[:, 3] >= top) & (matrix[:, 3] < down)
        indexes_in, cxs_in = matrix[:, 0][inside], matrix[:, 2][inside]
        for j in indexes_in[np.argsort(cxs_in, kind="stable")]:
            final.append(int(j))
            assert bands[int(j)] == -1, "a region in two bands"
            bands[int(j)] = i
    return final, matrix, edges, bands


def order_and_id_of_texts(found_polygons_text_region, matrix_of_orders, indexes_sorted):
    order_of_texts, id_of_texts = [], []
    for mm in range(len(found_polygons_text_region)):
        id_of_texts.append('r' + str(mm))
        index_matrix = matrix_of_orders[:, 0][(matrix_of_orders[:, 1] == 1) & (matrix_of_orders[:, 4] == mm)]
        order_of_texts.append(int(np.where(np.asarray(indexes_sorted) == index_matrix)[0][0]))
    return order_of_texts, id_of_texts


def _hull(points):
    """Convex hull (monotone chain) of integer points, collinear points dropped: a simple polygon, so its centroid lies inside it."""
    pts = sorted(set(map(tuple, points)))
    if len(pts) <= 2:
        return pts

    def half(seq):
        out = []
        for p in seq:
            while len(out) >= 2 and (out[-1][0] - out[-2][0]) * (p[1] - out[-2][1]) - (out[-1][1] - out[-2][1]) * (p[0] - out[-2][0]) <= 0:
                out.pop()
            out.append(p)
        return out[:-1]
    return half(pts) + half(pts[::-1])


def random_contour(rng, H, W):
    """A convex integer polygon inside an H x W plane, either orientation, open or closed like the reference's rings; now and then
    degenerate (1 or 2 points, collinear)."""
    kind = rng.integers(0, 10)
    if kind == 0:
        return rng.integers(0, [W, H], size=(int(rng.integers(1, 3)), 2))
    if kind == 1:
        x = np.sort(rng.integers(0, W, size=3))
        return np.stack([x, np.full(3, int(rng.integers(0, H)))], axis=1)
    x0, y0 = int(rng.integers(0, W)), int(rng.integers(0, H))
    x1, y1 = int(rng.integers(x0, W)), int(rng.integers(y0, H))
    pts = np.array(_hull(rng.integers([x0, y0], [x1 + 1, y1 + 1], size=(int(rng.integers(3, 12)), 2)).tolist()), np.int64).reshape(-1, 2)
    if rng.integers(0, 2):
        pts = pts[::-1]
    return np.concatenate([pts, pts[:1]]) if rng.integers(0, 3) == 0 else pts


def random_plane(rng, H, W):
    """A uint8 plane of text-line-like bars with stored values up to 255 (the rows are summed as stored)."""
    plane = np.zeros((H, W), np.uint8)
    y = int(rng.integers(0, 30))
    while y < H:
        t = int(rng.integers(1, 25))
        if rng.integers(0, 4):
            x0 = int(rng.integers(0, W))
            plane[y:y + t, x0:int(rng.integers(x0, W)) + 1] = rng.integers(1, 256) if rng.integers(0, 3) == 0 else 1
        y += t + int(rng.integers(1, 60))
    if rng.integers(0, 5) == 0:
        plane |= (rng.integers(0, 40, size=(H, W)) == 0).astype(np.uint8)
    return plane


def _rect(x0, y0, x1, y1, clockwise=False):
    pts = [[x0, y0], [x0, y1], [x1, y1], [x1, y0]]
    return np.array(pts[::-1] if clockwise else pts, np.int64).reshape(-1, 1, 2)      # the reference indexes [:, 0, 0]


def synthetic_cases():
    """Small (plane, contours) inputs of the order fixture (tests/golden/make_order_golden.py holds the reference's outputs for them)."""
    cases = []
    plane = np.zeros((300, 400), np.uint8)
    for y in (20, 120, 220):
        plane[y:y + 40, 10:390] = 1
    cases.append((plane, [_rect(260, 125, 380, 155), _rect(10, 225, 390, 255), _rect(10, 122, 120, 158, True), _rect(200, 22, 390, 58),
                          _rect(140, 124, 250, 156), _rect(10, 20, 190, 60, True)]))
    plane = np.zeros((90, 61), np.uint8)                         # text from the first row on, values up to 255, an odd width
    plane[0:14, 3:50] = 255
    plane[40:52, 3:50] = 7
    plane[75:90, 3:50] = 255                                     # ... and to the last row
    cases.append((plane, [_rect(3, 76, 50, 89), _rect(30, 41, 50, 51), _rect(3, 0, 50, 13), _rect(3, 40, 25, 52)]))
    rng = np.random.default_rng(1802)
    for _ in range(4):
        H, W = int(rng.integers(60, 500)), int(rng.integers(40, 300))
        plane = random_plane(rng, H, W)
        contours = []
        for _ in range(int(rng.integers(3, 10))):
            x0, y0 = int(rng.integers(0, W - 8)), int(rng.integers(0, H - 8))
            contours.append(_rect(x0, y0, int(rng.integers(x0 + 2, W)), int(rng.integers(y0 + 2, H)), bool(rng.integers(0, 2))))
        cases.append((plane, contours))
    return cases


def fixture_cases(golden_dir):
    """The (plane, contours) inputs of the order fixture, in its order: the textline planes of slopes_golden.npz with the reference's
    rings for their region maps from contours_golden.npz, then synthetic_cases()."""
    import os
    slopes = np.load(os.path.join(golden_dir, "slopes_golden.npz"))
    traced = np.load(os.path.join(golden_dir, "contours_golden.npz"))
    cases = []
    for j in range(int(traced["n"])):
        from_slopes, k = (int(v) for v in traced[f"source{j}"])
        if not from_slopes:
            continue
        h, w = (int(v) for v in slopes[f"shape{k}"])
        plane = np.unpackbits(slopes[f"textlines{k}"])[:h * w].reshape(h, w)
        at, rings = 0, []
        for length in traced[f"lengths{j}"]:
            rings.append(traced[f"points{j}"][at:at + int(length)].astype(np.uint).reshape(-1, 1, 2))
            at += int(length)
        cases.append((plane, rings))
    return cases + synthetic_cases()
