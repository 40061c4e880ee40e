"""Literal Python restatement of the contour half of ``textline_contours_postprocessing`` (main.py:1492-1511) and of the
``cv2.pointPolygonTest`` loop of ``seperate_lines`` (main.py:780-791), written from the OpenCV 4.5.1 text and NOT from csrc/line_extent.h
(tests/test_line_extent_cpu.py holds the library's host twin to it; tests/golden/make_line_extent_golden.py feeds it to the reference's own
functions as cv2 stubs).  Where the header reduces a rule to bit tricks, this file spells the rule out:

  * fill_poly: the drawn outline (every lattice point of every edge) plus a scanline even-odd fill with exact rational crossings;
  * threshrot: ``oracle.deskew.warp_affine_cubic_replicate`` on float64 (the float path) and numpy's OWN ``astype(np.uint8)``;
  * find_contours_tree: OpenCV's border follower with ITS direction numbering (0 = east, counter-clockwise) and ITS marks written into a
    signed image (1, 2, -126), every border in discovery order;
  * point_polygon_test: the measureDist loop with ``np.float32`` points and float64 arithmetic, returning the signed distance itself.

[EXT] cv2 is not installed anywhere this runs: all of this is unpinned against a real OpenCV.  Nothing here is product code."""
from fractions import Fraction

import numpy as np

from oracle import deskew as dk


def fill_poly(ring, w, h):
    """cv2.fillPoly(np.zeros((h, w)), [ring], 255) != 0 for a ring of int (x, y) points whose edges are horizontal, vertical or exact
    diagonals: uint8 [h, w] of 0 / 1."""
    ring = [(int(x), int(y)) for x, y in np.asarray(ring).reshape(-1, 2)]
    img = np.zeros((h, w), np.uint8)
    edges = list(zip(ring, ring[1:] + ring[:1]))
    for (x0, y0), (x1, y1) in edges:                 # the outline: Line() of an axis-parallel or diagonal segment is its lattice points
        steps = max(abs(x1 - x0), abs(y1 - y0))
        assert abs(x1 - x0) in (0, steps) and abs(y1 - y0) in (0, steps), "not a chain edge"
        for t in range(steps + 1):
            x = x0 + (0 if steps == 0 else (x1 - x0) // steps * t)
            y = y0 + (0 if steps == 0 else (y1 - y0) // steps * t)
            img[y, x] = 1
    for py in range(h):                              # the interior: even-odd over the crossings of the row, half-open in y
        xs = []
        for (x0, y0), (x1, y1) in edges:
            if y0 == y1 or not (min(y0, y1) <= py < max(y0, y1)):
                continue
            xs.append(Fraction(x0) + Fraction(py - y0) * Fraction(x1 - x0, y1 - y0))
        for px in range(w):
            if img[py, px] == 0 and sum(1 for x in xs if x < px) % 2 == 1:
                img[py, px] = 1
    return img


def threshrot(filled, slope):
    """main.py:1503-1507 on one channel: rotate_image (float64), .astype(np.uint8), threshold(., 0, 255, 0): uint8 [h, w] of 0 / 255."""
    rot = dk.rotate_image(filled.astype(np.float64) * 255.0, slope)
    with np.errstate(invalid="ignore"):
        cast = rot.astype(np.uint8)
    return np.where(cast > 0, 255, 0).astype(np.uint8)


# OpenCV's CV_INIT_3X3_DELTAS order: 0 = E, 1 = NE, 2 = N, 3 = NW, 4 = W, 5 = SW, 6 = S, 7 = SE (x, y with y pointing down)
_DELTAS = [(1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1)]


def _fetch_contour(img, x, y, is_hole):
    """icvFetchContour(..., CV_CHAIN_APPROX_SIMPLE) at padded coordinates (x, y): the kept points, marks written into img."""
    nbd = 2
    pts = []
    s_end = s = 0 if is_hole else 4
    while True:
        s = (s - 1) & 7
        i1 = (x + _DELTAS[s][0], y + _DELTAS[s][1])
        if img[i1[1], i1[0]] != 0 or s == s_end:
            break
    if s == s_end:                                   # single pixel domain
        img[y, x] = nbd - 128
        return [(x - 1, y - 1)]
    i0 = (x, y)
    i3 = i0
    prev_s = s ^ 4
    while True:
        s_end = s
        while s < 15:
            s += 1
            i4 = (i3[0] + _DELTAS[s & 7][0], i3[1] + _DELTAS[s & 7][1])
            if img[i4[1], i4[0]] != 0:
                break
        s &= 7
        if ((s - 1) & 0xffffffff) < s_end:           # (unsigned)(s - 1) < (unsigned)s_end: the "right" bound
            img[i3[1], i3[0]] = nbd - 128
        elif img[i3[1], i3[0]] == 1:
            img[i3[1], i3[0]] = nbd
        if s != prev_s:
            pts.append((i3[0] - 1, i3[1] - 1))
            prev_s = s
        if i4 == i0 and i3 == i1:
            break
        i3 = i4
        s = (s + 4) & 7
    return pts


def find_contours_tree(mask):
    """Every border cv2.findContours(mask, RETR_TREE, CHAIN_APPROX_SIMPLE) follows, in DISCOVERY order: a list of (is_hole, int [N, 2])."""
    mask = np.asarray(mask) != 0
    h, w = mask.shape
    img = np.zeros((h + 2, w + 2), np.int16)         # (int16 holding schar values: 0, 1, 2, -126)
    img[1:-1, 1:-1] = mask
    out = []
    for y in range(1, h + 1):
        x = 1
        prev = int(img[y, 0])
        while x < w + 1:                             # the scanner's width excludes the rightmost (padding) column
            p = int(img[y, x])
            if p != prev:
                is_hole = False
                follow = True
                if not (prev == 0 and p == 1):
                    if p != 0 or prev < 1:
                        follow = False
                    is_hole = True
                if follow:
                    pts = _fetch_contour(img, x - (1 if is_hole else 0), y, is_hole)
                    out.append((is_hole, np.array(pts, np.int64).reshape(-1, 2)))
                    prev = int(img[y, x])            # cvFindNextContour is re-entered at x + 1 and reads prev = img[x] afresh
                    x += 1
                    continue
            prev = p
            x += 1
    return out


def winner(borders):
    """np.argmax of the point counts over the list as cv2 returns it -- REVERSE discovery order [EXT, assumed] -- as an index into
    ``borders`` (discovery order), and whether the maximum is shared.  None: no border (np.argmax([]) raises)."""
    if not borders:
        return None, False
    counts = [len(b[1]) for b in borders][::-1]
    k = int(np.argmax(counts))
    return len(borders) - 1 - k, counts.count(counts[k]) > 1


def point_polygon_test(contour, pt):
    """cv2.pointPolygonTest(contour (int points), pt, True): the signed distance as float64."""
    cnt = np.asarray(contour).reshape(-1, 2)
    total = cnt.shape[0]
    ptx, pty = np.float32(pt[0]), np.float32(pt[1])
    if total == 0:
        return -np.finfo(np.float64).max
    min_dist_num, min_dist_denom, counter = float(np.finfo(np.float32).max), 1.0, 0
    vx, vy = np.float32(cnt[-1, 0]), np.float32(cnt[-1, 1])
    for i in range(total):
        v0x, v0y = vx, vy
        vx, vy = np.float32(cnt[i, 0]), np.float32(cnt[i, 1])
        dx, dy = float(vx - v0x), float(vy - v0y)            # Point2f differences (float32), then held in doubles
        dx1, dy1 = float(ptx - v0x), float(pty - v0y)
        dx2, dy2 = float(ptx - vx), float(pty - vy)
        dist_denom = 1.0
        if dx1 * dx + dy1 * dy <= 0:
            dist_num = dx1 * dx1 + dy1 * dy1
        elif dx2 * dx + dy2 * dy >= 0:
            dist_num = dx2 * dx2 + dy2 * dy2
        else:
            dist_num = dy1 * dx - dx1 * dy
            dist_num *= dist_num
            dist_denom = dx * dx + dy * dy
        if dist_num * min_dist_denom < min_dist_num * dist_denom:
            min_dist_num, min_dist_denom = dist_num, dist_denom
            if min_dist_num == 0:
                break
        if (v0y <= pty and vy <= pty) or (v0y > pty and vy > pty):
            continue
        dist_num = dy1 * dx - dx1 * dy
        if dy < 0:
            dist_num = -dist_num
        counter += dist_num > 0
    result = float(np.sqrt(min_dist_num / min_dist_denom))
    return -result if counter % 2 == 0 else result


def line_extent(contour, w, peak):
    """main.py:780-791: (int(x_min), int(x_max)) of one line."""
    xv = np.linspace(0, w, 1000)
    distances = np.array([point_polygon_test(contour, (xv[mj], peak)) for mj in range(len(xv))])
    xvinside = xv[distances >= 0]
    if len(xvinside) == 0:
        return 0, w
    return int(np.min(xvinside)), int(np.max(xvinside))


def region(ring, box, slope, record, rot):
    """The whole step for one region: the fields of ``_capi.host_region_line_extents``'s record that the step decides."""
    x, y, w, h = (int(v) for v in box)
    local = np.asarray(ring).reshape(-1, 2).astype(np.int64) - np.array([x, y])
    filled = fill_poly(local, w, h)
    thr = threshrot(filled, slope)
    borders = find_contours_tree(thr)
    k, tie = winner(borders)
    out = dict(threshrot=thr, borders=len(borders), holes=sum(1 for b in borders if b[0]))
    if k is None:
        out.update(status=1, winner=np.zeros((0, 2), np.int64), is_hole=False, tie=False, extent=np.zeros((0, 2), np.int64),
                   boxes=np.zeros((0, 4, 2), np.int64), boxes_rot=np.zeros((0, 4, 2), np.int64))
        return out
    out.update(status=0, winner=borders[k][1], is_hole=bool(borders[k][0]), tie=tie)
    n = len(record["peaks"])
    extent = np.tile(np.array([0, w], np.int64), (n, 1))
    boxes, boxes_rot = np.array(record["boxes"], np.int64).reshape(n, 4, 2), np.array(record["boxes_rot"], np.int64).reshape(n, 4, 2)
    if abs(slope) <= 45 and record["branch"] != 2:
        a, b, c, d, x_d, y_d = rot
        for jj in range(n):
            x_min, x_max = line_extent(borders[k][1], w, int(record["peaks"][jj]))
            up, down = int(record["point_up"][jj]), int(record["point_down"][jj])
            extent[jj] = (x_min, x_max)
            p = [np.dot(np.array([[a, b], [c, d]]), [px, py]) for px, py in ((x_min, up), (x_max, up), (x_max, down), (x_min, down))]
            xr = [q[0] + x_d for q in p]
            yr = [q[1] + y_d for q in p]
            if xr[0] < 0:                            # x_min_rot1, x_min_rot4, point_up_rot1, point_up_rot2 (main.py:803-810)
                xr[0] = 0
            if xr[3] < 0:
                xr[3] = 0
            if yr[0] < 0:
                yr[0] = 0
            if yr[1] < 0:
                yr[1] = 0
            boxes_rot[jj] = [[int(xr[i]), int(yr[i])] for i in range(4)]
            boxes[jj] = [[x_min, up], [x_max, up], [x_max, down], [x_min, down]]
    out.update(extent=extent, boxes=boxes, boxes_rot=boxes_rot)
    return out
