"""Reference restatement of OpenCV's border follower for OUTER borders (cv2.findContours, the part of icvFetchContour an outer border
takes), in numpy and plain Python, for CHAIN_APPROX_NONE and CHAIN_APPROX_SIMPLE [EXT, restated, unpinned like the rest of cv2].
Written from the description of the walk, with OpenCV's own direction codes; nothing here is imported from the product.

Direction code s: 0 = E, 1 = NE, 2 = N, 3 = NW, 4 = W, 5 = SW, 6 = S, 7 = SE -- counter-clockwise on the screen (y pointing down) as s
grows.  For the component of the first pixel i0 in raster order:

  * s = 4 (west); turn CLOCKWISE (s - 1) until a component pixel i1 is met or s is west again (a single pixel: one point);
  * i3 = i0, prev_s = s ^ 4.  Loop: from s (the direction that points back at the pixel the walk came from) turn COUNTER-CLOCKWISE
    (s + 1) until a component pixel i4 is met; NONE keeps i3, SIMPLE keeps i3 when s != prev_s; prev_s = s; stop when i4 == i0 and
    i3 == i1; else i3 = i4, s = s + 4.
"""
import numpy as np

_DX = (1, 1, 0, -1, -1, -1, 0, 1)           # OpenCV's icvCodeDeltas
_DY = (0, -1, -1, -1, 0, 1, 1, 1)


def follow_outer_border(comp, simple=True):
    """Points [(x, y), ...] of the outer border of the ONE 8-connected component ``comp`` (bool [H, W]) describes."""
    comp = np.asarray(comp, bool)
    H, W = comp.shape
    pad = np.zeros((H + 2, W + 2), bool)
    pad[1:-1, 1:-1] = comp
    ys, xs = np.nonzero(comp)
    i0 = (int(xs[0]), int(ys[0]))                            # np.nonzero is row-major: the first pixel in raster order

    def at(p, s):
        return (p[0] + _DX[s & 7], p[1] + _DY[s & 7])

    def inside(p):
        return bool(pad[p[1] + 1, p[0] + 1])
    s_end = s = 4
    while True:
        s = (s - 1) & 7
        i1 = at(i0, s)
        if inside(i1) or s == s_end:
            break
    if s == s_end:
        return [i0]
    out = []
    i3, prev_s = i0, s ^ 4
    for _ in range(8 * H * W + 8):
        while True:
            s += 1
            i4 = at(i3, s)
            if inside(i4):
                break
        s &= 7
        if not simple or s != prev_s:
            out.append(i3)
        prev_s = s
        if i4 == i0 and i3 == i1:
            return out
        i3 = i4
        s = (s + 4) & 7
    raise AssertionError("the border did not close")


def area2(points):
    """|doubled shoelace sum| of a closed ring of (x, y)."""
    p = np.asarray(points, np.int64).reshape(-1, 2)
    x, y = p[:, 0], p[:, 1]
    return abs(int(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y)))


def mask_contours(mask, simple=True):
    """What ``sbbseg_mask_contours_host`` must give for a raw mask (!= 0): per 8-connected component, by DESCENDING first pixel in raster
    order, (box [x, y, w, h], doubled area, points int32 [N, 2]).  scipy numbers components by first pixel in raster order."""
    from scipy import ndimage
    lab, n = ndimage.label(np.asarray(mask) != 0, structure=np.ones((3, 3), int))
    out = []
    for k in range(n, 0, -1):
        pts = follow_outer_border(lab == k, simple)
        chain = pts if not simple else follow_outer_border(lab == k, False)
        p = np.asarray(pts, np.int32).reshape(-1, 2)
        box = [int(p[:, 0].min()), int(p[:, 1].min()), int(p[:, 0].max() - p[:, 0].min() + 1), int(p[:, 1].max() - p[:, 1].min() + 1)]
        out.append((box, area2(chain), p, len(chain)))
    return out
