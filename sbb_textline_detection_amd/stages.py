"""The three stage wrappers that call the hot path and the steps either side of
it that section 8(f) ranks next, with the reference's names and call pattern:

    get_image_and_scales            main.py:196-214   upscale rule (2800 px high, or x1.2), INTER_NEAREST
    otsu_copy                       main.py:178-194   per-channel Otsu, channel-0 result in all 3 channels (quirk kept)
    extract_page   (model part)     main.py:384-392   border model, patches=False
    extract_text_regions            main.py:439-454   Otsu'd page, layout model (4 classes), patches=True
    textline_contours               main.py:490-503   textline model, patches=True, returns channel 0

    extract_page   (glue part)      main.py:394-426   border mask -> dilate x 6 -> largest blob -> box -> crop (device)
    erode x 3 / dilate x 4          main.py:2074-2075 on the layout map (device)

    return_deskew_slope             main.py:1601-1718 the deskew search of ONE region: rotate-and-project on the device (one launch
                                                      per sweep), the 1-D peak logic on the host with the reference's own scipy calls

    get_text_region_contours_and_boxes  main.py:456-480   the BOXES of the text regions (``self.boxes``), on the device
    do_work_of_slopes (slope half)  main.py:1721-1748 one deskew slope per box: crop, erode x 2 and the rotate-and-project of ALL boxes in
                                                      one batched sweep on the device (``get_slopes``), the peak logic (Gaussian, find_peaks,
                                                      std) and the angle selection on the device too (``statistics="host"``: scipy)
    textline_contours_postprocessing (mask half)  main.py:1472-1487 per box: crop * 255, OPEN, CLOSE, rotate_image by the box's slope, != 0
                                                      -- ``dst``, and the row / column sums the line splitters open on (main.py:539, 1020), for
                                                      ALL boxes in one batched pass on the device (``get_line_masks``)

Out of scope: the contour half of textline_contours_postprocessing (main.py:1492-1511), seperate_lines / seperate_lines_vertical after
their projection, the polygons, the reading order and PAGE-XML.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from .model import SegModel, start_new_session_and_model
from .predict import do_prediction


def scaled_size(h: int, w: int) -> Tuple[int, int]:
    """main.py:201-207: pages under 2500 px go to 2800 px height, everything else x1.2 (aspect kept)."""
    if h < 2500:
        hi = 2800
    else:
        hi = int(h * 1.2)
    return hi, int(hi * w / float(h))


def otsu_threshold_u8(ch: np.ndarray) -> int:
    """cv2.threshold(..., THRESH_BINARY + THRESH_OTSU) threshold value [EXT: OpenCV getThreshVal_Otsu_8u]:
    mean from the integer first moment times 1/N, probabilities h[i] * (1/N), strict `>` (first maximum).
    Host mirror of the device kernel (csrc/page_glue.hip otsu_threshold_kernel), for foreign model objects."""
    h = np.bincount(np.ascontiguousarray(ch, np.uint8).reshape(-1), minlength=256)
    scale = 1.0 / float(h.sum())
    mu = 0.0
    for i in range(256):
        mu += float(i) * float(h[i])
    mu *= scale
    q1 = mu1 = best_sigma = 0.0
    best = 0
    eps = float(np.finfo(np.float32).eps)
    for i in range(256):
        p_i = float(h[i]) * scale
        mu1 *= q1
        q1 += p_i
        q2 = 1.0 - q1
        if min(q1, q2) < eps or max(q1, q2) > 1.0 - eps:
            continue
        mu1 = (mu1 + float(i) * p_i) / q1
        mu2 = (mu - q1 * mu1) / q2
        d = mu1 - mu2
        sigma = q1 * q2 * d * d
        if sigma > best_sigma:
            best_sigma, best = sigma, i
    return best


def otsu_copy(img: np.ndarray) -> np.ndarray:
    """main.py:178-194.  Thresholds of all three channels are computed, but the channel-0 result is
    written to all three output channels (reference quirk, lines 191-193).  float64 HxWx3, values 0/255."""
    t = otsu_threshold_u8(np.ascontiguousarray(img[:, :, 0], np.uint8))
    b = np.where(img[:, :, 0] > t, 255.0, 0.0)
    return np.repeat(b[:, :, None], 3, axis=2)


def host_morph(plane: np.ndarray, is_max: bool, ksize: int, iterations: int) -> np.ndarray:
    """Host mirror of sbbseg_morph (foreign model objects only): one clipped (n(k-1)+1)-wide separable min / max."""
    r = (ksize - 1) // 2 * iterations
    a = np.ascontiguousarray(plane, np.uint8)
    fill = 0 if is_max else 255
    f = np.maximum if is_max else np.minimum
    for axis in (1, 0):
        p = np.pad(a, [(r, r) if ax == axis else (0, 0) for ax in (0, 1)], constant_values=fill)
        out = np.full_like(a, fill)
        for d in range(2 * r + 1):
            out = f(out, p[:, d:d + a.shape[1]] if axis == 1 else p[d:d + a.shape[0], :])
        a = out
    return a


def host_page_box(mask: np.ndarray):
    """Host mirror of sbbseg_page_box_dev (foreign model objects only): dilate x 6, then the component whose outer contour has
    the largest cv2.contourArea, traced by the library's host code (``sbbseg_debug_largest_contour``: no GPU involved)."""
    d = host_morph(np.where(np.asarray(mask) > 0, 255, 0).astype(np.uint8), True, 5, 6)
    from . import _capi
    return _capi.host_largest_contour(d)


def host_text_regions_present(regions: np.ndarray, label: int = 1, min_area: float = 0.00001) -> bool:
    """Host mirror of sbbseg_text_regions_present_dev (foreign model objects only; main.py:456-480): class mask -> OPEN -> CLOSE ->
    the largest outer-contour area (the library's host tracer, no GPU) >= min_area x H x W."""
    a = np.asarray(regions)
    m = np.all(a == label, axis=-1) if a.ndim == 3 else a == label
    p = np.where(m, 255, 0).astype(np.uint8)
    p = host_morph(host_morph(p, False, 5, 1), True, 5, 2)             # OPEN's erode + dilate, CLOSE's dilate ...
    p = host_morph(p, False, 5, 1)                                     # ... and erode
    if not p.any():
        return False
    from . import _capi
    return _capi.host_largest_contour_area2(p) * 0.5 >= min_area * float(p.shape[0] * p.shape[1])


def _host_parentless_components(regions: np.ndarray, label: int):
    """The front end of the two host mirrors below: class mask -> OPEN -> CLOSE, scipy's 8-connected labels (numbered by first pixel in
    raster order), which of them have no parent (4-adjacent to the background connected to the frame), and their slices."""
    from scipy import ndimage
    a = np.asarray(regions)
    m = np.all(a == label, axis=-1) if a.ndim == 3 else a == label
    p = np.where(m, 255, 0).astype(np.uint8)
    p = host_morph(host_morph(p, False, 5, 1), True, 5, 2)             # OPEN's erode + dilate, CLOSE's dilate ...
    p = host_morph(p, False, 5, 1)                                     # ... and erode
    lab, n = ndimage.label(p > 0, structure=np.ones((3, 3), int))      # numbered by first pixel in raster order
    back, _ = ndimage.label(np.pad(p == 0, 1, constant_values=True))   # 4-connected background, with the frame around the image
    outer = back == back[0, 0]
    beside = outer[1:-1, :-2] | outer[1:-1, 2:] | outer[:-2, 1:-1] | outer[2:, 1:-1]
    parentless = np.zeros(n + 1, bool)
    parentless[np.unique(lab[beside & (lab > 0)])] = True
    return lab, parentless, ndimage.find_objects(lab)


def host_text_region_boxes(regions: np.ndarray, label: int = 1, min_area: float = 0.00001, max_area: float = 1.0):
    """Host mirror of sbbseg_text_region_boxes_dev (foreign model objects, CPU-only checks; main.py:456-480): class mask -> OPEN -> CLOSE ->
    [x, y, w, h] of every 8-connected component that is 4-adjacent to the background connected to the frame (no parent) and whose
    outer-contour area (the library's host tracer, no GPU) lies in [min_area, max_area] x H x W.  Order [EXT, unpinned]: first pixel in
    raster order, descending -- the reverse discovery order assumed for cv2.findContours' list."""
    from . import _capi
    lab, parentless, slices = _host_parentless_components(regions, label)
    lo, hi = min_area * float(lab.shape[0] * lab.shape[1]), max_area * float(lab.shape[0] * lab.shape[1])
    boxes = []
    for k, sl in reversed(list(enumerate(slices, start=1))):
        if not parentless[k]:
            continue
        area = _capi.host_largest_contour_area2(np.where(lab[sl] == k, 255, 0).astype(np.uint8)) * 0.5
        if lo <= area <= hi:
            boxes.append([sl[1].start, sl[0].start, sl[1].stop - sl[1].start, sl[0].stop - sl[0].start])
    return boxes


def host_text_region_contours(regions: np.ndarray, label: int = 1, min_area: float = 0.00001, max_area: float = 1.0):
    """Host mirror of sbbseg_text_region_contours_dev (foreign model objects, CPU-only checks; main.py:456-481): the same components as
    ``host_text_region_boxes``, each traced by the library's host tracer (``sbbseg_mask_contours_host``, no GPU) and kept when it has at
    least three points and its area lies in the window.  Returns ``(boxes, contours)``: [[x, y, w, h], ...] and one int32 [N, 2] array of
    (x, y) per box, CHAIN_APPROX_SIMPLE points in OpenCV's order."""
    from . import _capi
    lab, parentless, slices = _host_parentless_components(regions, label)
    lo, hi = min_area * float(lab.shape[0] * lab.shape[1]), max_area * float(lab.shape[0] * lab.shape[1])
    boxes, contours = [], []
    for k, sl in reversed(list(enumerate(slices, start=1))):
        if not parentless[k]:
            continue
        (box,), area2, _, pts = _capi.mask_contours_host_tables(np.where(lab[sl] == k, 255, 0).astype(np.uint8))
        if len(pts) >= 3 and lo <= int(area2[0]) * 0.5 <= hi:
            boxes.append([int(box[0]) + sl[1].start, int(box[1]) + sl[0].start, int(box[2]), int(box[3])])
            contours.append(pts + np.array([sl[1].start, sl[0].start], np.int32))
    return boxes, contours


def closed_rings(contours):
    """The contours as the reference's filter_contours_area_of_image returns them (main.py:85-90): ``np.uint`` [N + 1, 1, 2], the ring
    of ``polygon.exterior.coords`` -- the first point repeated at the end."""
    return [np.concatenate([c, c[:1]]).astype(np.uint).reshape(-1, 1, 2) for c in contours]


def _profile_statistics(y: np.ndarray, sigma: float, multiplier: float):
    """get_standard_deviation_of_summed_textline_patch_along_width (main.py:1545-1599) from the row sums on: smoothed profile z,
    its maxima and the minima of the padded, negated profile (scipy, as the reference), the "deep" minima below
    mean(maxima > 10) * (1 - 1/multiplier), and std(z)."""
    from scipy.ndimage import gaussian_filter1d
    from scipy.signal import find_peaks
    y = np.asarray(y, np.float64)
    padded = np.zeros(len(y) + 20)
    padded[10:10 + len(y)] = y
    flipped = np.zeros(len(padded) + 20)
    flipped[10:10 + len(padded)] = padded.max() - padded
    z = gaussian_filter1d(y, sigma)
    minima = find_peaks(gaussian_filter1d(flipped, sigma), height=0)[0] - 20
    maxima = find_peaks(z, height=0)[0]
    tops = z[maxima]
    tops = tops[tops > 10]
    lows = z[minima]                                        # IndexError for a minimum in the right-hand padding: caller's except
    with np.errstate(all="ignore"):
        level = np.mean(tops) if tops.size else np.float64("nan")
    return lows[lows < level - level / multiplier], np.std(z)


def _deskew_sweep(profiles: np.ndarray, angles: np.ndarray, sigma: float) -> float:
    """One angle loop of return_deskew_slope (main.py:1630-1667): std of the smoothed profile per angle, arg max.  Kept: an angle
    without deep minima (their mean is NaN) is left out of the list, and the winner's position in the SHORTENED list indexes
    the full angle array (main.py:1655-1665)."""
    spread = []
    for k in range(len(angles)):
        try:
            lows, sd = _profile_statistics(profiles[k], sigma, 20.3)
            if lows.size == 0:
                continue                                    # np.mean([]) is NaN -> the reference skips the append
        except Exception:                                   # main.py:1652-1655
            sd = 0
        spread.append(sd)
    return float(angles[int(np.argmax(np.array(spread)))]) if spread else 0.0


def return_deskew_slope(img_patch: np.ndarray, sigma_des: float, ctx=None) -> float:
    """``textline_detector.return_deskew_slope`` (main.py:1601-1718): the rotation angle, out of 80 in [-25, 25] (and 30 in
    [-90, -50] when the first answer is steeper than 15 degrees), whose row profile of the rotated region mask varies most.
    The reference rotates the padded mask 80-110 times with cv2.warpAffine on the CPU (and forks cpu_count() processes over
    the regions, main.py:1760-1799); here one sweep is ONE launch (``sbbseg_deskew_profiles``).  ``ctx``: a
    ``_capi.Context`` (any finalized handle: the call does not touch the network)."""
    if ctx is None:
        raise RuntimeError("return_deskew_slope needs a library handle (SegModel.ctx): there is no CPU fallback")
    mask = np.ascontiguousarray(np.asarray(img_patch) != 0, np.uint8) if np.asarray(img_patch).dtype != np.uint8 else np.ascontiguousarray(img_patch)
    angles = np.linspace(-25, 25, 80)                                              # main.py:1622
    ang = _deskew_sweep(ctx.deskew_profiles(mask, angles), angles, sigma_des)
    if abs(ang) > 15:                                                              # main.py:1669-1670
        angles = np.linspace(-90, -50, 30)
        ang = _deskew_sweep(ctx.deskew_profiles(mask, angles), angles, sigma_des)
    return ang


def get_slopes(textline_mask: np.ndarray, boxes, ctx=None, sigma_des: float = 2, statistics: str = "device"):
    """The slope half of ``do_work_of_slopes`` (main.py:1728-1748) for all boxes of a page: a list of float, one per box.  The textline
    map is uploaded once; crop, ``cv2.erode(crop, kernel, iterations=2)`` and the 80 rotations of every box run as ONE batched sweep on the
    device, a second batched sweep of 30 angles covers only the boxes whose first answer is steeper than 15 degrees (main.py:1669-1670).
    Then the reference's clean-up: a failed search (its 999) and |slope| > 120.5 become 0 (main.py:1744-1747).
    ``statistics="device"`` (default): the peak logic and the angle selection run on the device too (``sbbseg_region_deskew_slopes_dev``:
    the row counts never leave it, only the winners come back), with float64 results equal bit for bit to scipy's.  ``statistics="host"``:
    the row counts are copied back (``sbbseg_region_deskew_profiles_dev``) and the peak logic runs per region on the host with the
    reference's own scipy calls (``_deskew_sweep``) -- the A/B path and the tests' yardstick; same slopes.
    ``ctx``: a ``_capi.Context`` (any finalized handle)."""
    if statistics not in ("device", "host"):
        raise ValueError("statistics must be 'device' or 'host', not %r" % (statistics,))
    if ctx is None:
        raise RuntimeError("get_slopes needs a library handle (SegModel.ctx): there is no CPU fallback")
    plane = np.ascontiguousarray(textline_mask, np.uint8)
    boxes = [[int(v) for v in b] for b in boxes]
    if not boxes:
        return []
    d_plane = ctx.stage(plane)
    if statistics == "device":
        from . import _capi
        weights = None if sigma_des == 2 else _capi.gaussian_weights(sigma_des)          # (the library carries the table of sigma = 2)
        return ctx.region_deskew_slopes_dev(d_plane, plane.shape[0], plane.shape[1], boxes, 2, weights)

    def sweep(which, angles):
        found = {}
        profiles = ctx.region_deskew_profiles_dev(d_plane, plane.shape[0], plane.shape[1], [boxes[r] for r in which], angles, 2)
        for r, prof in zip(which, profiles):
            try:
                found[r] = _deskew_sweep(prof, angles, sigma_des)
            except Exception:                                       # main.py:1739-1740
                found[r] = 999
        return found
    slopes = sweep(list(range(len(boxes))), np.linspace(-25, 25, 80))                          # main.py:1622
    steep = [r for r, ang in slopes.items() if ang != 999 and abs(ang) > 15]                   # main.py:1669-1670
    if steep:
        slopes.update(sweep(steep, np.linspace(-90, -50, 30)))
    return [0 if (ang == 999 or abs(ang) > 120.5) else ang for ang in (slopes[r] for r in range(len(boxes)))]


def _line_masks_args(textline_mask, boxes, slopes, ctx, name):
    if ctx is None:
        raise RuntimeError(name + " needs a library handle (SegModel.ctx): there is no CPU fallback")
    plane = np.ascontiguousarray(textline_mask, np.uint8)
    boxes = [[int(v) for v in b] for b in boxes]
    if slopes is not None and len(slopes) != len(boxes):
        raise ValueError("one slope per box: %d boxes, %d slopes" % (len(boxes), len(slopes)))
    return plane, boxes


def get_line_masks(textline_mask: np.ndarray, boxes, slopes, ctx=None, masks: bool = True):
    """The mask half of ``textline_contours_postprocessing`` (main.py:1472-1487) as ``do_work_of_slopes`` calls it (main.py:1750) for all
    boxes of a page: a list, one entry per box, of ``(dst, rows, cols)``.  ``dst`` (uint8 [h, w] of 0 / 1; None with ``masks=False``) is
    the box's textline crop, eroded x 2, * 255, opened and closed with the 5 x 5 kernel, rotated by the box's slope (``rotate_image``:
    OpenCV's fixed-point bicubic on uint8) and binarised; ``rows`` = ``dst.sum(axis=1)`` (int64 [h]) is what ``seperate_lines`` opens on,
    ``cols`` = ``dst.sum(axis=0)`` (int64 [w]) what ``seperate_lines_vertical`` opens on -- the caller picks by ``abs(slope) > 45``
    (main.py:1514).  The textline map is uploaded once; all boxes run in a fixed number of launches (``sbbseg_region_line_masks_dev``).
    ``slopes``: what ``get_slopes`` returned for these boxes.  ``ctx``: a ``_capi.Context`` (any finalized handle)."""
    plane, boxes = _line_masks_args(textline_mask, boxes, slopes, ctx, "get_line_masks")
    if not boxes:
        return []
    return ctx.region_line_masks_dev(ctx.stage(plane), plane.shape[0], plane.shape[1], boxes, [float(s) for s in slopes], 2, masks)


def get_slopes_and_line_masks(textline_mask: np.ndarray, boxes, ctx=None, sigma_des: float = 2, masks: bool = True):
    """``get_slopes`` (statistic on the device) and ``get_line_masks`` with the slopes it found, the textline map staged ONCE for both:
    (slopes, line masks)."""
    plane, boxes = _line_masks_args(textline_mask, boxes, None, ctx, "get_slopes_and_line_masks")
    if not boxes:
        return [], []
    from . import _capi
    d_plane = ctx.stage(plane)
    weights = None if sigma_des == 2 else _capi.gaussian_weights(sigma_des)
    slopes = ctx.region_deskew_slopes_dev(d_plane, plane.shape[0], plane.shape[1], boxes, 2, weights)
    return slopes, ctx.region_line_masks_dev(d_plane, plane.shape[0], plane.shape[1], boxes, slopes, 2, masks)


def get_line_extents(boxes, slopes, records, contours, ctx=None):
    """The contour half of ``textline_contours_postprocessing`` (main.py:1492-1511) and its consumer, ``cv2.pointPolygonTest`` inside
    ``seperate_lines``: per box its ring (``get_text_region_contours``'s, page coordinates) is filled, rotated by the box's slope, cast and
    thresholded as the reference does it, the border with the most points is found among ALL borders of that image, and every line of
    the horizontal splitter is cut to it: x_min / x_max of the 1000 samples of the peak row that lie inside.  ``records``: what
    ``get_line_boxes`` returned for these boxes.  Returns the records with ``boxes`` / ``boxes_rot`` rewritten (branches 0, 3, 4; branch 2
    and the vertical splitter keep 0 .. w), ``extent`` int32 [lines, 2] and ``contour`` (the winner's record); a region whose rotated
    contour has no border at all has no lines, as the reference's bare except leaves it.  All boxes share the launches on the device with
    a ``ctx`` (``sbbseg_region_line_extents_dev``); without one the library's serial host twin runs box by box: the same bits."""
    from . import _capi
    boxes = [[int(v) for v in b] for b in boxes]
    if not (len(boxes) == len(slopes) == len(records) == len(contours)):
        raise ValueError("one slope, one record and one ring per box: %d boxes, %d slopes, %d records, %d rings"
                         % (len(boxes), len(slopes), len(records), len(contours)))
    if not boxes:
        return []
    if ctx is not None:
        return ctx.region_line_extents_dev(boxes, [float(s) for s in slopes], records, contours)
    return [_capi.host_region_line_extents(c, b, float(s), r) for c, b, s, r in zip(contours, boxes, slopes, records)]


def get_line_boxes(textline_mask: np.ndarray, boxes, slopes, ctx=None, contours=None):
    """What ``textline_contours_postprocessing`` (main.py:1472-1524) gets from ``seperate_lines`` / ``seperate_lines_vertical`` for all
    boxes of a page: ``get_line_masks``' steps and then the splitter of every box on its own projection, the projections staying on the
    device (``sbbseg_region_line_boxes_dev``).  One record per box (``_capi.line_split_host``): status, sigma, raised, branch, peaks,
    point_up, point_down, boxes, boxes_rot; ``boxes_rot`` is the reference's ``textline_boxes_rot``, [] where it returns [].
    ``contours``: one ring per box (``get_text_region_contours``) -- the lines are then cut to the region's filled, rotated contour
    (``get_line_extents``), which is what the reference returns.  Without it (the default) every line has the reference's FALLBACK x
    extent 0 .. w (main.py:786-788)."""
    plane, boxes = _line_masks_args(textline_mask, boxes, slopes, ctx, "get_line_boxes")
    if not boxes:
        return []
    records = ctx.region_line_boxes_dev(ctx.stage(plane), plane.shape[0], plane.shape[1], boxes, [float(s) for s in slopes], 2)
    return records if contours is None else get_line_extents(boxes, slopes, records, contours, ctx)


def get_slopes_and_line_boxes(textline_mask: np.ndarray, boxes, ctx=None, sigma_des: float = 2):
    """``get_slopes`` and ``get_line_boxes`` with the slopes it found, the textline map staged ONCE for both: (slopes, line records)."""
    plane, boxes = _line_masks_args(textline_mask, boxes, None, ctx, "get_slopes_and_line_boxes")
    if not boxes:
        return [], []
    from . import _capi
    d_plane = ctx.stage(plane)
    weights = None if sigma_des == 2 else _capi.gaussian_weights(sigma_des)
    slopes = ctx.region_deskew_slopes_dev(d_plane, plane.shape[0], plane.shape[1], boxes, 2, weights)
    return slopes, ctx.region_line_boxes_dev(d_plane, plane.shape[0], plane.shape[1], boxes, slopes, 2)


def _order_result(rec):
    """(indexes_sorted, matrix_of_orders) of order_of_regions from the library's record (``_capi.host_region_order``)."""
    n = rec["band"].shape[0]
    matrix = np.zeros((n, 5))
    matrix[:, 0] = np.arange(n)
    matrix[:, 1] = 1
    matrix[:, 2:4] = rec["centroids"]
    matrix[:, 4] = np.arange(n)
    kept = int(np.count_nonzero(rec["band"] >= 0))               # a region in no band is left out, as the reference's masks leave it out
    return [int(v) for v in rec["sorted_index"][:kept]], matrix


def order_of_regions(textline_mask: np.ndarray, contours, ctx=None):
    """order_of_regions (main.py:1802-1889): ``(indexes_sorted, matrix_of_orders)`` as the reference returns them -- the region indices
    band by band (bands: between the minima of the smoothed row profile of ``textline_mask``), by ascending cx inside a band, and the
    float64 [n, 5] matrix {m, 1, cx, cy, m}.  ``contours``: the reference's rings ([N, 1, 2]) or [N, 2] point arrays; the region order is
    that of the list.  cx ties [EXT] by ascending index.  On the device with a ``ctx`` (``sbbseg_region_order``), else the library's
    serial host twin: the same bits."""
    from . import _capi
    mask = np.asarray(textline_mask)
    rec = ctx.region_order(mask, contours) if ctx is not None else _capi.host_region_order(mask, contours)
    return _order_result(rec)


def order_and_id_of_texts(found_polygons_text_region, matrix_of_orders, indexes_sorted):
    """order_and_id_of_texts (main.py:1894-1906): ``(order_of_texts, id_of_texts)`` -- per region its position in ``indexes_sorted`` and
    'r' + its index.  A region ``indexes_sorted`` does not hold raises IndexError, as the reference's ``np.where(...)[0][0]`` does."""
    matrix_of_orders = np.asarray(matrix_of_orders)
    position = {}
    for at, index in enumerate(indexes_sorted):
        position.setdefault(int(index), at)
    order_of_texts, id_of_texts = [], []
    for mm in range(len(found_polygons_text_region)):
        id_of_texts.append('r' + str(mm))
        rows = matrix_of_orders[:, 0][(matrix_of_orders[:, 1] == 1) & (matrix_of_orders[:, 4] == mm)]
        if rows.shape[0] != 1 or int(rows[0]) not in position:
            raise IndexError("index 0 is out of bounds for axis 0 with size 0")
        order_of_texts.append(position[int(rows[0])])
    return order_of_texts, id_of_texts


class InferenceStages:
    """The model-running part of ``textline_detector.run()`` (main.py:2056-2107)."""

    def __init__(self, model_page_dir: str, model_region_dir: str, model_textline_dir: str, device: int = 0,
                 model_kwargs: Optional[dict] = None):
        self.model_page_dir, self.model_region_dir, self.model_textline_dir = model_page_dir, model_region_dir, model_textline_dir
        self.kw = dict(model_kwargs or {}, device=device)
        self.image = None
        self.scale_y = self.scale_x = 1.0

    def get_image_and_scales(self, image_u8: np.ndarray) -> None:
        """Records the upscaled geometry (main.py:196-214).  The upscaled page itself is not built:
        the tile gather reads the stored page through the nearest-neighbour index tables."""
        self.image_stored = np.ascontiguousarray(image_u8, np.uint8)
        h, w = image_u8.shape[:2]
        self.img_hight_int, self.img_width_int = scaled_size(h, w)
        self.scale_y = self.img_hight_int / float(h)
        self.scale_x = self.img_width_int / float(w)

    def _scaled_page(self):
        from .predict import resize_nearest
        return resize_nearest(self.image_stored, self.img_hight_int, self.img_width_int)

    def extract_page_mask(self) -> np.ndarray:
        """Border model on the whole page (main.py:384-392): uint8 [H,W,3] at the *scaled* size."""
        model, session = start_new_session_and_model(self.model_page_dir, **self.kw)
        try:
            if isinstance(model, SegModel):
                # stored page -> (virtual) upscaled page -> model size: the two nearest maps are composed on the
                # library side, the 4200x3000 page is never built on the host
                return model.ctx.segment_whole_scaled(self.image_stored, self.img_hight_int, self.img_width_int,
                                                      self.img_hight_int, self.img_width_int, channels=3)
            img = self._scaled_page()
            return do_prediction(False, img, model, full_image_shape=img.shape)
        finally:
            session.close()

    def extract_page(self):
        """main.py:384-437: border model + page box + crop.  Returns (croped_page, page_coord) like the reference;
        ``self.cont_page`` holds the box corners.  The mask never leaves the device between the model and the box.
        Like the reference, an empty border mask is an error (np.argmax of an empty list raises there, main.py:399-401)."""
        model, session = start_new_session_and_model(self.model_page_dir, **self.kw)
        try:
            if isinstance(model, SegModel):
                self.page_mask, box, pixels = model.ctx.extract_page_box(self.image_stored, self.img_hight_int, self.img_width_int, channels=3)
            else:
                from .predict import resize_nearest
                img = self._scaled_page()
                self.page_mask = do_prediction(False, img, model, full_image_shape=img.shape)
                box, pixels = host_page_box(self.page_mask[:, :, 0])
            if pixels == 0:
                raise ValueError("attempt to get argmax of an empty sequence")          # what main.py:401 raises
            x, y, w, h = box
            self.page_box = (x, y, w, h)
            # crop_image_inside_box (main.py:174-176) on the upscaled page; built here only for the crop
            page = self._scaled_page()
            croped_page, page_coord = page[y:y + h, x:x + w], [y, y + h, x, x + w]
            self.cont_page = [np.array([[page_coord[2], page_coord[0]], [page_coord[3], page_coord[0]],
                                        [page_coord[3], page_coord[1]], [page_coord[2], page_coord[1]]])]
            return croped_page, page_coord
        finally:
            session.close()

    def clean_text_regions(self, text_regions: np.ndarray) -> np.ndarray:
        """main.py:2074-2075: cv2.erode(text_regions, kernel, iterations=3) then cv2.dilate(..., iterations=4), on the device."""
        model, session = start_new_session_and_model(self.model_region_dir, **self.kw)
        try:
            plane = np.ascontiguousarray(text_regions[:, :, 0] if text_regions.ndim == 3 else text_regions, np.uint8)
            if isinstance(model, SegModel):
                out = model.ctx.morph(model.ctx.morph(plane, 0, 5, 3), 1, 5, 4)
            else:
                out = host_morph(host_morph(plane, False, 5, 3), True, 5, 4)
            return np.repeat(out[:, :, None], 3, axis=2) if text_regions.ndim == 3 else out
        finally:
            session.close()

    def extract_text_regions(self, img_u8: Optional[np.ndarray] = None, box=None) -> np.ndarray:
        """main.py:439-454.  On a SegModel the whole wrapper is one library call: histogram, Otsu threshold,
        binarising tile gather (and, with img_u8=None, the rescale of the stored page), forward, stitch.
        ``box`` = (x, y, w, h) of extract_page on the upscaled page: the stage runs on that crop (what run() hands it,
        main.py:2061-2072) without the crop being built."""
        model, session = start_new_session_and_model(self.model_region_dir, **self.kw)
        try:
            if isinstance(model, SegModel):
                if img_u8 is None and box is not None:
                    lab, self.otsu_threshold = model.ctx.segment_crop(self.image_stored, self.img_hight_int, self.img_width_int, box,
                                                                      binarise=True, channels=3)
                elif img_u8 is None:
                    lab, self.otsu_threshold = model.ctx.segment_page_otsu(self.image_stored, self.img_hight_int, self.img_width_int,
                                                                           channels=3)
                else:
                    lab, self.otsu_threshold = model.ctx.segment_page_otsu(np.ascontiguousarray(img_u8, np.uint8), channels=3)
                return lab                                                 # main.py:366 layout: 3 equal channels
            if img_u8 is None:
                img_u8 = self._scaled_page()
                if box is not None:
                    img_u8 = img_u8[box[1]:box[1] + box[3], box[0]:box[0] + box[2]]
            img = otsu_copy(img_u8).astype(np.uint8)                       # main.py:443-444
            return do_prediction(True, img, model)                         # main.py:447
        finally:
            session.close()            # (the reference's gc.collect() after every stage frees TF graphs; nothing to free here)

    def textline_contours(self, img_u8: Optional[np.ndarray] = None, box=None) -> np.ndarray:
        """main.py:490-503.  With img_u8=None the stored page is segmented through the fused rescale
        (identical to running on the upscaled page), restricted to ``box`` (extract_page's crop) when one is given."""
        model, session = start_new_session_and_model(self.model_textline_dir, **self.kw)
        try:
            if img_u8 is None and isinstance(model, SegModel):
                if box is not None:
                    return model.ctx.segment_crop(self.image_stored, self.img_hight_int, self.img_width_int, box)[0]
                return model.ctx.segment_page_scaled(self.image_stored, self.img_hight_int, self.img_width_int)
            if img_u8 is None:
                img_u8 = self._scaled_page()
                if box is not None:
                    img_u8 = img_u8[box[1]:box[1] + box[3], box[0]:box[0] + box[2]]
            return do_prediction(True, img_u8.astype(np.uint8), model)[:, :, 0]
        finally:
            session.close()            # (the reference's gc.collect() after every stage frees TF graphs; nothing to free here)

    def page_box_only(self):
        """extract_page (main.py:384-437) without building the cropped array: (page mask, (x, y, w, h), page_coord).  The mask
        stays on the device between the border model and the box search; an empty mask raises like main.py:401."""
        model, session = start_new_session_and_model(self.model_page_dir, **self.kw)
        try:
            if isinstance(model, SegModel):
                mask, box, pixels = model.ctx.extract_page_box(self.image_stored, self.img_hight_int, self.img_width_int, channels=3)
            else:
                img = self._scaled_page()
                mask = do_prediction(False, img, model, full_image_shape=img.shape)
                box, pixels = host_page_box(mask[:, :, 0])
            if pixels == 0:
                raise ValueError("attempt to get argmax of an empty sequence")
            x, y, w, h = box
            self.page_mask, self.page_box = mask, (x, y, w, h)
            page_coord = [y, y + h, x, x + w]
            self.cont_page = [np.array([[page_coord[2], page_coord[0]], [page_coord[3], page_coord[0]],
                                        [page_coord[3], page_coord[1]], [page_coord[2], page_coord[1]]])]
            return mask, self.page_box, page_coord
        finally:
            session.close()

    def text_regions_present(self, regions: np.ndarray) -> bool:
        """get_text_region_contours_and_boxes(...) returns at least one contour (main.py:456-480; run() gates the textline model on
        it, main.py:2083-2096): class-1 mask -> MORPH_OPEN -> MORPH_CLOSE -> a parentless contour of area >= 1e-5 x H x W.  On the
        device for a SegModel (``sbbseg_text_regions_present_dev``); foreign model objects get the host mirror."""
        model, session = start_new_session_and_model(self.model_region_dir, **self.kw)
        try:
            if isinstance(model, SegModel):
                return model.ctx.text_regions_present(regions, 1, 0.00001)
            return host_text_regions_present(regions)
        finally:
            session.close()

    def get_text_region_boxes(self, regions: np.ndarray):
        """get_text_region_contours_and_boxes' ``self.boxes`` (main.py:456-480) for the cleaned layout map: a list of [x, y, w, h].  On the
        device for a SegModel (``sbbseg_text_region_boxes``); foreign model objects get the host mirror."""
        model, session = start_new_session_and_model(self.model_region_dir, **self.kw)
        try:
            if isinstance(model, SegModel):
                return model.ctx.text_region_boxes(regions, 1, 0.00001, 1.0)
            return host_text_region_boxes(regions)
        finally:
            session.close()

    def get_text_region_contours(self, regions: np.ndarray):
        """get_text_region_contours_and_boxes (main.py:456-481) for the cleaned layout map: returns what the reference returns -- a list
        of ``np.uint`` arrays [N + 1, 1, 2], each the closed ring of one kept contour -- and sets ``self.boxes``.  Traced on the device
        for a SegModel (``sbbseg_text_region_contours``); foreign model objects get the host mirror."""
        model, session = start_new_session_and_model(self.model_region_dir, **self.kw)
        try:
            if isinstance(model, SegModel):
                self.boxes, contours = model.ctx.text_region_contours(regions, 1, 0.00001, 1.0)
            else:
                self.boxes, contours = host_text_region_contours(regions)
            return closed_rings(contours)
        finally:
            session.close()

    def get_slopes(self, textlines: np.ndarray, boxes, statistics: str = "device"):
        """One deskew slope per box (``get_slopes``: main.py:1728-1748) on the textline model's handle."""
        model, session = start_new_session_and_model(self.model_textline_dir, **self.kw)
        try:
            if not isinstance(model, SegModel):
                raise RuntimeError("get_slopes needs a library handle (SegModel.ctx): there is no CPU fallback")
            return get_slopes(textlines, boxes, model.ctx, statistics=statistics)
        finally:
            session.close()

    def run_with_slopes(self, image_u8: np.ndarray, statistics: str = "device"):
        """``run()`` and the step the reference takes next (main.py:2080, 2111): the text-region boxes and one deskew slope per box.
        Returns run()'s four values plus (boxes, slopes), also kept as ``self.boxes`` / ``self.slopes`` like the reference; both are []
        when the textline model did not run."""
        page_mask, regions, textlines, page_coord = self.run(image_u8)
        self.boxes, self.slopes = [], []
        if textlines is not None:
            self.boxes = self.get_text_region_boxes(regions)
            self.slopes = self.get_slopes(textlines, self.boxes, statistics=statistics)
        return page_mask, regions, textlines, page_coord, self.boxes, self.slopes

    def get_line_masks(self, textlines: np.ndarray, boxes, slopes, masks: bool = True):
        """Per box (dst, row sums, column sums) (``get_line_masks``: main.py:1472-1487) on the textline model's handle."""
        model, session = start_new_session_and_model(self.model_textline_dir, **self.kw)
        try:
            if not isinstance(model, SegModel):
                raise RuntimeError("get_line_masks needs a library handle (SegModel.ctx): there is no CPU fallback")
            return get_line_masks(textlines, boxes, slopes, model.ctx, masks=masks)
        finally:
            session.close()

    def run_with_lines(self, image_u8: np.ndarray, statistics: str = "device", masks: bool = True):
        """``run_with_slopes`` and what the reference does with every slope in the same loop iteration (main.py:1750): the deskewed
        text-line mask of every box and its projections.  Returns run_with_slopes' six values plus the list of ``get_line_masks``, also
        kept as ``self.line_masks``; [] when the textline model did not run."""
        page_mask, regions, textlines, page_coord, boxes, slopes = self.run_with_slopes(image_u8, statistics=statistics)
        self.line_masks = []
        if textlines is not None:
            self.line_masks = self.get_line_masks(textlines, boxes, slopes, masks=masks)
        return page_mask, regions, textlines, page_coord, boxes, slopes, self.line_masks

    def get_line_boxes(self, textlines: np.ndarray, boxes, slopes):
        """Per box the line record of ``get_line_boxes`` (main.py:516-1457 after the projection) on the textline model's handle."""
        model, session = start_new_session_and_model(self.model_textline_dir, **self.kw)
        try:
            if not isinstance(model, SegModel):
                raise RuntimeError("get_line_boxes needs a library handle (SegModel.ctx): there is no CPU fallback")
            return get_line_boxes(textlines, boxes, slopes, model.ctx)
        finally:
            session.close()

    def run_with_line_boxes(self, image_u8: np.ndarray, statistics: str = "device", masks: bool = True):
        """``run_with_lines`` and the text lines of every box (``get_line_boxes``; x extent: the reference's fallback 0 .. w, the contour
        is not built).  Returns run_with_lines' seven values plus the list of line records, also kept as ``self.line_boxes``; [] when
        the textline model did not run."""
        out = self.run_with_lines(image_u8, statistics=statistics, masks=masks)
        self.line_boxes = []
        if out[2] is not None:
            self.line_boxes = self.get_line_boxes(out[2], out[4], out[5])
        return out + (self.line_boxes,)

    def _run_resident(self):
        """run()'s three stages with the stored page uploaded ONCE and kept in device memory for all of them (run() hands the same
        page to every stage, main.py:2061-2102), the border mask and the region map staying on the device between their model and
        their glue: ONE library call, ``sbbseg_run_page`` (round 5: neither PyTorch nor device pointers on this path -- the
        reference's environment is Keras / TF only).  Same return value as the stage-by-stage path below, which remains the path for
        foreign model objects and for SBBSEG_STAGES_RESIDENT=0.  Returns None when it does not apply."""
        import os
        if os.environ.get("SBBSEG_STAGES_RESIDENT", "1") == "0":
            return None
        opened = [start_new_session_and_model(d, **self.kw) for d in (self.model_page_dir, self.model_region_dir, self.model_textline_dir)]
        try:
            (m_page, _), (m_region, _), (m_text, _) = opened
            if not all(isinstance(m, SegModel) for m in (m_page, m_region, m_text)):
                return None
            from . import _capi
            # extract_page's errors propagate (main.py:2061 is outside the try); the other stages degrade inside the call
            mask, regions, textlines, info = _capi.run_page(m_page.ctx, m_region.ctx, m_text.ctx, self.image_stored,
                                                            self.img_hight_int, self.img_width_int, channels=3)
            x, y, w, h = (int(v) for v in info.box_xywh)
            self.page_box = (x, y, w, h)
            page_coord = [y, y + h, x, x + w]
            self.cont_page = [np.array([[page_coord[2], page_coord[0]], [page_coord[3], page_coord[0]],
                                        [page_coord[3], page_coord[1]], [page_coord[2], page_coord[1]]])]
            self.page_mask = mask
            if info.regions_ok:
                self.otsu_threshold = int(info.otsu_threshold)
            return mask, regions, textlines, page_coord
        finally:
            for _, session in opened:
                session.close()

    def run(self, image_u8: np.ndarray):
        """The model-running part of run() (main.py:2056-2107) with its chaining: border model -> page box -> the layout
        and textline models on the CROPPED page (main.py:2061, 2072, 2102), text regions cleaned by erode x 3 / dilate x 4
        (main.py:2074-2075).  Returns (page mask [Hs,Ws,3], cleaned regions [h,w,3], text lines [h,w], page_coord) with
        h x w = extract_page's box; the crop itself is never built on a SegModel.  (Round 3 added page_coord as a FOURTH element:
        callers that unpacked three must be updated -- INTEGRATION.md.)  Like the reference, a failed layout stage yields
        regions = None and skips the textline model (textlines = None); extract_page's errors propagate."""
        self.get_image_and_scales(image_u8)
        resident = self._run_resident()
        if resident is not None:
            return resident
        page_mask, box, page_coord = self.page_box_only()          # outside the try, like main.py:2061: its errors propagate
        # main.py:2069-2091: the layout stage and its post-processing sit in a bare try/except -- any failure (the reference: a crop
        # smaller than the model input breaks do_prediction's reshape, main.py:278-285; here: sbbseg_segment_crop refuses it) degrades
        # to "no regions"; the textline model only runs when text regions were found (main.py:2096 `if len(contours) > 0`: contours
        # are traced from the opened / closed class-1 mask and filtered by area, main.py:456-480 -- tracing them is out of scope,
        # their existence is not: text_regions_present)
        try:
            regions = self.extract_text_regions(box=box)
            regions = self.clean_text_regions(regions)
            has_text = self.text_regions_present(regions)           # main.py:2083, 2096
        except Exception:
            regions, has_text = None, False
        textlines = None
        if has_text:
            try:
                textlines = self.textline_contours(box=box)
            except Exception:                                       # main.py:2152-2157: the outer bare except -> empty result
                textlines = None
        return page_mask, regions, textlines, page_coord

    def run_pages(self, images, resident: bool = False):
        """``[self.run(img) for img in images]``, with the two patch stages pooled over the pages: the border model and the page box run
        page by page as in run(); the layout model then takes ALL pages' crops in one ``segment_views`` call (their tiles share launches
        although every crop has its own size), cleaning and the text-region gate run per page, and the textline model takes the crops of
        the pages that passed the gate in one more call.  A page whose crop cannot hold one input of a model is kept out of that model's
        call and gets what run() gives it (regions = None / textlines = None); extract_page's errors propagate.  Foreign model objects
        take the loop.
        ``resident=True`` (opt-in): ONE library call, ``sbbseg_run_pages`` -- every stored page is uploaded once and stays on the device for
        all three stages, the border forwards run at batch width (never split-K: the masks equal run()'s with split-K off on the border
        handle), the region maps stay on the device between the layout model, the cleaning and the gate.  Same tuples; raises what run()
        raises for the first page without a page box."""
        images = list(images)
        opened = [start_new_session_and_model(d, **self.kw) for d in (self.model_page_dir, self.model_region_dir, self.model_textline_dir)]
        try:
            (_, _), (m_region, _), (m_text, _) = opened
            if not all(isinstance(m, SegModel) for m, _ in opened):
                return [self.run(img) for img in images]
            if resident:
                from . import _capi
                stored = [np.ascontiguousarray(img, np.uint8) for img in images]
                out = _capi.run_pages(opened[0][0].ctx, m_region.ctx, m_text.ctx,
                                      [(img,) + scaled_size(*img.shape[:2]) for img in stored], channels=3) if stored else []
                results = []
                for mask, regions, textlines, info, status in out:
                    if status != 0:
                        raise ValueError("attempt to get argmax of an empty sequence")          # what main.py:401 raises
                    x, y, w, h = (int(v) for v in info.box_xywh)
                    results.append((mask, regions, textlines, [y, y + h, x, x + w]))
                return results

            def fits(model, box):
                H, W = model.ctx.model_info()[:2]
                return box[3] >= H and box[2] >= W

            pages = []
            for img in images:
                self.get_image_and_scales(img)
                page_mask, box, page_coord = self.page_box_only()      # outside any try, like main.py:2061
                pages.append(dict(stored=self.image_stored, hw=(self.img_hight_int, self.img_width_int), mask=page_mask, box=box,
                                  coord=page_coord, regions=None, textlines=None, has_text=False))
            todo = [p for p in pages if fits(m_region, p["box"])]
            if todo:
                out = m_region.segment_views([(p["stored"], p["hw"][0], p["hw"][1], p["box"], True) for p in todo], channels=3)
                for p, (lab, thr) in zip(todo, out):
                    p["regions"] = self.clean_text_regions(lab)         # main.py:2074-2075
                    p["has_text"] = self.text_regions_present(p["regions"])      # main.py:2083, 2096
                    self.otsu_threshold = thr
            todo = [p for p in pages if p["has_text"] and fits(m_text, p["box"])]
            if todo:
                out = m_text.segment_views([(p["stored"], p["hw"][0], p["hw"][1], p["box"], False) for p in todo])
                for p, (lab, _) in zip(todo, out):
                    p["textlines"] = lab
            return [(p["mask"], p["regions"], p["textlines"], p["coord"]) for p in pages]
        finally:
            for _, session in opened:
                session.close()

    def run_pages_with_line_boxes(self, images, masks: bool = False):
        """``[self.run_with_line_boxes(img, masks=masks) for img in images]`` with everything between the stored pages and the text lines
        resident: ONE ``sbbseg_run_pages`` (``run_pages(resident=True)``: raises what it raises), then, on the planes that call leaves on
        the device (``_capi.run_pages_planes``), the text-region boxes page by page on the cleaned layout plane (the component
        labelling works on one plane at a time) and ONE pooled call each for the slopes, the line masks and the line boxes of all pages'
        boxes (``planes_deskew_slopes_dev`` / ``planes_line_masks_dev`` / ``planes_line_boxes_dev``): no label map is uploaded again and
        the launches do not grow with the pages.  Pages are grouped (``_capi.group_pages_for_lines``) so that an archive beyond the
        library's per-call limits becomes several pooled calls.  Returns per page run_with_line_boxes' 8-tuple; boxes, slopes, masks
        and lines are [] where the textline model did not run.  The line-mask call runs only to return what run_with_lines returns (the
        line-boxes call repeats its kernels: the C entry points share no outputs).  Foreign model objects take the loop."""
        return self._run_pages_lines(images, masks, False)

    def run_pages_with_contours(self, images, masks: bool = False):
        """``run_pages_with_line_boxes`` plus, per page, the text-region contours (``get_text_region_contours``'s list; [] where the
        textline model did not run): a 9-tuple per page.  The per-page boxes call on the resident cleaned layout plane is replaced by the
        contours call (``text_region_contours_dev``): boxes and contours come out of the same launches, and no label plane leaves the
        device.  Foreign model objects take the loop."""
        return self._run_pages_lines(images, masks, True)

    def get_region_order(self, textlines: np.ndarray, contours):
        """``(order_of_texts, id_of_texts)`` of the text regions (order_of_regions + order_and_id_of_texts, main.py:2118-2119) on the
        textline model's handle; foreign model objects get the library's serial host twin."""
        model, session = start_new_session_and_model(self.model_textline_dir, **self.kw)
        try:
            indexes_sorted, matrix = order_of_regions(textlines, contours, model.ctx if isinstance(model, SegModel) else None)
            return order_and_id_of_texts(contours, matrix, indexes_sorted)
        finally:
            session.close()

    def run_pages_with_reading_order(self, images, masks: bool = False):
        """``run_pages_with_contours`` plus, per page, the reading order of its text regions (main.py:2118-2119): the 9-tuple +
        ``(order_of_texts, id_of_texts)``; ([], []) where the textline model did not run.  The order call for a page
        (``region_order_dev``) is made right after that page's contour call, while its contour table is resident, on the page's resident
        textline plane: neither a plane nor a polygon crosses the bus for it.  Foreign model objects take the loop with the host twin."""
        return self._run_pages_lines(images, masks, True, True)

    def run_pages_with_text_lines(self, images, masks: bool = False):
        """``run_pages_with_reading_order`` plus, per page, what ``do_work_of_slopes`` collects as ``all_found_texline_polygons``
        (main.py:1750-1756): per text region the list of its lines' 4 x 2 polygons (``textline_boxes_rot``, int32), [] for a region the
        reference leaves without lines -- a 12-tuple per page.  The lines of all pages' regions are cut to their regions' contours in ONE
        pooled call per page group (``region_line_extents_dev``), after the pooled line-box call; the line records in the tuple (index 7)
        are the cut ones.  Needs the library's own model objects: there is no loop for foreign ones."""
        return self._run_pages_lines(images, masks, True, True, True)

    def _run_pages_lines(self, images, masks: bool, contours: bool, order: bool = False, text_lines: bool = False):
        images = list(images)
        opened = [start_new_session_and_model(d, **self.kw) for d in (self.model_page_dir, self.model_region_dir, self.model_textline_dir)]
        try:
            if not all(isinstance(m, SegModel) for m, _ in opened):
                if text_lines:
                    raise RuntimeError("run_pages_with_text_lines needs the library's own models: there is no CPU fallback")
                out = []
                for img in images:
                    page = self.run_with_line_boxes(img, masks=masks)
                    if contours:
                        page = page + ((self.get_text_region_contours(page[1]) if page[2] is not None else []),)
                    if order:
                        page = page + (self.get_region_order(page[2], page[8]) if page[2] is not None else ([], []))
                    out.append(page)
                return out
            if not images:
                return []
            from . import _capi
            c_region, c_text = opened[1][0].ctx, opened[2][0].ctx
            runs = self.run_pages(images, resident=True)
            d_regions, d_textlines = _capi.run_pages_planes(c_region)
            n = len(runs)
            has_lines = [runs[k][2] is not None for k in range(n)]
            rings, orders = [[] for _ in range(n)], [([], []) for _ in range(n)]
            if contours:
                boxes = [[] for _ in range(n)]
                for k in range(n):
                    if not has_lines[k]:
                        continue
                    boxes[k], traced = c_region.text_region_contours_dev(*d_regions[k], 1, 0.00001, 1.0)
                    rings[k] = closed_rings(traced)
                    if order:                                    # while page k's contour table is resident
                        rec = c_region.region_order_dev(*d_textlines[k], None, len(traced))
                        indexes_sorted, matrix = _order_result(rec)
                        orders[k] = order_and_id_of_texts(traced, matrix, indexes_sorted)
            else:
                boxes = [c_region.text_region_boxes_dev(*d_regions[k], 1, 0.00001, 1.0) if has_lines[k] else [] for k in range(n)]
            slopes, line_masks, line_boxes = [[] for _ in range(n)], [[] for _ in range(n)], [[] for _ in range(n)]
            for group in _capi.group_pages_for_lines(boxes):
                planes, gb = [d_textlines[k] for k in group], [boxes[k] for k in group]
                if not any(gb):
                    continue
                gs = c_text.planes_deskew_slopes_dev(planes, gb, 2)
                gm = c_text.planes_line_masks_dev(planes, gb, gs, 2, masks)
                gl = c_text.planes_line_boxes_dev(planes, gb, gs, 2)
                if text_lines:                                   # the step reads no label plane: the boxes of the whole group share one call
                    cut = c_text.region_line_extents_dev([b for pb in gb for b in pb], [s for ps in gs for s in ps], [r for pr in gl for r in pr],
                                                         [ring for k in group for ring in rings[k]])
                    at = 0
                    for q in range(len(group)):
                        gl[q], at = cut[at:at + len(gb[q])], at + len(gb[q])
                for q, k in enumerate(group):
                    slopes[k], line_masks[k], line_boxes[k] = gs[q], gm[q], gl[q]
            polygons = [[[p for p in rec["boxes_rot"]] if rec["status"] == _capi.LINES_OK else [] for rec in line_boxes[k]] for k in range(n)]
            return [runs[k] + (boxes[k], slopes[k], line_masks[k], line_boxes[k]) + ((rings[k],) if contours else ()) + (orders[k] if order else ())
                    + ((polygons[k],) if text_lines else ()) for k in range(n)]
        finally:
            for _, session in opened:
                session.close()
