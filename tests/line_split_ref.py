"""numpy / scipy restatement of the two line splitters after the projection (tests/test_line_split_cpu.py, tests/test_gpu_line_split.py,
tests/golden/make_line_split_golden.py): ``seperate_lines`` (main.py:516-991) and ``seperate_lines_vertical`` (main.py:993-1457) on one
profile, with the real ``gaussian_filter1d`` and ``find_peaks``, the reference's control flow step by step (both ``try`` / ``except``
levels included) and the corners spelled ``a * x + b * y + d`` elementwise.  cv2.pointPolygonTest is taken to return -1 (the contour half
is out of scope), so every line has the fallback extent 0 .. w; return_contours_of_image / filter_contours_area_of_image inside the first
``try`` are dead and taken as non-raising [EXT] unpinned.  Nothing here is product code, and nothing here touches the GPU."""
import os
import warnings

import numpy as np
from scipy.ndimage import gaussian_filter1d
from scipy.signal import find_peaks

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "line_split_golden.npz")
OK, NONE = 0, 1
FIELDS = ("status", "sigma", "raised", "branch", "peaks", "point_up", "point_down", "boxes", "boxes_rot")


def rotation_terms(w, h, slope, rotation_matrix):
    """[cos, -sin, sin, cos, x_d, y_d] (main.py:517-524; main.py:996-1005 beyond 45 degrees) with the given getRotationMatrix2D."""
    thetha = slope + 90 if abs(slope) > 45 else slope
    M = np.asarray(rotation_matrix((w // 2, h // 2), -thetha)).reshape(2, 3)
    t = thetha / 180. * np.pi
    return [float(np.cos(t)), float(-np.sin(t)), float(np.sin(t)), float(np.cos(t)), float(M[0, 2]), float(M[1, 2])]


def _two_scans(y_padded, sigma):
    """main.py:553-561 / 621-629: (smoothed, smoothed flipped and padded, peaks, peaks_neg)."""
    smoothed = gaussian_filter1d(y_padded, sigma)
    up_to_down = -y_padded + np.max(y_padded)
    padded = np.zeros(len(up_to_down) + 40)
    padded[20:len(up_to_down) + 20] = up_to_down
    padded = gaussian_filter1d(padded, sigma)
    peaks, _ = find_peaks(smoothed, height=0)
    peaks_neg, _ = find_peaks(padded, height=0)
    return smoothed, padded, peaks, peaks_neg


def _split_at_breaks(arg, cluster_at):
    out = [arg[0:cluster_at[0] + 1]]
    for i in range(len(cluster_at) - 1):
        out.append(arg[cluster_at[i] + 1:cluster_at[i + 1] + 1])
    out.append(arg[cluster_at[len(cluster_at) - 1] + 1:])
    return out


def _merge(peaks, peaks_neg, clusters):
    """main.py:585-605 / 680-721: (peaks_new_tot, peaks_neg_new)."""
    if len(clusters) == 0:
        return peaks[:], peaks_neg[:]
    peaks_new, peaks_neg_new, extra = peaks[:], peaks_neg[:], []
    for cluster in clusters:
        lo, hi = np.min(peaks[cluster]), np.max(peaks[cluster])                 # IndexError: the positions come from peaks_neg
        extra.append(int((lo + hi) / 2.0))
        for c in cluster:
            peaks_new = peaks_new[peaks_new != peaks[c - 1]]                    # c == 0: numpy's -1 is the last peak
            peaks_new = peaks_new[peaks_new != peaks[c]]
            peaks_neg_new = peaks_neg_new[peaks_neg_new != peaks_neg[c]]
    return np.sort(list(peaks_new) + extra), peaks_neg_new


def _ratio_positions(padded, peaks_neg, top, threshold):
    arg = np.array(range(len(peaks_neg)))[padded[peaks_neg] / float(top) < threshold]
    diff = np.diff(arg)
    return arg, np.array(range(len(diff)))[diff > 1]


def first_sigma(y_padded):
    """main.py:551-617: (sigma_gaus, raised)."""
    try:
        _s, padded, peaks, peaks_neg = _two_scans(y_padded, 2)
        arg, cluster_at = _ratio_positions(padded, peaks_neg, np.max(padded[peaks_neg]), 0.3)
        clusters = _split_at_breaks(arg, cluster_at) if len(cluster_at) > 0 else []
        peaks_new_tot, _n = _merge(peaks, peaks_neg, clusters)
        sigma, raised = int(np.mean(np.diff(peaks_new_tot)) * (7. / 40.0)), False
    except Exception:
        sigma, raised = 12, True
    return max(sigma, 3), raised


def _corner(a, b, d, x, y, clamp):
    v = a * float(x) + b * float(y) + d
    hit = bool(clamp and v < 0)
    return int(0 if hit else v), hit


def line_split(y, other, vertical, rot):
    """One region: a record with FIELDS (see ``_capi.line_split_host``) plus ``clusters`` (clusters merged in the second pass) and
    ``clamped`` (a negative rotated corner was clamped).  ``y``: the row sums of dst, or its column sums with ``vertical``."""
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return _line_split(np.asarray(y, np.int64), int(other), bool(vertical), [float(v) for v in rot])


def _line_split(y, other, vertical, rot):
    n = len(y)
    rows, x_max = (other, n) if vertical else (n, other)                        # img_patch.shape
    y_padded = np.zeros(n + 40)
    y_padded[20:n + 20] = y
    sigma, raised = first_sigma(y_padded)
    rec = {"status": NONE, "sigma": sigma, "raised": raised, "branch": -1, "clusters": 0, "clamped": False}
    for name in ("peaks", "point_up", "point_down"):
        rec[name] = np.zeros(0, np.int32)
    rec["boxes"], rec["boxes_rot"] = np.zeros((0, 4, 2), np.int32), np.zeros((0, 4, 2), np.int32)
    lines = []                                                                  # (peak, point_up, point_down)
    try:                                                                        # the bare except of main.py:1520
        smoothed, padded, peaks, peaks_neg = _two_scans(y_padded, sigma)
        top = np.max(padded[peaks_neg]) if vertical else np.max(smoothed[peaks])                # main.py:1127 / 646
        arg, cluster_at = _ratio_positions(padded, peaks_neg, top, 0.42)
        clusters = []
        if len(cluster_at) >= 2:
            clusters = _split_at_breaks(arg, cluster_at)
        elif len(arg) >= 2 and len(cluster_at) == 0:
            clusters.append(arg[:])
        if len(arg) == 1:
            clusters.append(arg)
        rec["clusters"] = len(clusters)
        peaks, peaks_neg = _merge(peaks, peaks_neg, clusters)
        values = smoothed[peaks]
        mean, std = np.mean(values), np.std(values)
        peaks_neg = np.minimum(peaks_neg - 20 - 20, n - 1)                      # only values above len(x) - 1 are touched
        peaks = np.minimum(peaks - 20, n - 1)
        if len(peaks_neg) == len(peaks) + 1 and len(peaks) >= 3:
            rec["branch"] = 0
            for jj in range(len(peaks)):
                up, down = abs(peaks[jj] - peaks_neg[jj]), abs(peaks[jj] - peaks_neg[jj + 1])
                high = values[jj] > mean - std / 2.
                if jj == len(peaks) - 1:
                    lines.append((peaks[jj], peaks[jj] - int((1.3 if high else 1.4) * up), (x_max if vertical else rows) - 1))
                else:
                    lines.append((peaks[jj], peaks[jj] - int((1.1 if high else 1.23) * up), peaks[jj] + int((1.1 if high else 1.33) * down)))
        elif len(peaks) < 1:
            rec["branch"] = 1
        elif len(peaks) == 1:
            rec["branch"] = 2
            if vertical:
                raise NameError("point_up")                                     # main.py:1298 reads it before any assignment
            lines.append((peaks[0], 0, rows))
        elif len(peaks) == 2:
            rec["branch"] = 3
            dis = np.abs(peaks[1] - peaks[0])
            down = peaks[1] + int(1. / 1.8 * dis)
            lines.append((peaks[0], 0, peaks[0] + int(1. / 1.8 * dis)))
            lines.append((peaks[1], peaks[1] - int(1. / 1.8 * dis), rows - 2 if down >= rows else down))
        else:
            rec["branch"] = 4
            for jj in range(len(peaks)):
                if jj == 0:
                    dis = peaks[jj + 1] - peaks[jj]
                    up = peaks[jj] - int(1. / 1.9 * dis)
                    lines.append((peaks[jj], 1 if up < 0 else up, peaks[jj] + int(1. / 1.9 * dis)))
                elif jj == len(peaks) - 1:
                    dis = peaks[jj] - peaks[jj - 1]
                    down = peaks[jj] + int(1. / 1.7 * dis)
                    lines.append((peaks[jj], peaks[jj] - int(1. / 1.9 * dis), rows - 2 if down >= rows else down))
                else:
                    lines.append((peaks[jj], peaks[jj] - int(1. / 1.9 * (peaks[jj] - peaks[jj - 1])),
                                  peaks[jj] + int(1. / 1.9 * (peaks[jj + 1] - peaks[jj]))))
    except Exception:
        return rec
    a, b, c, d, x_d, y_d = rot
    boxes, boxes_rot = [], []
    for _peak, up, down in lines:
        up, down = int(up), int(down)
        boxes.append([[0, up], [x_max, up], [x_max, down], [0, down]])          # main.py:817-820 with x_min_cont, x_max_cont
        pts = [(up, 0), (down, 0), (down, rows), (up, rows)] if vertical else boxes[-1]
        clamp = [(True, True), (False, True), (False, False), (True, False)]    # x_min_rot1, point_up_rot1, point_up_rot2, x_min_rot4
        quad = []
        for (px, py), (cx, cy) in zip(pts, clamp):
            vx, hx = _corner(a, b, x_d, px, py, cx)
            vy, hy = _corner(c, d, y_d, px, py, cy)
            rec["clamped"] = rec["clamped"] or hx or hy
            quad.append([vx, vy])
        boxes_rot.append(quad)
    rec["status"] = OK
    rec["peaks"] = np.array([ln[0] for ln in lines], np.int32).reshape(-1)
    rec["point_up"] = np.array([ln[1] for ln in lines], np.int32).reshape(-1)
    rec["point_down"] = np.array([ln[2] for ln in lines], np.int32).reshape(-1)
    rec["boxes"] = np.array(boxes, np.int32).reshape(-1, 4, 2)
    rec["boxes_rot"] = np.array(boxes_rot, np.int32).reshape(-1, 4, 2)
    return rec


def same(got, want):
    """Every field of FIELDS equal (exactly)."""
    return all(np.array_equal(np.asarray(got[f]), np.asarray(want[f])) and np.asarray(got[f]).shape == np.asarray(want[f]).shape for f in FIELDS)


def load_golden():
    """The committed cases: a list of dicts with y, other, vertical, slope, rot and the reference's own record (FIELDS, clusters)."""
    g = np.load(GOLDEN)
    y_off, l_off = g["y_off"], g["line_off"]
    out = []
    for k in range(len(g["other"])):
        ls = slice(int(l_off[k]), int(l_off[k + 1]))
        out.append({"y": g["y"][int(y_off[k]):int(y_off[k + 1])], "other": int(g["other"][k]), "vertical": int(g["vertical"][k]),
                    "slope": float(g["slope"][k]), "rot": [float(v) for v in g["rot"][k]], "status": int(g["status"][k]),
                    "sigma": int(g["sigma"][k]), "raised": bool(g["raised"][k]), "branch": int(g["branch"][k]), "clusters": int(g["clusters"][k]),
                    "peaks": g["peaks"][ls], "point_up": g["boxes"][ls][:, 0, 1], "point_down": g["boxes"][ls][:, 2, 1], "boxes": g["boxes"][ls],
                    "boxes_rot": g["boxes_rot"][ls], "page": int(g["page"][k]), "box": int(g["box"][k])})
    return out


# ---- cases the CPU and the device tests share: each gives (profiles, others, slopes) ----

def _random_profiles(count=200, seed=5):
    rng = np.random.RandomState(seed)
    profiles, others, slopes = [], [], []
    for _ in range(count):
        n, period, other = int(rng.randint(1, 401)), int(rng.randint(4, 121)), int(rng.randint(1, 300))
        i = np.arange(n)
        y = (((i + rng.randint(0, period)) % period) < rng.uniform(0.2, 0.8) * period) * rng.randint(1, other + 1)
        y = (y + rng.randint(0, 3, n) * (rng.rand() < 0.5)).clip(0, other)
        if rng.rand() < 0.2:
            y[rng.randint(0, n):] = 0
        profiles.append(y.astype(np.int32))
        others.append(other)
        slopes.append(float(rng.choice([0, 2.0, -9.5, 21, 44, 46, -70, 90, rng.uniform(-90, 90)])))
    return profiles, others, slopes


def both_ends_profiles():
    """Mass at both ends only, each profile once beyond 45 degrees and once below."""
    profiles, others, slopes = [], [], []
    for n in (300, 400, 600):
        y = np.zeros(n, np.int32)
        y[:3] = y[-3:] = 50
        profiles += [y, y]
        others += [50, 50]
        slopes += [80.0, 2.0]
    return profiles, others, slopes


def long_zero_constant_profiles():
    """2100 samples (beyond what the device keeps in LDS), all zeros, a constant and a single sample."""
    long = ((np.arange(2100) % 70) < 30).astype(np.int32) * 55
    return ([long, long, np.zeros(57, np.int32), np.zeros(57, np.int32), np.full(80, 9, np.int32), np.full(80, 9, np.int32), np.array([4], np.int32)],
            [60, 60, 31, 31, 9, 9, 4], [1.5, -80.0, 0.0, 90.0, 3.0, 60.0, 0.0])


STRIPED = ((2049, 20), (3000, 24), (1500, 16), (2048, 12))       # (samples, period): more than 64 lines each
STRIPED_LINES = (103, 125, 94, 171)


def striped_profiles():
    """Half-period stripes of height 40 over the whole profile, slope 1."""
    return [(((np.arange(n) % period) < period // 2) * 40).astype(np.int32) for n, period in STRIPED], [40] * len(STRIPED), [1.0] * len(STRIPED)
