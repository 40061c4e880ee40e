"""csrc/contour_host.h -- the host labeller, the one border walker over a label plane and the host ranking -- alone, without a GPU and
without the library.

A small host program includes only that header, reads masks from a text file, labels each one, walks every component (an emit functor
counts and sums the kept points) and prints per component: root, pixels, box, doubled area, kept points, steps and status; then the
sum of the label plane and the host ranking's winner.  The program is built with the address and undefined-behaviour sanitizers (a
stand-alone host program: nothing is preloaded) -- the neighbour lookups of a shape on the plane's edge leave the plane, and a report
ends the program with a status.

What it prints is held to tests/contours_ref.py (OpenCV's follower, restated in Python) and to scipy's labelling."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy import ndimage

import contour_shapes
import contours_ref

OK, STEP_BOUND = 0, 1                             # csrc/contour_walk.h: kContourOk, kContourStepBound

_PROBE = r"""
#include "contour_host.h"
#include <cstdio>
#include <string>
using namespace sbbseg;

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    char name[64];
    int H, W;
    long long bound;                              // 0: contour_step_bound of the component's box
    while (fscanf(f, "%63s %d %d %lld", name, &H, &W, &bound) == 4) {
        std::vector<uint8_t> mask((size_t)H * W);
        for (size_t i = 0; i < mask.size(); ++i) {
            int v;
            if (fscanf(f, "%d", &v) != 1) return 3;
            mask[i] = (uint8_t)v;
        }
        std::vector<int> lab;
        std::vector<LabelComp> comps;
        label_mask(mask.data(), H, W, lab, comps);
        for (size_t q = comps.size(); q-- > 0;) {
            const LabelComp& k = comps[q];
            long long n = 0, sx = 0, sy = 0;
            auto emit = [&](int at, int x, int y) { if (at == n) ++n; sx += x; sy += y; };
            const ContourResult r = walk_label_contour(lab.data(), H, W, k.root, bound > 0 ? bound : label_comp_step_bound(k), emit);
            printf("%s comp %d %d %d %d %d %d %lld %d %lld %d %d %d %d %d %lld %lld %lld\n", name, k.root, k.pixels, k.x0, k.y0, k.x1, k.y1, r.area2,
                   r.n_points, r.steps, r.status, r.x0, r.y0, r.x1, r.y1, n, sx, sy);
        }
        long long sum = 0;
        for (int v : lab) sum += v;
        const LargestContour best = host_largest_contour(mask.data(), H, W);
        printf("%s plane %zu %lld %d %d %lld %d\n", name, comps.size(), sum, (int)best.any, best.comp.root, best.area2, best.status);
    }
    fclose(f);
    return 0;
}
"""


def shapes():
    """[(name, mask, step bound or 0)]"""
    hand = contour_shapes.hand_shapes()
    out = [(n, hand[n], 0) for n in ("single_pixel", "pinch", "ring_with_island", "touches_all_edges")]
    out.append(("line_1xN", np.ones((1, 9), np.uint8), 0))
    out.append(("full_plane", np.ones((4, 6), np.uint8), 0))              # every border pixel looks outside the plane
    out.append(("staircase40", contour_shapes.staircase(40), 0))
    out.append(("staircase40_bound50", contour_shapes.staircase(40), 50))
    return out


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("contour_host")
    (d / "probe.cpp").write_text(_PROBE)
    with open(d / "masks.txt", "w") as f:
        for name, m, bound in shapes():
            f.write("%s %d %d %d\n%s\n" % (name, m.shape[0], m.shape[1], bound, " ".join(str(int(v != 0)) for v in m.ravel())))
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sbb_textline_detection_amd", "csrc")
    # contour_host.h is plain C++: it must compile as such, without the HIP language and without the HIP runtime's headers
    res = subprocess.run([hipcc, "-x", "c++", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                          "-Xarch_host", "-fno-sanitize-recover=all", "-I", csrc, str(d / "probe.cpp"), "-o", str(d / "probe")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    out = subprocess.run([str(d / "probe"), str(d / "masks.txt")], capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr[-3000:]              # (a sanitizer report ends the program with a status)
    rows = {}
    for line in out.stdout.splitlines():
        f = line.split()
        rows.setdefault(f[0], {"comp": [], "plane": None})
        if f[1] == "comp":
            rows[f[0]]["comp"].append([int(v) for v in f[2:]])
        else:
            rows[f[0]]["plane"] = [int(v) for v in f[2:]]
    return rows


def test_header_is_host_only():
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sbb_textline_detection_amd", "csrc")
    text = open(os.path.join(csrc, "contour_host.h")).read()
    import re
    assert re.findall(r'#\s*include\s+"([^"]+)"', text) == ["contour_walk.h"]
    for word in ("HIPCHK", "REQUIRE", "hipMemcpy", "hipMalloc", "hipLaunch", "<<<", "ctx.h", "internal.h"):
        assert word not in text, word


def test_every_shape_was_walked(printed):
    assert sorted(printed) == sorted(n for n, _, _ in shapes())
    assert all(r["plane"] is not None for r in printed.values())


@pytest.mark.parametrize("name", [n for n, _, b in shapes() if not b])
def test_walk_and_labels_match_the_reference(printed, name):
    mask = dict((n, m) for n, m, _ in shapes())[name]
    want = contours_ref.mask_contours(mask)                      # by descending first pixel, as the program walks
    lab, n = ndimage.label(mask != 0, structure=np.ones((3, 3), int))
    got = printed[name]["comp"]
    assert len(got) == len(want) == n
    plane = np.full(mask.shape, -1, np.int64)
    for row, (box, a2, pts, chain_len), k in zip(got, want, range(n, 0, -1)):
        root, pixels, x0, y0, x1, y1, area2, n_points, steps, status, rx0, ry0, rx1, ry1, emitted, sx, sy = row
        ys, xs = np.nonzero(lab == k)
        assert root == int(ys[0]) * mask.shape[1] + int(xs[0]) and pixels == len(xs)
        assert [x0, y0, x1, y1] == [xs.min(), ys.min(), xs.max(), ys.max()] == [rx0, ry0, rx1, ry1]
        assert [x0, y0, x1 - x0 + 1, y1 - y0 + 1] == box
        assert status == OK and area2 == a2 and n_points == emitted == len(pts)
        assert steps == chain_len
        assert (sx, sy) == (int(pts[:, 0].sum()), int(pts[:, 1].sum()))
        plane[lab == k] = root
    n_comp, lab_sum, any_, best_root, best_area2, best_status = printed[name]["plane"]
    assert n_comp == n and lab_sum == int(plane.sum()) and any_ == 1 and best_status == OK
    areas = [w[1] for w in want]
    assert best_area2 == max(areas) and best_root == got[int(np.argmax(areas))][0]      # first maximum of the descending list: the later root


def test_known_figures(printed):
    one = printed["single_pixel"]["comp"]
    assert len(one) == 1 and one[0][6:9] == [0, 1, 1]                            # area 0, one point, a chain of one
    assert printed["pinch"]["comp"][0][7] == 10                                  # the pinch pixel lies on two straight runs
    assert [r[6] for r in printed["ring_with_island"]["comp"]] == [2 * 2 * 2, 2 * 10 * 10]      # island first (the later root), ring as if solid
    assert printed["line_1xN"]["comp"][0][6:8] == [0, 2]                         # a line has no area and two kept points
    assert printed["full_plane"]["comp"][0][6:8] == [2 * 3 * 5, 4]


def test_step_bound_is_a_status(printed):
    """The staircase needs more than 50 steps: the walk ends with kContourStepBound after exactly 50, the same plane closes with its own
    bound, and the ranking (which always uses the box bound) is not touched by the short bound."""
    short, full = printed["staircase40_bound50"], printed["staircase40"]
    assert len(short["comp"]) == 1 and short["comp"][0][9] == STEP_BOUND and short["comp"][0][8] == 50
    assert full["comp"][0][9] == OK and full["comp"][0][8] > 50
    assert short["plane"] == full["plane"] and full["plane"][5] == OK
