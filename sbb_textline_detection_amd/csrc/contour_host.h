// contour_host.h -- private, host only, plain C++17 (no HIP runtime): the outer contours of a mask or of a label plane on the host, on the
// one border follower the device runs too (contour_walk.h).  contour_glue.hip labels a host mask and walks it with these for the host twin
// of the tracer and for the host ranking.  (Its fallback on the device's label plane still has a tracer of its own: see trace_on_host.)
//
// A label plane holds, per foreground pixel, the ROOT of its 8-connected component -- the component's first pixel in raster order, as a
// pixel index -- and -1 elsewhere: what launch_largest_contour leaves in c->cc_parent and what label_mask writes.
#ifndef SBBSEG_CONTOUR_HOST_H
#define SBBSEG_CONTOUR_HOST_H

#include <stddef.h>
#include <vector>

#include "contour_walk.h"

namespace sbbseg {

// One component of a labelled mask: root, box {x0, y0, x1, y1} and pixel count.
struct LabelComp {
    int root, x0, y0, x1, y1, pixels;
};

// The outer border of the component `root` of the label plane `lab` [H][W], walked from the root: doubled area, box, steps and status
// (contour_walk.h; a neighbour outside the plane is background).  emit(k, x, y) gets kept point k; a caller that wants no points passes an
// empty one.  The caller turns a status other than kContourOk into its error.
template <typename Emit>
inline ContourResult walk_label_contour(const int* lab, int H, int W, int root, long long max_steps, Emit emit)
{
    auto nb = [&](int x, int y) {
        unsigned m = 0;
        for (int d = 0; d < 8; ++d) {
            const int xx = x + contour_step_x(d), yy = y + contour_step_y(d);
            if ((unsigned)xx < (unsigned)W && (unsigned)yy < (unsigned)H && lab[(size_t)yy * W + xx] == root) m |= 1u << d;
        }
        return m;
    };
    return contour_walk(nb, root % W, root / W, max_steps, emit);
}

// The label plane of mask != 0 (flood fill from every first pixel in raster order) and one record per component, in raster order of roots.
inline void label_mask(const uint8_t* mask, int H, int W, std::vector<int>& lab, std::vector<LabelComp>& comps)
{
    const long n = (long)H * W;
    lab.assign((size_t)n, -1);
    comps.clear();
    std::vector<long> stack;
    for (long s = 0; s < n; ++s) {
        if (!mask[s] || lab[s] >= 0) continue;
        LabelComp k = {(int)s, W, H, -1, -1, 0};
        stack.assign(1, s);
        lab[s] = (int)s;
        while (!stack.empty()) {
            const long i = stack.back();
            stack.pop_back();
            const int y = (int)(i / W), x = (int)(i - (long)y * W);
            ++k.pixels;
            k.x0 = x < k.x0 ? x : k.x0; k.x1 = x > k.x1 ? x : k.x1; k.y0 = y < k.y0 ? y : k.y0; k.y1 = y > k.y1 ? y : k.y1;
            for (int d = 0; d < 8; ++d) {
                const int yy = y + contour_step_y(d), xx = x + contour_step_x(d);
                if ((unsigned)yy >= (unsigned)H || (unsigned)xx >= (unsigned)W) continue;
                const long j = (long)yy * W + xx;
                if (mask[j] && lab[j] < 0) { lab[j] = (int)s; stack.push_back(j); }
            }
        }
        comps.push_back(k);
    }
}

inline long long label_comp_step_bound(const LabelComp& k) { return contour_step_bound((long long)(k.x1 - k.x0 + 1) * (k.y1 - k.y0 + 1)); }

// extract_page's ranking, exact, on the host (main.py:398-404): cv2.findContours(RETR_TREE) + cv2.contourArea + np.argmax.  Only the OUTER
// contour of a component can win (a hole's contour lies inside it), so: label the mask, walk every component's outer border, keep the
// largest doubled area.  Ties: the LAST component in raster order of first pixels [EXT, restated from OpenCV's contours.cpp, unpinned: the
// border-following scanner discovers outer borders in raster order and cvInsertNodeIntoTree puts each new contour at the HEAD of its
// parent's child list, so the list findContours returns runs in REVERSE discovery order and np.argmax's "first maximum" (main.py:400-401)
// is the last one discovered].
struct LargestContour {
    bool any;               // false: an empty mask
    LabelComp comp;         // the winner
    long long area2;        // its doubled contour area (0 for an empty mask)
    int bad_root, status;   // status != kContourOk: the walk of component bad_root ended early (cannot happen on label_mask's plane)
};
inline LargestContour host_largest_contour(const uint8_t* mask, int H, int W)
{
    std::vector<int> lab;
    std::vector<LabelComp> comps;
    label_mask(mask, H, W, lab, comps);
    LargestContour best = {false, {-1, 0, 0, -1, -1, 0}, 0, -1, kContourOk};
    for (const LabelComp& k : comps) {
        const ContourResult r = walk_label_contour(lab.data(), H, W, k.root, label_comp_step_bound(k), [](int, int, int) {});
        if (r.status != kContourOk) {
            best.bad_root = k.root; best.status = r.status;
            return best;
        }
        if (!best.any || r.area2 >= best.area2) { best.any = true; best.comp = k; best.area2 = r.area2; }      // ties: the later one
    }
    return best;
}

}  // namespace sbbseg

#endif
