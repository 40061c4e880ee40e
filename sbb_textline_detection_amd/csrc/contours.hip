// contours.hip -- the outer contour polygons of the components of a labelled plane (get_text_region_contours_and_boxes' contours,
// main.py:456-481: cv2.findContours(RETR_TREE, CHAIN_APPROX_SIMPLE) of the opened / closed class mask).  The walk itself is
// contour_walk.h's, shared with the host twin; this file deals it out:
//   * one wave owns one candidate root at a time (a block is one wave; more candidates than blocks: the blocks stride over the list);
//   * the LDS form first builds a bit map of `label == root` over the root's bounding box plus a one-pixel ring of zeros -- 32-bit words,
//     one row stride; the lanes read the int32 label plane along rows and pack 64 pixels with a ballot.  The test is the LABEL, not the
//     mask: another component may lie inside the box.  The ring takes every bounds test out of the walk;
//   * the global form (a bit map beyond the LDS limit) walks on the label plane itself and clips to the plane;
//   * the walk is the same in every lane (wave-uniform values, broadcast LDS reads); kept points are staged in LDS and the whole wave
//     stores them kContourStage at a time with plain vector stores;
//   * a walk ends after contour_step_bound(box pixels) steps at the latest, with a status the host turns into an error;
//   * two launches of the same kernel: a counting one (points, doubled area, box, status per candidate), then -- after contour_pack_kernel
//     has filtered the candidates and summed the point counts in candidate order -- a writing one.  No atomics: the tables are packed in
//     candidate order and come out bit-identical from run to run.
#include "internal.h"
#include "contour_walk.h"

namespace sbbseg {

namespace {

constexpr int kContourMaxBlocks = 1024;             // blocks of one tracer launch (four waves' worth per CU of a 256-CU device)

struct BitmapNb {
    const uint32_t* bits;     // row 0 = the ring above the box
    int stride, ox, oy;       // plane coordinates of bit map column / row 0
    __device__ __forceinline__ unsigned three(const uint32_t* p, int sh) const
    {
        return (unsigned)((((unsigned long long)p[1] << 32) | p[0]) >> sh) & 7u;      // columns x - 1, x, x + 1
    }
    __device__ __forceinline__ unsigned operator()(int x, int y) const
    {
        const int bx = x - ox - 1, by = y - oy - 1;             // the field's first column, the row above
        const uint32_t* p = bits + by * stride + (bx >> 5);
        const int sh = bx & 31;
        const unsigned a = three(p, sh), b = three(p + stride, sh), c = three(p + 2 * stride, sh);
        // E, SE, S, SW, W, NW, N, NE
        return ((b >> 2) & 1u) | (((c >> 2) & 1u) << 1) | (((c >> 1) & 1u) << 2) | ((c & 1u) << 3) | ((b & 1u) << 4) | ((a & 1u) << 5) |
               (((a >> 1) & 1u) << 6) | (((a >> 2) & 1u) << 7);
    }
};

struct PlaneNb {
    const int* parent;
    int H, W, root;
    __device__ __forceinline__ unsigned operator()(int x, int y) const
    {
        unsigned m = 0;
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            const int xx = x + contour_step_x(d), yy = y + contour_step_y(d);
            if ((unsigned)xx < (unsigned)W && (unsigned)yy < (unsigned)H && parent[(size_t)yy * W + xx] == root) m |= 1u << d;
        }
        return m;
    }
};

// kept point k of the contour: staged, and stored by the whole wave when the stage is full.  `out` == nullptr: the counting pass
struct StagedEmit {
    int2* stage;
    int2* out;
    int lane;
    __device__ __forceinline__ void operator()(int k, int x, int y) const
    {
        if (!out) return;
        const int at = k & (kContourStage - 1);
        if (lane == 0) stage[at] = make_int2(x, y);
        if (at == kContourStage - 1) {
            __syncthreads();
            out[k - (kContourStage - 1) + lane] = stage[lane];
            __syncthreads();
        }
    }
    __device__ __forceinline__ void finish(int n_points) const
    {
        if (!out) return;
        const int rest = n_points & (kContourStage - 1);
        __syncthreads();
        if (lane < rest) out[n_points - rest + lane] = stage[lane];
        __syncthreads();
    }
};

template <bool kLds>
__global__ __launch_bounds__(64) void contour_trace_kernel(const ContourParams p)
{
    __shared__ uint32_t bits[kLds ? kContourLdsBytes / 4 : 1];
    __shared__ int2 stage[kContourStage];
    const int lane = threadIdx.x;
    for (int k = blockIdx.x; k < p.n_cand; k += gridDim.x) {
        const ContourCand c = p.cand[k];                        // block-uniform
        const int form = contour_form(c.root, c.x0, c.y0, c.x1, c.y1, p.H, p.W, p.lds_limit);
        if ((form == kContourFormLds) != kLds) continue;        // (a bad record goes to the global form, which reports it)
        int2* out = nullptr;
        if (p.points) {
            const int slot = p.slot[k];
            if (slot < 0) continue;
            out = (int2*)p.points + p.point_off[slot];
        }
        if (form == kContourFormBad) {
            if (lane == 0) {
                ContourRec rec = {};
                rec.status = kContourBadBox;
                p.rec[k] = rec;
            }
            continue;
        }
        const int w = c.x1 - c.x0 + 1, h = c.y1 - c.y0 + 1;
        const int sx = c.root % p.W, sy = c.root / p.W;
        const long long bound = contour_step_bound((long long)w * h);
        const StagedEmit emit{stage, out, lane};
        ContourResult r;
        if (kLds) {
            const int stride = contour_bitmap_stride(w), chunks = (stride + 1) >> 1, total = chunks * (h + 2);
            __syncthreads();                                    // (the previous candidate's walk has ended in every lane)
            for (int t0 = 0; t0 < total; t0 += 4) {             // four 64-pixel pieces per round: their loads are in flight together
                int label[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int row = (t0 + u) / chunks, col = (t0 + u - row * chunks) * 64 + lane;
                    const bool in = row >= 1 && row <= h && col >= 1 && col <= w;      // (t0 + u >= total: row > h)
                    label[u] = in ? p.parent[(size_t)(c.y0 - 1 + row) * p.W + (c.x0 - 1 + col)] : -1;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int row = (t0 + u) / chunks, ch = t0 + u - row * chunks;
                    const unsigned long long word = __builtin_amdgcn_ballot_w64(label[u] == c.root);
                    if (lane == 0 && t0 + u < total) {
                        bits[row * stride + 2 * ch] = (uint32_t)word;
                        if (2 * ch + 1 < stride) bits[row * stride + 2 * ch + 1] = (uint32_t)(word >> 32);
                    }
                }
            }
            if (lane == 0) bits[(h + 2) * stride] = 0;          // the spare word behind the last row
            __syncthreads();
            r = contour_walk(BitmapNb{bits, stride, c.x0 - 1, c.y0 - 1}, sx, sy, bound, emit);
        } else {
            r = contour_walk(PlaneNb{p.parent, p.H, p.W, c.root}, sx, sy, bound, emit);
        }
        emit.finish(r.n_points);
        if (!p.points && lane == 0) {
            ContourRec rec;
            rec.area2 = r.area2; rec.n_points = r.n_points; rec.status = r.status;
            rec.x = r.x0; rec.y = r.y0; rec.w = r.x1 - r.x0 + 1; rec.h = r.y1 - r.y0 + 1;
            p.rec[k] = rec;
        }
    }
}

// Which candidates are kept and where their points go, in candidate order: one block walks the list in chunks of 256 with an exclusive
// scan of the keep flags and of the point counts.  filter: filter_contours_area_of_image's test (main.py:82-88) -- at least three
// points and lo <= area <= hi; without it every candidate is kept.  totals: contours, points, candidates whose walk failed, the first
// such candidate's status.
__global__ __launch_bounds__(256) void contour_pack_kernel(const ContourPackParams q)
{
    __shared__ int s_keep[256];
    __shared__ long long s_pts[256];
    __shared__ int s_first;
    const int t = threadIdx.x;
    int n_kept = 0, n_bad = 0, first_bad = 0;
    long long n_pts = 0;
    for (int base = 0; base < q.n_cand; base += 256) {
        const int k = base + t;
        ContourRec rec = {};
        bool keep = false, bad = false;
        if (k < q.n_cand) {
            rec = q.rec[k];
            bad = rec.status != kContourOk;
            const double area = (double)rec.area2 * 0.5;
            keep = !bad && (!q.filter || (rec.n_points >= 3 && area >= q.lo && area <= q.hi));
        }
        s_keep[t] = keep ? 1 : 0;
        s_pts[t] = keep ? rec.n_points : 0;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {               // inclusive scan
            const int a = t >= off ? s_keep[t - off] : 0;
            const long long b = t >= off ? s_pts[t - off] : 0;
            __syncthreads();
            s_keep[t] += a; s_pts[t] += b;
            __syncthreads();
        }
        if (k < q.n_cand) {
            const int slot = n_kept + s_keep[t] - 1;
            q.slot[k] = keep ? slot : -1;
            if (keep) {
                q.boxes[4 * slot] = rec.x; q.boxes[4 * slot + 1] = rec.y; q.boxes[4 * slot + 2] = rec.w; q.boxes[4 * slot + 3] = rec.h;
                q.area2[slot] = rec.area2;
                q.point_off[slot] = n_pts + s_pts[t] - rec.n_points;
            }
        }
        const int chunk_bad = __syncthreads_count(bad);
        if (chunk_bad && !n_bad) {                              // the first failed candidate of the list
            if (t == 0) s_first = 1 << 30;
            __syncthreads();
            if (bad) atomicMin(&s_first, t);
            __syncthreads();
            first_bad = q.rec[base + s_first].status;
        }
        n_bad += chunk_bad;
        n_kept += s_keep[255];
        n_pts += s_pts[255];
        __syncthreads();
    }
    if (t == 0) {
        q.point_off[n_kept] = n_pts;
        q.totals[0] = n_kept; q.totals[1] = n_pts; q.totals[2] = n_bad; q.totals[3] = first_bad;
    }
}

// every root of a labelled plane with its box, in no particular order (the host sorts the list)
__global__ __launch_bounds__(256) void contour_all_roots_kernel(const int* parent, const int* bx0, const int* by0, const int* bx1, const int* by1,
                                                                long n, int* n_found, ContourCand* list, int cap)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || parent[i] != (int)i) return;
    const int k = atomicAdd(n_found, 1);
    if (k >= cap) return;
    list[k] = ContourCand{(int)i, bx0[i], by0[i], bx1[i], by1[i], 0};
}

}  // namespace

hipError_t launch_contour_all_roots(const int* parent, const int* bx0, const int* by0, const int* bx1, const int* by1, long n, int* d_n,
                                    ContourCand* list, int cap, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(d_n, 0, sizeof(int), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(contour_all_roots_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, parent, bx0, by0, bx1, by1, n, d_n, list, cap);
    return hipGetLastError();
}

// Both forms stride over ALL candidates and skip those of the other form (as launch_line_split does); a form no candidate takes is not
// launched.
hipError_t launch_contour_trace(const ContourParams& p, bool any_lds, bool any_global, hipStream_t s)
{
    const unsigned grid = (unsigned)(p.n_cand < kContourMaxBlocks ? p.n_cand : kContourMaxBlocks);
    if (any_lds) hipLaunchKernelGGL(contour_trace_kernel<true>, dim3(grid), dim3(64), 0, s, p);
    if (any_global) hipLaunchKernelGGL(contour_trace_kernel<false>, dim3(grid), dim3(64), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_contour_pack(const ContourPackParams& q, hipStream_t s)
{
    hipLaunchKernelGGL(contour_pack_kernel, dim3(1), dim3(256), 0, s, q);
    return hipGetLastError();
}

}  // namespace sbbseg
