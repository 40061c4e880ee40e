// line_extent.hip -- the x extents of the text lines of every region of a call from the regions' filled, rotated contours.  The arithmetic is
// line_extent.h's (rules R1 .. R6 there), shared with the serial host twin; this file only deals it out.  All regions share the launches:
//   * fill: work items of (region, 8 rows) from prefix sums, a wave per row of the box.  Every lane owns one 32-pixel word of the row and
//     runs over the ring's edges (wave-uniform); the crossings' parity is a prefix xor inside the word and a ballot across the words.  The
//     wave of row 0 also checks the ring (chain edges, points inside the box) and writes the region's status;
//   * warp + threshold: the same work items, a wave per destination row, 64 bit-map columns per round; the sixteen taps are integer adds
//     of int64 table entries selected by the source bits, the result is one ballot per round, stored as two words of threshrot's bit map
//     (box + ring of zeros);
//   * border scan: one wave per region on threshrot's bit map and two planes of mark bits -- all three in LDS, or (beyond the LDS limit)
//     the bit map where it lies and the marks in a global workspace.  The lanes look for the next word with a border start 64 words at a
//     time; every walk runs the same in every lane (wave-uniform values, broadcast reads) and ends after contour_step_bound steps at the
//     latest.  A first launch counts the borders and records the winner, a second one re-walks the winner and stores its kept points at
//     the offsets the host summed from the counts;
//   * extents: a wave per (region, line): the 1000 samples go round the lanes, each against the winner's edges; first and last inside
//     sample by a wave reduction; lane 0 rewrites the corners through line_split.h's writer.
// One wave per region for the scan is chosen, not measured.  No atomics: every output is a plain vector store and the tables come out
// bit-identical from run to run.
#include "device_prims.h"
#include "line_extent.h"
#include "line_split.h"

namespace sbbseg {

namespace {

constexpr int kExtentBlock = 64 * kExtentRows;

// the region a work item of the fill / warp kernels belongs to (block0 ascends strictly: every region has at least one row)
__device__ __forceinline__ int extent_region_of_block(const ExtentParams& p, int block)
{
    int lo = 0, hi = p.n_regions - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (p.regions[mid].block0 <= block) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(kExtentBlock) void extent_fill_kernel(const ExtentParams p)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = extent_region_of_block(p, blockIdx.x);           // block-uniform
    const ExtentRegion& g = p.regions[r];
    const int py = ((int)blockIdx.x - g.block0) * kExtentRows + wave, w = g.w, h = g.h, ox = g.ox, oy = g.oy;
    const long long first = p.point_off[r];
    const int n = (int)(p.point_off[r + 1] - first);
    const int32_t* pts = p.points + 2 * first;
    if (py == 0) {
        bool bad = n <= 0;
        for (int i = lane; i < n; i += 64) {
            const int j = i + 1 < n ? i + 1 : 0;
            bad = bad || !extent_edge_ok(pts[2 * i] - ox, pts[2 * i + 1] - oy, pts[2 * j] - ox, pts[2 * j + 1] - oy, w, h);
        }
        const bool any_bad = __ballot(bad) != 0ull;
        if (lane == 0) p.rec[(size_t)r * kExtentRecInts + kExtentRecStatus] = any_bad ? kExtentBadRing : kExtentOk;
    }
    if (py >= h) return;                                            // (wave-uniform)
    const int stride = extent_src_stride(w);
    uint32_t* row = p.bits + g.src_off + (size_t)py * stride;
    uint32_t carry = 0;
    for (int w0 = 0; w0 < stride; w0 += 64) {
        const int wi = w0 + lane;
        uint32_t edge = 0, toggles = 0;
        for (int i = 0; i < n; ++i) {
            const int j = i + 1 < n ? i + 1 : 0;
            const ExtentEdgeRow e = extent_edge_row(pts[2 * i] - ox, pts[2 * i + 1] - oy, pts[2 * j] - ox, pts[2 * j + 1] - oy, py);
            edge |= extent_span_bits(e.lo, e.hi, 32 * wi);
            if (e.cross >= 0) toggles ^= extent_span_bits(e.cross, e.cross, 32 * wi);
        }
        uint32_t par = extent_prefix_xor(toggles);
        const unsigned long long odd = __ballot((par >> 31) != 0u);     // words that leave the parity flipped for those behind them
        const uint32_t below = (uint32_t)__popcll(odd & ((1ull << lane) - 1ull)) & 1u;
        par ^= (below ? ~0u : 0u) ^ carry;
        carry ^= (__popcll(odd) & 1) ? ~0u : 0u;
        if (wi < stride) row[wi] = (edge | par) & extent_span_bits(0, w - 1, 32 * wi);
    }
}

__global__ __launch_bounds__(kExtentBlock) void extent_warp_kernel(const ExtentParams p)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = extent_region_of_block(p, blockIdx.x);
    const ExtentRegion& g = p.regions[r];
    const int y = ((int)blockIdx.x - g.block0) * kExtentRows + wave, w = g.w, h = g.h;
    if (y >= h) return;
    const uint32_t* src = p.bits + g.src_off;
    const int stride = contour_bitmap_stride(w);
    uint32_t* row = p.bits + g.dst_off + (size_t)(y + 1) * stride;
    const double m0 = g.minv[0], m3 = g.minv[3];
    long long X0, Y0;
    line_mask_row_origin(g.minv, y, &X0, &Y0);
    for (int base = 0; base < 32 * stride; base += 64) {            // bit-map columns base .. base + 63 = pixels base - 1 .. base + 62
        const int x = base + lane - 1;
        const bool set = x >= 0 && x < w && extent_pixel(src, w, h, m0, m3, X0, Y0, x, p.wtab);
        const unsigned long long word = __ballot(set);
        if (lane == 0) {
            row[base >> 5] = (uint32_t)word;
            if ((base >> 5) + 1 < stride) row[(base >> 5) + 1] = (uint32_t)(word >> 32);
        }
    }
}

struct ExtentWaveNext {
    const ExtentMap* m;
    int lane;
    __device__ __forceinline__ int operator()(int y, int from) const
    {
        for (int base = from; base < m->stride; base += 64) {
            const int wi = base + lane;
            const bool any = wi < m->stride && extent_events(*m, y, wi) != 0u;
            const unsigned long long mask = __ballot(any);
            if (mask) return __builtin_amdgcn_readfirstlane(base + (int)__builtin_ctzll(mask));
        }
        return m->stride;
    }
};

// kept point k of the winner: staged, and stored by the whole wave when the stage is full (as the contour tracer does)
struct ExtentStagedEmit {
    int2* stage;
    int2* out;
    int lane;
    __device__ __forceinline__ void operator()(int k, int x, int y) const
    {
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
        const int rest = n_points & (kContourStage - 1);
        __syncthreads();
        if (lane < rest) out[n_points - rest + lane] = stage[lane];
        __syncthreads();
    }
};

template <bool kLds>
__global__ __launch_bounds__(64) void extent_scan_kernel(const ExtentParams p)
{
    __shared__ uint32_t lds[kLds ? kExtentLdsBytes / 4 : 1];
    __shared__ int2 stage[kContourStage];
    const int lane = threadIdx.x, r = blockIdx.x;
    const ExtentRegion& g = p.regions[r];
    const int w = g.w, h = g.h, stride = contour_bitmap_stride(w);
    const long long words = contour_bitmap_bytes(w, h) / 4;
    if ((3 * words * 4 <= (long long)p.lds_limit) != kLds) return;  // (block-uniform) the other instantiation's region
    int32_t* rec = p.rec + (size_t)r * kExtentRecInts;
    const int status = rec[kExtentRecStatus];
    const bool emit_pass = p.winner != nullptr;
    if (status != kExtentOk) return;                                // a bad ring; in the second pass also: no border, a broken walk
    ExtentMap m;
    m.stride = stride; m.w = w; m.h = h;
    const uint32_t* pix = p.bits + g.dst_off;
    if (kLds) {
        for (long long i = lane; i < words; i += 64) {
            lds[i] = pix[i];
            if (!emit_pass) { lds[words + i] = 0u; lds[2 * words + i] = 0u; }
        }
        __syncthreads();
        m.pix = lds; m.vis = lds + words; m.right = lds + 2 * words;
    } else {
        m.pix = pix; m.vis = p.marks + g.mark_off; m.right = m.vis + words;     // (zeroed by the host side)
    }
    if (!emit_pass) {
        const ExtentWinner win = extent_scan(m, ExtentWaveNext{&m, lane});
        if (lane == 0) {
            rec[kExtentRecStatus] = win.status; rec[kExtentRecBorders] = win.borders; rec[kExtentRecPoints] = win.n_points;
            rec[kExtentRecHole] = win.is_hole; rec[kExtentRecTie] = win.tie; rec[kExtentRecStartX] = win.sx; rec[kExtentRecStartY] = win.sy;
            rec[kExtentRecHoles] = win.holes;
        }
    } else {
        const ExtentStagedEmit emit{stage, (int2*)p.winner + g.win_off, lane};
        const ContourResult res = contour_walk_from(ExtentNb{m.pix, stride}, rec[kExtentRecStartX], rec[kExtentRecStartY],
                                                    rec[kExtentRecHole] ? 0 : 4, contour_step_bound((long long)w * h), emit, ContourNoMark{});
        emit.finish(res.n_points);
    }
}

__global__ __launch_bounds__(64) void extent_lines_kernel(const ExtentParams p)
{
    const int lane = threadIdx.x, slot = blockIdx.x;
    int lo = 0, hi = p.n_regions - 1;                               // (line_off ascends strictly: every region has room for lines)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (p.regions[mid].line_off <= slot) lo = mid;
        else hi = mid - 1;
    }
    const ExtentRegion& g = p.regions[lo];
    const int32_t* info = p.info + (size_t)lo * kLineInfoInts;
    if (info[kLineInfoStatus] != kLineOk || slot - g.line_off >= info[kLineInfoCount]) return;
    const int32_t* rec = p.rec + (size_t)lo * kExtentRecInts;
    const int branch = info[kLineInfoBranch], w = g.w;
    const bool rewrite = !g.vertical && rec[kExtentRecStatus] == kExtentOk && branch != kLineBranchOnePeak;
    const int peak = p.lines[3 * (size_t)slot], up = p.lines[3 * (size_t)slot + 1], down = p.lines[3 * (size_t)slot + 2];
    int x_min = 0, x_max = w;
    if (rewrite) {
        const int32_t* pts = p.winner + 2 * g.win_off;
        const int n = rec[kExtentRecPoints];
        const double step = g.step;
        int kmin = kExtentSamples, kmax = -1;
        for (int k = lane; k < kExtentSamples; k += 64)
            if (extent_inside(pts, n, (float)extent_sample(k, step, w), (float)peak)) {
                kmin = k < kmin ? k : kmin;
                kmax = k;
            }
        kmax = wave_max(kmax);
        kmin = -wave_max(-kmin);
        if (kmax >= 0) {
            x_min = (int)extent_sample(kmin, step, w);
            x_max = (int)extent_sample(kmax, step, w);
        }
    }
    if (lane != 0) return;
    p.extent[2 * (size_t)slot] = x_min;
    p.extent[2 * (size_t)slot + 1] = x_max;
    if (!rewrite) return;
    LineGeom lg;
    lg.n = g.h; lg.other = w; lg.vertical = 0;
    lg.r00 = g.rot[0]; lg.r01 = g.rot[1]; lg.r10 = g.rot[2]; lg.r11 = g.rot[3]; lg.xd = g.rot[4]; lg.yd = g.rot[5];
    line_box_with_extent(lg, x_min, x_max, up, down, p.box + 8 * (size_t)slot, p.rot + 8 * (size_t)slot);
}

}  // namespace

hipError_t launch_extent_masks(const ExtentParams& p, hipStream_t s)
{
    hipLaunchKernelGGL(extent_fill_kernel, dim3((unsigned)p.total_blocks), dim3(kExtentBlock), 0, s, p);
    hipLaunchKernelGGL(extent_warp_kernel, dim3((unsigned)p.total_blocks), dim3(kExtentBlock), 0, s, p);
    return hipGetLastError();
}

// Both forms take every region and skip those of the other form; a form no region takes is not launched.  p.winner == nullptr: the
// counting pass.
hipError_t launch_extent_scan(const ExtentParams& p, bool any_lds, bool any_global, hipStream_t s)
{
    if (any_lds) hipLaunchKernelGGL(extent_scan_kernel<true>, dim3((unsigned)p.n_regions), dim3(64), 0, s, p);
    if (any_global) hipLaunchKernelGGL(extent_scan_kernel<false>, dim3((unsigned)p.n_regions), dim3(64), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_extent_lines(const ExtentParams& p, hipStream_t s)
{
    hipLaunchKernelGGL(extent_lines_kernel, dim3((unsigned)p.total_lines), dim3(64), 0, s, p);
    return hipGetLastError();
}

}  // namespace sbbseg
