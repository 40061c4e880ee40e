// line_split.hip -- the text lines of every region of a page from the projection of its deskewed mask (seperate_lines, main.py:516-991,
// and seperate_lines_vertical, main.py:993-1457, after `img_patch.sum`).  The arithmetic is line_split.h's, shared with the CPU entry point
// and bit for bit scipy's / numpy's float64 results; this file only deals it out, like profile_stats.hip:
//   * one wave owns one region.  Each of the two passes (sigma 2, then the region's own sigma_gaus) smooths y_padded and the padded,
//     flipped profile across the lanes and scans both for maxima across the lanes; the maxima are compacted IN ORDER with a ballot (order
//     decides the cluster logic and numpy's pairwise sums);
//   * the cluster bookkeeping, the sigma estimate and the mean / std of the peak values run on lane 0;
//   * the boxes are written one line per lane;
//   * the arrays live in LDS up to kProfileLdsSamples profile samples; longer profiles run in a second instantiation of the same kernel on
//     a workspace in global memory.  Both give the same bits;
//   * region table, offsets and weights are wave-uniform and read through the scalar cache (loads only);
//   * every output is a plain vector store: no atomics, and the output buffers need no zero fill (a region writes its info and its first
//     `count` lines, nothing else);
//   * no FMA contraction, no float64 divide or sqrt instruction sequences: a build test holds the kernels to that.
#include "internal.h"
#include "line_split.h"

namespace sbbseg {

namespace {

constexpr size_t kLineSplitLdsBytes = line_work_bytes(kProfileLdsSamples);

// the maxima >= 0 of x[0 .. n), in order, into out; every lane returns their number
__device__ __forceinline__ int line_compact_peaks(const double* x, int n, int32_t* out, int lane)
{
    int m = 0;
    for (int base = 1; base < n - 1; base += 64) {
        const int i = base + lane;
        int mid = 0;
        const bool keep = i < n - 1 && line_peak_at(x, n, i, &mid);
        const unsigned long long mask = __ballot(keep);
        if (keep) out[m + __popcll(mask & ((1ull << lane) - 1ull))] = mid;
        m += __popcll(mask);
    }
    return m;
}

__device__ __forceinline__ void line_pass(const int32_t* y, int n, double top, const double* w, int sigma, const LineWork& k, int lane, int* P, int* Q)
{
    const int na = n + 2 * kLinePad, nb = n + 4 * kLinePad, radius = 4 * sigma;
    const PaddedSamplesP ys{y, n, kLinePad};
    const FlippedSamplesP fs{y, n, kLinePad, top};
    for (int i = lane; i < na; i += 64) k.a()[i] = smooth_sample(ys, na, w, radius, i);
    for (int i = lane; i < nb; i += 64) k.b()[i] = smooth_sample(fs, nb, w, radius, i);
    __syncthreads();
    *P = line_compact_peaks(k.a(), na, k.peaks(), lane);
    *Q = line_compact_peaks(k.b(), nb, k.negs(), lane);
    __syncthreads();
}

template <bool kLds>
__global__ __launch_bounds__(64) void line_split_kernel(const LineSplitParams p)
{
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) unsigned char lds_work[kLds ? kLineSplitLdsBytes : 16];
    __shared__ PairwiseStack stack;
    __shared__ LineSummary summary;
    __shared__ int sigma_sh;
    const int lane = threadIdx.x;
    const LineSplitRegion& reg = p.regions[blockIdx.x];             // block-uniform
    const int n = reg.n;
    if ((n <= kProfileLdsSamples) != kLds) return;
    const int32_t* y = p.profiles + reg.prof_off;
    const LineWork k{kLds ? lds_work : p.workspace + reg.ws_off, n, &stack};
    int32_t* info = p.info + (size_t)blockIdx.x * kLineInfoInts;

    int top = 0;                                                    // max(y_padded) = max(0, max(y))
    for (int i = lane; i < n; i += 64) top = max(top, y[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) top = max(top, __shfl_xor(top, off, 64));

    int P, Q;
    line_pass(y, n, (double)top, p.weights, kLineSigmaMin, k, lane, &P, &Q);       // (the table starts with sigma 2)
    if (lane == 0) {
        int raised;
        const int sigma = line_first_sigma(k, P, Q, &raised);
        info[kLineInfoSigma] = sigma; info[kLineInfoRaised] = raised;
        sigma_sh = sigma;
    }
    __syncthreads();
    const int sigma = sigma_sh;
    if (sigma > p.sigma_max) {
        if (lane == 0) { info[kLineInfoStatus] = kLineSigmaTooLarge; info[kLineInfoBranch] = kLineBranchNotReached; info[kLineInfoCount] = 0; }
        return;
    }
    line_pass(y, n, (double)top, p.weights + p.weight_off[sigma - kLineSigmaMin], sigma, k, lane, &P, &Q);
    if (lane == 0) {
        LineGeom g0;
        g0.n = n; g0.other = 0; g0.vertical = reg.vertical;        // (line_second reads nothing else)
        summary = line_second(k, g0, P, Q);
        info[kLineInfoStatus] = summary.status; info[kLineInfoBranch] = summary.branch; info[kLineInfoCount] = summary.count;
    }
    __syncthreads();
    const LineSummary s = summary;
    if (s.count == 0) return;
    LineGeom g;                                                     // (read late: the rotation terms are twelve scalar registers)
    g.n = n; g.other = reg.other; g.vertical = reg.vertical;
    g.r00 = reg.rot[0]; g.r01 = reg.rot[1]; g.r10 = reg.rot[2]; g.r11 = reg.rot[3]; g.xd = reg.rot[4]; g.yd = reg.rot[5];
    for (int jj = lane; jj < s.count; jj += 64) {
        const size_t at = (size_t)reg.line_off + jj;
        line_box(k, g, s, jj, p.pts + at * 3, p.box + at * 8, p.rot + at * 8);
    }
}

}  // namespace

// Both forms are launched over ALL regions and a block whose region belongs to the other form returns at once (before it touches its LDS):
// the launch count does not depend on the regions, and a page has tens of them, so the idle blocks cost less than a compacted list would.
hipError_t launch_line_split(const LineSplitParams& p, bool any_long, hipStream_t s)
{
    hipLaunchKernelGGL(line_split_kernel<true>, dim3((unsigned)p.n_regions), dim3(64), 0, s, p);
    if (any_long) hipLaunchKernelGGL(line_split_kernel<false>, dim3((unsigned)p.n_regions), dim3(64), 0, s, p);
    return hipGetLastError();
}

}  // namespace sbbseg
