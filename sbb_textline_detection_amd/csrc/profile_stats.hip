// profile_stats.hip -- the host half of the deskew search on the device: for every (region, angle) row profile of a sweep the statistic of
// get_standard_deviation_of_summed_textline_patch_along_width (main.py:1545-1599), then per region the angle selection of
// return_deskew_slope (main.py:1630-1667).  The arithmetic is profile_stat.h's, shared with the CPU entry point and bit for bit scipy's /
// numpy's float64 results; this file only deals it out:
//   * one wave owns one profile.  The two Gaussian smoothings (of y, and of the padded, flipped profile) are independent per sample and run
//     across the lanes, as do both peak scans: "does a peak start at sample i" needs no neighbour's answer.  The maxima above 10 are
//     compacted IN ORDER with a ballot (the pairwise sum of their mean depends on the order); the minima only feed two "is there any"
//     questions;
//   * numpy's pairwise sums (mean of the maxima, mean and squared deviations of z) keep numpy's order on lane 0;
//   * the smoothed profile z and the smoothed flipped profile live in LDS up to kProfileLdsSamples samples; longer profiles run in a second
//     instantiation of the same kernel on a workspace in global memory.  Both give the same bits;
//   * region table, weights and offsets are wave-uniform and read through the scalar cache (loads only), like region_deskew.hip's tables;
//   * no FMA contraction (profile_stat.h), no float64 divide or sqrt instruction sequences: a build test holds the kernels to that.
#include "internal.h"
#include "profile_stat.h"

namespace sbbseg {

namespace {

template <bool kLds>
__global__ __launch_bounds__(64) void profile_stat_kernel(const ProfileStatParams p)
{
#pragma clang fp contract(off)
    __shared__ double lds_z[kLds ? kProfileLdsSamples : 1];
    __shared__ double lds_g[kLds ? kProfileLdsSamples + kProfileFlipExtra : 1];
    __shared__ PairwiseStack stack;
    __shared__ double below_sh;
    const int lane = threadIdx.x;
    const int r = blockIdx.x / p.n_angles, a = blockIdx.x - r * p.n_angles;     // block-uniform
    const ProfileRegion& reg = p.regions[r];
    const int n = reg.S;
    if ((n <= kProfileLdsSamples) != kLds) return;
    const int nf = n + kProfileFlipExtra;
    const int32_t* y = p.counts + reg.count_off + (size_t)a * n;
    double *z, *g;
    if constexpr (kLds) {
        z = lds_z; g = lds_g;
    } else {
        z = p.workspace + reg.ws_off + (size_t)a * (size_t)(n + nf); g = z + n;
    }
    const double* w = p.weights;
    const int radius = p.radius;

    int top = 0;                                                    // max(padded) = max(0, max(y))
    for (int i = lane; i < n; i += 64) top = max(top, y[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) top = max(top, __shfl_xor(top, off, 64));

    const ProfileSamples ys{y};
    for (int i = lane; i < n; i += 64) z[i] = smooth_sample(ys, n, w, radius, i);
    __syncthreads();

    // maxima of z above 10, compacted in order into g (not yet in use)
    int m = 0;
    for (int base = 1; base < n - 1; base += 64) {
        const int i = base + lane;
        bool keep = false;
        double v = 0.0;
        if (i < n - 1) {
            int mid;
            if (peak_starts_at(z, n, i, &mid)) { v = z[mid]; keep = v >= 0.0 && v > 10.0; }
        }
        const unsigned long long mask = __ballot(keep);
        if (keep) g[m + __popcll(mask & ((1ull << lane) - 1ull))] = v;
        m += __popcll(mask);
    }
    __syncthreads();
    if (lane == 0) below_sh = deep_level(g, m, p.multiplier, &stack);
    __syncthreads();
    const double below = below_sh;
    __syncthreads();                                                // every lane holds `below` before g is overwritten

    const FlippedSamples fs{y, n, (double)top};
    for (int k = lane; k < nf; k += 64) g[k] = smooth_sample(fs, nf, w, radius, k);
    __syncthreads();

    bool oob = false, deep = false;
    for (int k = 1 + lane; k < nf - 1; k += 64) {
        int mid;
        if (!peak_starts_at(g, nf, k, &mid) || !(g[mid] >= 0.0)) continue;
        const int cls = classify_minimum(z, n, mid, below);
        oob |= cls == 2;
        deep |= cls == 1;
    }
    oob = __any(oob);
    deep = __any(deep);
    if (lane == 0) {
        const int state = oob ? kProfileException : (deep ? kProfileAppended : kProfileSkipped);
        double spread = 0.0;
        if (state == kProfileAppended) spread = std_of(z, n, &stack);
        p.spread[blockIdx.x] = spread;
        p.state[blockIdx.x] = (uint8_t)state;
        if (p.below) p.below[blockIdx.x] = below;
    }
    if (p.smooth) {                                                 // (debug entry point only: z is not written after the first smoothing)
        double* out = p.smooth + reg.count_off + (size_t)a * n;
        for (int i = lane; i < n; i += 64) out[i] = z[i];
    }
}

// one thread per region: the winner of its sweep
__global__ __launch_bounds__(64) void profile_winner_kernel(const ProfileStatParams p)
{
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= p.n_regions) return;
    p.winner[r] = sweep_winner(p.spread + (size_t)r * p.n_angles, p.state + (size_t)r * p.n_angles, p.n_angles);
}

// soft_div / soft_sqrt on operands of any class, one per thread (sbbseg_debug_soft_arith)
__global__ __launch_bounds__(256) void soft_arith_kernel(int op, const double* a, const double* b, long long n, double* out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = op == 0 ? soft_div(a[i], b[i]) : soft_sqrt(a[i]);
}

}  // namespace

hipError_t launch_soft_arith(int op, const double* a, const double* b, long long n, double* out, hipStream_t s)
{
    hipLaunchKernelGGL(soft_arith_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, op, a, b, n, out);
    return hipGetLastError();
}

hipError_t launch_profile_statistics(const ProfileStatParams& p, bool any_long, hipStream_t s)
{
    const unsigned grid = (unsigned)(p.n_regions * p.n_angles);
    hipLaunchKernelGGL(profile_stat_kernel<true>, dim3(grid), dim3(64), 0, s, p);
    if (any_long) hipLaunchKernelGGL(profile_stat_kernel<false>, dim3(grid), dim3(64), 0, s, p);
    hipLaunchKernelGGL(profile_winner_kernel, dim3((unsigned)((p.n_regions + 63) / 64)), dim3(64), 0, s, p);
    return hipGetLastError();
}

}  // namespace sbbseg
