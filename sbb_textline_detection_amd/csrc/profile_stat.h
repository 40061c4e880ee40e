// profile_stat.h -- the 1-D statistic of the deskew search on ONE row profile, as plain float64 C++ for host and device code:
// get_standard_deviation_of_summed_textline_patch_along_width (main.py:1545-1599) as stages._profile_statistics restates it, plus the
// bookkeeping of one angle loop of return_deskew_slope (main.py:1630-1667).  The host path is scipy's gaussian_filter1d / find_peaks and
// numpy's mean / std; everything here reproduces their float64 results bit for bit, so the arg max over the angles (where equal maxima
// do occur: mirrored angles give mirrored profiles) and find_peaks' exact comparisons decide the same.
//
//   * every multiply and add is rounded on its own (no FMA contraction: `fp contract(off)` in every function);
//   * sums are numpy's pairwise sums, in numpy's order;
//   * the few divisions and the square root are done on the integer mantissas (soft_div / soft_sqrt, round to nearest even): the device's
//     float64 divide and sqrt expand to FMA sequences, and the kernels that include this file are held to "no v_fma_f64" by a build test.
#ifndef SBBSEG_PROFILE_STAT_H
#define SBBSEG_PROFILE_STAT_H

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SBB_HD __host__ __device__ __forceinline__
#else
#define SBB_HD inline
#endif

namespace sbbseg {

constexpr int kProfilePad = 10;                     // zeros either side of y, and again either side of max - padded (main.py:1552-1560)
constexpr int kProfileFlipExtra = 4 * kProfilePad;  // len(flipped) - len(y)
enum { kProfileAppended = 0, kProfileSkipped = 1, kProfileException = 2 };

// gaussian_filter1d(., sigma = 2): scipy's _gaussian_kernel1d(2, 0, 8)[8:], the only sigma the reference uses (main.py:1737)
constexpr int kSigma2Radius = 8;
#define SBBSEG_SIGMA2_WEIGHTS                                                                                                              \
    {0x1.98862a07ae7b4p-3, 0x1.68856f9ab1982p-3, 0x1.ef9093fc46e5ap-4, 0x1.0941b71ceef37p-4, 0x1.ba4d4125ffd2ap-6, 0x1.1f30504e20207p-7, \
     0x1.227362b5fc92dp-9, 0x1.c98b8c5d0dda5p-12, 0x1.18aad19e4159bp-14}

SBB_HD uint64_t f64_bits(double x) { uint64_t u; memcpy(&u, &x, 8); return u; }
SBB_HD double f64_from_bits(uint64_t u) { double x; memcpy(&x, &u, 8); return x; }
SBB_HD int clz64(uint64_t v) { return __builtin_clzll(v); }

// a / b, IEEE-754 binary64, round to nearest even, all classes of operands (subnormals included); NaN results are the canonical quiet NaN
SBB_HD double soft_div(double a, double b)
{
    const uint64_t kMant = (1ull << 52) - 1, kInf = 0x7ffull << 52, kNan = 0x7ff8ull << 48;
    const uint64_t ua = f64_bits(a), ub = f64_bits(b), sign = (ua ^ ub) & (1ull << 63);
    int ea = (int)((ua >> 52) & 0x7ff), eb = (int)((ub >> 52) & 0x7ff);
    uint64_t ma = ua & kMant, mb = ub & kMant;
    if (ea == 0x7ff) return f64_from_bits((ma || eb == 0x7ff) ? kNan : (sign | kInf));               // NaN / ., inf / inf, inf / x
    if (eb == 0x7ff) return f64_from_bits(mb ? kNan : sign);                                         // . / NaN, x / inf
    if (eb == 0 && mb == 0) return f64_from_bits((ea == 0 && ma == 0) ? kNan : (sign | kInf));       // 0 / 0, x / 0
    if (ea == 0 && ma == 0) return f64_from_bits(sign);
    if (ea == 0) { const int s = clz64(ma) - 11; ma <<= s; ea = 1 - s; } else ma |= 1ull << 52;
    if (eb == 0) { const int s = clz64(mb) - 11; mb <<= s; eb = 1 - s; } else mb |= 1ull << 52;
    int E = ea - eb + 1023;
    if (ma < mb) { ma <<= 1; --E; }                                 // now 1 <= ma / mb < 2
    uint64_t q = 0, rem = ma;                                       // q = floor(ma / mb * 2^54): 55 bits, restoring division
    for (int i = 0; i < 55; ++i) {
        q <<= 1;
        if (rem >= mb) { rem -= mb; q |= 1; }
        rem <<= 1;
    }
    const uint64_t sticky = rem != 0;
    int shift = 2;                                                  // 53 mantissa bits + guard + round
    if (E <= 0) { shift += 1 - E; E = 0; if (shift > 62) shift = 62; }      // subnormal result (q < 2^55: a longer shift rounds to 0 as well)
    const uint64_t half = 1ull << (shift - 1), lost = q & ((half << 1) - 1);
    uint64_t m = q >> shift;
    if ((lost & half) && ((lost & (half - 1)) || sticky || (m & 1))) ++m;
    if (E == 0) return f64_from_bits(sign | m);                     // (m == 2^52 is the smallest normal: the bit pattern is already right)
    if (m == (1ull << 53)) { m >>= 1; ++E; }
    if (E >= 0x7ff) return f64_from_bits(sign | kInf);
    return f64_from_bits(sign | ((uint64_t)E << 52) | (m & kMant));
}

// sqrt(x), IEEE-754 binary64, round to nearest even
SBB_HD double soft_sqrt(double x)
{
    const uint64_t kMant = (1ull << 52) - 1, kNan = 0x7ff8ull << 48;
    const uint64_t u = f64_bits(x);
    int e = (int)((u >> 52) & 0x7ff);
    uint64_t m = u & kMant;
    if (e == 0 && m == 0) return x;                                 // +-0
    if (e == 0x7ff) return (m || (u >> 63)) ? f64_from_bits(kNan) : x;
    if (u >> 63) return f64_from_bits(kNan);
    if (e == 0) { const int s = clz64(m) - 11; m <<= s; e = 1 - s; } else m |= 1ull << 52;
    e -= 1023;
    if (e & 1) { m <<= 1; --e; }                                    // even exponent, m in [2^52, 2^54)
    uint64_t root = 0, rem = 0;                                     // root = floor(sqrt(m * 2^54)): 54 bits, two radicand bits per step
    for (int i = 0; i < 54; ++i) {
        const uint64_t pair = i < 27 ? (m >> (52 - 2 * i)) & 3 : 0;
        rem = (rem << 2) | pair;
        const uint64_t trial = (root << 2) | 1;
        root <<= 1;
        if (rem >= trial) { rem -= trial; root |= 1; }
    }
    uint64_t r = root >> 1;
    if ((root & 1) && (rem != 0 || (r & 1))) ++r;
    int E = e / 2 + 1023;                                           // (e is even; negative values divide exactly)
    if (r == (1ull << 53)) { r >>= 1; ++E; }
    return f64_from_bits(((uint64_t)E << 52) | (r & kMant));
}

// index i of an array of n samples extended by scipy's mode="reflect" (d c b a | a b c d | d c b a), any i, also for n < radius
SBB_HD int reflect_index(int i, int n)
{
    if ((unsigned)i < (unsigned)n) return i;
    const int p = 2 * n;
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

// the profile y as float64
struct ProfileSamples {
    const int32_t* y;
    SBB_HD double operator()(int i) const { return (double)y[i]; }
};

// `flipped` of main.py:1552-1560: max(padded) - padded between ten zeros on either side, padded = y between ten zeros; n + 40 samples
struct FlippedSamples {
    const int32_t* y;
    int n;
    double top;                                                     // max(padded) = max(0, max(y))
    SBB_HD double operator()(int k) const
    {
#pragma clang fp contract(off)
        if (k < kProfilePad || k >= n + 3 * kProfilePad) return 0.0;
        const int j = k - 2 * kProfilePad;
        return top - (((unsigned)j < (unsigned)n) ? (double)y[j] : 0.0);
    }
};

// The same two arrays for any pad (line_split.h: pad 20, main.py:544-556): y between `pad` zeros, n + 2 * pad samples ...
struct PaddedSamplesP {
    const int32_t* y;
    int n, pad;
    SBB_HD double operator()(int k) const
    {
        const int j = k - pad;
        return ((unsigned)j < (unsigned)n) ? (double)y[j] : 0.0;
    }
};

// ... and max(padded) - padded between another `pad` zeros on either side, n + 4 * pad samples
struct FlippedSamplesP {
    const int32_t* y;
    int n, pad;
    double top;                                                     // max(padded) = max(0, max(y))
    SBB_HD double operator()(int k) const
    {
#pragma clang fp contract(off)
        if (k < pad || k >= n + 3 * pad) return 0.0;
        const int j = k - 2 * pad;
        return top - (((unsigned)j < (unsigned)n) ? (double)y[j] : 0.0);
    }
};

// one sample of scipy.ndimage.gaussian_filter1d(e, sigma) (correlate1d's symmetric branch): w[j] = the normalised weight at distance j
template <class Samples>
SBB_HD double smooth_sample(const Samples& e, int n, const double* w, int radius, int c)
{
#pragma clang fp contract(off)
    double t = e(c) * w[0];
    for (int j = radius; j >= 1; --j) {
        const double pair = e(reflect_index(c - j, n)) + e(reflect_index(c + j, n));
        const double prod = pair * w[j];
        t = t + prod;
    }
    return t;
}

// scipy.signal.find_peaks' _local_maxima_1d, asked about ONE sample: does a peak START at i (1 <= i <= n - 2)?  x[i - 1] < x[i] and the
// run of equal values that starts at i ends in a smaller one; *mid = (first + last) // 2 of the run.  The serial scan visits exactly the
// samples for which this holds (inside a run x[i - 1] == x[i]), in increasing order.
template <class Ptr>
SBB_HD bool peak_starts_at(Ptr x, int n, int i, int* mid)
{
    const double v = x[i];
    if (!(x[i - 1] < v)) return false;
    int ahead = i + 1;
    while (ahead < n - 1 && x[ahead] == v) ++ahead;
    if (!(x[ahead] < v)) return false;
    *mid = (i + ahead - 1) / 2;
    return true;
}

// numpy's pairwise sum (umath loops, DOUBLE_pairwise_sum) of f(0) .. f(n - 1).  The recursion is unrolled on an explicit stack, which the
// caller provides (LDS on the device: a dynamically indexed local array would live in scratch memory).
struct PairwiseStack {
    int off[40], len[40];                                           // pending ranges; len < 0: add the two values on top
    double val[24];
};

template <class F>
SBB_HD double pairwise_block(const F& f, int o, int n)
{
#pragma clang fp contract(off)
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res = res + f(o + i);
        return res;
    }
    double r0 = f(o), r1 = f(o + 1), r2 = f(o + 2), r3 = f(o + 3), r4 = f(o + 4), r5 = f(o + 5), r6 = f(o + 6), r7 = f(o + 7);
    int i;
    for (i = 8; i < n - (n % 8); i += 8) {
        r0 = r0 + f(o + i); r1 = r1 + f(o + i + 1); r2 = r2 + f(o + i + 2); r3 = r3 + f(o + i + 3);
        r4 = r4 + f(o + i + 4); r5 = r5 + f(o + i + 5); r6 = r6 + f(o + i + 6); r7 = r7 + f(o + i + 7);
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i) res = res + f(o + i);
    return res;
}

template <class F>
SBB_HD double pairwise_range(const F& f, int first, int n, PairwiseStack* st)
{
#pragma clang fp contract(off)
    if (n <= 128) return pairwise_block(f, first, n);
    int top = 0, vtop = 0;
    st->off[0] = first; st->len[0] = n; top = 1;
    while (top > 0) {
        --top;
        const int o = st->off[top], l = st->len[top];
        if (l < 0) {
            const double b = st->val[--vtop], a = st->val[--vtop];
            st->val[vtop++] = a + b;
        } else if (l <= 128) {
            st->val[vtop++] = pairwise_block(f, o, l);
        } else {
            int half = l / 2;
            half -= half % 8;
            st->len[top++] = -1;                                    // popped last: left + right
            st->off[top] = o + half; st->len[top++] = l - half;
            st->off[top] = o; st->len[top++] = half;                // popped first
        }
    }
    return st->val[0];
}

// np.add.reduce of f(0) .. f(n - 1) (what np.sum, np.mean and np.std call): numpy hands its add loop at most one ufunc buffer (8192
// elements, numpy's default bufsize) at a time, so the pairwise sum is taken per stretch of 8192 and the stretches are added up in order,
// starting from 0.  Up to 8192 elements that is the pairwise sum of the whole.
constexpr int kNumpySumStretch = 8192;

template <class F>
SBB_HD double pairwise_sum(const F& f, int n, PairwiseStack* st)
{
#pragma clang fp contract(off)
    if (n <= kNumpySumStretch) return pairwise_range(f, 0, n, st);
    double res = 0.0;
    for (int first = 0; first < n; first += kNumpySumStretch) {
        const int len = n - first < kNumpySumStretch ? n - first : kNumpySumStretch;
        res = res + pairwise_range(f, first, len, st);
    }
    return res;
}

template <class Ptr>
struct PlainTerms {
    Ptr z;
    SBB_HD double operator()(int i) const { return z[i]; }
};

// |z - mean|^2 as numpy's _var forms it: x = z - mean, then x * x
template <class Ptr>
struct SquaredDeviations {
    Ptr z;
    double mean;
    SBB_HD double operator()(int i) const
    {
#pragma clang fp contract(off)
        const double d = z[i] - mean;
        return d * d;
    }
};

// np.mean of m values
template <class Ptr>
SBB_HD double mean_of(Ptr v, int m, PairwiseStack* st)
{
    return soft_div(pairwise_sum(PlainTerms<Ptr>{v}, m, st), (double)m);
}

// np.std(z) of n >= 1 values
template <class Ptr>
SBB_HD double std_of(Ptr z, int n, PairwiseStack* st)
{
    const double mean = mean_of(z, n, st);
    return soft_sqrt(soft_div(pairwise_sum(SquaredDeviations<Ptr>{z, mean}, n, st), (double)n));
}

// the level a "deep" minimum must lie below: mean(tops) * (1 - 1 / multiplier) as the reference writes it; NaN without tops
template <class Ptr>
SBB_HD double deep_level(Ptr tops, int m, double multiplier, PairwiseStack* st)
{
#pragma clang fp contract(off)
    if (m == 0) return f64_from_bits(0x7ff8ull << 48);
    const double level = mean_of(tops, m, st);
    return level - soft_div(level, multiplier);
}

// One minimum (peak of the smoothed `flipped` at position `mid`, value >= 0 checked by the caller): z[mid - 20] with numpy's indexing.
// Returns 2 for the reference's IndexError, 1 for a deep minimum, 0 otherwise.
template <class Ptr>
SBB_HD int classify_minimum(Ptr z, int n, int mid, double below)
{
    int idx = mid - 2 * kProfilePad;
    if (idx >= n || idx < -n) return 2;
    if (idx < 0) idx += n;
    return z[idx] < below ? 1 : 0;
}

// The whole statistic of one profile, serially (the CPU entry point; the kernels of profile_stats.hip deal the same steps out to the lanes
// of a wave).  z: n doubles, g: n + 40 doubles of workspace; z holds the smoothed profile afterwards.  Returns the state, *spread = np.std(z)
// for kProfileAppended and 0 otherwise.  Optional (debug entry point): smooth_out = a copy of z, *below_out = what deep_level returned.
inline int profile_statistic_serial(const int32_t* y, int n, const double* w, int radius, double multiplier, double* z, double* g,
                                    PairwiseStack* st, double* spread, double* smooth_out = nullptr, double* below_out = nullptr)
{
    int top = 0;
    for (int i = 0; i < n; ++i) top = y[i] > top ? y[i] : top;
    const ProfileSamples ys{y};
    for (int i = 0; i < n; ++i) z[i] = smooth_sample(ys, n, w, radius, i);
    int m = 0;
    for (int i = 1; i < n - 1; ++i) {
        int mid;
        if (peak_starts_at(z, n, i, &mid) && z[mid] >= 0.0 && z[mid] > 10.0) g[m++] = z[mid];
    }
    const double below = deep_level(g, m, multiplier, st);
    if (smooth_out) memcpy(smooth_out, z, (size_t)n * sizeof(double));
    if (below_out) *below_out = below;
    const FlippedSamples fs{y, n, (double)top};
    const int nf = n + kProfileFlipExtra;
    for (int k = 0; k < nf; ++k) g[k] = smooth_sample(fs, nf, w, radius, k);
    bool oob = false, deep = false;
    for (int k = 1; k < nf - 1; ++k) {
        int mid;
        if (!peak_starts_at(g, nf, k, &mid) || !(g[mid] >= 0.0)) continue;
        const int cls = classify_minimum(z, n, mid, below);
        oob |= cls == 2;
        deep |= cls == 1;
    }
    *spread = 0.0;
    if (oob) return kProfileException;
    if (!deep) return kProfileSkipped;
    *spread = std_of(z, n, st);
    return kProfileAppended;
}

// main.py:1655-1665: the first maximum of the appended spreads; its POSITION in the shortened list indexes the full angle array.  -1: nothing
// appended.  An "exception" angle is appended with spread 0.
SBB_HD int sweep_winner(const double* spread, const uint8_t* state, int n_angles)
{
    int pos = 0, best = -1;
    double best_v = 0.0;
    for (int a = 0; a < n_angles; ++a) {
        if (state[a] == kProfileSkipped) continue;
        const double v = state[a] == kProfileAppended ? spread[a] : 0.0;
        if (best < 0 || v > best_v) { best = pos; best_v = v; }
        ++pos;
    }
    return best;
}

}  // namespace sbbseg

#endif  // SBBSEG_PROFILE_STAT_H
