// rt_display.hip -- the display transform (rt_scene_display): a float colour of high dynamic range is
// metered (a luminance histogram of sixteen bins per octave resolves an exposure), exposed, tone-mapped and packed,
// linearly (im_pack_colour, today's pack) or sRGB-encoded by a table of 255 thresholds.
//
// Variant 0 (the product): dp_pass<METER, APPLY>, workgroups of 256 threads striding over the frame, one 16-byte load
//   per pixel. METER: the histogram is counted in LDS with integer atomics, one copy per workgroup, and flushed with one
//   global atomic per non-empty bin. APPLY: the thresholds are staged in LDS and a code is an 8-step branch-free binary
//   search. dp_resolve: one workgroup of 512 threads, a lane per bin; the prefix sum and the 64-bit sum in LDS.
//   AUTO: dp_pass<1, 0>, dp_resolve, dp_pass<0, 1>; LAGGED: dp_pass<1, 1>, dp_resolve; MANUAL: dp_pass<0, 1>.
// Variant 1 (the yardstick): dp_plain, a thread per pixel, global atomics straight into the histogram, a code counted
//   with 255 compares against the table in global memory; dp_resolve_plain, one thread's serial loop.
//
// Both evaluate dp_bin / dp_curve below on the same values in the same order, and the histogram is integers: the same
// bits. Only + - * / and compares; the library is built with -ffp-contract=off and correctly rounded division.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstdlib>

#include "rt_filter.h"
#include "rt_internal.h"

namespace {

constexpr int DP_BLOCK = 256;
constexpr int DP_APPLY_GROUPS = 4096;  // workgroups of dp_pass<0, 1> at most, and
constexpr int DP_METER_GROUPS = 1024;  // of dp_pass<1, 0> and dp_pass<1, 1>: by the grid sweep of DESIGN.md 6r
constexpr int DP_BINS = RT_DISPLAY_BINS;
constexpr int DP_BIN0 = 1776;          // bits(2^-16) >> 19
// LDS copies of the histogram in a workgroup of dp_pass: 1 = one for the workgroup, 4 = one per wave (make
// EXTRA=-DDP_HIST_COPIES=4). One: by the measurement of DESIGN.md 6r
#ifndef DP_HIST_COPIES
#define DP_HIST_COPIES 1
#endif
static_assert(DP_HIST_COPIES == 1 || DP_HIST_COPIES == 4, "one histogram per workgroup, or one per wave");

struct DpArgs {                        // by value
    unsigned n;                        // pixels: at most 2^30
    const float4 *in;
    const int2 *id;                    // null: every pixel may be metered
    float4 *out;                       // null, or may be `in`
    uint32_t *pixels;                  // null, or the packed words
    const float *state;                // null: E = exposure; else E = state[3] == 1 ? state[0] : exposure
    uint32_t *hist;                    // the scene's histogram, zero at the head of the call
    const float *table;                // T[256] on the device
    float exposure, white2;            // white2 = white * white
    int curve, transfer;
};

struct DpResolve {
    uint32_t *hist;
    float *state;
    uint32_t *hist_out;                // null, or the caller's
    float exposure, key, min_e, max_e, adapt;
    int low, high;
    float npx;                         // (float)(width * height)
};

// the bin of a luminance, or -1 if it is not metered (l <= 0, not finite, a NaN)
__device__ __forceinline__ int dp_bin(float l)
{
    if (!(l > 0.f) || !(l < __builtin_inff())) return -1;
    int k = (int)(__float_as_uint(l) >> 19) - DP_BIN0;
    k = k < 0 ? 0 : k;
    return k > DP_BINS - 1 ? DP_BINS - 1 : k;
}
__device__ __forceinline__ int dp_metered_bin(const DpArgs &a, unsigned p, const float4 &v)
{
    const int k = dp_bin(im_luma(v.x, v.y, v.z));
    if (k < 0 || !a.id) return k;
    return a.id[p].x >= 0 ? k : -1;    // the id is read only where the luminance counts
}
__device__ __forceinline__ float dp_exposure(const float *state, float exposure)
{
    float E = exposure;
    if (state) {
        const float4 s = *(const float4 *)state;
        if (s.w == 1.f) E = s.x;
    }
    return E;
}
__device__ __forceinline__ float dp_unit(float o)
{
    o = im_max(o, 0.f);
    return o > 1.f ? 1.f : o;
}
__device__ __forceinline__ float dp_aces(float c)
{
    float x = im_max(c, 0.f);
    x = x > 1024.f ? 1024.f : x;
    return dp_unit((x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f));
}
// steps 3 and 4: the display-linear colour of (r, g, b) under exposure E
__device__ __forceinline__ void dp_curve(const DpArgs &a, float E, float &r, float &g, float &b)
{
    r = r * E; g = g * E; b = b * E;
    if (a.curve == RT_DISPLAY_REINHARD) {
        const float L = im_max(im_luma(r, g, b), 0.f);
        const float s = (1.f + L / a.white2) / (1.f + L);
        r = dp_unit(r * s); g = dp_unit(g * s); b = dp_unit(b * s);
    } else if (a.curve == RT_DISPLAY_ACES) {
        r = dp_aces(r); g = dp_aces(g); b = dp_aces(b);
    }
}
// the number of v in 1 .. 255 with o >= T[v], T increasing: eight steps, no branch; a NaN compares false throughout
__device__ __forceinline__ uint32_t dp_code_search(const float *T, float o)
{
    uint32_t c = 0;
#pragma unroll
    for (uint32_t step = 128; step; step >>= 1) c += o >= T[c + step] ? step : 0u;
    return c;
}
__device__ __forceinline__ uint32_t dp_code_count(const float *T, float o)
{
    uint32_t c = 0;
    for (int v = 1; v < 256; ++v) c += o >= T[v] ? 1u : 0u;
    return c;
}
template <bool SEARCH>
__device__ __forceinline__ void dp_apply(const DpArgs &a, const float *T, float E, unsigned p, const float4 &v)
{
    float r = v.x, g = v.y, b = v.z;
    dp_curve(a, E, r, g, b);
    if (a.out) a.out[p] = make_float4(r, g, b, v.w);
    if (!a.pixels) return;
    if (a.transfer == RT_DISPLAY_LINEAR) {
        a.pixels[p] = im_pack_colour(r, g, b);
    } else if (SEARCH) {
        a.pixels[p] = (dp_code_search(T, r) << 16) + (dp_code_search(T, g) << 8) + dp_code_search(T, b);
    } else {
        a.pixels[p] = (dp_code_count(T, r) << 16) + (dp_code_count(T, g) << 8) + dp_code_count(T, b);
    }
}

template <bool METER, bool APPLY>
__global__ __launch_bounds__(DP_BLOCK) void dp_pass(const DpArgs a)
{
    __shared__ uint32_t hist[METER ? DP_HIST_COPIES * DP_BINS : 1];
    __shared__ float T[APPLY ? 256 : 1];
    const unsigned t = threadIdx.x;
    if constexpr (METER) {
        for (unsigned k = t; k < (unsigned)(DP_HIST_COPIES * DP_BINS); k += DP_BLOCK) hist[k] = 0;
    }
    [[maybe_unused]] uint32_t *const mine = hist + (DP_HIST_COPIES == 1 ? 0u : (t >> 6) * DP_BINS);
    float E = 0.f;
    if constexpr (APPLY) {
        T[t] = a.table[t];
        E = dp_exposure(a.state, a.exposure);
    }
    __syncthreads();
    const unsigned stride = gridDim.x * DP_BLOCK;
    for (unsigned p = blockIdx.x * DP_BLOCK + t; p < a.n; p += stride) {
        const float4 v = a.in[p];
        if constexpr (METER) {
            const int k = dp_metered_bin(a, p, v);
            if (k >= 0) atomicAdd(&mine[k], 1u);
        }
        if constexpr (APPLY) dp_apply<true>(a, T, E, p, v);
    }
    if constexpr (METER) {
        __syncthreads();
        for (unsigned k = t; k < (unsigned)DP_BINS; k += DP_BLOCK) {
            uint32_t c = hist[k];
            for (int w = 1; w < DP_HIST_COPIES; ++w) c += hist[w * DP_BINS + k];
            if (c) atomicAdd(&a.hist[k], c);
        }
    }
}

// The yardstick: meter / apply as dp_pass's template arguments, here uniforms
__global__ __launch_bounds__(DP_BLOCK) void dp_plain(const DpArgs a, int meter, int apply)
{
    const unsigned p = blockIdx.x * DP_BLOCK + threadIdx.x;
    if (p >= a.n) return;
    const float4 v = a.in[p];
    if (meter) {
        const int k = dp_metered_bin(a, p, v);
        if (k >= 0) atomicAdd(&a.hist[k], 1u);
    }
    if (apply) dp_apply<false>(a, a.table, dp_exposure(a.state, a.exposure), p, v);
}

// Step 2 from the totals: N metered pixels, s = sum take_k k over the window [lo, hi). One thread.
__device__ __forceinline__ void dp_resolve_state(const DpResolve &r, uint32_t N, unsigned long long s, unsigned long long lo,
                                                 unsigned long long hi)
{
    const float4 st = *(const float4 *)r.state;
    const float e0 = st.x;
    const bool valid0 = st.w == 1.f;
    if (N == 0) {
        *(float4 *)r.state = make_float4(valid0 ? e0 : r.exposure, 0.f, 0.f, 1.f);
        return;
    }
    const unsigned long long m = (s * 256ull) / (hi - lo);
    const float Lm = __uint_as_float(((uint32_t)DP_BIN0 << 19) + ((uint32_t)m << 11) + (1u << 18));
    float et = r.key / Lm;
    et = et < r.min_e ? r.min_e : et;
    et = et > r.max_e ? r.max_e : et;
    const float e = (valid0 && r.adapt < 1.f) ? e0 + (et - e0) * r.adapt : et;
    *(float4 *)r.state = make_float4(e, Lm, (float)N / r.npx, 1.f);
}
__device__ __forceinline__ unsigned long long dp_take(unsigned long long c0, unsigned long long c1, unsigned long long lo,
                                                      unsigned long long hi)
{
    const unsigned long long top = c1 < hi ? c1 : hi, bot = c0 > lo ? c0 : lo;
    return top > bot ? top - bot : 0ull;
}

__global__ __launch_bounds__(DP_BINS) void dp_resolve(const DpResolve r)
{
    __shared__ uint32_t cum[DP_BINS];               // inclusive prefix sums
    __shared__ unsigned long long part[DP_BINS];
    const unsigned k = threadIdx.x;
    const uint32_t h = r.hist[k];
    cum[k] = h;
    __syncthreads();
    for (unsigned d = 1; d < (unsigned)DP_BINS; d <<= 1) {
        const uint32_t add = k >= d ? cum[k - d] : 0u;
        __syncthreads();
        cum[k] += add;
        __syncthreads();
    }
    const uint32_t N = cum[DP_BINS - 1];
    const unsigned long long lo = ((unsigned long long)N * (unsigned)r.low) >> 10;
    const unsigned long long hi = ((unsigned long long)N * (unsigned)r.high + 1023ull) >> 10;
    part[k] = dp_take(cum[k] - h, cum[k], lo, hi) * k;
    __syncthreads();
    for (unsigned d = DP_BINS / 2; d; d >>= 1) {
        if (k < d) part[k] += part[k + d];
        __syncthreads();
    }
    if (N && r.hist_out) r.hist_out[k] = h;
    if (k == 0) dp_resolve_state(r, N, part[0], lo, hi);
}

__global__ void dp_resolve_plain(const DpResolve r)
{
    unsigned long long N = 0;
    for (int k = 0; k < DP_BINS; ++k) N += r.hist[k];
    const unsigned long long lo = (N * (unsigned)r.low) >> 10, hi = (N * (unsigned)r.high + 1023ull) >> 10;
    unsigned long long s = 0, c = 0;
    for (int k = 0; k < DP_BINS; ++k) {
        const unsigned long long h = r.hist[k];
        s += dp_take(c, c + h, lo, hi) * (unsigned)k;
        c += h;
        if (N && r.hist_out) r.hist_out[k] = (uint32_t)h;
    }
    dp_resolve_state(r, (uint32_t)N, s, lo, hi);
}

struct DpTable {
    float t[256];
    DpTable()
    {
        t[0] = 0.f;
        for (int v = 1; v < 256; ++v) {
            const double c = ((double)v - 0.5) / 255.0;
            t[v] = (float)(c <= 0.04045 ? c / 12.92 : std::pow((c + 0.055) / 1.055, 2.4));
        }
    }
};

}   // namespace

const float *rt_display_table()
{
    static const DpTable table;
    return table.t;
}

#define DP_HIP(expr)                                                         \
    do {                                                                     \
        hipError_t dp_e_ = (expr);                                           \
        if (dp_e_ != hipSuccess) return rt_hip_fail(dp_e_, #expr, __FILE__, __LINE__); \
    } while (0)

int rt_display_launch(const rt_display_desc *d, uint32_t *hist, const float *table, hipEvent_t *ev, int *n_ev, hipStream_t stream)
{
    const bool meter = d->meter != RT_DISPLAY_METER_MANUAL, apply = d->rgba_out || d->pixels;
    DpArgs a = {};
    a.n = (unsigned)d->width * (unsigned)d->height;
    a.in = (const float4 *)d->rgba_in;
    a.id = meter && !d->meter_sky ? (const int2 *)d->id : nullptr;
    a.out = (float4 *)d->rgba_out;
    a.pixels = d->pixels;
    a.state = meter ? d->state : nullptr;
    a.hist = hist;
    a.table = table;
    a.exposure = d->exposure;
    a.white2 = d->white * d->white;
    a.curve = d->curve;
    a.transfer = d->transfer;
    DpResolve r = {};
    r.hist = hist;
    r.state = d->state;
    r.hist_out = d->histogram_out;
    r.exposure = d->exposure; r.key = d->key; r.min_e = d->min_exposure; r.max_e = d->max_exposure; r.adapt = d->adapt;
    r.low = d->meter_low; r.high = d->meter_high;
    r.npx = (float)a.n;
    // dp_pass: a workgroup per DP_BLOCK pixels up to a cap, from there on strided. A pass that meters has the lower
    // cap: a workgroup's flush is up to 512 global atomics however little it counted (the grid sweep)
    unsigned meter_cap = DP_METER_GROUPS, apply_cap = DP_APPLY_GROUPS;
#ifdef RT_TUNING
    auto tuned = [](const char *name, unsigned &v) {
        if (const char *e = getenv(name))
            if (atoi(e) > 0) v = (unsigned)atoi(e);
    };
    tuned("RT_DISPLAY_METER_GROUPS", meter_cap);
    tuned("RT_DISPLAY_APPLY_GROUPS", apply_cap);
#endif
    const unsigned groups = (a.n + DP_BLOCK - 1) / DP_BLOCK;
    const dim3 block(DP_BLOCK), metering(groups < meter_cap ? groups : meter_cap), applying(groups < apply_cap ? groups : apply_cap),
               whole(groups);
    int n = 0;
    auto stamp = [&]() { return ev ? hipEventRecord(ev[n++], stream) : hipSuccess; };
    // a call never sees an earlier call's counts, whatever became of that call
    if (meter) DP_HIP(hipMemsetAsync(hist, 0, sizeof(uint32_t) * DP_BINS, stream));
    DP_HIP(stamp());
    auto pass = [&](bool m, bool ap) {
        if (d->variant != 0) hipLaunchKernelGGL(dp_plain, whole, block, 0, stream, a, (int)m, (int)ap);
        else if (m && ap) hipLaunchKernelGGL((dp_pass<true, true>), metering, block, 0, stream, a);
        else if (m) hipLaunchKernelGGL((dp_pass<true, false>), metering, block, 0, stream, a);
        else hipLaunchKernelGGL((dp_pass<false, true>), applying, block, 0, stream, a);
        return hipGetLastError();
    };
    auto resolve = [&]() {
        if (d->variant != 0) hipLaunchKernelGGL(dp_resolve_plain, dim3(1), dim3(1), 0, stream, r);
        else hipLaunchKernelGGL(dp_resolve, dim3(1), dim3(DP_BINS), 0, stream, r);
        return hipGetLastError();
    };
    if (!meter) {
        DP_HIP(pass(false, true));
        DP_HIP(stamp());
    } else if (d->meter == RT_DISPLAY_METER_LAGGED || !apply) {
        DP_HIP(pass(true, apply));          // E is the state's as it stands: the resolve comes behind
        DP_HIP(stamp());
        DP_HIP(resolve());
        DP_HIP(stamp());
    } else {
        DP_HIP(pass(true, false));
        DP_HIP(stamp());
        DP_HIP(resolve());
        DP_HIP(stamp());
        DP_HIP(pass(false, true));          // E is what the resolve left in the state
        DP_HIP(stamp());
    }
    if (n_ev) *n_ev = n;
    return RT_OK;
}
