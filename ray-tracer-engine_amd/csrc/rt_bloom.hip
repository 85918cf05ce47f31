// rt_bloom.hip -- the bloom pass (rt_scene_bloom): the part of a float colour above a luminance threshold
// is filtered down a pyramid of half-resolution levels ([1 3 3 1] / 8, separable), walked back up with 2x bilinear
// steps that add every level on the way, and added to the frame ahead of the display transform.
//
// Variant 0 (the product): workgroups of 256 threads, one per tile of its launch's destination.
//   bl_down<BRIGHT>: a tile of BL_DOWN_TW x BL_DOWN_TH destination pixels. The (2 TW + 2) x (2 TH + 2) source region is
//   staged in LDS with one 16-byte load per texel (BRIGHT: the bright pass applied at the load, t and lim formed once
//   from a uniform load of the state), the horizontal step runs into a second LDS array of (2 TH + 2) x TW, the
//   vertical step out of it. bl_up<FINAL>: a tile of BL_UP_TW x BL_UP_TH pixels of the finer level; its (TW / 2 + 2) x
//   (TH / 2 + 2) texels of the coarser one are staged in LDS. <false> writes A_k over B_k, <true> is the combine.
// Variant 1 (the yardstick): bl_down_plain / bl_up_plain, a thread per output pixel, 16 and 4 taps straight from
//   global memory.
//
// Both evaluate bl_bright / bl_tap4 / bl_mix below on the same values in the same order: the same bits. Only + - *,
// one / and compares; the library is built with -ffp-contract=off and correctly rounded division.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_filter.h"
#include "rt_internal.h"

namespace {

constexpr int BL_BLOCK = 256;
// Tile shapes: by the sweep of DESIGN.md 6s (make EXTRA="-DBL_DOWN_TW=.. -DBL_DOWN_TH=.."). The same sweep capped the
// grids and let a workgroup stride over tiles: no cap was as fast as the best one, so there is none
#ifndef BL_DOWN_TW
#define BL_DOWN_TW 32
#endif
#ifndef BL_DOWN_TH
#define BL_DOWN_TH 8
#endif
#ifndef BL_UP_TW
#define BL_UP_TW 64
#endif
#ifndef BL_UP_TH
#define BL_UP_TH 4
#endif
static_assert(BL_DOWN_TW * BL_DOWN_TH == BL_BLOCK && BL_UP_TW * BL_UP_TH == BL_BLOCK, "a thread per pixel of a tile");
static_assert(BL_UP_TW % 2 == 0 && BL_UP_TH % 2 == 0, "an upsample tile starts on an even column and row");

struct BlDown {                        // by value
    const float4 *src;                 // ws x hs: rgba_in (BRIGHT) or B_{k-1}
    float4 *dst;                       // wd x hd, wd = (ws + 1) >> 1: B_k
    int ws, hs, wd, hd;
    const float *state;                // BRIGHT: null, or the display transform's state
    float threshold, limit;
};

struct BlUp {                          // by value
    const float4 *src;                 // wc x hc: A_{k+1}
    int wc, hc, wd, hd;                // wc = (wd + 1) >> 1
    float4 *level;                     // !FINAL: B_k, over which A_k is written
    float k;                           // !FINAL: spread; FINAL: strength
    const float4 *in;                  // FINAL: rgba_in
    float4 *out;                       // FINAL: null, or may be `in`
    uint32_t *pixels;                  // FINAL: null, or the packed words
    float4 *glow;                      // FINAL: null, or (T, 0)
};

__device__ __forceinline__ int bl_clamp(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

// step 1: t and lim on the scale the display transform will show the frame at
__device__ __forceinline__ void bl_scale(const float *state, float threshold, float limit, float &t, float &lim)
{
    float E = 1.f;
    if (state) {
        const float4 s = *(const float4 *)state;
        if (s.w == 1.f) E = s.x;
    }
    t = threshold / E;
    lim = limit / E;
}
__device__ __forceinline__ float bl_bright1(float c, float s, float lim)
{
    const float v = im_max(c * s, 0.f);
    return v > lim ? lim : v;
}
// step 2: Br(p)
__device__ __forceinline__ float4 bl_bright(const float4 &c, float t, float lim)
{
    const float l = im_luma(c.x, c.y, c.z);
    if (!(l > t) || !(l < __builtin_inff())) return make_float4(0.f, 0.f, 0.f, 0.f);
    const float s = (l - t) / l;
    return make_float4(bl_bright1(c.x, s, lim), bl_bright1(c.y, s, lim), bl_bright1(c.z, s, lim), 0.f);
}
// step 3: one direction of [1 3 3 1] / 8
__device__ __forceinline__ float bl_tap(float a, float b, float c, float d) { return ((a + d) + 3.f * (b + c)) * 0.125f; }
__device__ __forceinline__ float4 bl_tap4(const float4 &a, const float4 &b, const float4 &c, const float4 &d)
{
    return make_float4(bl_tap(a.x, b.x, c.x, d.x), bl_tap(a.y, b.y, c.y, d.y), bl_tap(a.z, b.z, c.z, d.z), 0.f);
}
// step 4: one direction of the 2x bilinear step, the nearer texel first
__device__ __forceinline__ float bl_lerp(float a, float b) { return 0.75f * a + 0.25f * b; }
__device__ __forceinline__ float4 bl_mix(const float4 &a, const float4 &b)
{
    return make_float4(bl_lerp(a.x, b.x), bl_lerp(a.y, b.y), bl_lerp(a.z, b.z), 0.f);
}
__device__ __forceinline__ float4 bl_up4(const float4 &cc, const float4 &nc, const float4 &cn, const float4 &nn)
{
    return bl_mix(bl_mix(cc, nc), bl_mix(cn, nn));    // G(cy), G(ny), then U
}
// steps 5 and 6 at pixel p of the finer level: `own` is bl_own(a, p), the pixel's B_k or rgba_in, U = Up(A_{k+1}) there
template <bool FINAL>
__device__ __forceinline__ float4 bl_own(const BlUp &a, size_t p) { return FINAL ? a.in[p] : a.level[p]; }
template <bool FINAL>
__device__ __forceinline__ void bl_store(const BlUp &a, size_t p, const float4 &own, const float4 &U)
{
    if constexpr (!FINAL) {
        const float4 b = own;
        a.level[p] = make_float4(b.x + a.k * U.x, b.y + a.k * U.y, b.z + a.k * U.z, 0.f);
    } else {
        const float4 c = own;
        const float r = U.x == 0.f ? c.x : c.x + a.k * U.x;
        const float g = U.y == 0.f ? c.y : c.y + a.k * U.y;
        const float b = U.z == 0.f ? c.z : c.z + a.k * U.z;
        if (a.out) a.out[p] = make_float4(r, g, b, c.w);
        if (a.pixels) a.pixels[p] = im_pack_colour(r, g, b);
        if (a.glow) a.glow[p] = U;
    }
}

template <bool BRIGHT>
__global__ __launch_bounds__(BL_BLOCK) void bl_down(const BlDown a)
{
    constexpr int TW = BL_DOWN_TW, TH = BL_DOWN_TH, SW = 2 * TW + 2, SH = 2 * TH + 2;
    __shared__ float4 src[SH * SW];    // slot (r, c): S(clampx(2 X0 - 1 + c), clampy(2 Y0 - 1 + r))
    __shared__ float4 hor[SH * TW];    // slot (r, c): H of destination column X0 + c on source row slot r
    const int tid = (int)threadIdx.x, lx = tid % TW, ly = tid / TW;
    [[maybe_unused]] float t = 0.f, lim = 0.f;
    if constexpr (BRIGHT) bl_scale(a.state, a.threshold, a.limit, t, lim);
    const int tiles_x = (a.wd + TW - 1) / TW, ty = (int)blockIdx.x / tiles_x;
    const int X0 = ((int)blockIdx.x - ty * tiles_x) * TW, Y0 = ty * TH;
    for (int i = tid; i < SH * SW; i += BL_BLOCK) {
        const int r = i / SW, c = i - r * SW;
        const int sx = bl_clamp(2 * X0 - 1 + c, a.ws), sy = bl_clamp(2 * Y0 - 1 + r, a.hs);
        const float4 v = a.src[(size_t)sy * (size_t)a.ws + (size_t)sx];
        src[i] = BRIGHT ? bl_bright(v, t, lim) : v;
    }
    __syncthreads();
    for (int i = tid; i < SH * TW; i += BL_BLOCK) {
        const int r = i / TW, c = i - r * TW;
        const float4 *row = src + r * SW + 2 * c;                           // x0, x1, x2, x3 of column X0 + c
        hor[i] = bl_tap4(row[0], row[1], row[2], row[3]);
    }
    __syncthreads();
    const int x = X0 + lx, y = Y0 + ly;
    if (x < a.wd && y < a.hd) {
        const float4 *col = hor + 2 * ly * TW + lx;                         // y0, y1, y2, y3 of row Y0 + ly
        a.dst[(size_t)y * (size_t)a.wd + (size_t)x] = bl_tap4(col[0], col[TW], col[2 * TW], col[3 * TW]);
    }
}

template <bool FINAL>
__global__ __launch_bounds__(BL_BLOCK) void bl_up(const BlUp a)
{
    constexpr int TW = BL_UP_TW, TH = BL_UP_TH, CW = TW / 2 + 2, CH = TH / 2 + 2;
    __shared__ float4 crs[CH * CW];    // slot (r, c): S(clampx(X0 / 2 - 1 + c), clampy(Y0 / 2 - 1 + r))
    const int tid = (int)threadIdx.x, lx = tid % TW, ly = tid / TW;
    const int tiles_x = (a.wd + TW - 1) / TW, ty = (int)blockIdx.x / tiles_x;
    const int X0 = ((int)blockIdx.x - ty * tiles_x) * TW, Y0 = ty * TH;
    // the pixel's own load is issued ahead of the staging, so that the barrier is waited for once, not twice
    const int x = X0 + lx, y = Y0 + ly;
    const bool inside = x < a.wd && y < a.hd;
    const size_t p = (size_t)y * (size_t)a.wd + (size_t)x;
    const float4 own = inside ? bl_own<FINAL>(a, p) : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = tid; i < CH * CW; i += BL_BLOCK) {
        const int r = i / CW, c = i - r * CW;
        const int sx = bl_clamp(X0 / 2 - 1 + c, a.wc), sy = bl_clamp(Y0 / 2 - 1 + r, a.hc);
        crs[i] = a.src[(size_t)sy * (size_t)a.wc + (size_t)sx];
    }
    __syncthreads();
    if (inside) {
        // X0 and Y0 are even: the parity of x is lx's, and cx sits in slot (lx >> 1) + 1
        const int sc = (lx >> 1) + 1, sn = sc + ((lx & 1) ? 1 : -1);
        const float4 *rc = crs + ((ly >> 1) + 1) * CW, *rn = rc + ((ly & 1) ? CW : -CW);
        bl_store<FINAL>(a, p, own, bl_up4(rc[sc], rc[sn], rn[sc], rn[sn]));
    }
}

// The yardstick: the same expressions on the same values in the same order, a thread per output pixel
__global__ __launch_bounds__(BL_BLOCK) void bl_down_plain(const BlDown a, int bright)
{
    const size_t p = (size_t)blockIdx.x * BL_BLOCK + threadIdx.x;
    if (p >= (size_t)a.wd * (size_t)a.hd) return;
    const int y = (int)(p / (size_t)a.wd), x = (int)(p - (size_t)y * (size_t)a.wd);
    float t = 0.f, lim = 0.f;
    if (bright) bl_scale(a.state, a.threshold, a.limit, t, lim);
    const int xs[4] = {bl_clamp(2 * x - 1, a.ws), 2 * x, bl_clamp(2 * x + 1, a.ws), bl_clamp(2 * x + 2, a.ws)};
    const int ys[4] = {bl_clamp(2 * y - 1, a.hs), 2 * y, bl_clamp(2 * y + 1, a.hs), bl_clamp(2 * y + 2, a.hs)};
    float4 H[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float4 S[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float4 v = a.src[(size_t)ys[j] * (size_t)a.ws + (size_t)xs[i]];
            S[i] = bright ? bl_bright(v, t, lim) : v;
        }
        H[j] = bl_tap4(S[0], S[1], S[2], S[3]);
    }
    a.dst[p] = bl_tap4(H[0], H[1], H[2], H[3]);
}

__global__ __launch_bounds__(BL_BLOCK) void bl_up_plain(const BlUp a, int final)
{
    const size_t p = (size_t)blockIdx.x * BL_BLOCK + threadIdx.x;
    if (p >= (size_t)a.wd * (size_t)a.hd) return;
    const int y = (int)(p / (size_t)a.wd), x = (int)(p - (size_t)y * (size_t)a.wd);
    const int cx = x >> 1, nx = bl_clamp(cx + ((x & 1) ? 1 : -1), a.wc);
    const int cy = y >> 1, ny = bl_clamp(cy + ((y & 1) ? 1 : -1), a.hc);
    const float4 *rc = a.src + (size_t)cy * (size_t)a.wc, *rn = a.src + (size_t)ny * (size_t)a.wc;
    const float4 U = bl_up4(rc[cx], rc[nx], rn[cx], rn[nx]);
    if (final) bl_store<true>(a, p, bl_own<true>(a, p), U);
    else bl_store<false>(a, p, bl_own<false>(a, p), U);
}

}   // namespace

#define BL_HIP(expr)                                                         \
    do {                                                                     \
        hipError_t bl_e_ = (expr);                                           \
        if (bl_e_ != hipSuccess) return rt_hip_fail(bl_e_, #expr, __FILE__, __LINE__); \
    } while (0)

size_t rt_bloom_pyramid_texels(int width, int height, int levels)
{
    size_t n = 0;
    for (int k = 1; k <= levels; ++k) {
        width = (width + 1) >> 1;
        height = (height + 1) >> 1;
        n += (size_t)width * (size_t)height;
    }
    return n;
}

int rt_bloom_launch(const rt_bloom_desc *d, float4 *pyramid, hipEvent_t *ev, int *n_ev, hipStream_t stream)
{
    const int L = d->levels;
    int w[RT_BLOOM_MAX_LEVELS + 1], h[RT_BLOOM_MAX_LEVELS + 1];
    float4 *B[RT_BLOOM_MAX_LEVELS + 1] = {};          // B[k], k >= 1: level k in the pyramid
    w[0] = d->width; h[0] = d->height;
    size_t at = 0;
    for (int k = 1; k <= L; ++k) {
        w[k] = (w[k - 1] + 1) >> 1;
        h[k] = (h[k - 1] + 1) >> 1;
        B[k] = pyramid + at;
        at += (size_t)w[k] * (size_t)h[k];
    }
    const bool plain = d->variant != 0;
    // a workgroup per tile, or per BL_BLOCK pixels: 2^22 at most, at 32768 x 32768
    auto grid = [&](int wd, int hd, int tw, int th) {
        if (plain) return dim3((unsigned)(((size_t)wd * (size_t)hd + BL_BLOCK - 1) / BL_BLOCK));
        return dim3((unsigned)((wd + tw - 1) / tw) * (unsigned)((hd + th - 1) / th));
    };
    const dim3 block(BL_BLOCK);
    int n = 0;
    auto stamp = [&]() { return ev ? hipEventRecord(ev[n++], stream) : hipSuccess; };
    BL_HIP(stamp());
    for (int k = 1; k <= L; ++k) {
        BlDown a = {};
        a.src = k == 1 ? (const float4 *)d->rgba_in : B[k - 1];
        a.dst = B[k];
        a.ws = w[k - 1]; a.hs = h[k - 1]; a.wd = w[k]; a.hd = h[k];
        a.state = d->state;
        a.threshold = d->threshold; a.limit = d->limit;
        const dim3 g = grid(a.wd, a.hd, BL_DOWN_TW, BL_DOWN_TH);
        if (plain) hipLaunchKernelGGL(bl_down_plain, g, block, 0, stream, a, (int)(k == 1));
        else if (k == 1) hipLaunchKernelGGL((bl_down<true>), g, block, 0, stream, a);
        else hipLaunchKernelGGL((bl_down<false>), g, block, 0, stream, a);
        BL_HIP(hipGetLastError());
        BL_HIP(stamp());
    }
    for (int k = L - 1; k >= 0; --k) {
        BlUp a = {};
        a.src = B[k + 1];
        a.wc = w[k + 1]; a.hc = h[k + 1]; a.wd = w[k]; a.hd = h[k];
        if (k > 0) {
            a.level = B[k];
            a.k = d->spread;
        } else {
            a.k = d->strength;
            a.in = (const float4 *)d->rgba_in;
            a.out = (float4 *)d->rgba_out;
            a.pixels = d->pixels;
            a.glow = (float4 *)d->glow_out;
        }
        const dim3 g = grid(a.wd, a.hd, BL_UP_TW, BL_UP_TH);
        if (plain) hipLaunchKernelGGL(bl_up_plain, g, block, 0, stream, a, (int)(k == 0));
        else if (k == 0) hipLaunchKernelGGL((bl_up<true>), g, block, 0, stream, a);
        else hipLaunchKernelGGL((bl_up<false>), g, block, 0, stream, a);
        BL_HIP(hipGetLastError());
        BL_HIP(stamp());
    }
    if (n_ev) *n_ev = n;
    return RT_OK;
}
