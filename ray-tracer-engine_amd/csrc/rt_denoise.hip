// rt_denoise.hip -- the two a-trous denoisers: the G-buffer-guided one (rt_scene_denoise), an
// edge-avoiding a-trous wavelet filter over a frame's rgba, steered by the frame's guides (aov_depth / aov_normal /
// aov_id / aov_albedo), and the variance-guided one (rt_scene_denoise_variance), the same filter with a
// per-pixel luminance threshold, S(p) = sigma_colour^2 * (3 x 3 mean of the variance) + sigma_floor^2. The variance
// starts from the temporal moments where the history is long, from the 7 x 7 neighbourhood where it is short, and is
// carried through the iterations beside the irradiance.
//
// One set of kernels, instantiated twice: VAR = false is rt_scene_denoise (a uniform threshold sigma_colour^2, or no
// colour factor), VAR = true adds the variance array -- its loads and staging, S(p), the sum of w w v and the variance
// outputs.
//
// Variant 0 (the product):
//   dn_pack          one thread per pixel: demodulates into the first irradiance buffer and packs what an iteration
//                    reads of the guides into one float4 (N.xyz, z) and one int (index) per pixel; the pixel's kind
//                    rides in the irradiance's fourth channel, which the filter does not use. 36 bytes per tap instead
//                    of 44 from four arrays, no division by the albedo after this pass. VAR: and the variance, one
//                    float per pixel, -1 for a pixel that is not valid (so that the 3 x 3 mean is nine 4-byte loads and
//                    no id test), the temporal v_0 where the history is long enough, -2 where vd_spatial has to fill
//                    it in.
//   vd_spatial       VAR only: 64 x 8 pixels and their halo of 3 staged in LDS (luminance, guides, key, kind: 28 B a
//                    record); a workgroup none of whose pixels carries -2 leaves before staging.
//   dn_iter_lds<S>   steps 1 ... 16: a tile of 64 consecutive pixels x 8 rows that are S apart (one wave per row) and
//                    its halo -- two rows of the same residue class above and below, 2 S columns left and right --
//                    are staged in LDS once (36 B a record, 29 ... 55 KB; VAR: the variance as a fourth array, 40 B a
//                    record, 61 440 B at S = 16), the 25 taps are ds_read_b128 / b32. The centre's 3 x 3 of adjacent
//                    variances is not in the residue-class tile for S > 1: it is read from global memory at every
//                    step, three contiguous runs per wave.
//   dn_iter_direct   step 32 (its halo of 128 columns would take 83 KB of LDS) and variant 2: one wave = 64
//                    consecutive pixels of one row, every tap one contiguous 1 KiB load per array through L1; the rows
//                    are walked residue class by residue class (y, y + s, y + 2 s, ...), so that the five rows a
//                    workgroup reads are those its neighbours in launch order read, and a column segment stays on one
//                    XCD (its L2 is not shared with the others).
//   The last iteration multiplies the albedo back, writes rgba_out (VAR: and variance_out) and packs `pixels` itself.
// Variant 1 (the yardstick): dn_plain, one thread per pixel, every tap from the caller's four guide arrays (VAR: and
//   the variance arrays), the demodulation of iteration 0 per tap, no packing, no LDS. VAR: vd_plain_v0 first forms v_0
//   of every pixel from the caller's arrays into a scratch float array (the 49 taps of the spatial estimate per pixel,
//   not per tap of a tap).
// Variant 2: variant 0 with dn_iter_direct at every step (what LDS staging buys is variant 2 minus variant 0); VAR: at
//   the one step the caller chooses (lds16).
//
// All evaluate dn_centre / dn_tap / dn_tap_centre below on the same values in the same order: the same bits, and with
// a variance of 0 the VAR = true result is the VAR = false one with sigma_colour = sigma_floor, bit for bit.
// Only + - * / and compares; the library is built with -ffp-contract=off and correctly rounded division.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_filter.h"
#include "rt_internal.h"

namespace {

constexpr int DN_ROW = 256;            // pixels of one row per workgroup of dn_iter_direct / dn_plain / dn_pack
constexpr int DN_TW = 64, DN_TH = 8;   // tile of dn_iter_lds and vd_spatial: one wave per row
constexpr float VD_VMAX = 1099511627776.f;      // 2^40
constexpr float VD_NEEDS_SPATIAL = -2.f, VD_NOT_VALID = -1.f;

struct DnArgs {                        // by value; what only VAR reads comes last, so that the others' part stays short
    int w, h, step, shift, demod, use_colour;  // use_colour: !VAR only (VAR always weighs the colour)
    float sigma_depth, sigma_colour2;          // sigma_colour2 = sigma_colour * sigma_colour (binary32)
    // caller's buffers
    const float4 *rgba_in;
    const float *depth;
    const float4 *normal, *albedo;
    const int2 *id;
    float4 *rgba_out;
    uint32_t *pixels;
    // irradiance in / out of this launch (w: the pixel's kind in variants 0 and 2) and the packed guides
    const float4 *src;
    float4 *dst;
    float4 *guide_w;                   // dn_pack's outputs
    int *key_w;
    const float4 *guide;
    const int *key;
    // VAR only: the caller's moments and variance, the variance in / out of this launch
    float sigma_floor2, spatial_boost, min_history;
    const float2 *moments;
    float *variance_out;
    const float *vsrc;
    float *vdst;
};

struct DnCentre {
    float nx, ny, nz, z, zden2, y, S;  // S: the colour factor's threshold
    int kind, index;
};
struct DnSum {
    float r, g, b, w, v;               // v: VAR only
};

__device__ __forceinline__ float dn_demod(float c, float a) { return c / im_max(a, IM_TINY); }
// a triangle's index does not take part in e_id: every triangle carries index 0
__device__ __forceinline__ int dn_index(int kind, int index) { return kind == RT_HIT_TRIANGLE ? 0 : index; }
__device__ __forceinline__ float dn_h(int d) { return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f); }
__device__ __forceinline__ float vd_g(int d) { return d == 0 ? 0.5f : 0.25f; }

// The centre without its threshold: VAR sets c.S = S(p) (vd_threshold) afterwards.
template <bool VAR>
__device__ __forceinline__ DnCentre dn_centre(const DnArgs &a, int kind, int index, float nx, float ny, float nz, float z,
                                              float r, float g, float b)
{
    DnCentre c;
    c.kind = kind; c.index = index;
    c.nx = nx; c.ny = ny; c.nz = nz; c.z = z;
    const float zden = a.sigma_depth * im_max(fabsf(z), IM_TINY);
    c.zden2 = zden * zden;
    c.y = (VAR || a.use_colour) ? im_luma(r, g, b) : 0.f;
    c.S = a.sigma_colour2;
    return c;
}
// e_n: max(N.N', 0) squared `shift` times
__device__ __forceinline__ float dn_en(const DnArgs &a, const DnCentre &c, float nx, float ny, float nz)
{
    const float dot = (c.nx * nx + c.ny * ny) + c.nz * nz;
    float m = dot > 0.f ? dot : 0.f;
    if (a.shift == 5) {                                 // the default, without the loop's scalar bookkeeping
        m = m * m; m = m * m; m = m * m; m = m * m; m = m * m;
    } else {
        for (int k = 0; k < a.shift; ++k) m = m * m;
    }
    return m;
}
// e_z = 1 / (1 + (dz / zden)^2) as zden^2 / (zden^2 + dz^2), e_c likewise: one division per factor, not two
__device__ __forceinline__ float dn_ez(const DnCentre &c, float z)
{
    const float dz = z - c.z;
    return c.zden2 / (c.zden2 + dz * dz);
}

// One tap that is inside the buffer and is not the centre. hh = h[dx] * h[dy] (exact); v: the tap's variance (VAR).
template <bool VAR>
__device__ __forceinline__ void dn_tap(const DnArgs &a, const DnCentre &c, float hh, int kind, int index, float nx, float ny,
                                       float nz, float z, float r, float g, float b, float v, DnSum &s)
{
    if (kind != c.kind || index != c.index) return;     // e_id = 0 (also: the tap is not valid, since c.kind >= 0)
    float w = hh * dn_en(a, c, nx, ny, nz);
    w = w * dn_ez(c, z);
    if (VAR || a.use_colour) {
        const float dl = im_luma(r, g, b) - c.y;
        w = w * (c.S / (c.S + dl * dl));
    }
    if (!(w > 0.f) || !(w < __builtin_inff())) return;
    s.r = s.r + w * r;
    s.g = s.g + w * g;
    s.b = s.b + w * b;
    s.w = s.w + w;
    if (VAR) s.v = s.v + (w * w) * v;
}
template <bool VAR>
__device__ __forceinline__ void dn_tap_centre(float r, float g, float b, float v, DnSum &s)
{
    const float w = 0.140625f;   // h[0] * h[0] = (6 / 16)^2, without the four factors
    s.r = s.r + w * r;
    s.g = s.g + w * g;
    s.b = s.b + w * b;
    s.w = s.w + w;
    if (VAR) s.v = s.v + (w * w) * v;
}

// What an iteration leaves for a valid pixel (kind_bits: the fourth channel between iterations) ...
template <bool VAR, bool LAST>
__device__ __forceinline__ void dn_write(const DnArgs &a, size_t p, const DnSum &s, float kind_bits)
{
    float r = s.r / s.w, g = s.g / s.w, b = s.b / s.w;
    const float v = VAR ? s.v / (s.w * s.w) : 0.f;
    if (!LAST) {
        a.dst[p] = make_float4(r, g, b, kind_bits);
        if (VAR) a.vdst[p] = v;
        return;
    }
    if (a.demod) {
        const float4 al = a.albedo[p];
        r = r * al.x; g = g * al.y; b = b * al.z;
    }
    a.rgba_out[p] = make_float4(r, g, b, 1.f);
    if (a.pixels) a.pixels[p] = im_pack_colour(r, g, b);
    if (VAR && a.variance_out) a.variance_out[p] = v;
}
// ... and for one that is not valid: `kept` between iterations, its input bits at the end.
template <bool VAR, bool LAST>
__device__ __forceinline__ void dn_write_sky(const DnArgs &a, size_t p, float4 kept)
{
    if (!LAST) {
        a.dst[p] = kept;
        if (VAR) a.vdst[p] = VD_NOT_VALID;
        return;
    }
    const float4 c = a.rgba_in[p];
    a.rgba_out[p] = c;
    if (a.pixels) a.pixels[p] = im_pack_colour(c.x, c.y, c.z);
    if (VAR && a.variance_out) a.variance_out[p] = 0.f;
}

// The temporal v_0: max(m2 - m1 m1, 0), over the albedo's squared luminance when demodulating, at most 2^40.
__device__ __forceinline__ float vd_temporal_v0(const DnArgs &a, size_t p)
{
    const float2 m = a.moments[p];
    float t = m.y - m.x * m.x;
    t = t > 0.f ? t : 0.f;
    if (a.demod) {
        const float4 al = a.albedo[p];
        const float ya = im_max(im_luma(al.x, al.y, al.z), IM_TINY);
        t = t / (ya * ya);
    }
    return t < VD_VMAX ? t : VD_VMAX;
}
__device__ __forceinline__ bool vd_is_temporal(const DnArgs &a, float n) { return a.moments != nullptr && n >= a.min_history; }

// The spatial estimate's sums: one tap that is not the centre, and the centre.
struct VdMoments {
    float W, s1, s2;
};
__device__ __forceinline__ void vd_spatial_tap(const DnArgs &a, const DnCentre &c, int kind, int index, float nx, float ny,
                                               float nz, float z, float y, VdMoments &s)
{
    if (kind != c.kind || index != c.index) return;
    const float w = dn_en(a, c, nx, ny, nz) * dn_ez(c, z);
    if (!(w > 0.f) || !(w < __builtin_inff())) return;
    s.W = s.W + w;
    s.s1 = s.s1 + w * y;
    s.s2 = s.s2 + w * (y * y);
}
__device__ __forceinline__ void vd_spatial_centre(float y, VdMoments &s)
{
    s.W = s.W + 1.f;
    s.s1 = s.s1 + 1.f * y;
    s.s2 = s.s2 + 1.f * (y * y);
}
__device__ __forceinline__ float vd_spatial_v0(const DnArgs &a, const VdMoments &s)
{
    const float mu1 = s.s1 / s.W, mu2 = s.s2 / s.W;
    float t = mu2 - mu1 * mu1;
    t = t > 0.f ? t : 0.f;
    t = t * a.spatial_boost;
    return t < VD_VMAX ? t : VD_VMAX;
}

// S(p) from the 3 x 3 of adjacent variances (v: an array with a negative value where the pixel is not valid; the
// centre is valid).
__device__ __forceinline__ float vd_threshold(const DnArgs &a, const float *v, int x, int y)
{
    float sv = 0.f, sg = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = y + dy;
        if (qy < 0 || qy >= a.h) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= a.w) continue;
            const float vq = v[(size_t)qy * a.w + qx];
            if (!(dx == 0 && dy == 0) && !(vq >= 0.f)) continue;
            const float gg = vd_g(dx) * vd_g(dy);
            sv = sv + gg * vq;
            sg = sg + gg;
        }
    }
    return a.sigma_colour2 * (sv / sg) + a.sigma_floor2;
}

// ---------------------------------------------------------------------------------------------------------------
// Launch order of dn_iter_direct: a 1-D grid of (column segment, row) pairs. Workgroup b runs on XCD b % 8, so the
// segment's low three bits are b's; the rows come residue class by residue class of the step.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool dn_direct_where(const DnArgs &a, int &x, int &y)
{
    const int nseg = (a.w + DN_ROW - 1) / DN_ROW;
    const int nseg8 = (nseg + 7) >> 3;
    const int b = (int)blockIdx.x;
    const int seg = ((b >> 3) % nseg8) * 8 + (b & 7);
    const int L = (b >> 3) / nseg8;               // position of the row in launch order, 0 .. h - 1
    const int q = a.h / a.step, rem = a.h - q * a.step;
    int cls, k;
    if (L < rem * (q + 1)) {
        cls = L / (q + 1);
        k = L - cls * (q + 1);
    } else {
        const int l2 = L - rem * (q + 1);          // q >= 1 here: rem * (q + 1) = h when q = 0
        cls = rem + l2 / q;
        k = l2 - (l2 / q) * q;
    }
    y = k * a.step + cls;
    x = seg * DN_ROW + (int)threadIdx.x;
    return seg < nseg && x < a.w;
}

template <bool VAR, bool LAST>
__global__ __launch_bounds__(DN_ROW) void dn_iter_direct(const DnArgs a)
{
    int x, y;
    if (!dn_direct_where(a, x, y)) return;
    const size_t p = (size_t)y * a.w + x;
    const float4 cp = a.src[p];
    const int kind = __float_as_int(cp.w);
    if (kind < 0) {                                // sky; a wave of 64 sky pixels ends here
        dn_write_sky<VAR, LAST>(a, p, cp);
        return;
    }
    const float4 gp = a.guide[p];
    DnCentre c = dn_centre<VAR>(a, kind, a.key[p], gp.x, gp.y, gp.z, gp.w, cp.x, cp.y, cp.z);
    if (VAR) c.S = vd_threshold(a, a.vsrc, x, y);
    DnSum s = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * a.step;
        if (qy < 0 || qy >= a.h) continue;         // wave-uniform
        // the row's five taps are loaded together (from a clamped column where a tap is outside), then weighted
        float4 cq[5], gq[5];
        int kq[5];
        float vq[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * a.step;
            const size_t q = (size_t)qy * a.w + (qx < 0 ? 0 : (qx >= a.w ? a.w - 1 : qx));
            if (!VAR && dx == 0 && dy == 0) continue;   // the centre's records are cp and gp; VAR needs its variance
            cq[dx + 2] = a.src[q];
            gq[dx + 2] = a.guide[q];
            kq[dx + 2] = a.key[q];
            if (VAR) vq[dx + 2] = a.vsrc[q];
        }
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            if (dx == 0 && dy == 0) {
                dn_tap_centre<VAR>(cp.x, cp.y, cp.z, vq[2], s);
                continue;
            }
            const int qx = x + dx * a.step;
            if (qx < 0 || qx >= a.w) continue;
            const float4 c4 = cq[dx + 2], g4 = gq[dx + 2];
            dn_tap<VAR>(a, c, dn_h(dx) * dn_h(dy), __float_as_int(c4.w), kq[dx + 2], g4.x, g4.y, g4.z, g4.w, c4.x, c4.y, c4.z,
                        vq[dx + 2], s);
        }
    }
    dn_write<VAR, LAST>(a, p, s, cp.w);
}

// Steps 1 ... 16: the tile and its halo from LDS. The tile is 64 consecutive pixels of 8 rows that are `S` apart (one
// residue class of the step), so the rows its taps need are 12 rows of the same class -- a halo of two rows above and
// below at any step -- and 2 S more columns on either side. A record outside the buffer is staged as "not valid"
// (kind -1), which no valid centre matches: the tap loop needs no bounds.
template <bool VAR, int S, bool LAST>
__global__ __launch_bounds__(DN_TW * DN_TH) void dn_iter_lds(const DnArgs a)
{
    constexpr int HALO = 2 * S, LW = DN_TW + 2 * HALO, LH = DN_TH + 4;
    __shared__ float4 l_col[LW * LH];
    __shared__ float4 l_gd[LW * LH];
    __shared__ int l_key[LW * LH];
    __shared__ float l_var[VAR ? LW * LH : 1];     // not referenced, so not allocated, without VAR
    // blockIdx.y = (residue class, group of 8 rows of it); every class gets the groups of the largest
    const int gpc = ((a.h + S - 1) / S + DN_TH - 1) / DN_TH;
    const int cls = (int)blockIdx.y / gpc, j0 = ((int)blockIdx.y - cls * gpc) * DN_TH;
    if (cls + j0 * S >= a.h) return;               // no row of the tile is in the buffer (the whole workgroup leaves)
    const int x0 = (int)blockIdx.x * DN_TW - HALO;
    for (int i = (int)threadIdx.x; i < LW * LH; i += DN_TW * DN_TH) {
        const int ly = i / LW, lx = i - ly * LW;
        const int gx = x0 + lx, gy = cls + (j0 + ly - 2) * S;
        float4 cq = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
        float4 gq = make_float4(0.f, 0.f, 0.f, 0.f);
        int kq = 0;
        float vq = 0.f;
        if (gx >= 0 && gx < a.w && gy >= 0 && gy < a.h) {
            const size_t q = (size_t)gy * a.w + gx;
            cq = a.src[q];
            if (__float_as_int(cq.w) >= 0) {
                gq = a.guide[q];
                kq = a.key[q];
                if constexpr (VAR) vq = a.vsrc[q];
            }
        }
        l_col[i] = cq;
        l_gd[i] = gq;
        l_key[i] = kq;
        if constexpr (VAR) l_var[i] = vq;
    }
    __syncthreads();
    const int tx = (int)threadIdx.x & (DN_TW - 1), ty = (int)threadIdx.x / DN_TW;
    const int x = (int)blockIdx.x * DN_TW + tx, y = cls + (j0 + ty) * S;
    if (x >= a.w || y >= a.h) return;
    const size_t p = (size_t)y * a.w + x;
    const int lp = (ty + 2) * LW + tx + HALO;
    const float4 cp = l_col[lp];
    const int kind = __float_as_int(cp.w);
    if (kind < 0) {
        dn_write_sky<VAR, LAST>(a, p, cp);
        return;
    }
    const float4 gp = l_gd[lp];
    DnCentre c = dn_centre<VAR>(a, kind, l_key[lp], gp.x, gp.y, gp.z, gp.w, cp.x, cp.y, cp.z);
    if (VAR) c.S = vd_threshold(a, a.vsrc, x, y);
    DnSum s = {0.f, 0.f, 0.f, 0.f, 0.f};
    auto variance = [&](int lq) {
        if constexpr (VAR) return l_var[lq];
        else return 0.f;
    };
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int lq = lp + dy * LW + dx * S;
            if (dx == 0 && dy == 0) {
                dn_tap_centre<VAR>(cp.x, cp.y, cp.z, variance(lq), s);
                continue;
            }
            const float4 cq = l_col[lq];
            const int kq = __float_as_int(cq.w);
            if (kq != c.kind) continue;            // skips what is outside the buffer and what is not valid
            const float4 gq = l_gd[lq];
            dn_tap<VAR>(a, c, dn_h(dx) * dn_h(dy), kq, l_key[lq], gq.x, gq.y, gq.z, gq.w, cq.x, cq.y, cq.z, variance(lq), s);
        }
    }
    dn_write<VAR, LAST>(a, p, s, cp.w);
}

template <bool VAR, int S>
hipError_t dn_launch_lds(const DnArgs &a, bool last, hipStream_t stream)
{
    const int gpc = ((a.h + S - 1) / S + DN_TH - 1) / DN_TH;
    const dim3 grid((a.w + DN_TW - 1) / DN_TW, gpc * S), block(DN_TW * DN_TH);
    if (last) hipLaunchKernelGGL((dn_iter_lds<VAR, S, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((dn_iter_lds<VAR, S, false>), grid, block, 0, stream, a);
    return hipGetLastError();
}

template <bool VAR>
__global__ __launch_bounds__(DN_ROW) void dn_pack(const DnArgs a)
{
    const size_t p = (size_t)blockIdx.x * DN_ROW + threadIdx.x;
    if (p >= (size_t)a.w * a.h) return;
    const int2 id = a.id[p];
    float4 c = a.rgba_in[p];
    if (id.x < 0) {                                // sky: no iteration reads its guides
        c.w = __int_as_float(-1);
        a.dst[p] = c;
        if (VAR) a.vdst[p] = VD_NOT_VALID;
        return;
    }
    if (VAR) a.vdst[p] = vd_is_temporal(a, c.w) ? vd_temporal_v0(a, p) : VD_NEEDS_SPATIAL;
    if (a.demod) {
        const float4 al = a.albedo[p];
        c.x = dn_demod(c.x, al.x); c.y = dn_demod(c.y, al.y); c.z = dn_demod(c.z, al.z);
    }
    c.w = __int_as_float(id.x);
    a.dst[p] = c;
    const float4 n = a.normal[p];
    a.guide_w[p] = make_float4(n.x, n.y, n.z, a.depth[p]);
    a.key_w[p] = dn_index(id.x, id.y);
}

// ---------------------------------------------------------------------------------------------------------------
// vd_spatial: v_0 of the pixels dn_pack marked, over the packed records (src: I_0 with the kind, guide, key); reads
// and writes a.vdst at the thread's own pixel only.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DN_TW * DN_TH) void vd_spatial(const DnArgs a)
{
    constexpr int HALO = 3, LW = DN_TW + 2 * HALO, LH = DN_TH + 2 * HALO;
    __shared__ float4 l_gd[LW * LH];
    __shared__ float l_y[LW * LH];
    __shared__ int l_kind[LW * LH];
    __shared__ int l_key[LW * LH];
    const int tx = (int)threadIdx.x & (DN_TW - 1), ty = (int)threadIdx.x / DN_TW;
    const int x = (int)blockIdx.x * DN_TW + tx, y = (int)blockIdx.y * DN_TH + ty;
    const bool inside = x < a.w && y < a.h;
    const size_t p = inside ? (size_t)y * a.w + x : 0;
    const bool needs = inside && a.vdst[p] == VD_NEEDS_SPATIAL;
    if (!__syncthreads_or(needs ? 1 : 0)) return;  // the whole workgroup leaves before staging
    const int x0 = (int)blockIdx.x * DN_TW - HALO, y0 = (int)blockIdx.y * DN_TH - HALO;
    for (int i = (int)threadIdx.x; i < LW * LH; i += DN_TW * DN_TH) {
        const int ly = i / LW, lx = i - ly * LW;
        const int gx = x0 + lx, gy = y0 + ly;
        float4 gq = make_float4(0.f, 0.f, 0.f, 0.f);
        float yq = 0.f;
        int kind = -1, kq = 0;
        if (gx >= 0 && gx < a.w && gy >= 0 && gy < a.h) {
            const size_t q = (size_t)gy * a.w + gx;
            const float4 cq = a.src[q];
            kind = __float_as_int(cq.w);
            if (kind >= 0) {
                yq = im_luma(cq.x, cq.y, cq.z);
                gq = a.guide[q];
                kq = a.key[q];
            }
        }
        l_gd[i] = gq;
        l_y[i] = yq;
        l_kind[i] = kind;
        l_key[i] = kq;
    }
    __syncthreads();
    if (!needs) return;
    const int lp = (ty + HALO) * LW + tx + HALO;
    const float4 gp = l_gd[lp];
    const DnCentre c = dn_centre<true>(a, l_kind[lp], l_key[lp], gp.x, gp.y, gp.z, gp.w, 0.f, 0.f, 0.f);
    VdMoments s = {0.f, 0.f, 0.f};
    for (int dy = -HALO; dy <= HALO; ++dy) {
#pragma unroll
        for (int dx = -HALO; dx <= HALO; ++dx) {
            const int lq = lp + dy * LW + dx;
            if (dx == 0 && dy == 0) {
                vd_spatial_centre(l_y[lq], s);
                continue;
            }
            const int kq = l_kind[lq];
            if (kq != c.kind) continue;            // skips what is outside the buffer and what is not valid
            const float4 gq = l_gd[lq];
            vd_spatial_tap(a, c, kq, l_key[lq], gq.x, gq.y, gq.z, gq.w, l_y[lq], s);
        }
    }
    a.vdst[p] = vd_spatial_v0(a, s);
}

// ---------------------------------------------------------------------------------------------------------------
// The yardstick: everything from the caller's arrays.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 dn_irradiance0(const DnArgs &a, size_t q)
{
    float4 cq = a.rgba_in[q];
    if (a.demod) {
        const float4 al = a.albedo[q];
        cq.x = dn_demod(cq.x, al.x); cq.y = dn_demod(cq.y, al.y); cq.z = dn_demod(cq.z, al.z);
    }
    return cq;
}

__global__ __launch_bounds__(DN_ROW) void vd_plain_v0(const DnArgs a)
{
    const int x = (int)blockIdx.x * DN_ROW + (int)threadIdx.x, y = (int)blockIdx.y;
    if (x >= a.w) return;
    const size_t p = (size_t)y * a.w + x;
    const int2 id = a.id[p];
    if (id.x < 0) {
        a.vdst[p] = VD_NOT_VALID;
        return;
    }
    if (vd_is_temporal(a, a.rgba_in[p].w)) {
        a.vdst[p] = vd_temporal_v0(a, p);
        return;
    }
    const float4 np = a.normal[p];
    const DnCentre c = dn_centre<true>(a, id.x, dn_index(id.x, id.y), np.x, np.y, np.z, a.depth[p], 0.f, 0.f, 0.f);
    VdMoments s = {0.f, 0.f, 0.f};
    for (int dy = -3; dy <= 3; ++dy) {
        const int qy = y + dy;
        if (qy < 0 || qy >= a.h) continue;
        for (int dx = -3; dx <= 3; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= a.w) continue;
            const size_t q = (size_t)qy * a.w + qx;
            if (dx == 0 && dy == 0) {
                const float4 cq = dn_irradiance0(a, q);
                vd_spatial_centre(im_luma(cq.x, cq.y, cq.z), s);
                continue;
            }
            const int2 iq = a.id[q];
            if (iq.x < 0) continue;
            const float4 cq = dn_irradiance0(a, q);
            const float4 nq = a.normal[q];
            vd_spatial_tap(a, c, iq.x, dn_index(iq.x, iq.y), nq.x, nq.y, nq.z, a.depth[q], im_luma(cq.x, cq.y, cq.z), s);
        }
    }
    a.vdst[p] = vd_spatial_v0(a, s);
}

// FIRST: the irradiance is the caller's rgba, demodulated per tap (a.src is not read).
template <bool VAR, bool FIRST, bool LAST>
__global__ __launch_bounds__(DN_ROW) void dn_plain(const DnArgs a)
{
    const int x = (int)blockIdx.x * DN_ROW + (int)threadIdx.x, y = (int)blockIdx.y;
    if (x >= a.w) return;
    const size_t p = (size_t)y * a.w + x;
    const int2 id = a.id[p];
    if (id.x < 0) {                                // between iterations no tap reads its irradiance
        if (LAST) dn_write_sky<VAR, true>(a, p, make_float4(0.f, 0.f, 0.f, 0.f));
        else if (VAR) a.vdst[p] = VD_NOT_VALID;
        return;
    }
    auto irradiance = [&](size_t q) { return FIRST ? dn_irradiance0(a, q) : a.src[q]; };
    const float4 cp = irradiance(p);
    const float4 np = a.normal[p];
    DnCentre c = dn_centre<VAR>(a, id.x, dn_index(id.x, id.y), np.x, np.y, np.z, a.depth[p], cp.x, cp.y, cp.z);
    if (VAR) c.S = vd_threshold(a, a.vsrc, x, y);
    DnSum s = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * a.step;
        if (qy < 0 || qy >= a.h) continue;
        for (int dx = -2; dx <= 2; ++dx) {
            if (dx == 0 && dy == 0) {
                dn_tap_centre<VAR>(cp.x, cp.y, cp.z, VAR ? a.vsrc[p] : 0.f, s);
                continue;
            }
            const int qx = x + dx * a.step;
            if (qx < 0 || qx >= a.w) continue;
            const size_t q = (size_t)qy * a.w + qx;
            const int2 iq = a.id[q];
            if (iq.x < 0) continue;
            const float4 cq = irradiance(q);
            const float4 nq = a.normal[q];
            dn_tap<VAR>(a, c, dn_h(dx) * dn_h(dy), iq.x, dn_index(iq.x, iq.y), nq.x, nq.y, nq.z, a.depth[q], cq.x, cq.y, cq.z,
                        VAR ? a.vsrc[q] : 0.f, s);
        }
    }
    dn_write<VAR, LAST>(a, p, s, 1.f);
}

// The traffic floor's yardstick (tools/bench_denoise.py): a float4 copy of n16 float4s.
__global__ __launch_bounds__(256) void dn_copy16(const float4 *__restrict__ src, float4 *__restrict__ dst, size_t n16)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n16) dst[i] = src[i];
}

template <typename K>
hipError_t dn_launch(K kernel, dim3 grid, dim3 block, const DnArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, a);
    return hipGetLastError();
}

#define DN_HIP(...)   /* variadic: an expression may name a template with several arguments */ \
    do {                                                                     \
        hipError_t dn_e_ = (__VA_ARGS__);                                    \
        if (dn_e_ != hipSuccess) return rt_hip_fail(dn_e_, #__VA_ARGS__, __FILE__, __LINE__); \
    } while (0)

// Both filters' launches. n_lds: how many leading iterations of variants 0 and 2 run dn_iter_lds (the others
// dn_iter_direct); var0 / var1: null without VAR. An event is recorded before the first launch and after every one.
template <bool VAR>
int dn_run(const RtAtrousDesc *d, int n_lds, float4 *col0, float4 *col1, float4 *guide, int *key, float *var0, float *var1,
           hipEvent_t *ev, hipStream_t stream)
{
    DnArgs a = {};
    a.w = d->width; a.h = d->height;
    a.shift = d->normal_shift;
    a.demod = d->demodulate != 0;
    a.use_colour = d->sigma_colour > 0.f;
    a.sigma_depth = d->sigma_depth;
    a.sigma_colour2 = d->sigma_colour * d->sigma_colour;
    a.sigma_floor2 = d->sigma_floor * d->sigma_floor;
    a.spatial_boost = d->spatial_boost;
    a.min_history = (float)d->min_history;
    a.rgba_in = (const float4 *)d->rgba_in;
    a.depth = d->depth;
    a.normal = (const float4 *)d->normal;
    a.albedo = (const float4 *)d->albedo;
    a.id = (const int2 *)d->id;
    a.moments = (const float2 *)d->moments;
    a.rgba_out = (float4 *)d->rgba_out;
    a.pixels = d->pixels;
    a.variance_out = d->variance_out;
    a.guide = guide; a.key = key;
    a.guide_w = guide; a.key_w = key;
    const size_t npx = (size_t)a.w * a.h;
    const int n = d->iterations;
    float4 *buf[2] = {col0, col1};
    float *var[2] = {var0, var1};
    int nev = 0;
    if (ev) DN_HIP(hipEventRecord(ev[nev++], stream));

    if (d->variant == 1) {
        if (n == 1 && d->rgba_out == d->rgba_in) {   // one launch reads the neighbours it would overwrite: from a copy
            DN_HIP(hipMemcpyAsync(col1, d->rgba_in, npx * sizeof(float4), hipMemcpyDeviceToDevice, stream));
            a.rgba_in = col1;
        }
        const dim3 grid((a.w + DN_ROW - 1) / DN_ROW, a.h), block(DN_ROW);
        if (VAR) {
            a.vdst = var[0];
            DN_HIP(dn_launch(vd_plain_v0, grid, block, a, stream));
            if (ev) DN_HIP(hipEventRecord(ev[nev++], stream));
        }
        for (int i = 0; i < n; ++i) {
            a.step = 1 << i;
            a.src = buf[(i + 1) & 1];               // of iteration i - 1 (not read by the first)
            a.dst = buf[i & 1];
            a.vsrc = var[i & 1];
            a.vdst = var[(i + 1) & 1];
            const bool last = i == n - 1;
            if (i == 0) DN_HIP(last ? dn_launch(dn_plain<VAR, true, true>, grid, block, a, stream) : dn_launch(dn_plain<VAR, true, false>, grid, block, a, stream));
            else DN_HIP(last ? dn_launch(dn_plain<VAR, false, true>, grid, block, a, stream) : dn_launch(dn_plain<VAR, false, false>, grid, block, a, stream));
            if (ev) DN_HIP(hipEventRecord(ev[nev++], stream));
        }
        return RT_OK;
    }

    a.dst = buf[0];
    a.vdst = var[0];
    DN_HIP(dn_launch(dn_pack<VAR>, dim3((unsigned)((npx + DN_ROW - 1) / DN_ROW)), dim3(DN_ROW), a, stream));
    if (ev) DN_HIP(hipEventRecord(ev[nev++], stream));
    if (VAR) {
        a.src = buf[0];
        DN_HIP(dn_launch(vd_spatial, dim3((a.w + DN_TW - 1) / DN_TW, (a.h + DN_TH - 1) / DN_TH), dim3(DN_TW * DN_TH), a, stream));
        if (ev) DN_HIP(hipEventRecord(ev[nev++], stream));
    }
    for (int i = 0; i < n; ++i) {
        a.step = 1 << i;
        a.src = buf[i & 1];
        a.dst = buf[(i + 1) & 1];
        a.vsrc = var[i & 1];
        a.vdst = var[(i + 1) & 1];
        const bool last = i == n - 1;
        if (i < n_lds) {
            DN_HIP(i == 0 ? dn_launch_lds<VAR, 1>(a, last, stream) : i == 1 ? dn_launch_lds<VAR, 2>(a, last, stream) :
                   i == 2 ? dn_launch_lds<VAR, 4>(a, last, stream) : i == 3 ? dn_launch_lds<VAR, 8>(a, last, stream) :
                            dn_launch_lds<VAR, 16>(a, last, stream));
        } else {
            const int nseg8 = ((a.w + DN_ROW - 1) / DN_ROW + 7) >> 3;
            const dim3 grid((unsigned)((size_t)nseg8 * 8 * a.h)), block(DN_ROW);
            DN_HIP(last ? dn_launch(dn_iter_direct<VAR, true>, grid, block, a, stream) : dn_launch(dn_iter_direct<VAR, false>, grid, block, a, stream));
        }
        if (ev) DN_HIP(hipEventRecord(ev[nev++], stream));
    }
    return RT_OK;
}

}   // namespace

// d: validated. col0 / col1 / guide / key: the scene's scratch, room for width * height pixels (guide and key may be
// null for variant 1). ev: null, or iterations + 2 timing events, recorded around every launch.
int rt_denoise_launch(const RtAtrousDesc *d, float4 *col0, float4 *col1, float4 *guide, int *key, hipEvent_t *ev,
                      hipStream_t stream)
{
    return dn_run<false>(d, d->variant == 0 ? 5 : 0, col0, col1, guide, key, nullptr, nullptr, ev, stream);
}

// The same with var0 / var1, room for width * height floats each. ev: null, or iterations + 3 timing events. lds16:
// step 16 runs dn_iter_lds<16> (else dn_iter_direct).
int rt_vdenoise_launch(const RtAtrousDesc *d, float4 *col0, float4 *col1, float4 *guide, int *key, float *var0, float *var1,
                       bool lds16, hipEvent_t *ev, hipStream_t stream)
{
    return dn_run<true>(d, lds16 ? 5 : 4, col0, col1, guide, key, var0, var1, ev, stream);
}

// bytes / 16 float4s from src to dst (both 16-byte aligned device buffers, disjoint): the copy the traffic floor of
// DESIGN.md 6f is measured with.
extern "C" int rt_debug_copy16(const void *src, void *dst, size_t n16, void *stream)
{
    if (!src || !dst || (((uintptr_t)src | (uintptr_t)dst) & 15u)) return RT_ERR_INVALID;
    if (n16 == 0) return RT_OK;
    hipLaunchKernelGGL(dn_copy16, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float4 *)src, (float4 *)dst, n16);
    DN_HIP(hipGetLastError());
    return RT_OK;
}
