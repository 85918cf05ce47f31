// rt_vdenoise.hip -- the variance-guided denoiser (rt_scene_denoise_variance): rt_denoise.hip's a-trous
// filter with a per-pixel luminance threshold, S(p) = sigma_colour^2 * (3 x 3 mean of the variance) + sigma_floor^2.
// The variance starts from the temporal moments where the history is long, from the 7 x 7 neighbourhood where it is
// short, and is carried through the iterations beside the irradiance.
//
// Variant 0 (the product):
//   vd_pack          dn_pack plus the variance: one float per pixel, -1 for a pixel that is not valid (so that the
//                    3 x 3 mean is nine 4-byte loads and no id test), the temporal v_0 where the history is long
//                    enough, -2 where the spatial pass has to fill it in.
//   vd_spatial       64 x 8 pixels and their halo of 3 staged in LDS (luminance, guides, key, kind: 28 B a record); a
//                    workgroup none of whose pixels carries -2 leaves before staging.
//   vd_iter_lds<S>   steps 1 ... 16: dn_iter_lds<S> with the variance as a fourth staged array (40 B a record, 61 440 B
//                    at S = 16). The centre's 3 x 3 of adjacent variances is not in the residue-class tile for S > 1: it
//                    is read from global memory at every step, three contiguous runs per wave.
//   vd_iter_direct   step 32: dn_iter_direct with the variance array.
//   The last iteration multiplies the albedo back and writes rgba_out, pixels and variance_out itself.
// Variant 1 (the yardstick): vd_plain_v0 forms v_0 of every pixel from the caller's arrays into a scratch float array
//   (the 49 taps of the spatial estimate per pixel, not per tap of a tap); vd_plain, one thread per pixel, every tap from
//   the caller's arrays and the variance arrays, the demodulation of iteration 0 per tap.
//
// The weights are rt_denoise.hip's, restated here word for word (that file is not touched: its inline functions live in
// its anonymous namespace): the same operations on the same values in the same order, so that with a variance of 0 the
// result is rt_scene_denoise's with sigma_colour = sigma_floor, bit for bit. Only + - * / and compares.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_internal.h"

namespace {

constexpr int VD_ROW = 256;            // pixels of one row per workgroup of vd_iter_direct / vd_plain / vd_pack
constexpr int VD_TW = 64, VD_TH = 8;   // tile of vd_iter_lds and vd_spatial: one wave per row
constexpr float VD_TINY = 0.0009765625f;        // 2^-10
constexpr float VD_VMAX = 1099511627776.f;      // 2^40
constexpr float VD_NEEDS_SPATIAL = -2.f, VD_NOT_VALID = -1.f;

struct VdArgs {                        // by value
    int w, h, step, shift, demod;
    float sigma_depth, sigma_colour2, sigma_floor2, spatial_boost, min_history;
    // caller's buffers
    const float4 *rgba_in;
    const float *depth;
    const float4 *normal, *albedo;
    const int2 *id;
    const float2 *moments;
    float4 *rgba_out;
    uint32_t *pixels;
    float *variance_out;
    // irradiance and variance in / out of this launch, and the packed guides
    const float4 *src;
    float4 *dst;
    const float *vsrc;
    float *vdst;
    float4 *guide_w;                   // vd_pack's outputs
    int *key_w;
    const float4 *guide;
    const int *key;
};

struct VdCentre {
    float nx, ny, nz, z, zden2, y, S;
    int kind, index;
};
struct VdSum {
    float r, g, b, w, v;
};

__device__ __forceinline__ float vd_max(float a, float b) { return a > b ? a : b; }   // a NaN `a` gives b
__device__ __forceinline__ float vd_luma(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
__device__ __forceinline__ float vd_demod(float c, float a) { return c / vd_max(a, VD_TINY); }
__device__ __forceinline__ uint32_t vd_pack_colour(float r, float g, float b)
{
    int ir = (int)(r * 254.f), ig = (int)(g * 254.f), ib = (int)(b * 254.f);
    if (ir > 255) ir = 255;
    if (ig > 255) ig = 255;
    if (ib > 255) ib = 255;
    return (uint32_t)(((ir & 0xff) << 16) + ((ig & 0xff) << 8) + (ib & 0xff));
}
__device__ __forceinline__ int vd_index(int kind, int index) { return kind == RT_HIT_TRIANGLE ? 0 : index; }
__device__ __forceinline__ float vd_h(int d) { return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f); }
__device__ __forceinline__ float vd_g(int d) { return d == 0 ? 0.5f : 0.25f; }

__device__ __forceinline__ VdCentre vd_centre(const VdArgs &a, int kind, int index, float nx, float ny, float nz, float z,
                                              float r, float g, float b)
{
    VdCentre c;
    c.kind = kind; c.index = index;
    c.nx = nx; c.ny = ny; c.nz = nz; c.z = z;
    const float zden = a.sigma_depth * vd_max(fabsf(z), VD_TINY);
    c.zden2 = zden * zden;
    c.y = vd_luma(r, g, b);
    c.S = 0.f;
    return c;
}
// e_n: max(N.N', 0) squared `shift` times
__device__ __forceinline__ float vd_en(const VdArgs &a, const VdCentre &c, float nx, float ny, float nz)
{
    const float dot = (c.nx * nx + c.ny * ny) + c.nz * nz;
    float m = dot > 0.f ? dot : 0.f;
    if (a.shift == 5) {
        m = m * m; m = m * m; m = m * m; m = m * m; m = m * m;
    } else {
        for (int k = 0; k < a.shift; ++k) m = m * m;
    }
    return m;
}
__device__ __forceinline__ float vd_ez(const VdCentre &c, float z)
{
    const float dz = z - c.z;
    return c.zden2 / (c.zden2 + dz * dz);
}

// The temporal v_0: max(m2 - m1 m1, 0), over the albedo's squared luminance when demodulating, at most 2^40.
__device__ __forceinline__ float vd_temporal_v0(const VdArgs &a, size_t p)
{
    const float2 m = a.moments[p];
    float t = m.y - m.x * m.x;
    t = t > 0.f ? t : 0.f;
    if (a.demod) {
        const float4 al = a.albedo[p];
        const float ya = vd_max(vd_luma(al.x, al.y, al.z), VD_TINY);
        t = t / (ya * ya);
    }
    return t < VD_VMAX ? t : VD_VMAX;
}
__device__ __forceinline__ bool vd_is_temporal(const VdArgs &a, float n) { return a.moments != nullptr && n >= a.min_history; }

// The spatial estimate's sums: one tap that is not the centre, and the centre.
struct VdMoments {
    float W, s1, s2;
};
__device__ __forceinline__ void vd_spatial_tap(const VdArgs &a, const VdCentre &c, int kind, int index, float nx, float ny,
                                               float nz, float z, float y, VdMoments &s)
{
    if (kind != c.kind || index != c.index) return;
    const float w = vd_en(a, c, nx, ny, nz) * vd_ez(c, z);
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
__device__ __forceinline__ float vd_spatial_v0(const VdArgs &a, const VdMoments &s)
{
    const float mu1 = s.s1 / s.W, mu2 = s.s2 / s.W;
    float t = mu2 - mu1 * mu1;
    t = t > 0.f ? t : 0.f;
    t = t * a.spatial_boost;
    return t < VD_VMAX ? t : VD_VMAX;
}

// S(p) from the 3 x 3 of adjacent variances (v: an array with a negative value where the pixel is not valid; the
// centre is valid).
__device__ __forceinline__ float vd_threshold(const VdArgs &a, const float *v, int x, int y)
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

// One tap that is inside the buffer and is not the centre. hh = h[dx] * h[dy] (exact).
__device__ __forceinline__ void vd_tap(const VdArgs &a, const VdCentre &c, float hh, int kind, int index, float nx, float ny,
                                       float nz, float z, float r, float g, float b, float v, VdSum &s)
{
    if (kind != c.kind || index != c.index) return;
    float w = hh * vd_en(a, c, nx, ny, nz);
    w = w * vd_ez(c, z);
    const float dl = vd_luma(r, g, b) - c.y;
    w = w * (c.S / (c.S + dl * dl));
    if (!(w > 0.f) || !(w < __builtin_inff())) return;
    s.r = s.r + w * r;
    s.g = s.g + w * g;
    s.b = s.b + w * b;
    s.w = s.w + w;
    s.v = s.v + (w * w) * v;
}
__device__ __forceinline__ void vd_tap_centre(float r, float g, float b, float v, VdSum &s)
{
    const float w = 0.140625f;
    s.r = s.r + w * r;
    s.g = s.g + w * g;
    s.b = s.b + w * b;
    s.w = s.w + w;
    s.v = s.v + (w * w) * v;
}

// What an iteration leaves for a valid pixel and for one that is not.
template <bool LAST>
__device__ __forceinline__ void vd_write(const VdArgs &a, size_t p, const VdSum &s, float kind_bits)
{
    float r = s.r / s.w, g = s.g / s.w, b = s.b / s.w;
    const float v = s.v / (s.w * s.w);
    if (!LAST) {
        a.dst[p] = make_float4(r, g, b, kind_bits);
        a.vdst[p] = v;
        return;
    }
    if (a.demod) {
        const float4 al = a.albedo[p];
        r = r * al.x; g = g * al.y; b = b * al.z;
    }
    a.rgba_out[p] = make_float4(r, g, b, 1.f);
    if (a.pixels) a.pixels[p] = vd_pack_colour(r, g, b);
    if (a.variance_out) a.variance_out[p] = v;
}
template <bool LAST>
__device__ __forceinline__ void vd_write_sky(const VdArgs &a, size_t p, float4 kept)
{
    if (!LAST) {
        a.dst[p] = kept;
        a.vdst[p] = VD_NOT_VALID;
        return;
    }
    const float4 c = a.rgba_in[p];
    a.rgba_out[p] = c;
    if (a.pixels) a.pixels[p] = vd_pack_colour(c.x, c.y, c.z);
    if (a.variance_out) a.variance_out[p] = 0.f;
}

// ---------------------------------------------------------------------------------------------------------------
// vd_pack
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VD_ROW) void vd_pack(const VdArgs a)
{
    const size_t p = (size_t)blockIdx.x * VD_ROW + threadIdx.x;
    if (p >= (size_t)a.w * a.h) return;
    const int2 id = a.id[p];
    float4 c = a.rgba_in[p];
    if (id.x < 0) {                                // sky: no iteration reads its guides
        c.w = __int_as_float(-1);
        a.dst[p] = c;
        a.vdst[p] = VD_NOT_VALID;
        return;
    }
    a.vdst[p] = vd_is_temporal(a, c.w) ? vd_temporal_v0(a, p) : VD_NEEDS_SPATIAL;
    if (a.demod) {
        const float4 al = a.albedo[p];
        c.x = vd_demod(c.x, al.x); c.y = vd_demod(c.y, al.y); c.z = vd_demod(c.z, al.z);
    }
    c.w = __int_as_float(id.x);
    a.dst[p] = c;
    const float4 n = a.normal[p];
    a.guide_w[p] = make_float4(n.x, n.y, n.z, a.depth[p]);
    a.key_w[p] = vd_index(id.x, id.y);
}

// ---------------------------------------------------------------------------------------------------------------
// vd_spatial: v_0 of the pixels vd_pack marked, over the packed records (src: I_0 with the kind, guide, key); reads
// and writes a.vdst at the thread's own pixel only.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VD_TW * VD_TH) void vd_spatial(const VdArgs a)
{
    constexpr int HALO = 3, LW = VD_TW + 2 * HALO, LH = VD_TH + 2 * HALO;
    __shared__ float4 l_gd[LW * LH];
    __shared__ float l_y[LW * LH];
    __shared__ int l_kind[LW * LH];
    __shared__ int l_key[LW * LH];
    const int tx = (int)threadIdx.x & (VD_TW - 1), ty = (int)threadIdx.x / VD_TW;
    const int x = (int)blockIdx.x * VD_TW + tx, y = (int)blockIdx.y * VD_TH + ty;
    const bool inside = x < a.w && y < a.h;
    const size_t p = inside ? (size_t)y * a.w + x : 0;
    const bool needs = inside && a.vdst[p] == VD_NEEDS_SPATIAL;
    if (!__syncthreads_or(needs ? 1 : 0)) return;  // the whole workgroup leaves before staging
    const int x0 = (int)blockIdx.x * VD_TW - HALO, y0 = (int)blockIdx.y * VD_TH - HALO;
    for (int i = (int)threadIdx.x; i < LW * LH; i += VD_TW * VD_TH) {
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
                yq = vd_luma(cq.x, cq.y, cq.z);
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
    VdCentre c = vd_centre(a, l_kind[lp], l_key[lp], gp.x, gp.y, gp.z, gp.w, 0.f, 0.f, 0.f);
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
// vd_iter_direct (dn_iter_direct's launch order and wave shape)
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool vd_direct_where(const VdArgs &a, int &x, int &y)
{
    const int nseg = (a.w + VD_ROW - 1) / VD_ROW;
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
    x = seg * VD_ROW + (int)threadIdx.x;
    return seg < nseg && x < a.w;
}

template <bool LAST>
__global__ __launch_bounds__(VD_ROW) void vd_iter_direct(const VdArgs a)
{
    int x, y;
    if (!vd_direct_where(a, x, y)) return;
    const size_t p = (size_t)y * a.w + x;
    const float4 cp = a.src[p];
    const int kind = __float_as_int(cp.w);
    if (kind < 0) {
        vd_write_sky<LAST>(a, p, cp);
        return;
    }
    const float4 gp = a.guide[p];
    VdCentre c = vd_centre(a, kind, a.key[p], gp.x, gp.y, gp.z, gp.w, cp.x, cp.y, cp.z);
    c.S = vd_threshold(a, a.vsrc, x, y);
    VdSum s = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * a.step;
        if (qy < 0 || qy >= a.h) continue;         // wave-uniform
        float4 cq[5], gq[5];
        int kq[5];
        float vq[5];
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * a.step;
            const size_t q = (size_t)qy * a.w + (qx < 0 ? 0 : (qx >= a.w ? a.w - 1 : qx));
            cq[dx + 2] = a.src[q];
            gq[dx + 2] = a.guide[q];
            kq[dx + 2] = a.key[q];
            vq[dx + 2] = a.vsrc[q];
        }
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            if (dx == 0 && dy == 0) {
                vd_tap_centre(cp.x, cp.y, cp.z, vq[2], s);
                continue;
            }
            const int qx = x + dx * a.step;
            if (qx < 0 || qx >= a.w) continue;
            const float4 c4 = cq[dx + 2], g4 = gq[dx + 2];
            vd_tap(a, c, vd_h(dx) * vd_h(dy), __float_as_int(c4.w), kq[dx + 2], g4.x, g4.y, g4.z, g4.w, c4.x, c4.y, c4.z,
                   vq[dx + 2], s);
        }
    }
    vd_write<LAST>(a, p, s, cp.w);
}

// ---------------------------------------------------------------------------------------------------------------
// vd_iter_lds<S> (dn_iter_lds<S>'s tile: 64 pixels x 8 rows of one residue class, 12 rows and 64 + 4 S columns staged)
// ---------------------------------------------------------------------------------------------------------------
template <int S, bool LAST>
__global__ __launch_bounds__(VD_TW * VD_TH) void vd_iter_lds(const VdArgs a)
{
    constexpr int HALO = 2 * S, LW = VD_TW + 2 * HALO, LH = VD_TH + 4;
    __shared__ float4 l_col[LW * LH];
    __shared__ float4 l_gd[LW * LH];
    __shared__ int l_key[LW * LH];
    __shared__ float l_var[LW * LH];
    const int gpc = ((a.h + S - 1) / S + VD_TH - 1) / VD_TH;
    const int cls = (int)blockIdx.y / gpc, j0 = ((int)blockIdx.y - cls * gpc) * VD_TH;
    if (cls + j0 * S >= a.h) return;               // no row of the tile is in the buffer (the whole workgroup leaves)
    const int x0 = (int)blockIdx.x * VD_TW - HALO;
    for (int i = (int)threadIdx.x; i < LW * LH; i += VD_TW * VD_TH) {
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
                vq = a.vsrc[q];
            }
        }
        l_col[i] = cq;
        l_gd[i] = gq;
        l_key[i] = kq;
        l_var[i] = vq;
    }
    __syncthreads();
    const int tx = (int)threadIdx.x & (VD_TW - 1), ty = (int)threadIdx.x / VD_TW;
    const int x = (int)blockIdx.x * VD_TW + tx, y = cls + (j0 + ty) * S;
    if (x >= a.w || y >= a.h) return;
    const size_t p = (size_t)y * a.w + x;
    const int lp = (ty + 2) * LW + tx + HALO;
    const float4 cp = l_col[lp];
    const int kind = __float_as_int(cp.w);
    if (kind < 0) {
        vd_write_sky<LAST>(a, p, cp);
        return;
    }
    const float4 gp = l_gd[lp];
    VdCentre c = vd_centre(a, kind, l_key[lp], gp.x, gp.y, gp.z, gp.w, cp.x, cp.y, cp.z);
    c.S = vd_threshold(a, a.vsrc, x, y);
    VdSum s = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int lq = lp + dy * LW + dx * S;
            if (dx == 0 && dy == 0) {
                vd_tap_centre(cp.x, cp.y, cp.z, l_var[lq], s);
                continue;
            }
            const float4 cq = l_col[lq];
            const int kq = __float_as_int(cq.w);
            if (kq != c.kind) continue;            // skips what is outside the buffer and what is not valid
            const float4 gq = l_gd[lq];
            vd_tap(a, c, vd_h(dx) * vd_h(dy), kq, l_key[lq], gq.x, gq.y, gq.z, gq.w, cq.x, cq.y, cq.z, l_var[lq], s);
        }
    }
    vd_write<LAST>(a, p, s, cp.w);
}

template <int S>
hipError_t vd_launch_lds(const VdArgs &a, bool last, hipStream_t stream)
{
    const int gpc = ((a.h + S - 1) / S + VD_TH - 1) / VD_TH;
    const dim3 grid((a.w + VD_TW - 1) / VD_TW, gpc * S), block(VD_TW * VD_TH);
    if (last) hipLaunchKernelGGL((vd_iter_lds<S, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((vd_iter_lds<S, false>), grid, block, 0, stream, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// The yardstick: everything from the caller's arrays.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 vd_irradiance0(const VdArgs &a, size_t q)
{
    float4 cq = a.rgba_in[q];
    if (a.demod) {
        const float4 al = a.albedo[q];
        cq.x = vd_demod(cq.x, al.x); cq.y = vd_demod(cq.y, al.y); cq.z = vd_demod(cq.z, al.z);
    }
    return cq;
}

__global__ __launch_bounds__(VD_ROW) void vd_plain_v0(const VdArgs a)
{
    const int x = (int)blockIdx.x * VD_ROW + (int)threadIdx.x, y = (int)blockIdx.y;
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
    const VdCentre c = vd_centre(a, id.x, vd_index(id.x, id.y), np.x, np.y, np.z, a.depth[p], 0.f, 0.f, 0.f);
    VdMoments s = {0.f, 0.f, 0.f};
    for (int dy = -3; dy <= 3; ++dy) {
        const int qy = y + dy;
        if (qy < 0 || qy >= a.h) continue;
        for (int dx = -3; dx <= 3; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= a.w) continue;
            const size_t q = (size_t)qy * a.w + qx;
            if (dx == 0 && dy == 0) {
                const float4 cq = vd_irradiance0(a, q);
                vd_spatial_centre(vd_luma(cq.x, cq.y, cq.z), s);
                continue;
            }
            const int2 iq = a.id[q];
            if (iq.x < 0) continue;
            const float4 cq = vd_irradiance0(a, q);
            const float4 nq = a.normal[q];
            vd_spatial_tap(a, c, iq.x, vd_index(iq.x, iq.y), nq.x, nq.y, nq.z, a.depth[q], vd_luma(cq.x, cq.y, cq.z), s);
        }
    }
    a.vdst[p] = vd_spatial_v0(a, s);
}

// FIRST: the irradiance is the caller's rgba, demodulated per tap (a.src is not read).
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(VD_ROW) void vd_plain(const VdArgs a)
{
    const int x = (int)blockIdx.x * VD_ROW + (int)threadIdx.x, y = (int)blockIdx.y;
    if (x >= a.w) return;
    const size_t p = (size_t)y * a.w + x;
    const int2 id = a.id[p];
    if (id.x < 0) {
        if (LAST) vd_write_sky<true>(a, p, make_float4(0.f, 0.f, 0.f, 0.f));
        else a.vdst[p] = VD_NOT_VALID;
        return;
    }
    auto irradiance = [&](size_t q) { return FIRST ? vd_irradiance0(a, q) : a.src[q]; };
    const float4 cp = irradiance(p);
    const float4 np = a.normal[p];
    VdCentre c = vd_centre(a, id.x, vd_index(id.x, id.y), np.x, np.y, np.z, a.depth[p], cp.x, cp.y, cp.z);
    c.S = vd_threshold(a, a.vsrc, x, y);
    VdSum s = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * a.step;
        if (qy < 0 || qy >= a.h) continue;
        for (int dx = -2; dx <= 2; ++dx) {
            if (dx == 0 && dy == 0) {
                vd_tap_centre(cp.x, cp.y, cp.z, a.vsrc[p], s);
                continue;
            }
            const int qx = x + dx * a.step;
            if (qx < 0 || qx >= a.w) continue;
            const size_t q = (size_t)qy * a.w + qx;
            const int2 iq = a.id[q];
            if (iq.x < 0) continue;
            const float4 cq = irradiance(q);
            const float4 nq = a.normal[q];
            vd_tap(a, c, vd_h(dx) * vd_h(dy), iq.x, vd_index(iq.x, iq.y), nq.x, nq.y, nq.z, a.depth[q], cq.x, cq.y, cq.z,
                   a.vsrc[q], s);
        }
    }
    vd_write<LAST>(a, p, s, 1.f);
}

template <typename K>
hipError_t vd_launch(K kernel, dim3 grid, dim3 block, const VdArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, a);
    return hipGetLastError();
}

}   // namespace

#define VD_HIP(expr)                                                         \
    do {                                                                     \
        hipError_t vd_e_ = (expr);                                           \
        if (vd_e_ != hipSuccess) return rt_hip_fail(vd_e_, #expr, __FILE__, __LINE__); \
    } while (0)

// d: validated, in this build's layout. col0 / col1 / guide / key / var0 / var1: the scene's scratch, room for
// width * height pixels each (guide and key may be null for variant 1). ev: null, or iterations + 3 timing events,
// recorded around every launch. lds16: step 16 runs vd_iter_lds<16> (else vd_iter_direct).
int rt_vdenoise_launch(const rt_vdenoise_desc *d, float4 *col0, float4 *col1, float4 *guide, int *key, float *var0,
                       float *var1, bool lds16, hipEvent_t *ev, hipStream_t stream)
{
    VdArgs a = {};
    a.w = d->width; a.h = d->height;
    a.shift = d->normal_shift;
    a.demod = d->demodulate != 0;
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
    if (ev) VD_HIP(hipEventRecord(ev[nev++], stream));

    if (d->variant == 1) {
        if (n == 1 && d->rgba_out == d->rgba_in) {   // one launch reads the neighbours it would overwrite: from a copy
            VD_HIP(hipMemcpyAsync(col1, d->rgba_in, npx * sizeof(float4), hipMemcpyDeviceToDevice, stream));
            a.rgba_in = col1;
        }
        const dim3 grid((a.w + VD_ROW - 1) / VD_ROW, a.h), block(VD_ROW);
        a.vdst = var[0];
        VD_HIP(vd_launch(vd_plain_v0, grid, block, a, stream));
        if (ev) VD_HIP(hipEventRecord(ev[nev++], stream));
        for (int i = 0; i < n; ++i) {
            a.step = 1 << i;
            a.src = buf[(i + 1) & 1];               // of iteration i - 1 (not read by the first)
            a.dst = buf[i & 1];
            a.vsrc = var[i & 1];
            a.vdst = var[(i + 1) & 1];
            const bool last = i == n - 1;
            if (i == 0) VD_HIP(last ? vd_launch(vd_plain<true, true>, grid, block, a, stream) : vd_launch(vd_plain<true, false>, grid, block, a, stream));
            else VD_HIP(last ? vd_launch(vd_plain<false, true>, grid, block, a, stream) : vd_launch(vd_plain<false, false>, grid, block, a, stream));
            if (ev) VD_HIP(hipEventRecord(ev[nev++], stream));
        }
        return RT_OK;
    }

    a.dst = buf[0];
    a.vdst = var[0];
    VD_HIP(vd_launch(vd_pack, dim3((unsigned)((npx + VD_ROW - 1) / VD_ROW)), dim3(VD_ROW), a, stream));
    if (ev) VD_HIP(hipEventRecord(ev[nev++], stream));
    a.src = buf[0];
    VD_HIP(vd_launch(vd_spatial, dim3((a.w + VD_TW - 1) / VD_TW, (a.h + VD_TH - 1) / VD_TH), dim3(VD_TW * VD_TH), a, stream));
    if (ev) VD_HIP(hipEventRecord(ev[nev++], stream));
    for (int i = 0; i < n; ++i) {
        a.step = 1 << i;
        a.src = buf[i & 1];
        a.dst = buf[(i + 1) & 1];
        a.vsrc = var[i & 1];
        a.vdst = var[(i + 1) & 1];
        const bool last = i == n - 1;
        if (i < 4 || (i == 4 && lds16)) {
            VD_HIP(i == 0 ? vd_launch_lds<1>(a, last, stream) : i == 1 ? vd_launch_lds<2>(a, last, stream) :
                   i == 2 ? vd_launch_lds<4>(a, last, stream) : i == 3 ? vd_launch_lds<8>(a, last, stream) :
                            vd_launch_lds<16>(a, last, stream));
        } else {
            const int nseg8 = ((a.w + VD_ROW - 1) / VD_ROW + 7) >> 3;
            const dim3 grid((unsigned)((size_t)nseg8 * 8 * a.h)), block(VD_ROW);
            VD_HIP(last ? vd_launch(vd_iter_direct<true>, grid, block, a, stream) : vd_launch(vd_iter_direct<false>, grid, block, a, stream));
        }
        if (ev) VD_HIP(hipEventRecord(ev[nev++], stream));
    }
    return RT_OK;
}
