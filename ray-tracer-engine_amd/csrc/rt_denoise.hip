// rt_denoise.hip -- the G-buffer-guided denoiser (rt_scene_denoise): an edge-avoiding a-trous wavelet
// filter over a frame's rgba, steered by the frame's guides (aov_depth / aov_normal / aov_id / aov_albedo).
//
// Variant 0 (the product):
//   dn_pack          one thread per pixel: demodulates into the first irradiance buffer and packs what an iteration
//                    reads of the guides into one float4 (N.xyz, z) and one int (index) per pixel; the pixel's kind
//                    rides in the irradiance's fourth channel, which the filter does not use. 36 bytes per tap instead
//                    of 44 from four arrays, no division by the albedo after this pass.
//   dn_iter_lds<S>   steps 1 ... 16: a tile of 64 consecutive pixels x 8 rows that are S apart (one wave per row) and
//                    its halo -- two rows of the same residue class above and below, 2 S columns left and right --
//                    are staged in LDS once (29 ... 55 KB), the 25 taps are ds_read_b128 / b32.
//   dn_iter_direct   step 32 (its halo of 128 columns would take 83 KB of LDS) and variant 2: one wave = 64
//                    consecutive pixels of one row, every tap one contiguous 1 KiB load per array through L1; the rows
//                    are walked residue class by residue class (y, y + s, y + 2 s, ...), so that the five rows a
//                    workgroup reads are those its neighbours in launch order read, and a column segment stays on one
//                    XCD (its L2 is not shared with the others).
//   The last iteration multiplies the albedo back, writes rgba_out and packs `pixels` itself.
// Variant 1 (the yardstick): dn_plain, one thread per pixel, every tap from the caller's four guide arrays, the
//   demodulation of iteration 0 per tap, no packing, no LDS.
// Variant 2: variant 0 with dn_iter_direct at every step (what LDS staging buys is variant 2 minus variant 0).
//
// All three evaluate dn_centre / dn_tap / dn_tap_centre below on the same values in the same order: the same bits.
// Only + - * / and compares; the library is built with -ffp-contract=off and correctly rounded division.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_internal.h"

namespace {

constexpr int DN_ROW = 256;            // pixels of one row per workgroup of dn_iter_direct / dn_plain / dn_pack
constexpr int DN_TW = 64, DN_TH = 8;   // tile of dn_iter_lds: one wave per row

struct DnArgs {                        // by value
    int w, h, step, shift, demod, use_colour;
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
};

struct DnCentre {
    float nx, ny, nz, z, zden2, y;
    int kind, index;
};
struct DnSum {
    float r, g, b, w;
};

__device__ __forceinline__ float dn_max(float a, float b) { return a > b ? a : b; }   // a NaN `a` gives b
__device__ __forceinline__ float dn_luma(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
__device__ __forceinline__ float dn_demod(float c, float a) { return c / dn_max(a, 0.0009765625f); }
// float -> int as the frame kernel's f2i (v_cvt_i32_f32: truncation, NaN -> 0, saturating) and rgbToInt (kernel.cu:547-556)
__device__ __forceinline__ uint32_t dn_pack_colour(float r, float g, float b)
{
    int ir = (int)(r * 254.f), ig = (int)(g * 254.f), ib = (int)(b * 254.f);
    if (ir > 255) ir = 255;
    if (ig > 255) ig = 255;
    if (ib > 255) ib = 255;
    return (uint32_t)(((ir & 0xff) << 16) + ((ig & 0xff) << 8) + (ib & 0xff));
}
// a triangle's index does not take part in e_id: every triangle carries index 0
__device__ __forceinline__ int dn_index(int kind, int index) { return kind == RT_HIT_TRIANGLE ? 0 : index; }

__device__ __forceinline__ DnCentre dn_centre(const DnArgs &a, int kind, int index, float nx, float ny, float nz, float z,
                                              float r, float g, float b)
{
    DnCentre c;
    c.kind = kind; c.index = index;
    c.nx = nx; c.ny = ny; c.nz = nz; c.z = z;
    const float zden = a.sigma_depth * dn_max(fabsf(z), 0.0009765625f);
    c.zden2 = zden * zden;
    c.y = a.use_colour ? dn_luma(r, g, b) : 0.f;
    return c;
}

// One tap that is inside the buffer and is not the centre. hh = h[dx] * h[dy] (exact).
__device__ __forceinline__ void dn_tap(const DnArgs &a, const DnCentre &c, float hh, int kind, int index, float nx, float ny,
                                       float nz, float z, float r, float g, float b, DnSum &s)
{
    if (kind != c.kind || index != c.index) return;     // e_id = 0 (also: the tap is not valid, since c.kind >= 0)
    const float dot = (c.nx * nx + c.ny * ny) + c.nz * nz;
    float m = dot > 0.f ? dot : 0.f;
    if (a.shift == 5) {                                 // the default, without the loop's scalar bookkeeping
        m = m * m; m = m * m; m = m * m; m = m * m; m = m * m;
    } else {
        for (int k = 0; k < a.shift; ++k) m = m * m;
    }
    float w = hh * m;
    // e_z = 1 / (1 + (dz / zden)^2) as zden^2 / (zden^2 + dz^2), e_c likewise: one division per factor, not two
    const float dz = z - c.z;
    w = w * (c.zden2 / (c.zden2 + dz * dz));
    if (a.use_colour) {
        const float dl = dn_luma(r, g, b) - c.y;
        w = w * (a.sigma_colour2 / (a.sigma_colour2 + dl * dl));
    }
    if (!(w > 0.f) || !(w < __builtin_inff())) return;
    s.r = s.r + w * r;
    s.g = s.g + w * g;
    s.b = s.b + w * b;
    s.w = s.w + w;
}
__device__ __forceinline__ void dn_tap_centre(float r, float g, float b, DnSum &s)
{
    const float w = 0.140625f;   // h[0] * h[0] = (6 / 16)^2, without the four factors
    s.r = s.r + w * r;
    s.g = s.g + w * g;
    s.b = s.b + w * b;
    s.w = s.w + w;
}
__device__ __forceinline__ float dn_h(int d) { return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f); }

// The last iteration's outputs for a valid pixel.
__device__ __forceinline__ void dn_write_result(const DnArgs &a, size_t p, float r, float g, float b)
{
    if (a.demod) {
        const float4 al = a.albedo[p];
        r = r * al.x; g = g * al.y; b = b * al.z;
    }
    a.rgba_out[p] = make_float4(r, g, b, 1.f);
    if (a.pixels) a.pixels[p] = dn_pack_colour(r, g, b);
}
// ... and for a pixel that is not valid: its input bits.
__device__ __forceinline__ void dn_write_sky(const DnArgs &a, size_t p)
{
    const float4 c = a.rgba_in[p];
    a.rgba_out[p] = c;
    if (a.pixels) a.pixels[p] = dn_pack_colour(c.x, c.y, c.z);
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

template <bool LAST>
__global__ __launch_bounds__(DN_ROW) void dn_iter_direct(const DnArgs a)
{
    int x, y;
    if (!dn_direct_where(a, x, y)) return;
    const size_t p = (size_t)y * a.w + x;
    const float4 cp = a.src[p];
    const int kind = __float_as_int(cp.w);
    if (kind < 0) {                                // sky; a wave of 64 sky pixels ends here
        if (LAST) dn_write_sky(a, p);
        else a.dst[p] = cp;
        return;
    }
    const float4 gp = a.guide[p];
    const DnCentre c = dn_centre(a, kind, a.key[p], gp.x, gp.y, gp.z, gp.w, cp.x, cp.y, cp.z);
    DnSum s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * a.step;
        if (qy < 0 || qy >= a.h) continue;         // wave-uniform
        // the row's five taps are loaded together (from a clamped column where a tap is outside), then weighted
        float4 cq[5], gq[5];
        int kq[5];
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            if (dx == 0 && dy == 0) continue;
            const int qx = x + dx * a.step;
            const size_t q = (size_t)qy * a.w + (qx < 0 ? 0 : (qx >= a.w ? a.w - 1 : qx));
            cq[dx + 2] = a.src[q];
            gq[dx + 2] = a.guide[q];
            kq[dx + 2] = a.key[q];
        }
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            if (dx == 0 && dy == 0) {
                dn_tap_centre(cp.x, cp.y, cp.z, s);
                continue;
            }
            const int qx = x + dx * a.step;
            if (qx < 0 || qx >= a.w) continue;
            const float4 c4 = cq[dx + 2], g4 = gq[dx + 2];
            dn_tap(a, c, dn_h(dx) * dn_h(dy), __float_as_int(c4.w), kq[dx + 2], g4.x, g4.y, g4.z, g4.w, c4.x, c4.y, c4.z, s);
        }
    }
    const float r = s.r / s.w, g = s.g / s.w, b = s.b / s.w;
    if (LAST) dn_write_result(a, p, r, g, b);
    else a.dst[p] = make_float4(r, g, b, cp.w);
}

// Steps 1 ... 16: the tile and its halo from LDS. The tile is 64 consecutive pixels of 8 rows that are `S` apart (one
// residue class of the step), so the rows its taps need are 12 rows of the same class -- a halo of two rows above and
// below at any step -- and 2 S more columns on either side. A record outside the buffer is staged as "not valid"
// (kind -1), which no valid centre matches: the tap loop needs no bounds.
template <int S, bool LAST>
__global__ __launch_bounds__(DN_TW * DN_TH) void dn_iter_lds(const DnArgs a)
{
    constexpr int HALO = 2 * S, LW = DN_TW + 2 * HALO, LH = DN_TH + 4;
    __shared__ float4 l_col[LW * LH];
    __shared__ float4 l_gd[LW * LH];
    __shared__ int l_key[LW * LH];
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
        if (gx >= 0 && gx < a.w && gy >= 0 && gy < a.h) {
            const size_t q = (size_t)gy * a.w + gx;
            cq = a.src[q];
            if (__float_as_int(cq.w) >= 0) {
                gq = a.guide[q];
                kq = a.key[q];
            }
        }
        l_col[i] = cq;
        l_gd[i] = gq;
        l_key[i] = kq;
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
        if (LAST) dn_write_sky(a, p);
        else a.dst[p] = cp;
        return;
    }
    const float4 gp = l_gd[lp];
    const DnCentre c = dn_centre(a, kind, l_key[lp], gp.x, gp.y, gp.z, gp.w, cp.x, cp.y, cp.z);
    DnSum s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            if (dx == 0 && dy == 0) {
                dn_tap_centre(cp.x, cp.y, cp.z, s);
                continue;
            }
            const int lq = lp + dy * LW + dx * S;
            const float4 cq = l_col[lq];
            const int kq = __float_as_int(cq.w);
            if (kq != c.kind) continue;            // skips what is outside the buffer and what is not valid
            const float4 gq = l_gd[lq];
            dn_tap(a, c, dn_h(dx) * dn_h(dy), kq, l_key[lq], gq.x, gq.y, gq.z, gq.w, cq.x, cq.y, cq.z, s);
        }
    }
    const float r = s.r / s.w, g = s.g / s.w, b = s.b / s.w;
    if (LAST) dn_write_result(a, p, r, g, b);
    else a.dst[p] = make_float4(r, g, b, cp.w);
}

template <int S>
hipError_t dn_launch_lds(const DnArgs &a, bool last, hipStream_t stream)
{
    const int gpc = ((a.h + S - 1) / S + DN_TH - 1) / DN_TH;
    const dim3 grid((a.w + DN_TW - 1) / DN_TW, gpc * S), block(DN_TW * DN_TH);
    if (last) hipLaunchKernelGGL((dn_iter_lds<S, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((dn_iter_lds<S, false>), grid, block, 0, stream, a);
    return hipGetLastError();
}

__global__ __launch_bounds__(DN_ROW) void dn_pack(const DnArgs a)
{
    const size_t p = (size_t)blockIdx.x * DN_ROW + threadIdx.x;
    if (p >= (size_t)a.w * a.h) return;
    const int2 id = a.id[p];
    float4 c = a.rgba_in[p];
    if (id.x < 0) {                                // sky: no iteration reads its guides
        c.w = __int_as_float(-1);
        a.dst[p] = c;
        return;
    }
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

// The yardstick: every tap from the caller's arrays. FIRST: the irradiance is the caller's rgba, demodulated per tap.
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(DN_ROW) void dn_plain(const DnArgs a)
{
    const int x = (int)blockIdx.x * DN_ROW + (int)threadIdx.x, y = (int)blockIdx.y;
    if (x >= a.w) return;
    const size_t p = (size_t)y * a.w + x;
    const int2 id = a.id[p];
    if (id.x < 0) {
        if (LAST) dn_write_sky(a, p);
        return;
    }
    auto irradiance = [&](size_t q) {
        float4 cq = a.src[q];
        if (FIRST && a.demod) {
            const float4 al = a.albedo[q];
            cq.x = dn_demod(cq.x, al.x); cq.y = dn_demod(cq.y, al.y); cq.z = dn_demod(cq.z, al.z);
        }
        return cq;
    };
    const float4 cp = irradiance(p);
    const float4 np = a.normal[p];
    const DnCentre c = dn_centre(a, id.x, dn_index(id.x, id.y), np.x, np.y, np.z, a.depth[p], cp.x, cp.y, cp.z);
    DnSum s = {0.f, 0.f, 0.f, 0.f};
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * a.step;
        if (qy < 0 || qy >= a.h) continue;
        for (int dx = -2; dx <= 2; ++dx) {
            if (dx == 0 && dy == 0) {
                dn_tap_centre(cp.x, cp.y, cp.z, s);
                continue;
            }
            const int qx = x + dx * a.step;
            if (qx < 0 || qx >= a.w) continue;
            const size_t q = (size_t)qy * a.w + qx;
            const int2 iq = a.id[q];
            if (iq.x < 0) continue;
            const float4 cq = irradiance(q);
            const float4 nq = a.normal[q];
            dn_tap(a, c, dn_h(dx) * dn_h(dy), iq.x, dn_index(iq.x, iq.y), nq.x, nq.y, nq.z, a.depth[q], cq.x, cq.y, cq.z, s);
        }
    }
    const float r = s.r / s.w, g = s.g / s.w, b = s.b / s.w;
    if (LAST) dn_write_result(a, p, r, g, b);
    else a.dst[p] = make_float4(r, g, b, 1.f);
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

}   // namespace

#define DN_HIP(expr)                                                         \
    do {                                                                     \
        hipError_t dn_e_ = (expr);                                           \
        if (dn_e_ != hipSuccess) return rt_hip_fail(dn_e_, #expr, __FILE__, __LINE__); \
    } while (0)

// d: validated, in this build's layout. col0 / col1 / guide / key: the scene's scratch, room for width * height
// pixels (guide and key may be null for variant 1). ev: null, or iterations + 2 timing events, recorded around every
// launch.
int rt_denoise_launch(const rt_denoise_desc *d, float4 *col0, float4 *col1, float4 *guide, int *key, hipEvent_t *ev,
                      hipStream_t stream)
{
    DnArgs a = {};
    a.w = d->width; a.h = d->height;
    a.shift = d->normal_shift;
    a.demod = d->demodulate != 0;
    a.use_colour = d->sigma_colour > 0.f;
    a.sigma_depth = d->sigma_depth; a.sigma_colour2 = d->sigma_colour * d->sigma_colour;
    a.rgba_in = (const float4 *)d->rgba_in;
    a.depth = d->depth;
    a.normal = (const float4 *)d->normal;
    a.albedo = (const float4 *)d->albedo;
    a.id = (const int2 *)d->id;
    a.rgba_out = (float4 *)d->rgba_out;
    a.pixels = d->pixels;
    a.guide = guide; a.key = key;
    a.guide_w = guide; a.key_w = key;
    const size_t npx = (size_t)a.w * a.h;
    const int n = d->iterations;
    float4 *buf[2] = {col0, col1};
    int nev = 0;
    if (ev) DN_HIP(hipEventRecord(ev[nev++], stream));

    if (d->variant == 1) {
        const float4 *first = a.rgba_in;
        if (n == 1 && d->rgba_out == d->rgba_in) {   // one launch reads the neighbours it would overwrite: from a copy
            DN_HIP(hipMemcpyAsync(col1, d->rgba_in, npx * sizeof(float4), hipMemcpyDeviceToDevice, stream));
            first = col1;
            a.rgba_in = col1;
        }
        const dim3 grid((a.w + DN_ROW - 1) / DN_ROW, a.h), block(DN_ROW);
        for (int i = 0; i < n; ++i) {
            a.step = 1 << i;
            a.src = i == 0 ? first : buf[(i - 1) & 1];
            a.dst = buf[i & 1];
            const bool last = i == n - 1;
            if (i == 0) DN_HIP(last ? dn_launch(dn_plain<true, true>, grid, block, a, stream) : dn_launch(dn_plain<true, false>, grid, block, a, stream));
            else DN_HIP(last ? dn_launch(dn_plain<false, true>, grid, block, a, stream) : dn_launch(dn_plain<false, false>, grid, block, a, stream));
            if (ev) DN_HIP(hipEventRecord(ev[nev++], stream));
        }
        return RT_OK;
    }

    a.dst = buf[0];
    DN_HIP(dn_launch(dn_pack, dim3((unsigned)((npx + DN_ROW - 1) / DN_ROW)), dim3(DN_ROW), a, stream));
    if (ev) DN_HIP(hipEventRecord(ev[nev++], stream));
    for (int i = 0; i < n; ++i) {
        a.step = 1 << i;
        a.src = buf[i & 1];
        a.dst = buf[(i + 1) & 1];
        const bool last = i == n - 1;
        if (d->variant == 0 && i < 5) {
            DN_HIP(i == 0 ? dn_launch_lds<1>(a, last, stream) : i == 1 ? dn_launch_lds<2>(a, last, stream) :
                   i == 2 ? dn_launch_lds<4>(a, last, stream) : i == 3 ? dn_launch_lds<8>(a, last, stream) :
                            dn_launch_lds<16>(a, last, stream));
        } else {
            const int nseg8 = ((a.w + DN_ROW - 1) / DN_ROW + 7) >> 3;
            const dim3 grid((unsigned)((size_t)nseg8 * 8 * a.h)), block(DN_ROW);
            DN_HIP(last ? dn_launch(dn_iter_direct<true>, grid, block, a, stream) : dn_launch(dn_iter_direct<false>, grid, block, a, stream));
        }
        if (ev) DN_HIP(hipEventRecord(ev[nev++], stream));
    }
    return RT_OK;
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
