// rt_upsample.hip -- guided upsampling (rt_scene_upsample): a colour rendered at w x h is brought to
// W x H. A selected hi pixel takes the mean of the four lo pixels around its centre, each weighted by its bilinear
// factor times the denoiser's normal and depth factors (rt_denoise.hip) with the hi pixel as the centre,
// and counted only if it shows the same object; every other pixel takes `base`, or the plain bilinear mean.
//
// Variant 0 (the product): up_plain, one thread per hi pixel, workgroups of 256 consecutive pixels of one row, the taps
//   visited one after the other from the caller's arrays, a tap's guides read only once its id agreed. A pixel that is
//   not selected reads its id and its base pixel and nothing else: every access of a wave is one contiguous run.
// Variant 1 (the other implementation, kept for the cross-check and the measurement): for W = 2 w and H = 2 h, up_quad.
//   A lane owns a lo pixel (X, Y) and the 2 x 2 hi pixels it covers, whose sixteen taps are the 3 x 3 lo pixels around
//   (X, Y); a wave is 64 consecutive lo pixels of one row. Each lane loads the records of its own column only (rows
//   Y - 1, Y, Y + 1); columns X - 1 and X + 1 are what the neighbouring lanes loaded and come over by ds_bpermute
//   (__shfl); the wave's first and last lane load theirs. The rows are walked top to bottom, which visits every
//   pixel's taps in tap order. With `base`, a wave none of whose 256 hi pixels is selected copies base, packs and
//   leaves without touching the lo arrays. It was written as the product and lost: 0.133 ms against up_plain's 0.097
//   at 3840 x 2160 with 13 % of the pixels selected -- a lane's two pixels of a row make every load and
//   store of the copy path a 32-byte stride, and the nine records cost 120 registers. Other ratios: up_plain.
//
// Both evaluate up_centre / up_tap / up_finish below on the same values in the same order: the same bits.
// Only + - * / and compares; the library is built with -ffp-contract=off and correctly rounded division.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_filter.h"
#include "rt_internal.h"

namespace {

constexpr int UP_ROW = 256;            // hi pixels of one row per workgroup of up_plain
constexpr int UP_TW = 64, UP_TH = 4;   // lo tile of up_quad: one wave per lo row

struct UpArgs {                        // by value
    int W, H, w, h;
    float sx, sy;                      // (float)w / (float)W, (float)h / (float)H
    const float4 *rgba_lo, *normal_lo, *albedo_lo;
    const float *depth_lo;
    const int2 *id_lo;
    const float4 *normal, *albedo, *base;
    const float *depth;
    const int2 *id;
    float4 *rgba_out;
    uint32_t *pixels;
    uint8_t *source;
    const uint8_t *ssel, *psel, *csel; // null with a count of 0
    int nss, nps, ncs;
    int use_tables, shift, demod;
    float sigma;
};

struct UpCentre {
    int kind, index;
    float nx, ny, nz, z, zden2;
};
struct UpRec {                         // a lo pixel: a stays unset without demodulation
    int2 id;
    float z;
    float nx, ny, nz;
    float r, g, b;
    float ar, ag, ab;
};
struct UpSum {
    float r, g, b, w;                  // the guided mean
    float fr, fg, fb, fw;              // the plain bilinear mean (only without base)
};

__device__ __forceinline__ bool up_selected(const UpArgs &a, int2 id)
{
    if (id.x < 0) return false;
    if (!a.use_tables) return true;
    if (id.x == RT_HIT_SPHERE) return (unsigned)id.y < (unsigned)a.nss && a.ssel[id.y] != 0;
    if (id.x == RT_HIT_PLANE) return (unsigned)id.y < (unsigned)a.nps && a.psel[id.y] != 0;
    if (id.x == RT_HIT_CUBE) return (unsigned)id.y < (unsigned)a.ncs && a.csel[id.y] != 0;
    return false;
}
// where a hi coordinate lands in the lo buffer: the tap pair's first coordinate and the bilinear fraction
__device__ __forceinline__ void up_pos(int x, float s, int &x0, float &ax)
{
    const float f = ((float)x + 0.5f) * s - 0.5f;
    int i = (int)f;
    if ((float)i > f) i -= 1;
    x0 = i;
    ax = f - (float)i;
}
__device__ __forceinline__ float up_weight(int k, float ax, float ay)
{
    const float wx = (k & 1) ? ax : 1.f - ax, wy = (k & 2) ? ay : 1.f - ay;
    return wx * wy;
}
__device__ __forceinline__ UpCentre up_centre(const UpArgs &a, size_t p, int2 id)
{
    UpCentre c;
    c.kind = id.x; c.index = id.y;
    const float4 n = a.normal[p];
    c.nx = n.x; c.ny = n.y; c.nz = n.z;
    c.z = a.depth[p];
    const float zden = a.sigma * im_max(fabsf(c.z), IM_TINY);
    c.zden2 = zden * zden;
    return c;
}
__device__ __forceinline__ bool up_same_object(const UpCentre &c, int2 id)
{
    return id.x == c.kind && (c.kind == RT_HIT_TRIANGLE || id.y == c.index);
}
// One tap inside the lo buffer with bilinear factor bq. weigh: the pixel is selected; plain: there is no base.
__device__ __forceinline__ void up_tap(const UpArgs &a, const UpCentre &c, bool weigh, bool plain, float bq, const UpRec &q,
                                       UpSum &s)
{
    if (plain && bq > 0.f) {
        s.fr = s.fr + bq * q.r;
        s.fg = s.fg + bq * q.g;
        s.fb = s.fb + bq * q.b;
        s.fw = s.fw + bq;
    }
    if (!weigh || !up_same_object(c, q.id)) return;
    float m = im_max((c.nx * q.nx + c.ny * q.ny) + c.nz * q.nz, 0.f);
    if (a.shift == 5) {                                 // the default, without the loop's scalar bookkeeping
        m = m * m; m = m * m; m = m * m; m = m * m; m = m * m;
    } else {
        for (int k = 0; k < a.shift; ++k) m = m * m;
    }
    const float dz = q.z - c.z;
    const float wq = (bq * m) * (c.zden2 / (c.zden2 + dz * dz));
    if (!(wq > 0.f) || !(wq < __builtin_inff())) return;
    float r = q.r, g = q.g, b = q.b;
    if (a.demod) {
        r = r / im_max(q.ar, IM_TINY);
        g = g / im_max(q.ag, IM_TINY);
        b = b / im_max(q.ab, IM_TINY);
    }
    s.r = s.r + wq * r;
    s.g = s.g + wq * g;
    s.b = s.b + wq * b;
    s.w = s.w + wq;
}
__device__ __forceinline__ void up_write(const UpArgs &a, size_t p, float r, float g, float b, int src)
{
    a.rgba_out[p] = make_float4(r, g, b, 1.f);
    if (a.pixels) a.pixels[p] = im_pack_colour(r, g, b);
    if (a.source) a.source[p] = (uint8_t)src;
}
// a pixel that is not upsampled, with base: src 0, or 2 for a selected pixel without a counting tap
__device__ __forceinline__ void up_write_base(const UpArgs &a, size_t p, int src)
{
    const float4 v = a.base[p];
    if (a.rgba_out != a.base) a.rgba_out[p] = v;
    if (a.pixels) a.pixels[p] = im_pack_colour(v.x, v.y, v.z);
    if (a.source) a.source[p] = (uint8_t)src;
}
__device__ __forceinline__ void up_finish(const UpArgs &a, size_t p, bool selected, const UpSum &s)
{
    if (selected && s.w > 0.f) {
        float r = s.r / s.w, g = s.g / s.w, b = s.b / s.w;
        if (a.demod) {
            const float4 al = a.albedo[p];
            r = r * al.x; g = g * al.y; b = b * al.z;
        }
        up_write(a, p, r, g, b, 1);
    } else if (a.base) {
        up_write_base(a, p, selected ? 2 : 0);
    } else {
        up_write(a, p, s.fr / s.fw, s.fg / s.fw, s.fb / s.fw, selected ? 2 : 0);
    }
}

__device__ __forceinline__ void up_load_colour(const UpArgs &a, size_t q, UpRec &r)
{
    const float4 c = a.rgba_lo[q];
    r.r = c.x; r.g = c.y; r.b = c.z;
}
__device__ __forceinline__ void up_load_guides(const UpArgs &a, size_t q, UpRec &r)
{
    r.z = a.depth_lo[q];
    const float4 n = a.normal_lo[q];
    r.nx = n.x; r.ny = n.y; r.nz = n.z;
    if (a.demod) {
        const float4 al = a.albedo_lo[q];
        r.ar = al.x; r.ag = al.y; r.ab = al.z;
    }
}

__global__ __launch_bounds__(UP_ROW) void up_plain(const UpArgs a)
{
    const int x = (int)blockIdx.x * UP_ROW + (int)threadIdx.x, y = (int)blockIdx.y;
    if (x >= a.W) return;
    const size_t p = (size_t)y * a.W + x;
    const int2 id = a.id[p];
    const bool selected = up_selected(a, id), plain = a.base == nullptr;
    if (!selected && !plain) {
        up_write_base(a, p, 0);
        return;
    }
    UpCentre c = {};
    if (selected) c = up_centre(a, p, id);
    int x0, y0;
    float ax, ay;
    up_pos(x, a.sx, x0, ax);
    up_pos(y, a.sy, y0, ay);
    UpSum s = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < 4; ++k) {
        const int tx = x0 + (k & 1), ty = y0 + (k >> 1);
        if (tx < 0 || tx >= a.w || ty < 0 || ty >= a.h) continue;
        const size_t q = (size_t)ty * a.w + tx;
        UpRec r = {};
        r.id = a.id_lo[q];
        const bool same = selected && up_same_object(c, r.id);
        if (!same && !plain) continue;
        up_load_colour(a, q, r);
        if (same) up_load_guides(a, q, r);
        up_tap(a, c, selected, plain, up_weight(k, ax, ay), r, s);
    }
    up_finish(a, p, selected, s);
}

__device__ __forceinline__ UpRec up_load(const UpArgs &a, size_t q)
{
    UpRec r = {};
    r.id = a.id_lo[q];
    up_load_colour(a, q, r);
    up_load_guides(a, q, r);
    return r;
}
// the record the lane `delta` to the right holds (delta = -1: to the left); the wave's end lanes get their own back
template <bool DEMOD>
__device__ __forceinline__ UpRec up_from_lane(const UpRec &r, int delta)
{
    const int self = (int)(threadIdx.x & 63), to = self + delta, src = to < 0 || to > 63 ? self : to;
    UpRec o;
    o.id.x = __shfl(r.id.x, src); o.id.y = __shfl(r.id.y, src);
    o.z = __shfl(r.z, src);
    o.nx = __shfl(r.nx, src); o.ny = __shfl(r.ny, src); o.nz = __shfl(r.nz, src);
    o.r = __shfl(r.r, src); o.g = __shfl(r.g, src); o.b = __shfl(r.b, src);
    o.ar = DEMOD ? __shfl(r.ar, src) : 0.f;
    o.ag = DEMOD ? __shfl(r.ag, src) : 0.f;
    o.ab = DEMOD ? __shfl(r.ab, src) : 0.f;
    return o;
}

// Variant 1 at the exact 2 x ratio (W = 2 w, H = 2 h). No lane leaves before the exchanges but with its whole
// wave. The pixel (2 X + i, 2 Y + j) has x0 = X - 1 + i, y0 = Y - 1 + j (up_pos is exact here: (x + 0.5) / 2 - 0.5 has
// at most 17 significant bits), so its tap k is column i + (k & 1), row j + (k >> 1) of the 3 x 3 records.
template <bool DEMOD>
__global__ __launch_bounds__(UP_TW * UP_TH) void up_quad(const UpArgs a)
{
    const int lane = (int)threadIdx.x & (UP_TW - 1);
    const int X = (int)blockIdx.x * UP_TW + lane, Y = (int)blockIdx.y * UP_TH + (int)threadIdx.x / UP_TW;
    if (Y >= a.h) return;                                   // the whole wave
    const bool inside = X < a.w, plain = a.base == nullptr;
    size_t p[2][2];
    int2 id[2][2];
    bool sel[2][2];
    bool any = false;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            p[j][i] = inside ? (size_t)(2 * Y + j) * a.W + (size_t)(2 * X + i) : 0;
            id[j][i] = inside ? a.id[p[j][i]] : make_int2(-1, 0);
            sel[j][i] = up_selected(a, id[j][i]);
            any = any || sel[j][i];
        }
    if (!plain && __ballot(any) == 0) {                     // nothing to upsample in this wave
        if (inside) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int i = 0; i < 2; ++i) up_write_base(a, p[j][i], 0);
        }
        return;
    }
    UpCentre c[2][2] = {};
    int x0[2], y0;
    float ax[2], ay[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        up_pos(2 * X + i, a.sx, x0[i], ax[i]);
        up_pos(2 * Y + i, a.sy, y0, ay[i]);            // y0 = Y - 1 + i: the rows walked below
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i)
            if (sel[j][i]) c[j][i] = up_centre(a, p[j][i], id[j][i]);
    UpSum s[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) s[j][i] = UpSum{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // coordinates clamped to the buffer: a record that stands in for one outside is never a tap
    const int cx = X < a.w ? X : a.w - 1, cxl = cx > 0 ? cx - 1 : 0, cxr = cx + 1 < a.w ? cx + 1 : a.w - 1;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int ty = Y - 1 + r, cy = ty < 0 ? 0 : (ty >= a.h ? a.h - 1 : ty);
        const size_t row = (size_t)cy * a.w;
        UpRec rec[3];
        rec[1] = up_load(a, row + cx);
        rec[0] = up_from_lane<DEMOD>(rec[1], -1);
        rec[2] = up_from_lane<DEMOD>(rec[1], 1);
        if (lane == 0) rec[0] = up_load(a, row + cxl);
        if (lane == UP_TW - 1) rec[2] = up_load(a, row + cxr);
        if (!inside || ty < 0 || ty >= a.h) continue;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int kr = r - j;                           // the tap row of the pixels in quad row j
            if (kr < 0 || kr > 1) continue;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if (!sel[j][i] && !plain) continue;
#pragma unroll
                for (int kc = 0; kc < 2; ++kc) {
                    const int tx = x0[i] + kc;
                    if (tx < 0 || tx >= a.w) continue;
                    up_tap(a, c[j][i], sel[j][i], plain, up_weight(kr * 2 + kc, ax[i], ay[j]), rec[i + kc], s[j][i]);
                }
            }
        }
    }
    if (!inside) return;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) up_finish(a, p[j][i], sel[j][i], s[j][i]);
}

}   // namespace

#define UP_HIP(expr)                                                         \
    do {                                                                     \
        hipError_t up_e_ = (expr);                                           \
        if (up_e_ != hipSuccess) return rt_hip_fail(up_e_, #expr, __FILE__, __LINE__); \
    } while (0)

int rt_upsample_launch(const rt_upsample_desc *d, hipEvent_t *ev, hipStream_t stream)
{
    UpArgs a = {};
    a.W = d->width; a.H = d->height; a.w = d->lo_width; a.h = d->lo_height;
    a.sx = (float)a.w / (float)a.W;
    a.sy = (float)a.h / (float)a.H;
    a.rgba_lo = (const float4 *)d->rgba_lo;
    a.normal_lo = (const float4 *)d->normal_lo;
    a.albedo_lo = (const float4 *)d->albedo_lo;
    a.depth_lo = d->depth_lo;
    a.id_lo = (const int2 *)d->id_lo;
    a.normal = (const float4 *)d->normal;
    a.albedo = (const float4 *)d->albedo;
    a.base = (const float4 *)d->base;
    a.depth = d->depth;
    a.id = (const int2 *)d->id;
    a.rgba_out = (float4 *)d->rgba_out;
    a.pixels = d->pixels;
    a.source = d->source;
    a.use_tables = d->use_tables != 0;
    a.nss = a.use_tables && d->sphere_select ? d->n_sphere_select : 0;
    a.nps = a.use_tables && d->plane_select ? d->n_plane_select : 0;
    a.ncs = a.use_tables && d->cube_select ? d->n_cube_select : 0;
    a.ssel = a.nss ? d->sphere_select : nullptr;
    a.psel = a.nps ? d->plane_select : nullptr;
    a.csel = a.ncs ? d->cube_select : nullptr;
    a.shift = d->normal_shift;
    a.demod = d->demodulate != 0;
    a.sigma = d->sigma_depth;
    if (ev) UP_HIP(hipEventRecord(ev[0], stream));
    // up_quad serves the exact 2 x ratio only
    if (d->variant == 0 || a.W != 2 * a.w || a.H != 2 * a.h) {
        hipLaunchKernelGGL(up_plain, dim3((a.W + UP_ROW - 1) / UP_ROW, a.H), dim3(UP_ROW), 0, stream, a);
    } else {
        const dim3 grid((a.w + UP_TW - 1) / UP_TW, (a.h + UP_TH - 1) / UP_TH), block(UP_TW * UP_TH);
        if (a.demod) hipLaunchKernelGGL(up_quad<true>, grid, block, 0, stream, a);
        else hipLaunchKernelGGL(up_quad<false>, grid, block, 0, stream, a);
    }
    UP_HIP(hipGetLastError());
    if (ev) UP_HIP(hipEventRecord(ev[1], stream));
    return RT_OK;
}
