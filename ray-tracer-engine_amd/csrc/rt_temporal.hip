// rt_temporal.hip -- temporal accumulation (rt_scene_temporal; rt_scene_temporal_motion): a
// frame's colour is blended into the history of the previous frame, which is found by taking the pixel's world point
// (its primary ray times aov_depth, less the displacement of the sphere or cube it shows) into the previous view and
// gathering the four pixels around where it lands; a tap counts only if the previous frame's guides (id, depth,
// normal) say it shows the same surface. The motion entry can also clamp the history to the colour box of the current
// frame's 3 x 3 neighbourhood.
//
// One set of kernels serves both entries. MOTION compiles in the displacement lookup, the single tap of a static pixel
// under identical views beside reprojected movers, and the clamp; without it none of their code or registers exist.
// rt_scene_temporal launches the instantiations without MOTION, and so does the motion entry with `reset`, or with no
// table and no clamp; every other call of the motion entry launches those with MOTION.
//
// Variant 1 (the yardstick): tp_plain, one thread per pixel, workgroups of 256 consecutive pixels of one row in grid
//   order, the taps visited one after the other, each tap's arrays read only once the tap's id agreed; the nine colours
//   of the box read straight from rgba_in.
// Variant 0 (the product): tp_product. A wave is 64 consecutive pixels of one row, so every array of a tap is one
//   contiguous run of about 1 KiB under small camera motion (the taps are a shifted copy of the tile). Each lane loads
//   the records of its left column only (x0, rows y0 and y0 + 1), all of them before any is tested; the right column
//   (x0 + 1) is what the next lane loaded for its own x0, and comes over by ds_bpermute (__shfl_down) -- 10 wave-wide
//   loads instead of 20 per pixel. A lane whose neighbour loaded another pixel (the wave's last lane, a depth edge,
//   the frame's border) loads its right column itself. A workgroup is four such rows, in row-major order with the
//   grid's width padded to a multiple of eight tiles: the tiles below one another then run on one XCD (tile b runs on
//   XCD b % 8; the eight L2s are not shared) and the frame is still streamed row band by row band. With MOTION and the
//   clamp the tile's rgba_in is staged with a one-pixel halo in LDS (66 x 6 float4: a wave reads 64 consecutive 16-byte
//   slots of one row, which ds_read_b128 serves without a bank conflict). Without MOTION, `reset` or identical views
//   leave one tap or none and nothing to exchange: variant 0 launches tp_plain. With MOTION and identical views it
//   launches tp_product, since movers are reprojected.
//   What was measured and not kept: 64 x 8 tiles walked column segment by column segment per XCD
//   (slower than the yardstick: the frame is no longer streamed), other tile shapes in row-major order (the
//   yardstick's time at 3840 x 2160), a packed record per previous pixel (a pass of its own costs more than it saves).
//
// Both variants evaluate tp_into_prev / tp_tap / tp_finish below on the same values in the same order: the same bits.
// Only + - * / and compares; the library is built with -ffp-contract=off and correctly rounded division.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_cast.h"
#include "rt_filter.h"
#include "rt_internal.h"

namespace {

constexpr int TP_ROW = 256;            // pixels of one row per workgroup of tp_plain
constexpr int TP_TW = 64, TP_TH = 4;   // tile of tp_product: one wave per row
constexpr int TP_LW = TP_TW + 2, TP_LH = TP_TH + 2;        // MOTION: the staged tile with its halo
constexpr int TP_HALO = 2 * TP_LW + 2 * TP_TH;             // its border: two rows, two columns of TP_TH

struct TpArgs {                        // by value
    int w, h, reset, same_view;
    float max_n, tol, cos2;            // (float)max_history, depth_tolerance, normal_cos_min^2 (binary32)
    float ox, oy, oz, cp, sp, cy, sy;  // the current view (rt_view_terms)
    float pox, poy, poz, pcp, psp, pcy, psy, pa;   // the previous view and its aspect
    float eye_nz;
    const float *dx_tab, *dy_tab;      // the current view's ray tables (null where no pixel is reprojected: not read)
    const float4 *rgba_in, *normal;
    const float *depth;
    const int2 *id;
    const float4 *prev_rgba, *prev_normal;
    const float *prev_depth;
    const int2 *prev_id;
    const float2 *prev_moments;
    float4 *rgba_out;
    float2 *moments_out;
    uint32_t *pixels;
    // read with MOTION only
    const float4 *smot, *cmot;         // a displacement per sphere / cube (null with a count of 0)
    int nsm, ncm, clamp;
    float slack, clamp_n;              // clamp_slack, (float)clamp_history
};

struct TpSum {
    float r, g, b, n, m1, m2, w;
};

__device__ __forceinline__ void tp_write(const TpArgs &a, size_t p, float r, float g, float b, float n, float m1, float m2)
{
    a.rgba_out[p] = make_float4(r, g, b, n);
    if (a.moments_out) a.moments_out[p] = make_float2(m1, m2);
    if (a.pixels) a.pixels[p] = im_pack_colour(r, g, b);
}
// a pixel without history: (c, 1), moments (Y, Y Y)
__device__ __forceinline__ void tp_write_new(const TpArgs &a, size_t p, float4 c)
{
    const float y = im_luma(c.x, c.y, c.z);
    tp_write(a, p, c.x, c.y, c.z, 1.f, y, y * y);
}

// The pixel's primary ray as rt_scene_primary_rays forms it (rf_primary_dir) and its world point.
__device__ __forceinline__ V3 tp_world(const TpArgs &a, int x, int y, float t)
{
    RtFrameConsts fc;
    fc.width = a.w; fc.height = a.h; fc.y0 = 0;
    fc.dx_tab = a.dx_tab; fc.dy_tab = a.dy_tab;
    fc.eye_nz = a.eye_nz;
    fc.cos_pitch = a.cp; fc.sin_pitch = a.sp; fc.cos_yaw = a.cy; fc.sin_yaw = a.sy;
    const V3 D = rf_primary_dir(fc, y * a.w + x);
    V3 P;
    P.x = a.ox + D.x * t; P.y = a.oy + D.y * t; P.z = a.oz + D.z * t;
    return P;
}
// Where a world point lands in the previous view: false if it has no history for reasons of geometry. qq: squared
// distance to the previous eye.
__device__ __forceinline__ bool tp_into_prev(const TpArgs &a, float px, float py, float pz, float &fx, float &fy, float &qq)
{
    const float qx = px - a.pox, qy = py - a.poy, qz = pz - a.poz;
    qq = (qx * qx + qy * qy) + qz * qz;
    const float vx = qx * a.pcy - qz * a.psy;
    const float z1 = qx * a.psy + qz * a.pcy;
    const float vy = qy * a.pcp + z1 * a.psp;
    const float vz = z1 * a.pcp - qy * a.psp;
    if (!(vz > 0.f)) return false;
    const float s = (1.f / a.pa) / vz;
    const float dx = vx * s, dy = vy * s;
    const float half = (float)a.w * 0.5f;
    fx = ((dx + 1.f) / a.pa) * half - 0.5f;
    fy = ((dy + 1.f) / a.pa) * half - 0.5f;
    return fx >= -1.f && fx <= (float)a.w && fy >= -1.f && fy <= (float)a.h;
}
// floor of a value in [-1, 32768]: truncation, corrected for negative values
__device__ __forceinline__ int tp_floor(float f)
{
    int i = (int)f;
    if ((float)i > f) i -= 1;
    return i;
}

// The displacement of the object a pixel shows: planes, triangles and indices outside the table do not move.
template <bool MOTION>
__device__ __forceinline__ float4 tp_motion(const TpArgs &a, int2 id)
{
    if constexpr (MOTION) {
        if (id.x == RT_HIT_SPHERE && (unsigned)id.y < (unsigned)a.nsm) return a.smot[id.y];
        if (id.x == RT_HIT_CUBE && (unsigned)id.y < (unsigned)a.ncm) return a.cmot[id.y];
    }
    return make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ bool tp_static(float4 m) { return m.x == 0.f && m.y == 0.f && m.z == 0.f; }

// One tap that is inside the previous buffer: its weight and its record; (kind, index, n, qq): the pixel's own.
__device__ __forceinline__ void tp_tap(const TpArgs &a, int2 id, float4 n, float qq, float wt, int2 pid, float pt, float4 pn,
                                       float4 pc, float2 pm, TpSum &s)
{
    if (pid.x != id.x || pid.y != id.y) return;
    float dd = pt * pt - qq;
    if (dd < 0.f) dd = -dd;
    if (!(dd <= a.tol * qq)) return;
    const float dot = (n.x * pn.x + n.y * pn.y) + n.z * pn.z;
    if (!(dot > 0.f)) return;
    const float nn = (n.x * n.x + n.y * n.y) + n.z * n.z, pp = (pn.x * pn.x + pn.y * pn.y) + pn.z * pn.z;
    if (!(dot * dot >= a.cos2 * (nn * pp))) return;
    s.w = s.w + wt;
    s.r = s.r + wt * pc.x;
    s.g = s.g + wt * pc.y;
    s.b = s.b + wt * pc.z;
    s.n = s.n + wt * pc.w;
    s.m1 = s.m1 + wt * pm.x;
    s.m2 = s.m2 + wt * pm.y;
}

// The key of a float in the total order of the bit patterns, and min / max in that order: independent of the order in
// which the nine values are visited (equal keys are equal bits).
__device__ __forceinline__ uint32_t tp_key(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float tp_min(float a, float b) { return tp_key(a) <= tp_key(b) ? a : b; }
__device__ __forceinline__ float tp_max(float a, float b) { return tp_key(a) >= tp_key(b) ? a : b; }

struct TpBox {
    float lo[3], hi[3];
};
// nb(dx, dy): rgba_in at the pixel's neighbour, coordinates clamped to the buffer
template <class Nb>
__device__ __forceinline__ TpBox tp_box(const Nb &nb)
{
    const float4 c = nb(0, 0);
    TpBox b = {{c.x, c.y, c.z}, {c.x, c.y, c.z}};
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        if (k == 4) continue;
        const float4 v = nb(k % 3 - 1, k / 3 - 1);
        b.lo[0] = tp_min(b.lo[0], v.x); b.hi[0] = tp_max(b.hi[0], v.x);
        b.lo[1] = tp_min(b.lo[1], v.y); b.hi[1] = tp_max(b.hi[1], v.y);
        b.lo[2] = tp_min(b.lo[2], v.z); b.hi[2] = tp_max(b.hi[2], v.z);
    }
    return b;
}
struct TpNbGlobal {
    const float4 *in;
    int w, h, x, y;
    __device__ __forceinline__ float4 operator()(int dx, int dy) const
    {
        int qx = x + dx, qy = y + dy;
        qx = qx < 0 ? 0 : (qx >= w ? w - 1 : qx);
        qy = qy < 0 ? 0 : (qy >= h ? h - 1 : qy);
        return in[(size_t)qy * w + qx];
    }
};
struct TpNbLds {
    const float4 *centre;              // the pixel's own slot in the staged tile
    __device__ __forceinline__ float4 operator()(int dx, int dy) const { return centre[dy * TP_LW + dx]; }
};

// The blend of the colour into the gathered history; MOTION: the history clamped to the box first (nb is read then only).
template <bool MOTION, class Nb>
__device__ __forceinline__ void tp_finish(const TpArgs &a, size_t p, float4 c, const TpSum &s, const Nb &nb)
{
    if (!(s.w > 0.f)) {
        tp_write_new(a, p, c);
        return;
    }
    float h[3] = {s.r / s.w, s.g / s.w, s.b / s.w};
    float nh = s.n / s.w;
    if constexpr (MOTION) {
        if (a.clamp) {
            const TpBox b = tp_box(nb);
            bool clamped = false;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float e = (b.hi[k] - b.lo[k]) * a.slack;
                const float lo = b.lo[k] - e, hi = b.hi[k] + e;
                if (h[k] < lo) {
                    h[k] = lo;
                    clamped = true;
                } else if (h[k] > hi) {
                    h[k] = hi;
                    clamped = true;
                }
            }
            if (clamped && nh > a.clamp_n) nh = a.clamp_n;
        }
    }
    float n = nh + 1.f;
    if (!(n < a.max_n)) n = a.max_n;
    const float al = 1.f / n;
    const float r = h[0] + (c.x - h[0]) * al, g = h[1] + (c.y - h[1]) * al, bl = h[2] + (c.z - h[2]) * al;
    float m1 = 0.f, m2 = 0.f;
    if (a.moments_out) {
        const float h1 = s.m1 / s.w, h2 = s.m2 / s.w;
        const float y = im_luma(c.x, c.y, c.z);
        m1 = h1 + (y - h1) * al;
        m2 = h2 + (y * y - h2) * al;
    }
    tp_write(a, p, r, g, bl, n, m1, m2);
}

// What every pixel does before its taps, its colour read: false if the pixel was written as one without history.
// The instantiations with MOTION are not launched with `reset`.
template <bool MOTION>
__device__ __forceinline__ bool tp_begin(const TpArgs &a, size_t p, float4 c, int2 &id, float &t)
{
    if (!MOTION && a.reset) {
        tp_write_new(a, p, c);
        return false;
    }
    id = a.id[p];
    t = a.depth[p];
    if (id.x < 0 || !(t > 0.f) || !(t < __builtin_inff())) {
        tp_write_new(a, p, c);
        return false;
    }
    return true;
}

// identical views, a static pixel: the only tap is the pixel itself with weight 1, tested against the pixel's own depth
__device__ __forceinline__ TpSum tp_single_tap(const TpArgs &a, size_t p, int2 id, float t)
{
    TpSum s = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float2 pm = (a.moments_out && a.prev_moments) ? a.prev_moments[p] : make_float2(0.f, 0.f);
    tp_tap(a, id, a.normal[p], t * t, 1.f, a.prev_id[p], a.prev_depth[p], a.prev_normal[p], a.prev_rgba[p], pm, s);
    return s;
}

__device__ __forceinline__ float tp_weight(int k, float ax, float ay)
{
    const float wx = (k & 1) ? ax : 1.f - ax, wy = (k & 2) ? ay : 1.f - ay;
    return wx * wy;
}

template <bool MOTION>
__global__ __launch_bounds__(TP_ROW) void tp_plain(const TpArgs a)
{
    const int x = (int)blockIdx.x * TP_ROW + (int)threadIdx.x, y = (int)blockIdx.y;
    if (x >= a.w) return;
    const size_t p = (size_t)y * a.w + x;
    const float4 c = a.rgba_in[p];
    int2 id;
    float t;
    if (!tp_begin<MOTION>(a, p, c, id, t)) return;
    const TpNbGlobal nb = {a.rgba_in, a.w, a.h, x, y};
    const float4 m = tp_motion<MOTION>(a, id);
    if (a.same_view && tp_static(m)) {
        tp_finish<MOTION>(a, p, c, tp_single_tap(a, p, id, t), nb);
        return;
    }
    const V3 P = tp_world(a, x, y, t);
    float fx, fy, qq;
    if (!tp_into_prev(a, P.x - m.x, P.y - m.y, P.z - m.z, fx, fy, qq)) {
        tp_write_new(a, p, c);
        return;
    }
    const int x0 = tp_floor(fx), y0 = tp_floor(fy);
    const float ax = fx - (float)x0, ay = fy - (float)y0;
    const float4 n = a.normal[p];
    const bool moments = a.moments_out && a.prev_moments;
    TpSum s = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < 4; ++k) {
        const int tx = x0 + (k & 1), ty = y0 + (k >> 1);
        if (tx < 0 || tx >= a.w || ty < 0 || ty >= a.h) continue;
        const size_t q = (size_t)ty * a.w + tx;
        const int2 pid = a.prev_id[q];
        if (pid.x != id.x || pid.y != id.y) continue;
        tp_tap(a, id, n, qq, tp_weight(k, ax, ay), pid, a.prev_depth[q], a.prev_normal[q], a.prev_rgba[q],
               moments ? a.prev_moments[q] : make_float2(0.f, 0.f), s);
    }
    tp_finish<MOTION>(a, p, c, s, nb);
}

// One row of a tap pair: the record at column x0 is loaded, the record at column x0 + 1 is the one the next lane loaded
// for its own x0 whenever that is the same pixel (under small camera motion: always, but for the wave's last lane).
struct TpRec {
    int2 id;
    float t;
    float4 n, c;
    float2 m;
};
template <bool MOMENTS>
__device__ __forceinline__ TpRec tp_load(const TpArgs &a, int q)
{
    TpRec r;
    r.id = a.prev_id[q];
    r.t = a.prev_depth[q];
    r.n = a.prev_normal[q];
    r.c = a.prev_rgba[q];
    r.m = MOMENTS ? a.prev_moments[q] : make_float2(0.f, 0.f);
    return r;
}
template <bool MOMENTS>
__device__ __forceinline__ TpRec tp_next_lane(const TpRec &r)
{
    TpRec o;
    o.id.x = __shfl_down(r.id.x, 1); o.id.y = __shfl_down(r.id.y, 1);
    o.t = __shfl_down(r.t, 1);
    o.n.x = __shfl_down(r.n.x, 1); o.n.y = __shfl_down(r.n.y, 1); o.n.z = __shfl_down(r.n.z, 1);
    o.n.w = 0.f;
    o.c.x = __shfl_down(r.c.x, 1); o.c.y = __shfl_down(r.c.y, 1); o.c.z = __shfl_down(r.c.z, 1); o.c.w = __shfl_down(r.c.w, 1);
    o.m.x = MOMENTS ? __shfl_down(r.m.x, 1) : 0.f;
    o.m.y = MOMENTS ? __shfl_down(r.m.y, 1) : 0.f;
    return o;
}

// The product kernel: tiles of 64 x 4 pixels (one wave per row) in row-major order, the grid's width padded to a
// multiple of 8 tiles so that the tiles below one another share an XCD. No lane leaves before the exchange. Without
// MOTION it is launched for moving views only (neither reset nor same_view).
// MOTION: a tile of the padding leaves as a whole; of every other tile each lane stages a colour (its own, or the
// frame's nearest for a lane past the right or bottom edge) and the first TP_HALO lanes one halo slot each, and nobody
// leaves before the barrier and the exchange. The barrier stands right behind the staging: holding it back until every
// lane's tap loads were issued keeps 110 registers alive instead of 75 and took 1.38 x rt_scene_temporal's time at
// 3840 x 2160 against this form's 1.16. The staging is written here and forms the lane's slot from lx and
// ly: as a helper that formed it from threadIdx.x again the pass was 0.005 ms slower there with the clamp on
// (profiles/temporal_merge_ab.json). With identical views static lanes take the single tap and sit the exchange out;
// movers go through the reprojection.
template <bool MOTION, bool MOMENTS>
__global__ __launch_bounds__(TP_TW * TP_TH) void tp_product(const TpArgs a)
{
    __shared__ float4 tile[TP_LH * TP_LW];         // MOTION only
    const int nsegp = (((a.w + TP_TW - 1) / TP_TW + 7) >> 3) << 3;
    const int b = (int)blockIdx.x;
    const int tyi = b / nsegp, seg = b - tyi * nsegp;
    const int lx = (int)threadIdx.x & (TP_TW - 1), ly = (int)threadIdx.x / TP_TW;
    const int x = seg * TP_TW + lx, y = tyi * TP_TH + ly;
    const bool inside = x < a.w && y < a.h;
    size_t p = inside ? (size_t)y * a.w + x : 0;
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (MOTION) {
        if (seg * TP_TW >= a.w) return;            // a tile of the padding: the whole workgroup
        p = (size_t)(y < a.h ? y : a.h - 1) * a.w + (x < a.w ? x : a.w - 1);       // its own if inside
        c = a.rgba_in[p];
        if (a.clamp) {
            tile[(ly + 1) * TP_LW + lx + 1] = c;
            const int i = (int)threadIdx.x;
            if (i < TP_HALO) {
                int hx, hy;
                if (i < 2 * TP_LW) {
                    hx = i < TP_LW ? i : i - TP_LW;
                    hy = i < TP_LW ? 0 : TP_LH - 1;
                } else {
                    const int j = i - 2 * TP_LW;
                    hx = j < TP_TH ? 0 : TP_LW - 1;
                    hy = 1 + (j < TP_TH ? j : j - TP_TH);
                }
                int gx = seg * TP_TW - 1 + hx, gy = tyi * TP_TH - 1 + hy;
                gx = gx < 0 ? 0 : (gx >= a.w ? a.w - 1 : gx);
                gy = gy < 0 ? 0 : (gy >= a.h ? a.h - 1 : gy);
                tile[hy * TP_LW + hx] = a.rgba_in[(size_t)gy * a.w + gx];
            }
            __syncthreads();
        }
    }
    const TpNbLds nb = {&tile[(ly + 1) * TP_LW + lx + 1]};
    int2 id = make_int2(-1, 0);
    float t = 0.f;
    bool live = false;
    float fx = 0.f, fy = 0.f, qq = 0.f;
    if (inside) {
        if constexpr (!MOTION) c = a.rgba_in[p];   // MOTION: read above, by every lane
        if (tp_begin<MOTION>(a, p, c, id, t)) {
            const float4 m = tp_motion<MOTION>(a, id);
            if (MOTION && a.same_view && tp_static(m)) {
                tp_finish<MOTION>(a, p, c, tp_single_tap(a, p, id, t), nb);
            } else {
                const V3 P = tp_world(a, x, y, t);
                live = tp_into_prev(a, P.x - m.x, P.y - m.y, P.z - m.z, fx, fy, qq);
                if (!live) tp_write_new(a, p, c);
            }
        }
    }
    int x0 = 0, y0 = 0;
    int ql[2] = {-1, -1}, qr[2] = {-2, -2};        // the pixels a live lane loads / wants from the next lane
    TpRec L[2] = {}, R[2] = {};
    float4 n = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {
        x0 = tp_floor(fx); y0 = tp_floor(fy);
        n = a.normal[p];
        const int cx0 = x0 < 0 ? 0 : (x0 >= a.w ? a.w - 1 : x0), cx1 = x0 + 1 >= a.w ? a.w - 1 : x0 + 1;   // x0 + 1 >= 0
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int ty = y0 + r, cy = ty < 0 ? 0 : (ty >= a.h ? a.h - 1 : ty);
            ql[r] = cy * a.w + cx0;
            qr[r] = cy * a.w + cx1;
            L[r] = tp_load<MOMENTS>(a, ql[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int nq = __shfl_down(ql[r], 1);      // the last lane gets its own
        R[r] = tp_next_lane<MOMENTS>(L[r]);
        if (live && nq != qr[r]) R[r] = tp_load<MOMENTS>(a, qr[r]);
    }
    if (!live) return;
    const float ax = fx - (float)x0, ay = fy - (float)y0;
    TpSum s = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int tx = x0 + (k & 1), ty = y0 + (k >> 1);
        if (tx < 0 || tx >= a.w || ty < 0 || ty >= a.h) continue;
        const TpRec &q = (k & 1) ? R[k >> 1] : L[k >> 1];
        tp_tap(a, id, n, qq, tp_weight(k, ax, ay), q.id, q.t, q.n, q.c, q.m, s);
    }
    tp_finish<MOTION>(a, p, c, s, nb);
}

}   // namespace

#define TP_HIP(expr)                                                         \
    do {                                                                     \
        hipError_t tp_e_ = (expr);                                           \
        if (tp_e_ != hipSuccess) return rt_hip_fail(tp_e_, #expr, __FILE__, __LINE__); \
    } while (0)

static TpArgs tp_args(const rt_tmotion_desc *d, const float *dx_tab, const float *dy_tab, const float view[7],
                      const float prev_view[7], bool same_view)
{
    TpArgs a = {};
    a.w = d->width; a.h = d->height;
    a.reset = d->reset != 0;
    a.same_view = same_view;
    a.max_n = (float)d->max_history;
    a.tol = d->depth_tolerance;
    a.cos2 = d->normal_cos_min * d->normal_cos_min;
    a.ox = view[0]; a.oy = view[1]; a.oz = view[2];
    a.cp = view[3]; a.sp = view[4]; a.cy = view[5]; a.sy = view[6];
    a.pox = prev_view[0]; a.poy = prev_view[1]; a.poz = prev_view[2];
    a.pcp = prev_view[3]; a.psp = prev_view[4]; a.pcy = prev_view[5]; a.psy = prev_view[6];
    a.pa = d->prev_aspect;
    a.eye_nz = 0.f - (-1.f / d->aspect);   // as rt_build_frame_consts
    a.dx_tab = dx_tab; a.dy_tab = dy_tab;
    a.rgba_in = (const float4 *)d->rgba_in;
    a.normal = (const float4 *)d->normal;
    a.depth = d->depth;
    a.id = (const int2 *)d->id;
    a.prev_rgba = (const float4 *)d->prev_rgba;
    a.prev_normal = (const float4 *)d->prev_normal;
    a.prev_depth = d->prev_depth;
    a.prev_id = (const int2 *)d->prev_id;
    a.prev_moments = (const float2 *)d->prev_moments;
    a.rgba_out = (float4 *)d->rgba_out;
    a.moments_out = (float2 *)d->moments_out;
    a.pixels = d->pixels;
    a.nsm = d->sphere_motion ? d->n_sphere_motion : 0;
    a.ncm = d->cube_motion ? d->n_cube_motion : 0;
    a.smot = a.nsm ? (const float4 *)d->sphere_motion : nullptr;
    a.cmot = a.ncm ? (const float4 *)d->cube_motion : nullptr;
    a.clamp = d->clamp != 0;
    a.slack = d->clamp_slack;
    a.clamp_n = (float)d->clamp_history;
    return a;
}

int rt_temporal_launch(const rt_tmotion_desc *d, const float *dx_tab, const float *dy_tab, const float view[7],
                       const float prev_view[7], bool same_view, hipEvent_t *ev, hipStream_t stream)
{
    const TpArgs a = tp_args(d, dx_tab, dy_tab, view, prev_view, same_view);
    // nothing moves and nothing is clamped, or no history is read: the instantiations without MOTION compute it
    const bool motion = !a.reset && (a.nsm != 0 || a.ncm != 0 || a.clamp);
    const bool moments = a.moments_out && a.prev_moments;
    void (*kernel)(TpArgs);
    dim3 grid, block;
    // without MOTION, reset and identical views read no neighbour: the product is then the plain kernel
    if (d->variant == 1 || (!motion && (a.reset || a.same_view))) {
        kernel = motion ? tp_plain<true> : tp_plain<false>;
        grid = dim3((a.w + TP_ROW - 1) / TP_ROW, a.h);
        block = dim3(TP_ROW);
    } else {
        kernel = motion ? (moments ? tp_product<true, true> : tp_product<true, false>)
                        : (moments ? tp_product<false, true> : tp_product<false, false>);
        const int nseg8 = ((a.w + TP_TW - 1) / TP_TW + 7) >> 3, nty = (a.h + TP_TH - 1) / TP_TH;
        grid = dim3((unsigned)((size_t)nseg8 * 8 * nty));
        block = dim3(TP_TW * TP_TH);
    }
    if (ev) TP_HIP(hipEventRecord(ev[0], stream));
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, a);
    TP_HIP(hipGetLastError());
    if (ev) TP_HIP(hipEventRecord(ev[1], stream));
    return RT_OK;
}
