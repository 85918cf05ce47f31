// rt_exact.h -- the arithmetic that decides a pixel, in the reference's evaluation order, and its lean twins: the
// normalise family, lean_sqrt / LeanRcp, the texel index, the brightness tables, rgb_to_int, RayK / Quad /
// intersect_tail* and the plane, cube, triangle and box tests. Included by rt_cull.h (and so by the frame kernel)
// and by rt_bvh.h for the passes that walk the sphere BVH.
#pragma once
#include "rt_math.h"
#include "rt_wave.h"

namespace {

// ---------------------------------------------------------------------------
// exact (reference-order) vector helpers, kernel.cu:46-108
// ---------------------------------------------------------------------------
__device__ __forceinline__ float dot3(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// normalise(vec3d&): l = sqrtf(dot); if (l != 0) v /= l (in place) and return it,
// else return (0,0,0) leaving v alone. The reference divides in binary64 and
// narrows; for binary32 operands that equals the correctly rounded binary32
// quotient (53 >= 2*24+2), so a float division reproduces it bit for bit.
__device__ __forceinline__ V3 normalise_inplace(V3 &v)
{
    const float l = __builtin_sqrtf(dot3(v, v));
    if (l != 0.f) {
        v.x = v.x / l;
        v.y = v.y / l;
        v.z = v.z / l;
        return v;
    }
    return V3{0.f, 0.f, 0.f};
}

// ---------------------------------------------------------------------------
// The same normalise() -- and the same correctly rounded binary32 square root --
// without the instructions that only matter outside the ordinary range.
//
// hipcc expands an IEEE `a / b` into v_div_scale (x2), v_rcp, four FMAs, a multiply,
// v_div_fmas and v_div_fixup, and an IEEE sqrtf into a pre-scaling select, v_sqrt, the
// one-ulp-down / one-ulp-up residual test and a class fix-up (see the disassembly of
// normalise_inplace above: 55 instructions). Pre-scaling and fix-up only act on
// denormal, huge, zero, infinite or NaN operands; for operands in an ordinary range
// v_div_scale returns its operand unchanged and clears VCC, v_div_fmas is then a plain
// FMA and v_div_fixup returns its first operand. The division below is that expansion
// with exactly these no-ops left out -- every remaining instruction is the one the full
// expansion executes, on the same operands -- and the reciprocal refinement (which
// depends on the divisor only) shared by the three quotients; lean_sqrt() is the
// compiler's OTHER correctly rounded square root (see there), verified against sqrtf on
// every float of its range. Lanes outside the safe range take the full IEEE expansion:
//   every component >= 2^-48 in magnitude (so dot >= 2^-96, above sqrt's pre-scaling
//   threshold, no quotient below 2^-68, no numerator the scaling would touch) and
//   dot <= 2^40.
// A zero component is "unsafe" (the lean sequence would lose the sign of -0).
// tests/test_gpu_parity.py compares both functions with the IEEE ones exhaustively
// (sqrt: every float of the range) and on 2^28 random vectors; the brute-force and
// force-slow kernels keep the IEEE forms, so every cull-vs-brute comparison checks
// them against each other as well.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float lean_sqrt(float x)   // x in [2^-96, 2^126]
{
    // The compiler's expansion of a correctly rounded binary32 square root for results that cannot be denormal:
    // reciprocal square root, one coupled Newton step for the root and half its reciprocal, one residual correction --
    // one transcendental and seven multiply(-add)s of the cheap issue class. (Round 2 used its other expansion -- v_sqrt,
    // the neighbours one ulp down and up, two residuals, two compares, two selects -- whose compares and selects issue at
    // half that rate.) Equal to sqrtf on EVERY float of [2^-96, 2^40]: rt_debug_shortcuts(1).
    const float r = __builtin_amdgcn_rsqf(x);
    float g = x * r;
    float h = 0.5f * r;
    const float e = __builtin_fmaf(-h, g, 0.5f);
    h = __builtin_fmaf(h, e, h);
    g = __builtin_fmaf(g, e, g);
    const float d = __builtin_fmaf(-g, g, x);
    return __builtin_fmaf(d, h, g);
}

struct LeanRcp {   // the divisor-only part of the division expansion
    float d, r;
    __device__ __forceinline__ explicit LeanRcp(float den) : d(den)
    {
        const float r0 = __builtin_amdgcn_rcpf(den);
        const float e0 = __builtin_fmaf(-den, r0, 1.f);
        r = __builtin_fmaf(e0, r0, r0);
    }
    __device__ __forceinline__ float divide(float n) const
    {
        const float q0 = n * r;
        const float e1 = __builtin_fmaf(-d, q0, n);
        const float q1 = __builtin_fmaf(e1, r, q0);
        const float e2 = __builtin_fmaf(-d, q1, n);
        return __builtin_fmaf(e2, r, q1);
    }
};

// PREC: 0 = the IEEE forms as hipcc expands them, 1 = lean (the same bits, see above), 2 = FAST: the opt-in
// approximate mode of rt_launch_opts.fast (hardware reciprocal square root / reciprocal / square root,
// binary32 trigonometry, FMA contraction) -- NOT bit-exact; north_star's tolerance is 1e-5 relative per
// channel away from the discrete decisions (a shadow sample, a texel, a silhouette), see DESIGN.md section 4c.
template <int PREC>
__device__ __forceinline__ V3 normalise_t(V3 &v)
{
    if constexpr (PREC == 0) {
        return normalise_inplace(v);
    } else if constexpr (PREC == 2) {
        const float d2 = __builtin_fmaf(v.x, v.x, __builtin_fmaf(v.y, v.y, v.z * v.z));
        if (d2 > 0.f) {   // a zero vector stays as it is and (0,0,0) is returned, as normalise() does
            const float inv = __builtin_amdgcn_rsqf(d2);
            v.x *= inv; v.y *= inv; v.z *= inv;
            return v;
        }
        return V3{0.f, 0.f, 0.f};
    } else {
        const float d2 = dot3(v, v);
        const float amin = __builtin_fminf(__builtin_fminf(__builtin_fabsf(v.x), __builtin_fabsf(v.y)), __builtin_fabsf(v.z));
        const bool safe = (amin >= 0x1.0p-48f) & (d2 <= 0x1.0p40f);   // false for a NaN anywhere
        if (__builtin_expect(!safe, 0)) return normalise_inplace(v);
        const LeanRcp rl(lean_sqrt(d2));
        v.x = rl.divide(v.x);
        v.y = rl.divide(v.y);
        v.z = rl.divide(v.z);
        return v;
    }
}

// normalise() of a vector whose z component is +-0 by construction (castLightRay's rotation axis cross((0,0,1), n),
// kernel.cu:1465): the general lean form calls a zero component unsafe (it would lose the sign of -0) and such a vector
// would take the IEEE expansion every time. Here z*z = +0 adds nothing to (x*x + y*y) -- the same dot bit for bit -- and
// (+-0) / l = +-0 for the positive finite l of the safe range: z stays as it is, x and y take the lean division.
template <int PREC>
__device__ __forceinline__ V3 normalise_z0_t(V3 &v)
{
    if constexpr (PREC != 1) {
        return normalise_t<PREC>(v);
    } else {
        const float d2 = dot3(v, v);
        const float amin = __builtin_fminf(__builtin_fabsf(v.x), __builtin_fabsf(v.y));
        const bool safe = (amin >= 0x1.0p-48f) & (d2 <= 0x1.0p40f) & (v.z == 0.f);   // false for a NaN anywhere
        if (__builtin_expect(!safe, 0)) return normalise_inplace(v);
        const LeanRcp rl(lean_sqrt(d2));
        v.x = rl.divide(v.x);
        v.y = rl.divide(v.y);
        return v;
    }
}

// ---------------------------------------------------------------------------
// Texel index of a unit normal without binary64: castRay's (tx, ty) (kernel.cu:1402-1403)
// only ever select a texel, c_index = (int)(ty*maxY)*maxX + (int)(tx*maxX) (kernel.cu:1653).
// approx_sphere_uv() evaluates tx = (1 + atan2(n.z, n.x)/3.1415)/2 and ty = acos(n.y)/3.1415
// in binary32 with absolute error below RT_UV_DELTA (budget: quotient after one Newton step
// 0.5 ulp, degree-8 polynomial 1.2e-8 + ~1 ulp of evaluation, all quadrant reconstruction done
// in units of the RESULT so that no step rounds at the magnitude of pi: 1.7e-7 for tx, 2.6e-7
// for ty; rt_debug_uv measures it on the device and tests/test_gpu_parity.py asserts half of
// RT_UV_DELTA). A lane is "sure" when both products tx*W, ty*H stay at least
// mu = size * (RT_UV_DELTA + 2^-22) away from every integer (the second term covers the
// rounding of the two float products): then truncation gives the same column and row as the
// exact value would. Unsure lanes (about 5 % of the 8x8 tiles contain one at 512x512) -- and
// anything negative or NaN -- take the exact binary64 path.
// ---------------------------------------------------------------------------
#define RT_UV_DELTA 5.0e-7f

// atan(a) for a in [0, 1], absolute error < 1.0e-7 (Chebyshev fit of atan(sqrt(s))/sqrt(s), degree 8 in s)
__device__ __forceinline__ float atan01(float a)
{
    const float s = a * a;
    float p = 0x1.73776ap-9f;
    p = __builtin_fmaf(p, s, -0x1.0639f6p-6f);
    p = __builtin_fmaf(p, s, 0x1.5ce0b0p-5f);
    p = __builtin_fmaf(p, s, -0x1.330372p-4f);
    p = __builtin_fmaf(p, s, 0x1.b3ae74p-4f);
    p = __builtin_fmaf(p, s, -0x1.22de60p-3f);
    p = __builtin_fmaf(p, s, 0x1.997232p-3f);
    p = __builtin_fmaf(p, s, -0x1.5554a2p-2f);
    p = __builtin_fmaf(p, s, 1.0f);
    return a * p;
}

// angle(y, x) * scale for y >= 0 given as magnitudes: returns scale * atan2(ay, x) in [0, scale*pi],
// reconstructed in units of the result. k_half = scale*pi/2, k_full = scale*pi (both rounded once).
__device__ __forceinline__ float scaled_angle(float ay, float x, float scale, float k_half, float k_full)
{
    const float ax = __builtin_fabsf(x);
    const float mx = __builtin_fmaxf(ax, ay), mn = __builtin_fminf(ax, ay);
    const float r = __builtin_amdgcn_rcpf(mx);
    const float a0 = mn * r;
    const float a = __builtin_fmaf(__builtin_fmaf(-mx, a0, mn), r, a0);   // mn / mx to half an ulp (NaN for 0/0)
    float u = atan01(a) * scale;
    u = (ay > ax) ? k_half - u : u;
    u = (x < 0.f) ? k_full - u : u;
    return u;
}

__device__ __forceinline__ void approx_sphere_uv(V3 n, float &tx, float &ty)
{
    constexpr double kC = 1.0 / 3.1415, kPiD = 3.14159265358979323846;
    // tx = 0.5 + sign(n.z) * atan2(|n.z|, n.x) / (2 * 3.1415)
    const float u = scaled_angle(__builtin_fabsf(n.z), n.x, (float)(0.5 * kC), (float)(0.25 * kPiD * kC), (float)(0.5 * kPiD * kC));
    tx = __builtin_signbit(n.z) ? 0.5f - u : 0.5f + u;
    // ty = atan2(sqrt((1 - y)(1 + y)), y) / 3.1415; the root to about an ulp (one Newton step)
    const float q = (1.f - n.y) * (1.f + n.y);
    const float s0 = __builtin_amdgcn_sqrtf(q);
    const float rs = __builtin_amdgcn_rsqf(q);
    const float sy = (q > 0.f) ? __builtin_fmaf(__builtin_fmaf(-s0, s0, q), 0.5f * rs, s0) : 0.f;
    ty = scaled_angle(sy, n.y, (float)kC, (float)(0.5 * kPiD * kC), (float)(kPiD * kC));
    if (!(__builtin_fabsf(n.y) <= 1.f)) ty = __builtin_nanf("");   // the exact function returns NaN there
}

// Column/row selection with certainty: returns the linear index row*w + col when both products are
// clear of every integer by the margins, else -1 (the caller evaluates the exact expressions).
__device__ __forceinline__ int sure_texel(float tx, float ty, int w, int h, float mu_x, float mu_y)
{
    const float px = tx * (float)w, py = ty * (float)h;
    const float fx = __builtin_floorf(px), fy = __builtin_floorf(py);
    const float rx = px - fx, ry = py - fy;
    const bool sure = (rx > mu_x) & (rx < 1.f - mu_x) & (ry > mu_y) & (ry < 1.f - mu_y) & (fx >= 0.f) & (fy >= 0.f) &
                      (fx <= 16384.f) & (fy <= 16384.f);
    return sure ? (int)fy * w + (int)fx : -1;
}

// float -> int of the implicit conversions at kernel.cu:1653, 1157-1158, 1682:
// truncation toward zero, NaN -> 0, saturating (v_cvt_i32_f32 semantics, which
// are also CUDA's cvt.rzi.s32.f32).
__device__ __forceinline__ int f2i(float v) { return (int)v; }

// b after n executions of `b += 0.1` (float += double literal, kernel.cu:1538),
// starting from 0: depends only on how many samples were unshadowed. Literals
// instead of a table so that a per-lane n needs no memory (a kernarg array
// indexed per lane would live in scratch); the host re-derives the sequence and
// refuses to launch if it ever disagreed (rt_build_frame_consts).
__device__ __forceinline__ float brightness_steps(int n)
{
    float b = 0x0.0p+0f;
    b = n >= 1 ? 0x1.99999ap-4f : b;
    b = n >= 2 ? 0x1.99999ap-3f : b;
    b = n >= 3 ? 0x1.333334p-2f : b;
    b = n >= 4 ? 0x1.99999ap-2f : b;
    b = n >= 5 ? 0x1.000000p-1f : b;
    b = n >= 6 ? 0x1.333334p-1f : b;
    b = n >= 7 ? 0x1.666668p-1f : b;
    b = n >= 8 ? 0x1.99999cp-1f : b;
    b = n >= 9 ? 0x1.ccccd0p-1f : b;
    b = n >= 10 ? 0x1.000002p+0f : b;
    return b;
}

// The same eleven values for per-lane lookups (copied into LDS once per wave).
__device__ const float kBrightnessSteps[16] = {0x0.0p+0f,      0x1.99999ap-4f, 0x1.99999ap-3f, 0x1.333334p-2f,
                                               0x1.99999ap-2f, 0x1.000000p-1f, 0x1.333334p-1f, 0x1.666668p-1f,
                                               0x1.99999cp-1f, 0x1.ccccd0p-1f, 0x1.000002p+0f, 0.f, 0.f, 0.f, 0.f, 0.f};

// rtm::atan_eighth(0..8), for the same purpose (values checked against the function by
// tests/test_gpu_parity.py through the math debug ops, which use the LDS copy as well).
__device__ const double kAtanEighth[16] = {0x0.0p+0,
                                           0x1.fd5ba9aac2f6ep-4,
                                           0x1.f5b75f92c80ddp-3,
                                           0x1.6f61941e4def1p-2,
                                           0x1.dac670561bb4fp-2,
                                           0x1.1e00babdefeb4p-1,
                                           0x1.4978fa3269ee1p-1,
                                           0x1.700a7c5784634p-1,
                                           0x1.921fb54442d18p-1,
                                           0, 0, 0, 0, 0, 0, 0};

// rgbToInt, kernel.cu:547-556
__device__ __forceinline__ unsigned rgb_to_int(int r, int g, int b)
{
    if (r > 255) r = 255;
    if (g > 255) g = 255;
    if (b > 255) b = 255;
    return (unsigned)(((r & 0xff) << 16) + ((g & 0xff) << 8) + (b & 0xff));
}

// ---------------------------------------------------------------------------
// sphere::intersect, kernel.cu:293-354, on a table entry {cx,cy,cz,radius*radius}
// ---------------------------------------------------------------------------
struct RayK {          // a ray plus the one per-ray constant of the quadratic that every test needs
    float ox, oy, oz;
    float dx, dy, dz;
    float a4;          // 4*A (kernel.cu:334: B*B - 4*A*C)
    // 2*A, the divisor of both roots, only where a root is actually formed (the same expression on the same operands)
    __device__ __forceinline__ float a2() const { return 2.f * ((dx * dx + dy * dy) + dz * dz); }
};

__device__ __forceinline__ RayK make_ray(V3 o, V3 d)
{
    RayK r;
    r.ox = o.x; r.oy = o.y; r.oz = o.z;
    r.dx = d.x; r.dy = d.y; r.dz = d.z;
    const float A = (d.x * d.x + d.y * d.y) + d.z * d.z;
    r.a4 = 4.f * A;
    return r;
}

struct Quad {  // B, B*B and the discriminant, in the reference's evaluation order
    float h, B, BB, disc;
};

__device__ __forceinline__ Quad quadratic(const RayK &r, float4 s)
{
    const float ocx = r.ox - s.x, ocy = r.oy - s.y, ocz = r.oz - s.z;
    Quad q;
    q.h = (r.dx * ocx + r.dy * ocy) + r.dz * ocz;
    q.B = 2.f * q.h;
    const float C = ((ocx * ocx + ocy * ocy) + ocz * ocz) - s.w;
    q.BB = q.B * q.B;
    q.disc = q.BB - r.a4 * C;
    return q;
}

// FAST mode: the same quadratic with fused multiply-adds (11 instructions instead of 17)
__device__ __forceinline__ Quad quadratic_fast(const RayK &r, float4 s)
{
    const float ocx = r.ox - s.x, ocy = r.oy - s.y, ocz = r.oz - s.z;
    Quad q;
    q.h = __builtin_fmaf(r.dx, ocx, __builtin_fmaf(r.dy, ocy, r.dz * ocz));
    q.B = 2.f * q.h;
    const float C = __builtin_fmaf(ocx, ocx, __builtin_fmaf(ocy, ocy, __builtin_fmaf(ocz, ocz, -s.w)));
    q.BB = q.B * q.B;
    q.disc = __builtin_fmaf(-r.a4, C, q.BB);
    return q;
}

// The tail of intersect once B and the discriminant are known.
__device__ __forceinline__ bool intersect_tail(const RayK &r, const Quad &q, float &t)
{
    const float sq = __builtin_sqrtf(q.disc);
    const float a2 = r.a2();
    t = (-q.B + sq) / a2;
    if (t == 0.f) return true;
    if (t >= RT_T_MIN) {
        const float t2 = (-q.B - sq) / a2;
        if (t > t2) t = t2;
        return true;
    }
    return false;
}

// The same tail with the lean square root and the lean divisions (see normalise_t above; both roots
// divide by the same 2A, so the divisor's part of the expansion is shared). Safe range, per lane:
// disc in [2^-96, 2^60], 2A in [2^-20, 2^20], both numerators between 2^-40 and 2^40 in magnitude --
// anything else (a zero numerator in particular: the reference's `t == 0` clause) takes the IEEE forms.
template <int PREC>
__device__ __forceinline__ bool intersect_tail_t(const RayK &r, const Quad &q, float &t)
{
    if constexpr (PREC == 0) {
        return intersect_tail(r, q, t);
    } else if constexpr (PREC == 2) {
        const float sq = __builtin_amdgcn_sqrtf(q.disc);
        const float inv = __builtin_amdgcn_rcpf(r.a2());
        t = (-q.B + sq) * inv;
        if (t == 0.f) return true;
        if (t >= RT_T_MIN) {
            const float t2 = (-q.B - sq) * inv;
            if (t > t2) t = t2;
            return true;
        }
        return false;
    } else {
        const float nb = -q.B, a2 = r.a2();
        const bool pre = (q.disc >= 0x1.0p-96f) & (q.disc <= 0x1.0p60f) & (a2 >= 0x1.0p-20f) & (a2 <= 0x1.0p20f);
        if (__builtin_expect(!pre, 0)) return intersect_tail(r, q, t);
        const float sq = lean_sqrt(q.disc);
        const float n1 = nb + sq, n2 = nb - sq;
        const bool safe = (__builtin_fminf(__builtin_fabsf(n1), __builtin_fabsf(n2)) >= 0x1.0p-40f) &
                          (__builtin_fmaxf(__builtin_fabsf(n1), __builtin_fabsf(n2)) <= 0x1.0p40f);
        if (__builtin_expect(!safe, 0)) return intersect_tail(r, q, t);
        const LeanRcp ra(a2);
        t = ra.divide(n1);
        if (t >= RT_T_MIN) {           // t == 0 cannot happen here: |n1| >= 2^-40 and 2A <= 2^20
            const float t2 = ra.divide(n2);
            if (t > t2) t = t2;
            return true;
        }
        return false;
    }
}


// plane::intersect, kernel.cu:370-380
__device__ __forceinline__ bool plane_intersect(const RtPlaneDev &p, V3 o, V3 d, float &t)
{
    const float denom = (p.nx * d.x + p.ny * d.y) + p.nz * d.z;
    if (denom < 0.f) {
        const V3 pl0{p.ox - o.x, p.oy - o.y, p.oz - o.z};
        t = ((pl0.x * p.nx + pl0.y * p.ny) + pl0.z * p.nz) / denom;
        return t >= 0.f;
    }
    return false;
}

// cube::intersect, kernel.cu:457-485. min/max are the reference's macros
// (kernel.cu:16-26), whose NaN behaviour differs from fminf/fmaxf. `inv` is
// 1.f / Dir per component, hoisted out of the per-cube call.
#define RT_MAXM(a, b) (((a) > (b)) ? (a) : (b))
#define RT_MINM(a, b) (((a) < (b)) ? (a) : (b))
__device__ __forceinline__ bool cube_intersect(const RtCubeDev &c, V3 o, V3 inv, float &t)
{
    const float t1 = (c.ax - o.x) * inv.x, t2 = (c.bx - o.x) * inv.x;
    const float t3 = (c.ay - o.y) * inv.y, t4 = (c.by - o.y) * inv.y;
    const float t5 = (c.az - o.z) * inv.z, t6 = (c.bz - o.z) * inv.z;
    const float tmin = RT_MAXM(RT_MAXM(RT_MINM(t1, t2), RT_MINM(t3, t4)), RT_MINM(t5, t6));
    const float tmax = RT_MINM(RT_MINM(RT_MAXM(t1, t2), RT_MAXM(t3, t4)), RT_MAXM(t5, t6));
    if (tmax < 0.f) { t = tmax; return false; }
    if (tmax < tmin) { t = tmax; return false; }
    t = tmin;
    return true;
}

// mesh::rayIntersect (Moller-Trumbore), kernel.cu:1024-1059. The two double
// literals there (`a < 0.0000001`, `t > 0.0000001`) compare the widened float
// with 1e-7; 1e-7f is the smallest binary32 >= 1e-7, so `a < 1e-7f` and
// `t >= 1e-7f` are the same predicates.
__device__ __forceinline__ bool tri_intersect(V3 o, V3 d, const float *p0, const float *p1, const float *p2,
                                              float &t, float &u, float &v)
{
    const V3 e1{p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
    const V3 e2{p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
    const V3 h{d.y * e2.z - d.z * e2.y, d.z * e2.x - d.x * e2.z, d.x * e2.y - d.y * e2.x};
    const float a = dot3(e1, h);
    if (a > -0.0000001f && a < 0.0000001f) return false;
    const float f = 1.f / a;
    const V3 s{o.x - p0[0], o.y - p0[1], o.z - p0[2]};
    u = f * dot3(s, h);
    if (u < 0.f || u > 1.f) return false;
    const V3 q{s.y * e1.z - s.z * e1.y, s.z * e1.x - s.x * e1.z, s.x * e1.y - s.y * e1.x};
    v = f * dot3(d, q);
    if (v < 0.f || u + v > 1.f) return false;
    t = f * dot3(e2, q);
    return t >= 0.0000001f;
}

__device__ __forceinline__ bool box_intersect(const RtBoxDev &b, V3 o, V3 inv)
{
    RtCubeDev c;
    c.ax = b.lo[0]; c.ay = b.lo[1]; c.az = b.lo[2];
    c.bx = b.hi[0]; c.by = b.hi[1]; c.bz = b.hi[2];
    float t;
    return cube_intersect(c, o, inv, t);
}

}  // namespace
