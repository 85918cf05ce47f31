// rt_shadow.h -- shadow rays: ShadowChain (castLightRay's sample construction), shadow_test and the sample pre-pass
// (PreSure / presure_test). Included by rt_trace.inc for the frame kernel and by rt_cast.h for the passes that shade
// their own hits. (rt_cull.h: RT_BEHIND_FACTOR.)
#pragma once
#include "rt_cull.h"

namespace {

// ---------------------------------------------------------------------------
// castLightRay's sample construction, kernel.cu:1438-1468 (exact)
// ---------------------------------------------------------------------------
template <int LEAN>
struct ShadowChain {
    V3 toL;            // keeps being re-normalised in place by the reference
    // per-lane flags, kept as wave masks (scalar registers; see LM above)
    lmask stable;      // an iteration leaves toL as it found it: every later iteration repeats this one
    lmask fixed1;      // normalise() maps toL to itself: later iterations can only differ in `angle`
    lmask settled;     // toL has its final value (advance()); says nothing about the cached angle / matrix
    float angle;
    float m00, m01, m02, m10, m11, m12, m20, m21, m22;

    // FAST mode: toL itself is exact -- begin() and settle() run as in the exact kernel, because toL
    // multiplies the brightness continuously (kernel.cu:1541) -- but everything that only shapes the
    // sample directions (the angle to the light's edge, the rotation axis, angle and matrix of
    // kernel.cu:1444-1466) is computed ONCE per light from the settled toL, in binary32 with hardware
    // rsq / sqrt and fused multiply-adds, instead of being followed through the ten iterations.
    __device__ __forceinline__ void setup_fast(const RtLightDev &L, V3 start)
    {
        const V3 lpos{L.px, L.py, L.pz};
        const V3 P{-toL.z, 0.f, toL.x};                                     // cross(toL, (0,1,0))
        V3 e0{__builtin_fmaf(P.x, L.size, lpos.x) - start.x, lpos.y - start.y, __builtin_fmaf(P.z, L.size, lpos.z) - start.z};
        const V3 toEdge = normalise_t<2>(e0);
        angle = __builtin_cosf(2.f * __builtin_fmaf(toL.x, toEdge.x, __builtin_fmaf(toL.y, toEdge.y, toL.z * toEdge.z)));
        V3 ax0{-toL.y, toL.x, 0.f};                                         // cross((0,0,1), toL)
        const V3 axis = normalise_t<2>(ax0);
        const float cs = toL.z;                                             // cos(acos(toL.z))
        const float sn = __builtin_amdgcn_sqrtf(__builtin_fmaxf(__builtin_fmaf(-cs, cs, 1.f), 0.f));
        const float omc = 1.f - cs;
        m00 = __builtin_fmaf(axis.x, axis.x, cs);
        m01 = axis.x * axis.y * omc;
        m02 = -axis.y * sn;
        m10 = m01;
        m11 = __builtin_fmaf(axis.y * axis.y, omc, cs);
        m12 = -axis.x * sn;
        m20 = -axis.y * sn;
        m21 = axis.x * sn;
        m22 = cs;
        stable = ~0ull;
        fixed1 = ~0ull;
    }
    __device__ __forceinline__ V3 direction_fast(AuxPtr ax, const RtLightDev &L, int j)
    {
        const float z = __builtin_fmaf(ax->jf[j], 1.0f - angle, angle);
        const float sq = __builtin_amdgcn_sqrtf(__builtin_fmaf(-z, z, 1.f));   // NaN beyond |z| = 1, as the exact form
        const float x = sq * ax->jcos[j], y = sq * ax->jsin[j];
        V3 nd{L.px - __builtin_fmaf(x, m00, __builtin_fmaf(y, m10, z * m20)),
              L.py - __builtin_fmaf(x, m01, __builtin_fmaf(y, m11, z * m21)),
              L.pz - __builtin_fmaf(x, m02, __builtin_fmaf(y, m12, z * m22))};
        return normalise_t<2>(nd);
    }

    __device__ __forceinline__ void begin(V3 lpos, V3 start)
    {
        // toL = normalise(l.pos - start), kernel.cu:1438
        toL = V3{lpos.x - start.x, lpos.y - start.y, lpos.z - start.z};
        normalise_t<LEAN>(toL);
        stable = 0;
        fixed1 = 0;
        settled = 0;
        angle = 0.f;
        m00 = m01 = m02 = m10 = m11 = m12 = m20 = m21 = m22 = 0.f;
    }

    // One iteration's effect on toL alone (its two in-place normalisations, kernel.cu:1465-1466), for an iteration
    // whose sample direction nobody needs: the next direction() then starts from the toL that iteration would have left.
    // `stable` is not raised here -- the cached angle / matrix belong to whatever toL they were computed from, and
    // direction() recomputes them unless it established itself that toL no longer moves.
    __device__ __forceinline__ void advance()
    {
        const lmask act = LM(true);
        if ((act & ~(settled | stable)) == 0) return;
        if (LEAN) settled |= renormalise_is_identity();
        if (LEAN && (act & ~(settled | stable)) == 0) return;
        // (a wave mask is one value for the whole wave only in code every lane runs: the votes are taken AFTER the branch --
        // inside it, the lanes that skip it would keep a stale copy. A lane that skips leaves toL == tin: its bit is set
        // by the vote, as it already was.)
        const V3 tin = toL;
        V3 mid = toL;
        if (!lane_in(settled | stable)) {
            normalise_t<LEAN>(toL);
            mid = toL;
            normalise_t<LEAN>(toL);
        }
        settled |= (LM(toL.x == tin.x) & LM(toL.y == tin.y) & LM(toL.z == tin.z)) |
                   (LM(toL.x == mid.x) & LM(toL.y == mid.y) & LM(toL.z == mid.z));
    }

    // normalise(toL) leaves toL as it is, for sure: the squared length as normalise() forms it (dot3, kernel.cu:56-58) is
    // 1 or the next float, whose correctly rounded root is 1.0f (sqrt(1 + 2^-23) = 1 + 2^-24 - 2^-49 + ..., below the
    // midpoint 1 + 2^-24), and x / 1.0f = x. Then every later normalisation repeats that: toL has its final value. Five
    // multiply-adds and two compares where the pair of normalisations that would find it out takes eighty -- and half of
    // the lanes leave begin() that way, nearly all of the others the first pair. (Culling kernels only: the brute-force
    // and force-slow instantiations keep running the normalisations, so every cull-vs-brute comparison checks this.)
    __device__ __forceinline__ lmask renormalise_is_identity() const
    {
        const float d2 = dot3(toL, toL);
        return LM(d2 == 1.f) | LM(d2 == 0x1.000002p0f);   // false for a NaN
    }

    // The approximate sample frame of the pre-pass (see the frame kernel): from an approximate unit toL, binary32 with
    // hardware reciprocal square roots and fused multiply-adds, cos(acos z) = z and sin(acos z) = sqrt(1 - z^2). The
    // directions it yields differ from the exact chain's by less than RT_PRE_DELTA when the guards hold (returned flag;
    // direction_approx's `ok`): derivation in the frame kernel.
    __device__ __forceinline__ lmask setup_approx(const RtLightDev &L, V3 start, V3 t)
    {
        const V3 P{-t.z, 0.f, t.x};                                           // cross(toL, (0,1,0))
        const V3 e0{__builtin_fmaf(P.x, L.size, L.px) - start.x, L.py - start.y, __builtin_fmaf(P.z, L.size, L.pz) - start.z};
        const float e2 = __builtin_fmaf(e0.x, e0.x, __builtin_fmaf(e0.y, e0.y, e0.z * e0.z));
        const float dte = __builtin_fmaf(t.x, e0.x, __builtin_fmaf(t.y, e0.y, t.z * e0.z)) * __builtin_amdgcn_rsqf(e2);
        angle = __builtin_cosf(2.f * dte);
        const float q2 = __builtin_fmaf(t.x, t.x, t.y * t.y);
        const float rq = __builtin_amdgcn_rsqf(q2);
        const float axx = -t.y * rq, axy = t.x * rq;                           // axis = (0,0,1) x toL, normalised; az = 0
        const float cs = t.z;
        const float sn = __builtin_amdgcn_sqrtf(__builtin_fmaxf(__builtin_fmaf(-cs, cs, 1.f), 0.f));
        const float omc = 1.f - cs;
        m00 = __builtin_fmaf(axx, axx, cs);
        m01 = axx * axy * omc;
        m02 = -axy * sn;
        m10 = m01;
        m11 = __builtin_fmaf(axy * axy, omc, cs);
        m12 = -axx * sn;
        m20 = -axy * sn;
        m21 = axx * sn;
        m22 = cs;
        return LM(q2 >= 0.0025f) & LM(q2 <= 1.001f) & LM(e2 >= 1.0e-6f) & LM(e2 <= 1.0e30f) & LM(__builtin_fabsf(angle) <= 1.f);
    }
    __device__ __forceinline__ V3 direction_approx(AuxPtr ax, const RtLightDev &L, int j, bool &ok) const
    {
        const float z = __builtin_fmaf(ax->jf[j], 1.0f - angle, angle);
        const float zz = __builtin_fmaf(-z, z, 1.f);
        ok = zz >= 0.0025f;                                                    // sqrt(1 - z^2) >= 0.05: its slope in z stays below 20
        const float sq = __builtin_amdgcn_sqrtf(zz);
        const float x = sq * ax->jcos[j], y = sq * ax->jsin[j];
        V3 nd{L.px - __builtin_fmaf(x, m00, __builtin_fmaf(y, m10, z * m20)),
              L.py - __builtin_fmaf(x, m01, __builtin_fmaf(y, m11, z * m21)),
              L.pz - __builtin_fmaf(x, m02, __builtin_fmaf(y, m12, z * m22))};
        const float inv = __builtin_amdgcn_rsqf(__builtin_fmaf(nd.x, nd.x, __builtin_fmaf(nd.y, nd.y, nd.z * nd.z)));
        return V3{nd.x * inv, nd.y * inv, nd.z * inv};
    }

    // Only the evolution of toL over the ten iterations (two in-place
    // normalisations each, kernel.cu:1465-1466), for callers that need the final
    // toL of kernel.cu:1541 but none of the sample directions.
    __device__ __forceinline__ void settle()
    {
        const lmask act = LM(true);
#pragma unroll 1
        for (int j = 0; j < RT_SHADOW_SAMPLES; ++j) {
            if (LEAN) stable |= renormalise_is_identity();
            if ((act & ~stable) == 0) break;
            const V3 tin = toL;
            V3 mid = toL;
            if (!lane_in(stable)) {
                normalise_t<LEAN>(toL);
                mid = toL;
                normalise_t<LEAN>(toL);
            }
            // unchanged by the pair, or a fixed point of normalise(): toL has its final value (voted on after the branch,
            // see advance())
            stable |= (LM(toL.x == tin.x) & LM(toL.y == tin.y) & LM(toL.z == tin.z)) |
                      (LM(toL.x == mid.x) & LM(toL.y == mid.y) & LM(toL.z == mid.z));
        }
    }

    // Direction of sample j. Everything up to the rotation matrix depends on j
    // only through toL, which normalise() keeps re-normalising in place
    // (kernel.cu:1465-1466). Once two more normalisations leave toL
    // bit-identical, every later iteration reproduces the same values, so the
    // block is skipped (70 % of lanes are stable after j = 0, 99.6 % after j = 1).
    __device__ __forceinline__ V3 direction(AuxPtr ax, bool force_slow, const RtLightDev &L,
                                            V3 start, int j, const double *atab = nullptr)
    {
        const V3 lpos{L.px, L.py, L.pz};
        // the flags as per-lane values while the branches below assign them; back into the wave masks after the join
        bool st = lane_in(stable), f1 = lane_in(fixed1);
        if (!st || force_slow) {
            const V3 tin = toL;
            // P = cross(toL, (0,1,0)), kernel.cu:1444
            const V3 P{toL.y * 0.f - toL.z * 1.f, toL.z * 0.f - toL.x * 0.f, toL.x * 1.f - toL.y * 0.f};
            V3 e0{(lpos.x + P.x * L.size) - start.x, (lpos.y + P.y * L.size) - start.y,
                  (lpos.z + P.z * L.size) - start.z};
            const V3 toEdge = normalise_t<LEAN>(e0);                       // kernel.cu:1450
            angle = rtm::cosf_rt(dot3(toL, toEdge) * 2.f);                 // kernel.cu:1451
            // The rest depends on toL only through its next two in-place normalisations. Once
            // normalise() maps toL to itself (`fixed1`, 96 % of the lanes that are not `stable`
            // after the first iteration) those leave it -- and the axis, nAngle and the matrix
            // -- as they are: this iteration only had a new `angle` to compute, the next ones
            // repeat it.
            if (!f1 || force_slow) {
                // axis = normalise(cross((0,0,1), normalise(toL))), kernel.cu:1465
                const V3 n1 = normalise_t<LEAN>(toL);
                const V3 mid = toL;
                V3 ax0{0.f * n1.z - 1.f * n1.y, 1.f * n1.x - 0.f * n1.z, 0.f * n1.y - 0.f * n1.x};
                const V3 axis = normalise_z0_t<LEAN>(ax0);
                // nAngle = acosf(dot(normalise(toL), (0,0,1))), kernel.cu:1466
                const V3 n2 = normalise_t<LEAN>(toL);
                const float nAngle = rtm::acosf_rt((n2.x * 0.f + n2.y * 0.f) + n2.z * 1.f, atab);
                float sn, cs;
                rtm::sincosf_rt(nAngle, sn, cs);
                const float omc = 1.f - cs;
                // rotate(nAngle, axis), kernel.cu:1267-1277 (non-standard on purpose)
                m00 = cs + axis.x * axis.x;
                m01 = axis.x * axis.y * omc - axis.z * sn;
                m02 = axis.x * axis.z * omc - axis.y * sn;
                m10 = axis.y * axis.x * omc + axis.z * sn;
                m11 = cs + axis.y * axis.y * omc;
                m12 = axis.y * axis.z * omc - axis.x * sn;
                m20 = axis.z * axis.x * omc - axis.y * sn;
                m21 = axis.z * axis.y * omc + axis.x * sn;
                m22 = cs + axis.z * axis.z * omc;
                f1 = (toL.x == mid.x) && (toL.y == mid.y) && (toL.z == mid.z) &&
                     (n1.x == n2.x) && (n1.y == n2.y) && (n1.z == n2.z);
                st = (toL.x == tin.x) && (toL.y == tin.y) && (toL.z == tin.z);
            } else {
                st = true;
            }
        }
        stable = ballot64(st);
        fixed1 = ballot64(f1);
        const float z = ax->jf[j] * (1.0f - angle) + angle;                // kernel.cu:1453
        const float zz = 1.f - z * z;
        float sq;                                                          // kernel.cu:1462-1463
        if (LEAN && __builtin_expect(zz >= 0x1.0p-96f, 1)) sq = lean_sqrt(zz);   // zz <= 1
        else sq = __builtin_sqrtf(zz);
        const float x = sq * ax->jcos[j];
        const float y = sq * ax->jsin[j];
        // multiply(rot, {x,y,z}), kernel.cu:123-125
        const V3 rv{(x * m00 + y * m10) + z * m20, (x * m01 + y * m11) + z * m21,
                    (x * m02 + y * m12) + z * m22};
        V3 nd{lpos.x - rv.x, lpos.y - rv.y, lpos.z - rv.z};
        return normalise_t<LEAN>(nd);                                      // kernel.cu:1468
    }
};

// One shadow ray against one table entry: updates `shadowed` (any-hit,
// kernel.cu:1504-1508). Two shortcuts decide most entries without sqrt/div:
// h < -h_sure puts t above RT_T_MIN (-B >= 2*h_sure and sqrt(disc) >= 0), and
// "behind" (see RT_BEHIND_FACTOR) makes t strictly negative.
template <int LEAN = 0>
__device__ __forceinline__ void shadow_test(const RayK &sr, float4 s, bool &shadowed, bool force_slow)
{
    const Quad q = (LEAN == 2) ? quadratic_fast(sr, s) : quadratic(sr, s);
    bool need;
    if (force_slow) {
        need = !shadowed;
    } else {
        const bool cand = (q.disc >= 0.f) && !shadowed;
        // h < -2e-4*A puts t above RT_T_MIN (-B >= 4e-4*A, sqrt(disc) >= 0, divided by 2A); 5e-5 * (4A) is that
        // bound up to a rounding the strict margins of the argument swallow many times over
        const bool sure = cand && (q.h < -5.0e-5f * sr.a4);
        const bool behind = (q.h > 0.f) && (q.disc < q.BB * RT_BEHIND_FACTOR);
        shadowed = shadowed || sure;
        need = cand && !sure && !behind;
    }
    if (any64(need)) {
        if (need) {
            float t;
            if (intersect_tail_t<LEAN>(sr, q, t)) shadowed = true;
        }
    }
}

// The pre-pass of a light's ten samples (frame kernel): one shadow ray with an APPROXIMATE direction dq -- within
// RT_PRE_DELTA of the exact chain's direction d -- against one list entry. Decides, where it can, what the exact test
// (shadow_test above = intersect() of kernel.cu:293-354 for an any-hit) returns for d:
//   hit   the exact test returns true:  the line passes the centre solidly inside the radius, ahead of the origin;
//   miss  it returns false: no real root with margin, or the origin outside the sphere and the centre solidly behind.
// C = |oc|^2 - R^2 is formed by the exact test's own operations (same bits); only h = d.oc differs, by at most
// eta = (RT_PRE_DELTA + 2e-6) |oc| (the direction, and the rounding of either dot product), so |h| lies in
// [hm, hp] = [|hq| - eta, |hq| + eta]. The exact test's discriminant B^2 - 4AC carries at most 3.8e-6 |oc|^2 of rounding
// (rt_device.h), i.e. 9.5e-7 |oc|^2 on h^2 - C, and A = |d|^2 is 1 to 3e-7: 3e-6 |oc|^2 is the margin used.
//   hit:  hq + eta < -2.1e-4 (so h < -5e-5 * 4A: the exact kernel's `sure` clause, t >= 1e-4) and hm^2 - C >= 3e-6 |oc|^2
//         (so the float discriminant is >= 0);
//   miss: hp^2 - C <= -3e-6 |oc|^2 (float discriminant < 0: the root is a NaN, every comparison false), or
//         hq - eta > 0 and C > 1.002e-5 hp^2 (h > 0 and disc < 0.99999 B^2: the exact kernel's `behind` clause, t < 0).
// A non-finite entry satisfies neither. Lanes that are neither `hit` by some entry nor `miss`ed by all are left to the
// exact chain.
#define RT_PRE_DELTA 1.0e-5f
#ifndef RT_PRE_GROUP
#define RT_PRE_GROUP 2   // samples per pass of the pre-pass over a light's list (measured: 2 and 3 alike, 4 +1 %, 5 +5 %: every
                         // sample carries three wave masks, and a pass ends only when all of its samples are settled)
#endif
// N samples against one entry: oc, |oc|^2, C and the margins are the entry's and the pixel's, not the sample's -- 14 of a
// single test's 35 instructions, formed once per entry for all N directions.
template <int N>
struct PreSure { lmask hit[N], miss[N]; };   // wave masks (see LM)
template <int N>
__device__ __forceinline__ PreSure<N> presure_test(V3 o, const V3 (&dq)[N], float4 s)
{
    const float ocx = o.x - s.x, ocy = o.y - s.y, ocz = o.z - s.z;
    const float oc2 = (ocx * ocx + ocy * ocy) + ocz * ocz;
    const float C = oc2 - s.w;                                    // as quadratic(): the same bits
    const float eta = ((RT_PRE_DELTA + 2.0e-6f) * 1.0001f) * __builtin_amdgcn_sqrtf(oc2);
    const float m = 3.0e-6f * oc2;
    PreSure<N> r;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const float hq = __builtin_fmaf(dq[i].x, ocx, __builtin_fmaf(dq[i].y, ocy, dq[i].z * ocz));
        const float ah = __builtin_fabsf(hq);
        const float hp = ah + eta, hm = __builtin_fmaxf(ah - eta, 0.f);
        r.hit[i] = LM(hq + eta < -2.1e-4f) & LM(__builtin_fmaf(hm, hm, -C) >= m);
        r.miss[i] = LM(__builtin_fmaf(hp, hp, -C) <= -m) | (LM(hq - eta > 0.f) & LM(C > 1.002e-5f * (hp * hp)));
    }
    return r;
}

}  // namespace
