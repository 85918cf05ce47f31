// rt_cast.h -- the reference's casts over every kind of primitive, shared by the ray queries (rt_query.hip) and the
// whole-scene reflective passes (rt_reflect.hip): castRay's nearest hit (q_nearest) and hit record
// (q_hit_record), castLightRay's any-hit (q_occluded) and rayTrace's pixel body at a hit (q_shade_hit). One copy:
// every primitive test and the shadow chain are the frame kernel's own (rt_exact.h, rt_shadow.h), the spheres go through the BVH of rt_bvh.h.
// Device only.
#pragma once
#include "rt_bvh.h"
#include "rt_shadow.h"

namespace {

// castRay's nearest hit. kind -1: none (nt stays +inf). pos: the (leaf, triangle) position in tri_idx of a triangle
// hit, the list position of any other.
__device__ __forceinline__ float q_nearest(const RtFrameConsts &fc, AuxPtr ax, const RtReflectDev &rd, V3 O, V3 D,
                                           LdsStack stk, int &kind, int &pos)
{
    float nt = __builtin_inff();
    kind = -1;
    pos = -1;
    if (fc.n_boxes > 0) {   // kernel.cu:1293-1328: a leaf's triangles only if the ray passes the leaf's own box
        const V3 inv{1.f / D.x, 1.f / D.y, 1.f / D.z};
        for (int j = 0; j < fc.n_boxes; ++j) {
            const RtBoxDev bx = ax->boxes[j];
            if (!box_intersect(bx, O, inv)) continue;
            for (int i = 0; i < bx.len; ++i) {
                const float *tv = ax->tri9 + (size_t)(bx.start + i) * 9;
                float t, u, v;
                if (tri_intersect(O, D, tv, tv + 3, tv + 6, t, u, v) && t < nt) {
                    nt = t;
                    kind = RT_HIT_TRIANGLE;
                    pos = bx.start + i;
                }
            }
        }
    }
    {   // kernel.cu:1330-1342
        float ts;
        const int si = rf_cast<false>(rd, O.x, O.y, O.z, D.x, D.y, D.z, ts, stk);
        if (si >= 0 && ts < nt) {
            nt = ts;
            kind = RT_HIT_SPHERE;
            pos = si;
        }
    }
    if (fc.n_cubes > 0) {   // kernel.cu:1344-1356
        const V3 inv{1.f / D.x, 1.f / D.y, 1.f / D.z};
        for (int i = 0; i < fc.n_cubes; ++i) {
            float t;
            if (cube_intersect(ax->cubes[i], O, inv, t) && t < nt) {
                nt = t;
                kind = RT_HIT_CUBE;
                pos = i;
            }
        }
    }
    for (int i = 0; i < fc.n_planes; ++i) {   // kernel.cu:1359-1372
        float t;
        if (plane_intersect(ax->planes[i], O, D, t) && t < nt) {
            nt = t;
            kind = RT_HIT_PLANE;
            pos = i;
        }
    }
    if (nt == __builtin_inff()) kind = -1;   // kernel.cu:1374: a hit is nt != inf
    return nt;
}

// castLightRay's any-hit for one sample ray (kernel.cu:1475-1536): 1 if anything reports a hit
__device__ __forceinline__ int q_occluded(const RtFrameConsts &fc, AuxPtr ax, const RtReflectDev &rd, V3 O, V3 D,
                                          LdsStack stk)
{
    float t;
    if (rf_cast<true>(rd, O.x, O.y, O.z, D.x, D.y, D.z, t, stk)) return 1;
    if (fc.n_boxes > 0) {
        const V3 inv{1.f / D.x, 1.f / D.y, 1.f / D.z};
        for (int j = 0; j < fc.n_boxes; ++j) {
            const RtBoxDev bx = ax->boxes[j];
            if (!box_intersect(bx, O, inv)) continue;
            for (int i = 0; i < bx.len; ++i) {
                const float *tv = ax->tri9 + (size_t)(bx.start + i) * 9;
                float u, v;
                if (tri_intersect(O, D, tv, tv + 3, tv + 6, t, u, v)) return 1;
            }
        }
    }
    for (int i = 0; i < fc.n_planes; ++i)
        if (plane_intersect(ax->planes[i], O, D, t)) return 1;
    if (fc.n_cubes > 0) {
        const V3 inv{1.f / D.x, 1.f / D.y, 1.f / D.z};
        for (int i = 0; i < fc.n_cubes; ++i)
            if (cube_intersect(ax->cubes[i], O, inv, t)) return 1;
    }
    return 0;
}

// castRay's hit record (kernel.cu:1376-1426) as the frame kernel's brute-force instantiation forms it
__device__ __forceinline__ rt_hit q_hit_record(const RtFrameConsts &fc, AuxPtr ax, const RtReflectDev &rd, V3 O, V3 D,
                                               float nt, int kind, int pos)
{
    rt_hit h{};
    h.t = nt;
    h.kind = kind;
    h.index = -1;
    if (kind < 0) return h;
    const V3 hp{O.x + D.x * nt, O.y + D.y * nt, O.z + D.z * nt};
    V3 normal{0.f, 0.f, 0.f}, new_org = hp;
    float tx = 0.5f, ty = 0.5f;
    if (kind == RT_HIT_TRIANGLE) {   // kernel.cu:1378-1393
        const int ti = ax->tri_idx[pos];
        const RtTriDev *tp = ax->tris + ti;
        float hnt, hnu = 0.f, hnv = 0.f;
        (void)tri_intersect(O, D, tp->p0, tp->p1, tp->p2, hnt, hnu, hnv);
        const float w0 = 1 - hnu - hnv;
        if (fc.flags & RT_FLAG_MESH_NORMALS) {
            normal = V3{(tp->vn[0] * w0 + tp->vn[3] * hnu) + tp->vn[6] * hnv,
                        (tp->vn[1] * w0 + tp->vn[4] * hnu) + tp->vn[7] * hnv,
                        (tp->vn[2] * w0 + tp->vn[5] * hnu) + tp->vn[8] * hnv};
            normalise_inplace(normal);
        } else {
            normal = V3{tp->n[0], tp->n[1], tp->n[2]};
        }
        tx = (w0 * tp->vt[0]) + (hnu * tp->vt[2]) + (hnv * tp->vt[4]);
        ty = (w0 * tp->vt[1]) + (hnu * tp->vt[3]) + (hnv * tp->vt[5]);
        new_org = V3{normal.x + hp.x, normal.y + hp.y, normal.z + hp.z};   // add(normal, add(Org, Dir * nt))
        h.index = ti;
        h.u = hnu;
        h.v = hnv;
    } else if (kind == RT_HIT_PLANE) {   // kernel.cu:1407-1416: the normal as stored
        const RtPlaneDev p = ax->planes[pos];
        normal = V3{p.nx, p.ny, p.nz};
        h.index = pos;
    } else {                             // sphere / cube, kernel.cu:1396-1405, 1418-1425
        V3 c;
        if (kind == RT_HIT_SPHERE) {
            const float4 s = rd.spheres[pos];
            c = V3{s.x, s.y, s.z};
        } else {
            const RtCubeDev cb = ax->cubes[pos];
            c = V3{cb.cx, cb.cy, cb.cz};
        }
        normal = V3{hp.x - c.x, hp.y - c.y, hp.z - c.z};
        normalise_inplace(normal);
        // the literals 1, 3.1415, 0.5 make these binary64 expressions (kernel.cu:1402-1403), as in the frame kernel
        tx = (float)((1.0 + rtm::div_by_3p1415((double)rtm::atan2f_rt(normal.z, normal.x))) * 0.5);
        ty = (float)rtm::div_by_3p1415((double)rtm::acosf_rt(normal.y));
        h.index = pos;
    }
    h.tx = tx;
    h.ty = ty;
    h.normal = rt_vec3{normal.x, normal.y, normal.z};
    h.new_org = rt_vec3{new_org.x, new_org.y, new_org.z};
    return h;
}

// rayTrace's pixel body at a hit (kernel.cu:1643-1679): texel, then the three-light sum with ShadowChain's samples
// (brute-force precision, as rf_shade) and the all-kinds any-hit. Every lane with a hit calls it.
__device__ __forceinline__ void q_shade_hit(const RtFrameConsts &fc, AuxPtr ax, const RtReflectDev &rd, const rt_hit &h,
                                            LdsStack stk, float &fr, float &fg, float &fb)
{
    int ci = f2i(h.ty * (float)fc.tex_h) * fc.tex_w + f2i(h.tx * (float)fc.tex_w);
    const int last = fc.tex_w * fc.tex_h - 1;
    ci = ci < 0 ? 0 : (ci > last ? last : ci);   // documented clamp (as the frame kernel)
    const float tr = fc.tex_r[ci], tg = fc.tex_g[ci], tb = fc.tex_b[ci];
    const V3 normal{h.normal.x, h.normal.y, h.normal.z};
    // start_O = normal * 0.00001 + new_org, kernel.cu:1647
    const V3 start{normal.x * 0.00001f + h.new_org.x, normal.y * 0.00001f + h.new_org.y, normal.z * 0.00001f + h.new_org.z};
    fr = fg = fb = 0.f;
    for (int li = 0; li < fc.n_lights; ++li) {
        const RtLightDev L = ax->lights[li];
        ShadowChain<0> chain;
        chain.begin(V3{L.px, L.py, L.pz}, start);
        int unshadowed = 0;
#pragma unroll 1
        for (int j = 0; j < RT_SHADOW_SAMPLES; ++j) {
            const V3 d = chain.direction(ax, false, L, start, j);
            if (!q_occluded(fc, ax, rd, start, d, stk)) unshadowed += 1;   // kernel.cu:1537-1539
        }
        float bsum = brightness_steps(unshadowed);
        const float a = dot3(normal, chain.toL);                          // kernel.cu:1541
        bsum = bsum * (a > 0.f ? a : 0.f);
        fr = fr + bsum * L.r * tr;                                        // kernel.cu:1673-1675
        fg = fg + bsum * L.g * tg;
        fb = fb + bsum * L.b * tb;
    }
}

// The texel q_shade_hit reads for h: its index expression and its documented clamp, restated for the callers that need
// the texel beside the shaded colour (the paths of rt_indirect.hip)
__device__ __forceinline__ void q_hit_texel(const RtFrameConsts &fc, const rt_hit &h, float &tr, float &tg, float &tb)
{
    int ci = f2i(h.ty * (float)fc.tex_h) * fc.tex_w + f2i(h.tx * (float)fc.tex_w);
    const int last = fc.tex_w * fc.tex_h - 1;
    ci = ci < 0 ? 0 : (ci > last ? last : ci);
    tr = fc.tex_r[ci]; tg = fc.tex_g[ci]; tb = fc.tex_b[ci];
}

}  // namespace
