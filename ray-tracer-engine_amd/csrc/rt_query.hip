// rt_query.hip -- ray queries (rt_scene_trace_rays, rt_scene_primary_rays).
//
// One thread per caller ray, 256-thread workgroups, the sphere BVH's traversal stack in LDS (rt_bvh.h):
//   NEAREST   castRay (kernel.cu:1287-1431) as the frame kernel evaluates it: mesh leaves behind their own boxes, then
//             the spheres (rf_cast: the lexicographic minimum of (t, index), which is the strict loop's result; it
//             replaces the mesh's hit only if its t is smaller), then cubes and planes with the strict `t < nt`;
//   OCCLUDED  castLightRay's per-sample any-hit over every kind of primitive (kernel.cu:1475-1536);
//   SHADE     rayTrace's pixel body (kernel.cu:1633-1690): the texel, then per light the frame kernel's ShadowChain at
//             brute-force precision with the all-kinds any-hit above; getFColor on a miss.
// Every primitive test is the frame kernel's own (rt_trace.inc); the spheres go through rt_bvh.h. The brute-force
// variant (cull = 0) is the same kernels with the BVH replaced by the whole sphere list.
#include "rt_bvh.h"

namespace {

struct RtQueryDev {                // a query's arguments (by value)
    const rt_ray *rays;
    int n;
    rt_hit *hits;
    int *occluded;
    float *rgba;
    uint32_t *packed;
};

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

template <int MODE>
__global__ __launch_bounds__(RT_BVH_BLOCK) void rt_query_rays(const RtFrameConsts fc, const RtReflectDev rd,
                                                            const RtQueryDev q)
{
    __shared__ int stack_lds[RT_BVH_STACK * RT_BVH_BLOCK];
    const LdsStack stk{stack_lds, (int)threadIdx.x};
    const AuxPtr ax = (AuxPtr)(uintptr_t)fc.aux;
    const int i = (int)(blockIdx.x * RT_BVH_BLOCK + threadIdx.x);
    if (i >= q.n) return;
    const rt_ray r = q.rays[i];
    const V3 O{r.Org.x, r.Org.y, r.Org.z}, D{r.Dir.x, r.Dir.y, r.Dir.z};
    if (MODE == RT_QUERY_OCCLUDED) {
        q.occluded[i] = q_occluded(fc, ax, rd, O, D, stk);
        return;
    }
    int kind, pos;
    const float nt = q_nearest(fc, ax, rd, O, D, stk, kind, pos);
    const rt_hit h = q_hit_record(fc, ax, rd, O, D, nt, kind, pos);
    if (q.hits) q.hits[i] = h;
    if (MODE != RT_QUERY_SHADE) return;
    float fr, fg, fb;
    if (kind >= 0) q_shade_hit(fc, ax, rd, h, stk, fr, fg, fb);
    else rf_sky(ax, O, D, fr, fg, fb);
    // what the frame kernel stores at one sample: the sum over samples starts at 0, the weight is 1
    const float cr = 0.f + fr, cg = 0.f + fg, cb = 0.f + fb;
    if (q.rgba) reinterpret_cast<float4 *>(q.rgba)[i] = make_float4(cr, cg, cb, 1.f);
    if (q.packed) q.packed[i] = rgb_to_int(f2i(cr * 254.f), f2i(cg * 254.f), f2i(cb * 254.f));   // kernel.cu:1682
}

// The primary rays of the band, pixel pix at rays[pix]
__global__ __launch_bounds__(RT_BVH_BLOCK) void rt_query_primary(const RtFrameConsts fc, rt_ray *rays)
{
    const int npx = fc.width * fc.local_rows;
    const int pix = (int)(blockIdx.x * RT_BVH_BLOCK + threadIdx.x);
    if (pix >= npx) return;
    const V3 D = rf_primary_dir(fc, pix);
    rays[pix] = rt_ray{rt_vec3{fc.org_x, fc.org_y, fc.org_z}, rt_vec3{D.x, D.y, D.z}};
}

}  // namespace

int rt_query_launch(const RtFrameConsts *fc, const RtSphereBvh *bvh, const float4 *d_spheres, int n_spheres,
                    const rt_ray_query *q, hipStream_t stream)
{
    RtReflectDev rd{};
    rd.nodes = (bvh && bvh->ok) ? bvh->d_nodes.get() : nullptr;
    rd.lsph = bvh ? bvh->d_lsph.get() : nullptr;
    rd.order = bvh ? bvh->d_order.get() : nullptr;
    rd.spheres = d_spheres;
    rd.n = n_spheres;
    RtQueryDev qd{q->rays, q->n, q->hits, q->occluded, q->rgba, q->packed};
    const dim3 grid((unsigned)((q->n + RT_BVH_BLOCK - 1) / RT_BVH_BLOCK)), block(RT_BVH_BLOCK);
    if (q->mode == RT_QUERY_NEAREST) hipLaunchKernelGGL(rt_query_rays<RT_QUERY_NEAREST>, grid, block, 0, stream, *fc, rd, qd);
    else if (q->mode == RT_QUERY_OCCLUDED) hipLaunchKernelGGL(rt_query_rays<RT_QUERY_OCCLUDED>, grid, block, 0, stream, *fc, rd, qd);
    else hipLaunchKernelGGL(rt_query_rays<RT_QUERY_SHADE>, grid, block, 0, stream, *fc, rd, qd);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

int rt_query_launch_primary(const RtFrameConsts *fc, rt_ray *rays, hipStream_t stream)
{
    const int npx = fc->width * fc->local_rows;
    hipLaunchKernelGGL(rt_query_primary, dim3((unsigned)((npx + RT_BVH_BLOCK - 1) / RT_BVH_BLOCK)), dim3(RT_BVH_BLOCK), 0,
                       stream, *fc, rays);
    RT_HIP(hipGetLastError());
    return RT_OK;
}
