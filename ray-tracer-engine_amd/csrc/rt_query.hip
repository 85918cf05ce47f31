// rt_query.hip -- ray queries (rt_scene_trace_rays, rt_scene_primary_rays).
//
// One thread per caller ray, 256-thread workgroups, the sphere BVH's traversal stack in LDS (rt_bvh.h):
//   NEAREST   castRay (kernel.cu:1287-1431) as the frame kernel evaluates it: mesh leaves behind their own boxes, then
//             the spheres (rf_cast: the lexicographic minimum of (t, index), which is the strict loop's result; it
//             replaces the mesh's hit only if its t is smaller), then cubes and planes with the strict `t < nt`;
//   OCCLUDED  castLightRay's per-sample any-hit over every kind of primitive (kernel.cu:1475-1536);
//   SHADE     rayTrace's pixel body (kernel.cu:1633-1690): the texel, then per light the frame kernel's ShadowChain at
//             brute-force precision with the all-kinds any-hit above; getFColor on a miss.
// Every primitive test is the frame kernel's own (rt_exact.h, rt_shadow.h); the spheres go through rt_bvh.h. The casts themselves
// (q_nearest, q_hit_record, q_occluded, q_shade_hit) are in rt_cast.h, shared with the whole-scene reflective passes.
// The brute-force variant (cull = 0) is the same kernels with the BVH replaced by the whole sphere list.
#include "rt_cast.h"

namespace {

struct RtQueryDev {                // a query's arguments (by value)
    const rt_ray *rays;
    int n;
    rt_hit *hits;
    int *occluded;
    float *rgba;
    uint32_t *packed;
};

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
