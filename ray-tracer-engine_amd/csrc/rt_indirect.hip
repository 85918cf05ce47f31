// rt_indirect.hip -- one-bounce global illumination (rt_scene_indirect): a hashed diffuse gather pass.
//
// Every surface pixel of a frame's G-buffer casts `rays` cosine-distributed gather rays from its surface point; each
// is shaded exactly as a RT_QUERY_SHADE ray (rt_query.hip): direct light at what it hits through the casts of
// rt_cast.h, getFColor on a miss. Their mean times the pixel's albedo is added to the frame's colour.
//
// Two implementations, the same bits:
//   plain       one thread per pixel, 256-thread workgroups, loops over the rays: q_nearest, q_hit_record, then
//               q_shade_hit or rf_sky, and the sum, the albedo and the outputs in the same thread;
//   wavefront   per group of at most RT_INDIRECT_GROUP rays three passes in the shape of the reflective passes:
//     cast      over the group's (pixel, ray) slots: forms the ray and finds its nearest hit; a miss writes its sky
//               colour to the slot of a slab, a hit is ballot-compacted into a queue (one atomic per wave);
//     shade     a fixed grid over the queue, whose length it reads on the device: full waves of hits, each shaded and
//               written to its slot;
//     resolve   per pixel: the earlier groups' running sum plus the group's slots in ascending ray order, and -- the
//               last group -- the mean, the albedo and the outputs. Dead pixels are written here.
//   No float atomics: the order of the sum is the slab's. The queue holds as many entries as the group has slots.
// Which of the two rt_indirect_desc.variant 0 names is kIndirectWavefrontIsProduct below, by the measurement of
// DESIGN.md 6o. The brute-force variant (cull = 0) is the same kernels with the BVH replaced by the whole sphere list.
#include "rt_cast.h"

#include <algorithm>

#define RT_INDIRECT_BLOCK RT_BVH_BLOCK
#define RT_INDIRECT_GRID 2048    // workgroups of a shade launch at most (grid-stride over the queue)

// variant 0 runs the wavefront passes and variant 1 the plain kernel (true), or the other way round (false)
static const bool kIndirectWavefrontIsProduct = true;

struct RtIndirectDev {             // a call's arguments (by value)
    const float *depth;
    const float4 *normal;
    const int2 *id;
    const float4 *albedo;
    const float4 *rgba_in;
    float4 *rgba_out;
    uint32_t *pixels;
    int rays, ray_base;
    uint32_t seed;
    float strength;
};

// Step 3's direction for a pixel normal n (as step 2 leaves it) under `key`: a point u of the unit sphere by
// Marsaglia's method from at most six pairs of draws, G = normalise(n + u), n itself unless dot(G, n) > 0.
// Returns the pairs drawn until one qualified (1 .. 6), 0 when none did (u = 0).
__host__ __device__ __forceinline__ int rf_indirect_dir(V3 n, uint32_t key, V3 &G)
{
    const uint32_t kg = rf_mix(key ^ 0x47497261u);
    float ux = 0.f, uy = 0.f, uz = 0.f;
    int tries = 0;
#pragma unroll 1
    for (uint32_t t = 0; t < 6u; ++t) {
        const float x1 = (float)(rf_mix(kg + 0x9e3779b9u * (t * 2u + 1u)) >> 8) * 1.1920928955078125e-07f - 1.f;   // 2^-23
        const float x2 = (float)(rf_mix(kg + 0x9e3779b9u * (t * 2u + 2u)) >> 8) * 1.1920928955078125e-07f - 1.f;
        const float s = x1 * x1 + x2 * x2;
        if (s < 1.f) {
            const float r = __builtin_sqrtf(1.f - s);
            ux = (2.f * x1) * r;
            uy = (2.f * x2) * r;
            uz = 1.f - 2.f * s;
            tries = (int)t + 1;
            break;
        }
    }
    G = V3{n.x + ux, n.y + uy, n.z + uz};
    rf_normalise(G);
    if (!((G.x * n.x + G.y * n.y) + G.z * n.z > 0.f)) G = n;
    return tries;
}

namespace {

__device__ __forceinline__ bool ind_finite(float v) { return __builtin_fabsf(v) <= 3.4028234663852886e38f; }   // NaN: false

// Steps 1 and 2 for pixel p: false if it is dead; else its normal and the start of its gather rays
__device__ __forceinline__ bool ind_pixel(const RtFrameConsts &fc, const RtIndirectDev &d, int p, V3 &n, V3 &start)
{
    const int kind = d.id[p].x;
    const float depth = d.depth[p];
    const float4 ng = d.normal[p];
    const float nn = (ng.x * ng.x + ng.y * ng.y) + ng.z * ng.z;
    if (kind < 0 || !ind_finite(depth) || nn == 0.f || !ind_finite(nn)) return false;
    const V3 D = rf_primary_dir(fc, p);
    const V3 P{fc.org_x + D.x * depth, fc.org_y + D.y * depth, fc.org_z + D.z * depth};
    n = V3{ng.x, ng.y, ng.z};
    rf_normalise(n);
    if ((n.x * D.x + n.y * D.y) + n.z * D.z > 0.f) n = V3{-n.x, -n.y, -n.z};
    start = V3{n.x * 0.00001f + P.x, n.y * 0.00001f + P.y, n.z * 0.00001f + P.z};
    return true;
}

// The direction of ray j (counted from the call's first) of pixel p
__device__ __forceinline__ V3 ind_ray_dir(const RtFrameConsts &fc, const RtIndirectDev &d, int p, int j, V3 n)
{
    const int y = p / fc.width, x = p - y * fc.width;
    V3 G;
    rf_indirect_dir(n, rf_gloss_key((uint32_t)x, (uint32_t)y, (uint32_t)(d.ray_base + j), d.seed), G);
    return G;
}

__device__ __forceinline__ void ind_store(const RtIndirectDev &d, int p, float4 c)
{
    d.rgba_out[p] = c;
    if (d.pixels) d.pixels[p] = rgb_to_int(f2i(c.x * 254.f), f2i(c.y * 254.f), f2i(c.z * 254.f));
}

// A dead pixel's outputs (step 1)
__device__ __forceinline__ void ind_store_dead(const RtIndirectDev &d, int p)
{
    ind_store(d, p, d.rgba_in ? d.rgba_in[p] : make_float4(0.f, 0.f, 0.f, 1.f));
}

// Steps 4 to 6 for a live pixel whose sum over the call's rays is S
__device__ __forceinline__ void ind_finish(const RtIndirectDev &d, int p, float sr, float sg, float sb)
{
    const float nr = (float)d.rays;
    float ir = d.strength * (sr / nr), ig = d.strength * (sg / nr), ib = d.strength * (sb / nr);
    if (d.albedo) {
        const float4 a = d.albedo[p];
        ir = ir * a.x;
        ig = ig * a.y;
        ib = ib * a.z;
    }
    float4 c = make_float4(ir, ig, ib, 1.f);
    if (d.rgba_in) {
        const float4 in = d.rgba_in[p];
        c = make_float4(in.x + ir, in.y + ig, in.z + ib, in.w);
    }
    ind_store(d, p, c);
}

// The plain kernel: everything for pixel p in one thread
__global__ __launch_bounds__(RT_INDIRECT_BLOCK) void rt_indirect_plain(const RtFrameConsts fc, const RtReflectDev rd,
                                                                     const RtIndirectDev d)
{
    __shared__ int stack_lds[RT_BVH_STACK * RT_INDIRECT_BLOCK];
    const LdsStack stk{stack_lds, (int)threadIdx.x};
    const AuxPtr ax = (AuxPtr)(uintptr_t)fc.aux;
    const int p = (int)(blockIdx.x * RT_INDIRECT_BLOCK + threadIdx.x);
    if (p >= fc.width * fc.height) return;
    V3 n, start;
    if (!ind_pixel(fc, d, p, n, start)) {
        ind_store_dead(d, p);
        return;
    }
    float sr = 0.f, sg = 0.f, sb = 0.f;
#pragma unroll 1
    for (int j = 0; j < d.rays; ++j) {
        const V3 G = ind_ray_dir(fc, d, p, j, n);
        int kind, pos;
        const float nt = q_nearest(fc, ax, rd, start, G, stk, kind, pos);
        float fr, fg, fb;
        if (kind >= 0) {
            const rt_hit h = q_hit_record(fc, ax, rd, start, G, nt, kind, pos);
            q_shade_hit(fc, ax, rd, h, stk, fr, fg, fb);
        } else {
            rf_sky(ax, start, G, fr, fg, fb);
        }
        sr = sr + (0.f + fr);   // (what RT_QUERY_SHADE stores for the ray: the sum over one sample starts at 0)
        sg = sg + (0.f + fg);
        sb = sb + (0.f + fb);
    }
    ind_finish(d, p, sr, sg, sb);
}

// The cast pass of a group of g rays, the first of them ray j0 of the call: thread i is pixel i % npx at ray
// j0 + i / npx, and slot i of the slab and of the queue's index space
__global__ __launch_bounds__(RT_INDIRECT_BLOCK) void rt_indirect_cast(const RtFrameConsts fc, const RtReflectDev rd,
                                                                    const RtIndirectDev d, int j0, int g, float4 *slab,
                                                                    float4 *queue, int *count)
{
    __shared__ int stack_lds[RT_BVH_STACK * RT_INDIRECT_BLOCK];
    const LdsStack stk{stack_lds, (int)threadIdx.x};
    const AuxPtr ax = (AuxPtr)(uintptr_t)fc.aux;
    const int npx = fc.width * fc.height;
    const int i = (int)(blockIdx.x * RT_INDIRECT_BLOCK + threadIdx.x);   // (the host has checked that g * npx fits an int)
    bool push = false;
    V3 start{0.f, 0.f, 0.f}, G{0.f, 0.f, 0.f};
    float nt = 0.f;
    int kind = -1, pos = -1;
    if (i < g * npx) {
        const int j = i / npx, p = i - j * npx;
        V3 n;
        if (ind_pixel(fc, d, p, n, start)) {
            G = ind_ray_dir(fc, d, p, j0 + j, n);
            nt = q_nearest(fc, ax, rd, start, G, stk, kind, pos);
            if (kind >= 0) {
                push = true;
            } else {
                float fr, fg, fb;
                rf_sky(ax, start, G, fr, fg, fb);
                slab[i] = make_float4(0.f + fr, 0.f + fg, 0.f + fb, 0.f);
            }
        }
    }
    // append the wave's hits (one atomic per wave; every lane of the wave is here)
    const lmask m = ballot64(push);
    if (m == 0) return;
    const int leader = __builtin_ctzll(m);
    int b = 0;
    if ((int)(threadIdx.x & 63u) == leader) b = atomicAdd(count, __popcll(m));
    const int base = __builtin_amdgcn_readlane(b, leader);
    if (push) {
        float4 *e = queue + (size_t)RT_INDIRECT_ENTRY_F4 * (size_t)(base + lane_prefix(m));
        e[0] = make_float4(start.x, start.y, start.z, nt);
        e[1] = make_float4(G.x, G.y, G.z, __int_as_float(kind));
        e[2] = make_float4(__int_as_float(pos), __int_as_float(i), 0.f, 0.f);
    }
}

// The shade pass: a fixed grid walks the queue, whose length is read here, on the device
__global__ __launch_bounds__(RT_INDIRECT_BLOCK) void rt_indirect_shade(const RtFrameConsts fc, const RtReflectDev rd,
                                                                     const float4 *queue, const int *count, float4 *slab)
{
    __shared__ int stack_lds[RT_BVH_STACK * RT_INDIRECT_BLOCK];
    const LdsStack stk{stack_lds, (int)threadIdx.x};
    const AuxPtr ax = (AuxPtr)(uintptr_t)fc.aux;
    const int n_in = *count;
    for (int base = (int)blockIdx.x * RT_INDIRECT_BLOCK; base < n_in; base += (int)gridDim.x * RT_INDIRECT_BLOCK) {
        const int i = base + (int)threadIdx.x;
        if (i >= n_in) continue;
        const float4 *e = queue + (size_t)RT_INDIRECT_ENTRY_F4 * (size_t)i;
        const float4 e0 = e[0], e1 = e[1], e2 = e[2];
        const V3 O{e0.x, e0.y, e0.z}, D{e1.x, e1.y, e1.z};
        const rt_hit h = q_hit_record(fc, ax, rd, O, D, e0.w, __float_as_int(e1.w), __float_as_int(e2.x));
        float fr, fg, fb;
        q_shade_hit(fc, ax, rd, h, stk, fr, fg, fb);
        slab[__float_as_int(e2.y)] = make_float4(0.f + fr, 0.f + fg, 0.f + fb, 0.f);
    }
}

// The resolve pass of a group of g rays, one thread per pixel: S = (the earlier groups' sum, or +0) + the pixel's g
// slots in ascending ray order. Not the last group: S goes to `sum`. The last group: steps 4 to 6, and the dead pixels.
__global__ __launch_bounds__(RT_INDIRECT_BLOCK) void rt_indirect_resolve(const RtIndirectDev d, int npx, int g,
                                                                       const float4 *slab, float4 *sum, int first, int last)
{
    const int p = (int)(blockIdx.x * RT_INDIRECT_BLOCK + threadIdx.x);
    if (p >= npx) return;
    const float depth = d.depth[p];
    const float4 ng = d.normal[p];
    const float nn = (ng.x * ng.x + ng.y * ng.y) + ng.z * ng.z;
    if (d.id[p].x < 0 || !ind_finite(depth) || nn == 0.f || !ind_finite(nn)) {   // dead, as ind_pixel
        if (last) ind_store_dead(d, p);
        return;
    }
    float sr = 0.f, sg = 0.f, sb = 0.f;
    if (!first) {
        const float4 s = sum[p];
        sr = s.x; sg = s.y; sb = s.z;
    }
    for (int j = 0; j < g; ++j) {
        const float4 c = slab[(size_t)j * (size_t)npx + (size_t)p];
        sr = sr + c.x;
        sg = sg + c.y;
        sb = sb + c.z;
    }
    if (!last) {
        sum[p] = make_float4(sr, sg, sb, 0.f);
        return;
    }
    ind_finish(d, p, sr, sg, sb);
}

}  // namespace

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
int rt_indirect_launch(const rt_indirect_desc *d, const RtFrameConsts *fc, const RtSphereBvh *bvh, const float4 *d_spheres,
                       int n_spheres, const RtIndirectScratch *scratch, hipEvent_t *ev, int *n_ev, hipStream_t stream)
{
    RtReflectDev rd{};
    rd.nodes = (bvh && bvh->ok) ? bvh->d_nodes.get() : nullptr;
    rd.lsph = bvh ? bvh->d_lsph.get() : nullptr;
    rd.order = bvh ? bvh->d_order.get() : nullptr;
    rd.spheres = d_spheres;
    rd.n = n_spheres;
    const RtIndirectDev dd{d->depth, reinterpret_cast<const float4 *>(d->normal), reinterpret_cast<const int2 *>(d->id),
                           reinterpret_cast<const float4 *>(d->albedo), reinterpret_cast<const float4 *>(d->rgba_in),
                           reinterpret_cast<float4 *>(d->rgba_out), d->pixels, d->rays, d->ray_base, d->seed, d->strength};
    const int npx = fc->width * fc->height;
    const dim3 block(RT_INDIRECT_BLOCK), px_grid((unsigned)((npx + RT_INDIRECT_BLOCK - 1) / RT_INDIRECT_BLOCK));
    int marks = 0;
    auto mark = [&]() -> hipError_t {
        if (!ev) return hipSuccess;
        return hipEventRecord(ev[marks++], stream);
    };
    *n_ev = 0;
    RT_HIP(mark());
    if (!rt_indirect_wavefront(d->variant)) {
        hipLaunchKernelGGL(rt_indirect_plain, px_grid, block, 0, stream, *fc, rd, dd);
        RT_HIP(hipGetLastError());
        RT_HIP(mark());
        *n_ev = marks;
        return RT_OK;
    }
    const int groups = (d->rays + RT_INDIRECT_GROUP - 1) / RT_INDIRECT_GROUP;
    RT_HIP(hipMemsetAsync(scratch->count, 0, sizeof(int) * (size_t)groups, stream));
    for (int gi = 0; gi < groups; ++gi) {
        const int j0 = gi * RT_INDIRECT_GROUP, g = std::min(RT_INDIRECT_GROUP, d->rays - j0);
        const unsigned slot_blocks = (unsigned)(((long long)g * npx + RT_INDIRECT_BLOCK - 1) / RT_INDIRECT_BLOCK);
        hipLaunchKernelGGL(rt_indirect_cast, dim3(slot_blocks), block, 0, stream, *fc, rd, dd, j0, g, scratch->slab,
                           scratch->queue, scratch->count + gi);
        RT_HIP(hipGetLastError());
        RT_HIP(mark());
        hipLaunchKernelGGL(rt_indirect_shade, dim3(std::min<unsigned>(RT_INDIRECT_GRID, slot_blocks)), block, 0, stream, *fc,
                           rd, scratch->queue, scratch->count + gi, scratch->slab);
        RT_HIP(hipGetLastError());
        RT_HIP(mark());
        hipLaunchKernelGGL(rt_indirect_resolve, px_grid, block, 0, stream, dd, npx, g, scratch->slab, scratch->sum,
                           gi == 0 ? 1 : 0, gi == groups - 1 ? 1 : 0);
        RT_HIP(hipGetLastError());
        RT_HIP(mark());
    }
    *n_ev = marks;
    return RT_OK;
}

bool rt_indirect_wavefront(int variant) { return (variant == 0) == kIndirectWavefrontIsProduct; }

// ---------------------------------------------------------------------------
// host-only debug entry (tests)
// ---------------------------------------------------------------------------
extern "C" int rt_debug_indirect_dir(const rt_vec3 *n, const unsigned *key, int count, rt_vec3 *G, int *tries)
{
    if (!n || !key || !G || count < 0) {
        rt_set_error("rt_debug_indirect_dir: invalid argument");
        return RT_ERR_INVALID;
    }
    for (int i = 0; i < count; ++i) {
        V3 o;
        const int t = rf_indirect_dir(V3{n[i].x, n[i].y, n[i].z}, key[i], o);
        G[i].x = o.x; G[i].y = o.y; G[i].z = o.z;
        if (tries) tries[i] = t;
    }
    return RT_OK;
}
