// rt_indirect.hip -- global illumination (rt_scene_indirect; rt_scene_indirect_paths, 6p): a hashed
// diffuse gather pass with a bounce budget.
//
// Every surface pixel of a frame's G-buffer casts `rays` cosine-distributed gather rays from its surface point; each
// is a diffuse path of at most `bounces` shaded hits. A hit is shaded exactly as a RT_QUERY_SHADE ray (rt_query.hip):
// direct light through the casts of rt_cast.h; a miss is getFColor and ends the path. Unless the budget is spent, a hit
// spawns the next ray with the hit's texel in its throughput. The mean of the paths times the pixel's albedo is added
// to the frame's colour. bounces == 1 is rt_scene_indirect: the path is the gather ray.
//
// Two implementations, the same bits:
//   plain       one thread per pixel, 256-thread workgroups: a loop over the rays, in it the loop over the bounces
//               (q_nearest, q_hit_record, then q_shade_hit or rf_sky), then the sum, the albedo and the outputs;
//   wavefront   per group of at most RT_INDIRECT_GROUP rays, in the shape of the reflective passes:
//     cast      over the group's (pixel, ray) slots: forms the ray and finds its nearest hit; a miss writes its sky
//               colour to the slot of a slab, a hit is appended to queue 0 (one atomic per wave);
//     shade     once per bounce b, a fixed grid over queue b, whose length it reads on the device: shades the entry,
//               adds the term to the entry's slot (one writer per slot and pass: the order of the sum is the order of
//               the launches) and -- unless b is the last -- forms the next ray and casts it: a miss adds throughput x
//               sky to the slot at once, a hit is appended to queue b + 1 with its throughput and key. Two buffers
//               ping-pong; a pass pushes at most one entry per entry it read, so no queue outgrows the group's slots;
//     resolve   per pixel: the earlier groups' running sum plus the group's slots in ascending ray order, and -- the
//               last group -- the mean, the albedo and the outputs. Dead pixels are written here.
//   No float atomics: the order of the sum is the slab's.
// Emissive surfaces (rt_scene_set_emission) are a template parameter of the two kernels that shade a hit,
// EMIT: the colour q_shade_hit gives a hit gets the hit primitive's table entry added (ind_emit). The tables are an
// argument of the EMIT = true instantiations alone, which the host launches only when some kind has a table: every
// other call runs the EMIT = false ones, with the arguments they had before emission existed.
// Which of the two rt_indirect_desc.variant 0 names is kIndirectWavefrontIsProduct (bounces == 1, the measurement of
// DESIGN.md 6o) or kIndirectPathsWavefrontIsProduct (bounces > 1, that of 6p) below. The brute-force variant (cull = 0)
// is the same kernels with the BVH replaced by the whole sphere list.
#include "rt_cast.h"

#include <algorithm>

#define RT_INDIRECT_BLOCK RT_BVH_BLOCK
#define RT_INDIRECT_GRID 2048    // workgroups of a shade launch at most (grid-stride over the queue)

// variant 0 runs the wavefront passes and variant 1 the plain kernel (true), or the other way round (false)
static const bool kIndirectWavefrontIsProduct = true;
// the same choice for calls with bounces > 1, by the measurement of DESIGN.md 6p
static const bool kIndirectPathsWavefrontIsProduct = true;

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

// key_b of a path from its key_0: key_{b+1} = mix(key_b ^ 0x426f756e)
__host__ __device__ __forceinline__ uint32_t rf_indirect_path_key(uint32_t key, int b)
{
    for (int i = 0; i < b; ++i) key = rf_mix(key ^ 0x426f756eu);
    return key;
}

namespace {

__device__ __forceinline__ bool ind_finite(float v) { return __builtin_fabsf(v) <= 3.4028234663852886e38f; }   // NaN: false

// Step 1 for pixel p, the one statement of the dead-pixel rule: false if it is dead; else `live` gets its depth and
// normal as the G-buffer holds them. (A continuation, not a flag handed back with the values: the rule stays one branch
// at the head of its caller, and the plain kernels keep their registers to the digit.)
template <class F>
__device__ __forceinline__ bool ind_if_live(const RtIndirectDev &d, int p, F live)
{
    const int kind = d.id[p].x;
    const float depth = d.depth[p];
    const float4 ng = d.normal[p];
    const float nn = (ng.x * ng.x + ng.y * ng.y) + ng.z * ng.z;
    if (kind < 0 || !ind_finite(depth) || nn == 0.f || !ind_finite(nn)) return false;
    live(depth, ng);
    return true;
}

// Steps 1 and 2 for pixel p: false if it is dead; else its normal and the start of its gather rays
__device__ __forceinline__ bool ind_pixel(const RtFrameConsts &fc, const RtIndirectDev &d, int p, V3 &n, V3 &start)
{
    return ind_if_live(d, p, [&](float depth, float4 ng) {
        const V3 D = rf_primary_dir(fc, p);
        const V3 P{fc.org_x + D.x * depth, fc.org_y + D.y * depth, fc.org_z + D.z * depth};
        n = V3{ng.x, ng.y, ng.z};
        rf_normalise(n);
        if ((n.x * D.x + n.y * D.y) + n.z * D.z > 0.f) n = V3{-n.x, -n.y, -n.z};
        start = V3{n.x * 0.00001f + P.x, n.y * 0.00001f + P.y, n.z * 0.00001f + P.z};
    });
}

// key_0 of the path that ray j (counted from the call's first) of pixel p starts
__device__ __forceinline__ uint32_t ind_ray_key(const RtFrameConsts &fc, const RtIndirectDev &d, int p, int j)
{
    const int y = p / fc.width, x = p - y * fc.width;
    return rf_gloss_key((uint32_t)x, (uint32_t)y, (uint32_t)(d.ray_base + j), d.seed);
}

// The direction of that ray: step 3 under its key
__device__ __forceinline__ V3 ind_ray_dir(const RtFrameConsts &fc, const RtIndirectDev &d, int p, int j, V3 n)
{
    V3 G;
    rf_indirect_dir(n, ind_ray_key(fc, d, p, j), G);
    return G;
}

// Step (g) of a path at the hit h of ray(O, D) under `key`: false if the hit's normal is dead; else O, D and key become
// the next ray's
__device__ __forceinline__ bool ind_next_ray(const rt_hit &h, V3 &O, V3 &D, uint32_t &key)
{
    V3 n{h.normal.x, h.normal.y, h.normal.z};
    const float nn = (n.x * n.x + n.y * n.y) + n.z * n.z;
    if (nn == 0.f || !ind_finite(nn)) return false;
    rf_normalise(n);
    if ((n.x * D.x + n.y * D.y) + n.z * D.z > 0.f) n = V3{-n.x, -n.y, -n.z};
    const V3 P{O.x + D.x * h.t, O.y + D.y * h.t, O.z + D.z * h.t};
    O = V3{n.x * 0.00001f + P.x, n.y * 0.00001f + P.y, n.z * 0.00001f + P.z};
    key = rf_indirect_path_key(key, 1);
    V3 G;
    rf_indirect_dir(n, key, G);
    D = G;
    return true;
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

// What a gather hit emits: h's colour plus the entry of its (kind, index) in its kind's table; a triangle
// and a kind without a table emit nothing. The kind differs from lane to lane: one 16-byte vector load. Without tables
// (the EMIT = false instantiations pass none) the colour is q_shade_hit's.
__device__ __forceinline__ void ind_emit(const rt_hit &, float &, float &, float &) {}
__device__ __forceinline__ void ind_emit(const rt_hit &h, float &fr, float &fg, float &fb, const RtEmitDev &em)
{
    const float4 *t = h.kind == RT_HIT_SPHERE ? em.sphere : (h.kind == RT_HIT_PLANE ? em.plane : (h.kind == RT_HIT_CUBE ? em.cube : nullptr));
    if (!t) return;
    const float4 e = t[h.index];
    fr = fr + e.x;
    fg = fg + e.y;
    fb = fb + e.z;
}

// The plain kernel: everything for pixel p in one thread, per ray the loop of DESIGN.md 6p. ONE: the budget is the
// constant 1 and the loop over the bounces a single trip (6o's sr = sr + (0.f + fr)). EMIT: `em` is the emission tables
// (one RtEmitDev; without EMIT no argument at all)
template <bool ONE, bool EMIT, class... Em>
__global__ __launch_bounds__(RT_INDIRECT_BLOCK) void rt_indirect_plain(const RtFrameConsts fc, const RtReflectDev rd,
                                                                     const RtIndirectDev d, int budget, const Em... em)
{
    static_assert(sizeof...(Em) == (EMIT ? 1 : 0), "the tables go to the EMIT instantiations alone");
    const int bounces = ONE ? 1 : budget;
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
        V3 O = start, D = ind_ray_dir(fc, d, p, j, n);
        uint32_t key = ind_ray_key(fc, d, p, j);
        float lr = 0.f, lg = 0.f, lb = 0.f, tr = 1.f, tg = 1.f, tb = 1.f;
#pragma unroll 1
        for (int b = 0;; ++b) {
            int kind, pos;
            const float nt = q_nearest(fc, ax, rd, O, D, stk, kind, pos);
            float fr, fg, fb;
            rt_hit h{};
            if (kind >= 0) {
                h = q_hit_record(fc, ax, rd, O, D, nt, kind, pos);
                q_shade_hit(fc, ax, rd, h, stk, fr, fg, fb);
                ind_emit(h, fr, fg, fb, em...);
            } else {
                rf_sky(ax, O, D, fr, fg, fb);
            }
            if (b == 0) {
                lr = 0.f + fr; lg = 0.f + fg; lb = 0.f + fb;
            } else {
                lr = lr + tr * fr; lg = lg + tg * fg; lb = lb + tb * fb;
            }
            if (kind < 0 || b == bounces - 1) break;
            float ar, ag, ab;
            q_hit_texel(fc, h, ar, ag, ab);
            if (b == 0) {
                tr = ar; tg = ag; tb = ab;
            } else {
                tr = tr * ar; tg = tg * ag; tb = tb * ab;
            }
            if (!ind_next_ray(h, O, D, key)) break;
        }
        sr = sr + lr;
        sg = sg + lg;
        sb = sb + lb;
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
    const int at = rf_wave_append(push, count);   // (every lane of the wave is here)
    if (push) {
        float4 *e = queue + (size_t)RT_INDIRECT_ENTRY_F4 * (size_t)at;
        e[0] = make_float4(start.x, start.y, start.z, nt);
        e[1] = make_float4(G.x, G.y, G.z, __int_as_float(kind));
        e[2] = make_float4(__int_as_float(pos), __int_as_float(i), 0.f, 0.f);
    }
}

// The shade pass of bounce b over queue b: a fixed grid, the queue's length read here, on the device.
// FIRST: b == 0, the entries are the cast pass's (no throughput; the key is the slot's); LAST: b == bounces - 1, nothing
// continues (q_out and count_out are null). <true, true> is the shade pass of DESIGN.md 6o. Every lane of a wave makes
// every trip of the loop (its bounds are uniform) and reaches rf_wave_append: a lane without an entry is inactive by
// `act`, never by leaving. EMIT: as the plain kernel's.
template <bool FIRST, bool LAST, bool EMIT, class... Em>
__global__ __launch_bounds__(RT_INDIRECT_BLOCK) void rt_indirect_shade(const RtFrameConsts fc, const RtReflectDev rd,
                                                                     const RtIndirectDev d, int j0, const float4 *q_in,
                                                                     const int *count_in, float4 *q_out, int *count_out,
                                                                     float4 *slab, const Em... em)
{
    static_assert(sizeof...(Em) == (EMIT ? 1 : 0), "the tables go to the EMIT instantiations alone");
    __shared__ int stack_lds[RT_BVH_STACK * RT_INDIRECT_BLOCK];
    const LdsStack stk{stack_lds, (int)threadIdx.x};
    const AuxPtr ax = (AuxPtr)(uintptr_t)fc.aux;
    const int n_in = *count_in;
    constexpr int kIn = FIRST ? RT_INDIRECT_ENTRY_F4 : RT_INDIRECT_PATH_ENTRY_F4;
    for (int base = (int)blockIdx.x * RT_INDIRECT_BLOCK; base < n_in; base += (int)gridDim.x * RT_INDIRECT_BLOCK) {
        const int i = base + (int)threadIdx.x;
        const bool act = i < n_in;
        bool push = false;
        V3 O{0.f, 0.f, 0.f}, D{0.f, 0.f, 0.f};
        float nt = 0.f, tr = 0.f, tg = 0.f, tb = 0.f;
        int kind = -1, pos = -1, slot = 0;
        uint32_t key = 0;
        if (act) {
            const float4 *e = q_in + (size_t)kIn * (size_t)i;
            const float4 e0 = e[0], e1 = e[1], e2 = e[2];
            O = V3{e0.x, e0.y, e0.z};
            D = V3{e1.x, e1.y, e1.z};
            slot = __float_as_int(e2.y);
            const rt_hit h = q_hit_record(fc, ax, rd, O, D, e0.w, __float_as_int(e1.w), __float_as_int(e2.x));
            float fr, fg, fb;
            q_shade_hit(fc, ax, rd, h, stk, fr, fg, fb);
            ind_emit(h, fr, fg, fb, em...);
            float lr, lg, lb;
            if (FIRST) {
                lr = 0.f + fr; lg = 0.f + fg; lb = 0.f + fb;
                const int npx = fc.width * fc.height, j = slot / npx;
                key = ind_ray_key(fc, d, slot - j * npx, j0 + j);
            } else {
                const float4 e3 = e[3], s = slab[slot];
                tr = e3.x; tg = e3.y; tb = e3.z;
                key = (uint32_t)__float_as_int(e3.w);
                lr = s.x + tr * fr; lg = s.y + tg * fg; lb = s.z + tb * fb;
            }
            if (!LAST) {
                float ar, ag, ab;
                q_hit_texel(fc, h, ar, ag, ab);
                if (FIRST) {
                    tr = ar; tg = ag; tb = ab;
                } else {
                    tr = tr * ar; tg = tg * ag; tb = tb * ab;
                }
                if (ind_next_ray(h, O, D, key)) {
                    nt = q_nearest(fc, ax, rd, O, D, stk, kind, pos);
                    if (kind >= 0) {
                        push = true;
                    } else {   // the next bounce's miss, at once
                        rf_sky(ax, O, D, fr, fg, fb);
                        lr = lr + tr * fr; lg = lg + tg * fg; lb = lb + tb * fb;
                    }
                }
            }
            slab[slot] = make_float4(lr, lg, lb, 0.f);
        }
        if (!LAST) {   // append the wave's continuing paths
            const int at = rf_wave_append(push, count_out);
            if (push) {
                float4 *o = q_out + (size_t)RT_INDIRECT_PATH_ENTRY_F4 * (size_t)at;
                o[0] = make_float4(O.x, O.y, O.z, nt);
                o[1] = make_float4(D.x, D.y, D.z, __int_as_float(kind));
                o[2] = make_float4(__int_as_float(pos), __int_as_float(slot), 0.f, 0.f);
                o[3] = make_float4(tr, tg, tb, __int_as_float((int)key));
            }
        }
    }
}

// The resolve pass of a group of g rays, one thread per pixel: S = (the earlier groups' sum, or +0) + the pixel's g
// slots in ascending ray order. Not the last group: S goes to `sum`. The last group: steps 4 to 6, and the dead pixels.
__global__ __launch_bounds__(RT_INDIRECT_BLOCK) void rt_indirect_resolve(const RtIndirectDev d, int npx, int g,
                                                                       const float4 *slab, float4 *sum, int first, int last)
{
    const int p = (int)(blockIdx.x * RT_INDIRECT_BLOCK + threadIdx.x);
    if (p >= npx) return;
    if (!ind_if_live(d, p, [](float, float4) {})) {
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
int rt_indirect_launch(const rt_indirect_desc *d, int bounces, const RtFrameConsts *fc, const RtSphereBvh *bvh,
                       const float4 *d_spheres, int n_spheres, const RtEmitDev *emit, const RtIndirectScratch *scratch,
                       hipEvent_t *ev, int *n_ev, hipStream_t stream)
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
    if (!rt_indirect_wavefront(d->variant, bounces)) {
        if (emit) {
            const auto plain = bounces == 1 ? rt_indirect_plain<true, true, RtEmitDev> : rt_indirect_plain<false, true, RtEmitDev>;
            hipLaunchKernelGGL(plain, px_grid, block, 0, stream, *fc, rd, dd, bounces, *emit);
        } else {
            const auto plain = bounces == 1 ? rt_indirect_plain<true, false> : rt_indirect_plain<false, false>;
            hipLaunchKernelGGL(plain, px_grid, block, 0, stream, *fc, rd, dd, bounces);
        }
        RT_HIP(hipGetLastError());
        RT_HIP(mark());
        *n_ev = marks;
        return RT_OK;
    }
    const int groups = (d->rays + RT_INDIRECT_GROUP - 1) / RT_INDIRECT_GROUP;
    RT_HIP(hipMemsetAsync(scratch->count, 0, sizeof(int) * (size_t)groups * (size_t)bounces, stream));
    for (int gi = 0; gi < groups; ++gi) {
        const int j0 = gi * RT_INDIRECT_GROUP, g = std::min(RT_INDIRECT_GROUP, d->rays - j0);
        const unsigned slot_blocks = (unsigned)(((long long)g * npx + RT_INDIRECT_BLOCK - 1) / RT_INDIRECT_BLOCK);
        int *count = scratch->count + gi * bounces;   // one per bounce
        const dim3 shade_grid(std::min<unsigned>(RT_INDIRECT_GRID, slot_blocks));
        hipLaunchKernelGGL(rt_indirect_cast, dim3(slot_blocks), block, 0, stream, *fc, rd, dd, j0, g, scratch->slab,
                           scratch->queue, count);
        RT_HIP(hipGetLastError());
        RT_HIP(mark());
        for (int b = 0; b < bounces; ++b) {   // queue b -> queue b + 1: the two buffers in turn
            const bool first = b == 0, last = b == bounces - 1;
            const float4 *q_in = (b & 1) ? scratch->queue2 : scratch->queue;
            float4 *q_out = last ? nullptr : (b & 1) ? scratch->queue : scratch->queue2;
            int *const count_out = last ? nullptr : count + b + 1;
            if (emit) {
                const auto shade = first ? (last ? rt_indirect_shade<true, true, true, RtEmitDev> : rt_indirect_shade<true, false, true, RtEmitDev>)
                                         : (last ? rt_indirect_shade<false, true, true, RtEmitDev> : rt_indirect_shade<false, false, true, RtEmitDev>);
                hipLaunchKernelGGL(shade, shade_grid, block, 0, stream, *fc, rd, dd, j0, q_in, count + b, q_out, count_out,
                                   scratch->slab, *emit);
            } else {
                const auto shade = first ? (last ? rt_indirect_shade<true, true, false> : rt_indirect_shade<true, false, false>)
                                         : (last ? rt_indirect_shade<false, true, false> : rt_indirect_shade<false, false, false>);
                hipLaunchKernelGGL(shade, shade_grid, block, 0, stream, *fc, rd, dd, j0, q_in, count + b, q_out, count_out,
                                   scratch->slab);
            }
            RT_HIP(hipGetLastError());
            RT_HIP(mark());
        }
        hipLaunchKernelGGL(rt_indirect_resolve, px_grid, block, 0, stream, dd, npx, g, scratch->slab, scratch->sum,
                           gi == 0 ? 1 : 0, gi == groups - 1 ? 1 : 0);
        RT_HIP(hipGetLastError());
        RT_HIP(mark());
    }
    *n_ev = marks;
    return RT_OK;
}

bool rt_indirect_wavefront(int variant, int bounces)
{
    return (variant == 0) == (bounces > 1 ? kIndirectPathsWavefrontIsProduct : kIndirectWavefrontIsProduct);
}

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

extern "C" int rt_debug_indirect_path_key(const unsigned *key, int count, int b, unsigned *out)
{
    if (!key || !out || count < 0 || b < 0) {
        rt_set_error("rt_debug_indirect_path_key: invalid argument");
        return RT_ERR_INVALID;
    }
    for (int i = 0; i < count; ++i) out[i] = rf_indirect_path_key(key[i], b);
    return RT_OK;
}
