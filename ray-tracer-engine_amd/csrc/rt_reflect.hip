// rt_reflect.hip -- mirror reflections off spheres (rt_launch_opts.reflect_depth, DESIGN.md "Reflections").
//
// A reflective frame runs the frame kernel (rt_trace.inc) as it is, into rgba: that gives every pixel its primary
// term -- the three-light sum L of its primary hit, or its sky texel. Then, on the same stream and without a host wait:
//   primary   casts every pixel's primary ray again (nearest hit through the sphere BVH) and ballot-compacts the
//             pixels whose hit sphere has k = reflectivness > 0 into a queue: {pixel, R_1, w = k, c = (1-k) * L};
//   bounce b  (b = 1..D, one launch each, a fixed grid that reads the queue length on the device): nearest hit of
//             R_b through the BVH; a miss adds w * sky; a hit is shaded as the frame kernel shades one (texel, ten
//             shadow samples per light from the frame kernel's own ShadowChain, any-hit tests through the BVH) and
//             either adds w * L and ends (k = 0 or b = D) or adds (w * (1-k)) * L and queues R_{b+1} with w * k.
//             A pixel that ends writes rgba = (c, 1) and its packed word there and then: the pixels that never
//             entered the queue keep what the frame kernel wrote.
// Glass (transperancy tau > 0, DESIGN.md "Refraction") is one more kind of continuation: the term is (w * (1-tau)) * L,
// w becomes w * tau and R_{b+1} is the ray that passed through the sphere (rf_transmit). Both passes are templates on
// GLASS; the host launches GLASS = true only when some sphere has tau > 0, so mirror-only frames run today's code.
// The brute-force variant (opts.cull = 0) is the same kernels with the BVH replaced by the whole sphere list.
// Whole scenes (rt_scene_set_reflect_scope(RT_REFLECT_SCENE)) are a second template parameter, KINDS:
// the nearest hit is castRay over every kind of primitive (q_nearest), the hit frame is castRay's record for that kind
// (q_hit_record), k comes from the hit primitive's table (a triangle has k = 0) and L is shaded with castLightRay's
// any-hit over every kind (q_shade_hit) -- the ray queries' own functions. The host launches KINDS = true only when
// the scope is the scene and the scene holds a plane, a cube or a mesh: every other frame runs today's code.
//
// Supersampled frames (rt_scene_set_reflect_samples(RT_REFLECT_SAMPLES_MANY)) run the same passes over
// groups of at most RT_REFLECT_SAMPLE_GROUP samples: the frame kernel once per sample into a slab of a scene-owned
// [G][npx] buffer, the primary pass's SAMPLES = true instantiation over all G * npx pixel-samples (a queue entry's `pix`
// is then the slab index), the bounces as they are with the slab as their rgba, and rt_reflect_resolve, which sums a
// pixel's slab entries in ascending sample order and is the only pass that touches the caller's outputs.
//
// Glossy reflections (rt_scene_set_roughness) are a last template parameter, GLOSS: the mirror continuation
// of a hit whose roughness is > 0 is rf_gloss's -- the mirror direction plus roughness times a point of the unit ball,
// drawn by an integer hash of the pixel, the sample, the hit's index and the scene's seed, renormalised. The primary
// pass forms the pixel-sample's key and the queue entry carries it. The host launches GLOSS = true only when a
// roughness table the frame reads holds a value > 0: every other frame runs today's code.
//
// Fresnel glass (rt_scene_set_glass_model(RT_GLASS_FRESNEL)) is a template parameter of its own, FRESNEL: a
// glass hit is reflected with probability rf_fresnel and transmitted otherwise, by one more draw of the same key, and
// roughness on a glass sphere perturbs whichever ray it takes (rf_fresnel_continue). The host launches FRESNEL = true
// (with GLASS and GLOSS, for the key) only under that model in a frame with glass: every other frame runs today's code.
//
// The BVH and the per-ray pieces the ray queries share are in rt_bvh.h, the BVH's host build and its debug entries in
// rt_sphere_bvh.cpp, the all-kinds casts in rt_cast.h.
#include "rt_cast.h"

#include <algorithm>
#include <cstring>
#include <vector>

#define RT_REFLECT_BLOCK RT_BVH_BLOCK
#define RT_BOUNCE_GRID 2048    // workgroups of a bounce launch (grid-stride over the queue)
#define RT_REFLECT_SAMPLE_GROUP 4   // samples of a supersampled frame that share one run of the passes (bounds the scratch)
#define RT_REFLECT_MAX_GROUPS ((RT_MAX_SPP + RT_REFLECT_SAMPLE_GROUP - 1) / RT_REFLECT_SAMPLE_GROUP)

struct QEntry {    // one queued ray: 48 bytes
    float ox, oy, oz, dx, dy, dz;
    float w, cr, cg, cb;
    int pix;       // band-local pixel index (a supersampled frame: sample slot * band pixels + that)
    int pad_;      // GLOSS: the pixel-sample's key (rf_gloss_key), formed by the primary pass and passed on unchanged
};
static_assert(sizeof(QEntry) == 48, "QEntry is 48 bytes");

// The KINDS passes' tables beside RtReflectDev's per-sphere ones, and the GLOSS passes' seed (the last kernel argument)
struct RtKindsDev {
    const float *k_plane;          // reflectivness per plane (null: all 0)
    const float *k_cube;           // reflectivness per cube (null: all 0)
    const float *rough_plane;      // roughness per plane (null: all 0)
    const float *rough_cube;       // roughness per cube (null: all 0)
    uint32_t gloss_seed;           // rt_scene_set_gloss_seed
};

// reflect(I, N), kernel.cu:1282-1285: sub(I, multiply(multiply(N, dot(I, N)), 2)), the dot product left to right
__host__ __device__ __forceinline__ void rf_reflect(float ix, float iy, float iz, float nx, float ny, float nz, float &rx,
                                                    float &ry, float &rz)
{
    const float d = (ix * nx + iy * ny) + iz * nz;
    rx = ix - (nx * d) * 2.f;
    ry = iy - (ny * d) * 2.f;
    rz = iz - (nz * d) * 2.f;
}

// Glossy reflection: the integer mixer of the draws and the key are rf_mix and rf_gloss_key of rt_bvh.h.
// Component a of draw t for hit b under `key`: 24 bits of the mixed counter as an exact value of [-1, 1)
__host__ __device__ __forceinline__ float rf_gloss_draw(uint32_t key, uint32_t b, uint32_t t, uint32_t a)
{
    const uint32_t h = rf_mix(key + 0x9e3779b9u * ((b * 4u + t) * 3u + a + 1u));
    return (float)(h >> 8) * 1.1920928955078125e-07f - 1.f;   // 2^-23
}

// The glossy continuation of a hit with mirror direction R, normal N and roughness rho: u = the first of the draws
// t = 0..3 inside the unit ball (none: draw 3 halved), R' = normalise(R + rho * u), which is taken if it leaves the
// surface on R's side (dot(R', N) * dot(R, N) > 0, NaN fails) and else R. rho == 0 draws nothing and gives R.
// Returns what happened: 0 nothing drawn; 1 perturbed; | 2 the halved draw; | 4 R' rejected (the output is R).
__host__ __device__ __forceinline__ int rf_gloss(V3 R, V3 N, float rho, uint32_t key, uint32_t b, V3 &out)
{
    out = R;
    if (rho == 0.f) return 0;
    int what = 1 | 2;
    float ux = 0.f, uy = 0.f, uz = 0.f;
#pragma unroll 1
    for (uint32_t t = 0; t < 4u; ++t) {
        ux = rf_gloss_draw(key, b, t, 0u);
        uy = rf_gloss_draw(key, b, t, 1u);
        uz = rf_gloss_draw(key, b, t, 2u);
        if ((ux * ux + uy * uy) + uz * uz <= 1.f) {
            what = 1;
            break;
        }
    }
    if (what & 2) {
        ux = ux * 0.5f;
        uy = uy * 0.5f;
        uz = uz * 0.5f;
    }
    V3 G{R.x + rho * ux, R.y + rho * uy, R.z + rho * uz};
    rf_normalise(G);
    const float dg = (G.x * N.x + G.y * N.y) + G.z * N.z;
    const float dr = (R.x * N.x + R.y * N.y) + R.z * N.z;
    if (dg * dr > 0.f) out = G;
    else what |= 4;
    return what;
}

// refract(I, n, eta) for a normal n that faces against I: c = -dot(I, n) (left to right), q = 1 - (eta*eta) * (1 - c*c),
// s = sqrt(max(q, 0)) -- a negative radicand is taken as 0, no total internal reflection -- and I*eta + n*(eta*c - s),
// per component, not renormalised
__host__ __device__ __forceinline__ void rf_refract(float ix, float iy, float iz, float nx, float ny, float nz, float eta,
                                                    float &rx, float &ry, float &rz)
{
    const float c = -((ix * nx + iy * ny) + iz * nz);
    const float q = 1.f - (eta * eta) * (1.f - c * c);
    const float sq = __builtin_sqrtf(q > 0.f ? q : 0.f);
    const float f = eta * c - sq;
    rx = ix * eta + nx * f;
    ry = iy * eta + ny * f;
    rz = iz * eta + nz * f;
}

// The far root of sphere::intersect for (P, T) against s: rf_intersect's operations up to (-B + sqrt(disc)) / a2, before
// its min (from inside, intersect() returns the negative near root)
__host__ __device__ __forceinline__ float rf_far_root(V3 P, V3 T, float4 s)
{
    const float ocx = P.x - s.x, ocy = P.y - s.y, ocz = P.z - s.z;
    const float h = (T.x * ocx + T.y * ocy) + T.z * ocz;
    const float B = 2.f * h;
    const float C = ((ocx * ocx + ocy * ocy) + ocz * ocz) - s.w;
    const float A = (T.x * T.x + T.y * T.y) + T.z * T.z;
    const float disc = B * B - (4.f * A) * C;
    const float sq = __builtin_sqrtf(disc);
    const float a2 = 2.f * ((T.x * T.x + T.y * T.y) + T.z * T.z);
    return (-B + sq) / a2;
}

// The glass continuation of a hit on sphere s (DESIGN.md "Refraction"): D = the ray's direction, normal / start /
// new_org = the hit frame (rf_hit_frame). Writes R_{b+1} and returns 1 when the ray passed through the sphere (rule 4),
// 0 when it leaves undeviated from start_O (rule 1: dot(D, N) >= 0; rule 3: no positive far root from inside).
// The chord is not tested against other spheres. M: the exit normal of rule 4 (else the hit's normal).
__host__ __device__ __forceinline__ int rf_transmit(V3 D, V3 normal, V3 start, V3 new_org, float4 s, float ior, V3 &ro,
                                                    V3 &rd, V3 &M)
{
    ro = start;
    rd = D;
    M = normal;
    if ((D.x * normal.x + D.y * normal.y) + D.z * normal.z >= 0.f) return 0;   // rule 1
    V3 T;
    rf_refract(D.x, D.y, D.z, normal.x, normal.y, normal.z, 1.f / ior, T.x, T.y, T.z);
    const V3 P{normal.x * -0.00001f + new_org.x, normal.y * -0.00001f + new_org.y, normal.z * -0.00001f + new_org.z};
    const float t1 = rf_far_root(P, T, s);
    if (!(t1 > 0.f)) return 0;                                                   // rule 3 (NaN included)
    const V3 Q{P.x + T.x * t1, P.y + T.y * t1, P.z + T.z * t1};
    M = V3{Q.x - s.x, Q.y - s.y, Q.z - s.z};
    rf_normalise(M);
    rf_refract(T.x, T.y, T.z, -M.x, -M.y, -M.z, ior, rd.x, rd.y, rd.z);
    ro = V3{M.x * 0.00001f + Q.x, M.y * 0.00001f + Q.y, M.z * 0.00001f + Q.z};
    return 1;
}

__host__ __device__ __forceinline__ int rf_transmit(V3 D, V3 normal, V3 start, V3 new_org, float4 s, float ior, V3 &ro,
                                                    V3 &rd)
{
    V3 M;
    return rf_transmit(D, normal, start, new_org, s, ior, ro, rd, M);
}

// Fresnel glass (rt_scene_set_glass_model(RT_GLASS_FRESNEL)): the unpolarised reflectance of a dielectric
// of index ior at cosine c = -dot(D, N) of the incidence angle. The radicand is rf_refract's (eta = 1 / ior), clamped alike.
__host__ __device__ __forceinline__ float rf_fresnel(float c, float ior)
{
    const float eta = 1.f / ior;
    const float q = 1.f - (eta * eta) * (1.f - c * c);
    const float ct = __builtin_sqrtf(q > 0.f ? q : 0.f);
    const float rs = (c - ior * ct) / (c + ior * ct);
    const float rp = (ct - ior * c) / (ct + ior * c);
    return (rs * rs + rp * rp) * 0.5f;
}

// The draw of hit b under `key` that a Fresnel glass hit compares with its reflectance: 24 bits as an exact value of
// [0, 1). The inner mix with a constant keeps the stream apart from rf_gloss_draw's of the same key and b.
__host__ __device__ __forceinline__ float rf_fresnel_draw(uint32_t key, uint32_t b)
{
    const uint32_t h = rf_mix(rf_mix(key ^ 0x46726573u) + 0x9e3779b9u * (b + 1u));
    return (float)(h >> 8) * 5.9604644775390625e-08f;   // 2^-24
}

// What rf_fresnel_continue did: a mirror hit; a glass hit that left by rule 1 (nothing drawn), was reflected (u < F),
// went through the sphere (rule 4) or left by rule 3
enum { RF_MIRROR = 0, RF_RULE1 = 1, RF_REFLECTED = 2, RF_THROUGH = 3, RF_RULE3 = 4 };

// The continuation of hit b under the Fresnel model, of a mirror (glass = false) or of glass of index ior on sphere s:
// a glass hit with dot(D, N) < 0 is reflected with probability F = rf_fresnel and transmitted (rf_transmit) otherwise,
// by the draw u (a NaN F transmits). The mirror ray -- a mirror's or a reflected glass hit's -- is perturbed by rf_gloss
// against N where rho > 0, and so is the exit direction of a ray that went through, against the exit normal M. The
// branches are exclusive: one rf_gloss serves them all. F, u: 0 where nothing was drawn; what: rf_gloss's result.
__host__ __device__ __forceinline__ int rf_fresnel_continue(bool glass, V3 D, V3 normal, V3 start, V3 new_org, float4 s,
                                                            float ior, float rho, uint32_t key, uint32_t b, V3 &ro, V3 &rd,
                                                            float &F, float &u, int &what)
{
    int choice = RF_MIRROR;
    bool mirror = !glass;
    V3 gn = normal;   // the normal rf_gloss keeps the perturbed ray on the side of
    F = u = 0.f;
    ro = start;
    rd = D;
    if (glass) {
        const float dn = (D.x * normal.x + D.y * normal.y) + D.z * normal.z;
        if (dn >= 0.f) {                                                         // rule 1, as rf_transmit
            choice = RF_RULE1;
            rho = 0.f;
        } else {
            F = rf_fresnel(-dn, ior);
            u = rf_fresnel_draw(key, b);
            if (u < F) {
                choice = RF_REFLECTED;
                mirror = true;
            } else {
                choice = rf_transmit(D, normal, start, new_org, s, ior, ro, rd, gn) ? RF_THROUGH : RF_RULE3;
                if (choice == RF_RULE3) rho = 0.f;
            }
        }
    }
    if (mirror) rf_reflect(D.x, D.y, D.z, normal.x, normal.y, normal.z, rd.x, rd.y, rd.z);
    what = 0;
    if (rho > 0.f) {
        V3 G;
        what = rf_gloss(rd, gn, rho, key, b, G);
        rd = G;
    }
    return choice;
}

// ---------------------------------------------------------------------------
// device passes
// ---------------------------------------------------------------------------
namespace {

// Append the lanes with `push` set to the queue (one atomic per wave). Every lane of the wave calls it. (The sequence of
// rf_wave_append, rt_bvh.h, written out: through the helper four bounce kernels spill 2 to 4 more scalar registers.)
__device__ __forceinline__ void rf_push(bool push, const QEntry &e, QEntry *q, int *count)
{
    const lmask m = ballot64(push);
    if (m == 0) return;
    const int leader = __builtin_ctzll(m);
    int b = 0;
    if ((int)(threadIdx.x & 63u) == leader) b = atomicAdd(count, __popcll(m));
    const int base = __builtin_amdgcn_readlane(b, leader);
    if (push) q[base + lane_prefix(m)] = e;
}

// The three-light sum of rayTrace (kernel.cu:1643-1679) at a sphere hit, with castLightRay's sample construction
// taken from the frame kernel (ShadowChain, brute-force precision) and its any-hit loop through the BVH.
// Called by every lane of the wave in uniform control flow; `act` = this lane has a hit to shade.
__device__ __forceinline__ void rf_shade(const RtFrameConsts &fc, AuxPtr ax, const RtReflectDev &rd, bool act, V3 normal,
                                         V3 start, LdsStack stk, float &fr, float &fg, float &fb)
{
    fr = fg = fb = 0.f;
    float tr = 0.f, tg = 0.f, tb = 0.f;
    if (act) {
        const float tx = (float)((1.0 + rtm::div_by_3p1415((double)rtm::atan2f_rt(normal.z, normal.x))) * 0.5);
        const float ty = (float)rtm::div_by_3p1415((double)rtm::acosf_rt(normal.y));
        int ci = f2i(ty * (float)fc.tex_h) * fc.tex_w + f2i(tx * (float)fc.tex_w);
        const int last = fc.tex_w * fc.tex_h - 1;
        ci = ci < 0 ? 0 : (ci > last ? last : ci);   // documented clamp (as the frame kernel)
        tr = fc.tex_r[ci];
        tg = fc.tex_g[ci];
        tb = fc.tex_b[ci];
    }
    if (!any64(act)) return;
    if (act) {
        for (int li = 0; li < fc.n_lights; ++li) {
            const RtLightDev L = ax->lights[li];
            ShadowChain<0> chain;
            chain.begin(V3{L.px, L.py, L.pz}, start);
            int unshadowed = 0;
#pragma unroll 1
            for (int j = 0; j < RT_SHADOW_SAMPLES; ++j) {
                const V3 d = chain.direction(ax, false, L, start, j);
                float t;
                if (!rf_cast<true>(rd, start.x, start.y, start.z, d.x, d.y, d.z, t, stk)) unshadowed += 1;   // kernel.cu:1537-1539
            }
            float bsum = brightness_steps(unshadowed);
            const float a = dot3(normal, chain.toL);                    // kernel.cu:1541
            bsum = bsum * (a > 0.f ? a : 0.f);
            fr = fr + bsum * L.r * tr;                                  // kernel.cu:1673-1675
            fg = fg + bsum * L.g * tg;
            fb = fb + bsum * L.b * tb;
        }
    }
}

// rf_shade for a hit of any kind: rayTrace's pixel body at castRay's record h (q_shade_hit), under the same contract
__device__ __forceinline__ void rf_shade_kinds(const RtFrameConsts &fc, AuxPtr ax, const RtReflectDev &rd, bool act,
                                               const rt_hit &h, LdsStack stk, float &fr, float &fg, float &fb)
{
    fr = fg = fb = 0.f;
    if (!any64(act)) return;
    if (act) q_shade_hit(fc, ax, rd, h, stk, fr, fg, fb);
}

// k or roughness of the hit primitive: its kind's table (null: all 0) at its list position; a triangle has none
__device__ __forceinline__ float rf_kind_value(const float *sphere, const float *plane, const float *cube, int kind, int pos)
{
    if (kind == RT_HIT_SPHERE) return sphere ? sphere[pos] : 0.f;
    if (kind == RT_HIT_PLANE) return plane ? plane[pos] : 0.f;
    if (kind == RT_HIT_CUBE) return cube ? cube[pos] : 0.f;
    return 0.f;
}

// The continuation of hit b (0: the primary hit) at list position `hit` of `kind`, into e's origin, direction and pad_:
// glass (g = (tau, ior) with tau > 0; s = the hit sphere) goes through rf_transmit, anything else takes the mirror
// direction from start, which GLOSS perturbs where the hit's roughness is > 0. GLOSS passes the key on.
// FRESNEL (with GLASS and GLOSS): every continuation is rf_fresnel_continue's.
template <bool GLASS, bool KINDS, bool GLOSS, bool FRESNEL>
__device__ __forceinline__ void rf_continue(const RtReflectDev &rd, const RtKindsDev &kd, int kind, int hit, float2 g, V3 D,
                                            V3 normal, V3 start, V3 new_org, float4 s, uint32_t key, int b, QEntry &e)
{
    static_assert(!FRESNEL || (GLASS && GLOSS), "the Fresnel model needs glass and the key");
    if constexpr (FRESNEL) {
        const float rho = KINDS ? rf_kind_value(rd.rough, kd.rough_plane, kd.rough_cube, kind, hit)
                                : (rd.rough ? rd.rough[hit] : 0.f);
        V3 ro, rdir;
        float F, u;
        int what;
        rf_fresnel_continue(g.x > 0.f, D, normal, start, new_org, s, g.y, rho, key, (uint32_t)b, ro, rdir, F, u, what);
        e.ox = ro.x; e.oy = ro.y; e.oz = ro.z;
        e.dx = rdir.x; e.dy = rdir.y; e.dz = rdir.z;
        e.pad_ = (int)key;
        return;
    }
    if (GLASS && g.x > 0.f) {
        V3 ro, rdir;
        rf_transmit(D, normal, start, new_org, s, g.y, ro, rdir);
        e.ox = ro.x; e.oy = ro.y; e.oz = ro.z;
        e.dx = rdir.x; e.dy = rdir.y; e.dz = rdir.z;
    } else {
        e.ox = start.x; e.oy = start.y; e.oz = start.z;
        rf_reflect(D.x, D.y, D.z, normal.x, normal.y, normal.z, e.dx, e.dy, e.dz);
        if constexpr (GLOSS) {
            const float rho = KINDS ? rf_kind_value(rd.rough, kd.rough_plane, kd.rough_cube, kind, hit)
                                    : (rd.rough ? rd.rough[hit] : 0.f);
            if (rho > 0.f) {
                V3 Rg;
                rf_gloss(V3{e.dx, e.dy, e.dz}, normal, rho, key, (uint32_t)b, Rg);
                e.dx = Rg.x; e.dy = Rg.y; e.dz = Rg.z;
            }
        }
    }
    if constexpr (GLOSS) e.pad_ = (int)key;
}

__device__ __forceinline__ void rf_write(const RtFrameConsts &fc, int pix, float cr, float cg, float cb)
{
    if (fc.rgba) reinterpret_cast<float4 *>(fc.rgba)[pix] = make_float4(cr, cg, cb, 1.f);
    if (fc.packed && (fc.flags & RT_FLAG_RESOLVE))
        fc.packed[pix] = rgb_to_int(f2i(cr * 254.f), f2i(cg * 254.f), f2i(cb * 254.f));   // kernel.cu:1682
}

// The primary pass: every pixel of the band; queues those whose primary hit is reflective (or, GLASS, transparent).
// KINDS: the hit is castRay's over every kind (the frame kernel's own hit, as the G-buffers show for NEAREST).
// SAMPLES: a group of fc.spp samples, the first of them sample fc.sample_base of the raygen tables' total. Thread i is
// pixel i % npx at sample fc.sample_base + i / npx; fc.rgba is the group's slab [fc.spp][npx], where the frame kernel
// has left that sample's L at [i], and the queue entry's pix is i.
// GLOSS: some roughness table the frame reads holds a value > 0. Every queued entry carries the key of its
// pixel-sample, and the mirror continuation of a hit whose roughness is > 0 is rf_gloss's (hit 0 here, hit b in bounce b).
// FRESNEL: the glass model is RT_GLASS_FRESNEL and the frame has glass; a glass hit draws between the
// mirror ray and rf_transmit's, so the passes need the key: FRESNEL comes with GLASS and GLOSS only.
template <bool GLASS, bool KINDS, bool SAMPLES, bool GLOSS, bool FRESNEL>
__global__ __launch_bounds__(RT_REFLECT_BLOCK) void rt_reflect_primary(const RtFrameConsts fc, const RtReflectDev rd,
                                                                       QEntry *q, int *count, const RtKindsDev kd)
{
    __shared__ int stack_lds[RT_BVH_STACK * RT_REFLECT_BLOCK];
    const LdsStack stk{stack_lds, (int)threadIdx.x};
    const int npx = fc.width * fc.local_rows;
    const int pix = (int)(blockIdx.x * RT_REFLECT_BLOCK + threadIdx.x);   // SAMPLES: the slab index i
    const bool valid = pix < (SAMPLES ? fc.spp * npx : npx);               // (the host has checked that it fits an int)
    QEntry e{};
    bool push = false;
    if (valid) {
        V3 D;
        if constexpr (SAMPLES) {
            const int j = pix / npx;
            D = rf_primary_dir(fc, pix - j * npx, fc.sample_base + j);
        } else {
            D = rf_primary_dir(fc, pix);   // one sample: sample_base 0 is checked by the host
        }
        const V3 O{fc.org_x, fc.org_y, fc.org_z};
        float nt;
        int hit, kind = RT_HIT_SPHERE;                                          // hit: the list position within its kind
        float k;
        if constexpr (KINDS) {
            nt = q_nearest(fc, (AuxPtr)(uintptr_t)fc.aux, rd, O, D, stk, kind, hit);
            k = rf_kind_value(rd.k, kd.k_plane, kd.k_cube, kind, hit);
        } else {
            hit = rf_cast<false>(rd, O.x, O.y, O.z, D.x, D.y, D.z, nt, stk);
            k = (hit >= 0 && rd.k) ? rd.k[hit] : 0.f;
        }
        float2 g = make_float2(0.f, 0.f);                                       // (tau, ior)
        if (GLASS && hit >= 0 && kind == RT_HIT_SPHERE) {
            g = rd.glass[hit];
            if (g.x > 0.f) k = g.x;                                             // (k > 0 and tau > 0 are never both set)
        }
        if (k > 0.f) {
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);                         // the hit sphere (glass reads it)
            V3 normal, start, new_org;
            if constexpr (KINDS) {
                const rt_hit h = q_hit_record(fc, (AuxPtr)(uintptr_t)fc.aux, rd, O, D, nt, kind, hit);
                normal = V3{h.normal.x, h.normal.y, h.normal.z};
                new_org = V3{h.new_org.x, h.new_org.y, h.new_org.z};
                start = V3{normal.x * 0.00001f + new_org.x, normal.y * 0.00001f + new_org.y, normal.z * 0.00001f + new_org.z};
                if (GLASS && g.x > 0.f) s = rd.spheres[hit];
            } else {
                s = rd.spheres[hit];
                rf_hit_frame(O, D, nt, s, normal, start, new_org);
            }
            const float4 L = reinterpret_cast<const float4 *>(fc.rgba)[pix];   // the frame kernel's L for this hit
            const float f = 1.f - k;                                            // (w * (1 - k)) with w = 1
            uint32_t key = 0u;
            if constexpr (GLOSS) {
                // the pixel in the full frame (rows count from row 0 of the frame) and the absolute sample index
                const int sj = SAMPLES ? pix / npx : 0;
                const int lp = pix - sj * npx;
                const int ly = lp / fc.width;
                key = rf_gloss_key((uint32_t)(lp - ly * fc.width), (uint32_t)(fc.y0 + ly),
                                   (uint32_t)(SAMPLES ? fc.sample_base + sj : 0), kd.gloss_seed);
            }
            rf_continue<GLASS, KINDS, GLOSS, FRESNEL>(rd, kd, kind, hit, g, D, normal, start, new_org, s, key, 0, e);
            e.w = k;                                                            // w * k with w = 1
            e.cr = f * L.x; e.cg = f * L.y; e.cb = f * L.z;                     // the first term is assigned
            e.pix = pix;
            push = true;
        }
    }
    rf_push(push, e, q, count);
}

// Bounce b (1..depth): a fixed grid walks the queue of the previous pass; its length is read here, on the device.
template <bool GLASS, bool KINDS, bool GLOSS, bool FRESNEL>
__global__ __launch_bounds__(RT_REFLECT_BLOCK) void rt_reflect_bounce(const RtFrameConsts fc, const RtReflectDev rd, int b,
                                                                      const QEntry *qin, const int *count_in, QEntry *qout,
                                                                      int *count_out, const RtKindsDev kd)
{
    __shared__ int stack_lds[RT_BVH_STACK * RT_REFLECT_BLOCK];
    const LdsStack stk{stack_lds, (int)threadIdx.x};
    const AuxPtr ax = (AuxPtr)(uintptr_t)fc.aux;
    const int n_in = *count_in;
    for (int base = (int)blockIdx.x * RT_REFLECT_BLOCK; base < n_in; base += (int)gridDim.x * RT_REFLECT_BLOCK) {
        const int i = base + (int)threadIdx.x;
        const bool valid = i < n_in;
        QEntry e{};
        if (valid) e = qin[i];
        const V3 O{e.ox, e.oy, e.oz}, D{e.dx, e.dy, e.dz};
        float nt = 0.f;
        int hit = -1, kind = RT_HIT_SPHERE;   // hit: the list position within its kind
        bool act;
        V3 normal{0.f, 1.f, 0.f}, start{0.f, 0.f, 0.f};
        float Lr, Lg, Lb;
        if constexpr (KINDS) {
            if (valid) nt = q_nearest(fc, ax, rd, O, D, stk, kind, hit);
            act = valid && kind >= 0;
            rt_hit h{};
            if (act) {
                h = q_hit_record(fc, ax, rd, O, D, nt, kind, hit);
                normal = V3{h.normal.x, h.normal.y, h.normal.z};
                start = V3{normal.x * 0.00001f + h.new_org.x, normal.y * 0.00001f + h.new_org.y,
                           normal.z * 0.00001f + h.new_org.z};
            }
            rf_shade_kinds(fc, ax, rd, act, h, stk, Lr, Lg, Lb);
        } else {
            hit = valid ? rf_cast<false>(rd, O.x, O.y, O.z, D.x, D.y, D.z, nt, stk) : -1;
            act = valid && hit >= 0;
            if (act) rf_hit_frame(O, D, nt, rd.spheres[hit], normal, start);
            rf_shade(fc, ax, rd, act, normal, start, stk, Lr, Lg, Lb);
        }
        bool push = false;
        QEntry nx{};
        if (valid) {
            float cr = e.cr, cg = e.cg, cb = e.cb;
            bool done = true;
            if (!act) {                        // a miss: w * getFColor(R_b), and the pixel is done
                float sr, sg, sb;
                rf_sky(ax, O, D, sr, sg, sb);
                cr = cr + e.w * sr; cg = cg + e.w * sg; cb = cb + e.w * sb;
            } else {
                float k;
                if constexpr (KINDS) k = rf_kind_value(rd.k, kd.k_plane, kd.k_cube, kind, hit);
                else k = rd.k ? rd.k[hit] : 0.f;
                float2 g = make_float2(0.f, 0.f);   // (tau, ior)
                if (GLASS && kind == RT_HIT_SPHERE) {
                    g = rd.glass[hit];
                    if (g.x > 0.f) k = g.x;         // (k > 0 and tau > 0 are never both set)
                }
                if (k == 0.f || b == rd.depth) {
                    cr = cr + e.w * Lr; cg = cg + e.w * Lg; cb = cb + e.w * Lb;
                } else {
                    const float f = e.w * (1.f - k);
                    cr = cr + f * Lr; cg = cg + f * Lg; cb = cb + f * Lb;
                    V3 new_org{0.f, 0.f, 0.f};
                    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);   // the hit sphere (glass reads it)
                    if (GLASS && g.x > 0.f) {
                        // new_org again from O, D, nt (rf_hit_frame's operations): cheaper than keeping it across rf_shade
                        new_org = V3{O.x + D.x * nt, O.y + D.y * nt, O.z + D.z * nt};
                        s = rd.spheres[hit];
                    }
                    rf_continue<GLASS, KINDS, GLOSS, FRESNEL>(rd, kd, kind, hit, g, D, normal, start, new_org, s, (uint32_t)e.pad_, b, nx);
                    nx.w = e.w * k;
                    nx.cr = cr; nx.cg = cg; nx.cb = cb;
                    nx.pix = e.pix;
                    done = false;
                    push = true;
                }
            }
            if (done) rf_write(fc, e.pix, cr, cg, cb);
        }
        rf_push(push, nx, qout, count_out);
    }
}

// The resolve pass of a supersampled frame, one thread per band pixel: S = (the earlier groups' sum, or +0) + the
// group's g slab entries of the pixel in ascending sample order, per channel in binary32 (the frame kernel's
// acc = 0.f; acc = acc + fr). Not the last group: S goes to `sum`. The last group: the frame kernel's write-back for
// `n_samples` samples of `total` -- accumulate, rgba = (S, n_samples), the packed word of S / total.
__global__ __launch_bounds__(RT_REFLECT_BLOCK) void rt_reflect_resolve(const float4 *slab, int npx, int g, float4 *sum,
                                                                       int first, int last, float4 *rgba, uint32_t *packed,
                                                                       int flags, float n_samples, float total)
{
    const int pix = (int)(blockIdx.x * RT_REFLECT_BLOCK + threadIdx.x);
    if (pix >= npx) return;
    float r = 0.f, gr = 0.f, b = 0.f;
    if (!first) {
        const float4 s = sum[pix];
        r = s.x; gr = s.y; b = s.z;
    }
    for (int j = 0; j < g; ++j) {
        const float4 c = slab[(size_t)j * (size_t)npx + (size_t)pix];
        r = r + c.x;
        gr = gr + c.y;
        b = b + c.z;
    }
    if (!last) {
        sum[pix] = make_float4(r, gr, b, 0.f);
        return;
    }
    float w = n_samples;
    if (rgba) {
        if (flags & RT_FLAG_ACCUMULATE) {
            const float4 old = rgba[pix];
            r = old.x + r;
            gr = old.y + gr;
            b = old.z + b;
            w = old.w + w;
        }
        rgba[pix] = make_float4(r, gr, b, w);
    }
    if (packed && (flags & RT_FLAG_RESOLVE)) {
        float mr = r, mg = gr, mb = b;
        if (total != 1.f) {
            mr = r / total;
            mg = gr / total;
            mb = b / total;
        }
        packed[pix] = rgb_to_int(f2i(mr * 254.f), f2i(mg * 254.f), f2i(mb * 254.f));
    }
}

}  // namespace

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// One per-primitive table of the passes (reflectivness or roughness of a kind, or the spheres' glass pairs): what the
// host last set, and a device copy that changes only in upload() -- in rt_reflect_prepare, after the frames that may
// still read it. The passes are chosen and pointed by what the device holds (v_dev, pos_dev, dev()), never by v.
namespace {
struct RfTable {
    std::vector<float> v;                 // empty = all 0
    std::vector<float> v_dev;             // what the device copy holds
    bool dirty = false;                   // v changed since the last upload
    bool pos_dev = false;                 // v_dev holds a value > 0 (the roughness tables: whether GLOSS is needed)
    DevArray<float> d;
    void set(std::vector<float> nv)       // (the drop-in boundary sets the same materials every frame: no re-upload then)
    {
        if (nv == v) return;
        v.swap(nv);
        dirty = true;
    }
    void clear()
    {
        if (!v.empty()) dirty = true;
        v.clear();
    }
    hipError_t upload(hipStream_t stream)
    {
        if (!dirty) return hipSuccess;
        v_dev = v;
        pos_dev = std::any_of(v_dev.begin(), v_dev.end(), [](float x) { return x > 0.f; });
        if (!v_dev.empty()) {
            hipError_t e = d.reserve(v_dev.size());
            if (e == hipSuccess) e = hipMemcpyAsync(d.get(), v_dev.data(), sizeof(float) * v_dev.size(), hipMemcpyHostToDevice, stream);
            if (e != hipSuccess) return e;
        }
        dirty = false;
        return hipSuccess;
    }
    const float *dev() const { return v_dev.empty() ? nullptr : d.get(); }
};
}  // namespace

// The tables: reflectivness and roughness by kind (RT_HIT_SPHERE + i: sphere, plane, cube), and the spheres' glass
enum { RF_K = 0, RF_ROUGH = 3, RF_GLASS = 6, RF_TABLES = 7 };
static_assert(RT_HIT_PLANE == RT_HIT_SPHERE + 1 && RT_HIT_CUBE == RT_HIT_SPHERE + 2, "the tables are indexed by kind");

struct RtReflect {
    // tab[RF_K + i], tab[RF_ROUGH + i]: one value per primitive of kind i; the plane and cube tables are read only by
    // frames under RT_REFLECT_SCENE. tab[RF_GLASS]: (transperancy, ior) per sphere, interleaved; empty = no sphere has
    // tau > 0 (the device reads it as float2)
    RfTable tab[RF_TABLES];
    int scope = RT_REFLECT_SPHERES;       // rt_scene_set_reflect_scope
    int samples = RT_REFLECT_SAMPLES_ONE; // rt_scene_set_reflect_samples
    unsigned gloss_seed = 0;              // rt_scene_set_gloss_seed: a host-side value, read when a frame is launched
    int glass_model = RT_GLASS_PLAIN;     // rt_scene_set_glass_model: likewise
    RtSphereBvh bvh;                      // the sphere BVH (shared with the ray queries)
    // queues and counters
    DevArray<QEntry> d_q[2];
    DevArray<int> d_cnt;
    DevArray<float4> d_rgba;              // frame-kernel output when the caller gave no rgba
    // supersampled frames: the group's per-sample colours [G][npx] and, when there are several groups, their running sum
    DevArray<float4> d_slab, d_sum;
    // the last frame
    int last_groups = 1;                  // runs of the passes (a supersampled frame: its groups), one counter row each
    bool last_samples = false;            // it was a supersampled frame (its groups end with a resolve pass)
    int last_depth = 0;
    bool have_frame = false;
    // what rf_run_passes launched last (rt_debug_reflect_dispatch): the instantiation's flags, whether the passes
    // walked the sphere BVH, and how many groups of the frame have run; groups = 0 before any reflective frame
    struct {
        bool glass, kinds, samples, gloss, fresnel, bvh;
        int groups;
    } dispatch = {};
    int timing = 0;
    bool timed = false;
    HipEvent ev[RT_REFLECT_MAX_GROUPS][RT_MAX_REFLECT_DEPTH + 4];   // a row per group (a one-sample frame: row 0), rf_mark
    HipEvent done;                        // after the last pass of the last frame (rt_reflect_get_stats waits for it)
};

RtReflect *rt_reflect_create() { return new RtReflect(); }

RtSphereBvh *rt_reflect_bvh(RtReflect *r) { return &r->bvh; }

// (the scene has waited for its frames, which include the passes)
void rt_reflect_destroy(RtReflect *r) { delete r; }

// rt_scene_set_spheres: a new count clears the materials (the same count keeps them)
void rt_reflect_spheres_changed(RtReflect *r, int n_old, int n_new)
{
    if (n_old == n_new) return;
    for (int t : {RF_K, RF_GLASS, RF_ROUGH}) r->tab[t].clear();
}

// rt_scene_set_planes / rt_scene_set_cubes (which = 0 / 1): a new count clears the list's materials (the same count
// keeps them)
void rt_reflect_kind_list_changed(RtReflect *r, int which, int n_old, int n_new)
{
    if (n_old == n_new) return;
    for (int t : {RF_K, RF_ROUGH}) r->tab[t + 1 + which].clear();
}

// The setters below share their head -- NULL / 0 clears the entry's tables -- and their commit, RfTable::set; on a
// refusal nothing has changed. Each keeps its own checks in its own order.
template <typename M>
static std::vector<float> rf_reflectivness(const M *m, int n)
{
    std::vector<float> k((size_t)n);
    for (int i = 0; i < n; ++i) k[(size_t)i] = m[i].reflectivness;
    return k;
}

// the old entry sets every transperancy to 0
int rt_reflect_set_materials(RtReflect *r, const rt_material *m, int n, int n_spheres)
{
    if (!m || n == 0) {
        r->tab[RF_K].clear();
        r->tab[RF_GLASS].clear();
        return RT_OK;
    }
    if (n != n_spheres || n < 0) {
        rt_set_error("rt_scene_set_materials: %d materials for %d spheres (one per sphere, or NULL / 0)", n, n_spheres);
        return RT_ERR_INVALID;
    }
    for (int i = 0; i < n; ++i) {
        const float k = m[i].reflectivness;
        if (!(k >= 0.f && k <= 1.f)) {
            rt_set_error("rt_scene_set_materials: sphere %d: reflectivness %g is not in [0, 1]", i, (double)k);
            return RT_ERR_INVALID;
        }
        if (m[i].transperancy != 0.f || m[i].roughness != 0.f) {
            rt_set_error("rt_scene_set_materials: sphere %d: transperancy / roughness are not implemented (only reflectivness)", i);
            return RT_ERR_UNSUPPORTED;
        }
    }
    r->tab[RF_K].set(rf_reflectivness(m, n));
    r->tab[RF_GLASS].clear();
    return RT_OK;
}

int rt_reflect_set_materials_ex(RtReflect *r, const rt_material_ex *m, int n, int n_spheres)
{
    if (!m || n == 0) {
        r->tab[RF_K].clear();
        r->tab[RF_GLASS].clear();
        return RT_OK;
    }
    if (n != n_spheres || n < 0) {
        rt_set_error("rt_scene_set_materials_ex: %d materials for %d spheres (one per sphere, or NULL / 0)", n, n_spheres);
        return RT_ERR_INVALID;
    }
    bool any_glass = false;
    for (int i = 0; i < n; ++i) {   // every value first, then what is not implemented: nothing changes on an error
        const float k = m[i].reflectivness, tau = m[i].transperancy, ior = m[i].ior;
        if (!(k >= 0.f && k <= 1.f) || !(tau >= 0.f && tau <= 1.f)) {
            rt_set_error("rt_scene_set_materials_ex: sphere %d: reflectivness %g / transperancy %g is not in [0, 1]", i,
                         (double)k, (double)tau);
            return RT_ERR_INVALID;
        }
        if (tau > 0.f && !(ior >= 1.f && ior <= 4.f)) {
            rt_set_error("rt_scene_set_materials_ex: sphere %d: ior %g is not in [1, 4]", i, (double)ior);
            return RT_ERR_INVALID;
        }
        any_glass = any_glass || tau > 0.f;
    }
    for (int i = 0; i < n; ++i) {
        if (m[i].roughness != 0.f) {
            rt_set_error("rt_scene_set_materials_ex: sphere %d: roughness is not implemented", i);
            return RT_ERR_UNSUPPORTED;
        }
        if (m[i].reflectivness > 0.f && m[i].transperancy > 0.f) {
            rt_set_error("rt_scene_set_materials_ex: sphere %d: reflectivness and transperancy both > 0 (one continuation "
                         "per hit: a sphere is a mirror or glass)", i);
            return RT_ERR_UNSUPPORTED;
        }
    }
    std::vector<float> glass;
    if (any_glass) {
        glass.resize((size_t)2 * n);
        for (int i = 0; i < n; ++i) {
            const float tau = m[i].transperancy;
            glass[(size_t)2 * i] = tau;
            glass[(size_t)2 * i + 1] = tau > 0.f ? m[i].ior : 0.f;   // (ignored where tau == 0)
        }
    }
    r->tab[RF_K].set(rf_reflectivness(m, n));
    r->tab[RF_GLASS].set(std::move(glass));
    return RT_OK;
}

// rt_scene_set_plane_materials / rt_scene_set_cube_materials (which = 0 / 1): rt_reflect_set_materials' rules for a
// list of n_list entries, except that the values are checked before the count
int rt_reflect_set_kind_materials(RtReflect *r, int which, const rt_material *m, int n, int n_list)
{
    const char *fn = which == 0 ? "rt_scene_set_plane_materials" : "rt_scene_set_cube_materials";
    const char *what = which == 0 ? "plane" : "cube";
    RfTable &t = r->tab[RF_K + 1 + which];
    if (!m || n == 0) {
        t.clear();
        return RT_OK;
    }
    for (int i = 0; i < n; ++i) {   // every value first, then what is not implemented, then the count
        const float k = m[i].reflectivness;
        if (!(k >= 0.f && k <= 1.f)) {
            rt_set_error("%s: %s %d: reflectivness %g is not in [0, 1]", fn, what, i, (double)k);
            return RT_ERR_INVALID;
        }
    }
    for (int i = 0; i < n; ++i) {
        if (m[i].transperancy != 0.f || m[i].roughness != 0.f) {
            rt_set_error("%s: %s %d: transperancy / roughness are not implemented (only reflectivness; glass is a sphere "
                         "property)", fn, what, i);
            return RT_ERR_UNSUPPORTED;
        }
    }
    if (n != n_list) {
        rt_set_error("%s: %d materials for %d %ss (one per %s, or NULL / 0)", fn, n, n_list, what, what);
        return RT_ERR_INVALID;
    }
    t.set(rf_reflectivness(m, n));
    return RT_OK;
}

// rt_scene_set_roughness: one value in [0, 1] per primitive of `kind`'s list of n_list entries, or NULL / 0 to clear
int rt_reflect_set_roughness(RtReflect *r, int kind, const float *rho, int n, int n_list)
{
    if (kind != RT_HIT_SPHERE && kind != RT_HIT_PLANE && kind != RT_HIT_CUBE) {
        rt_set_error("rt_scene_set_roughness: kind %d is not RT_HIT_SPHERE, RT_HIT_PLANE or RT_HIT_CUBE", kind);
        return RT_ERR_INVALID;
    }
    const char *what = kind == RT_HIT_SPHERE ? "sphere" : (kind == RT_HIT_PLANE ? "plane" : "cube");
    RfTable &t = r->tab[RF_ROUGH + kind - RT_HIT_SPHERE];
    if (!rho || n == 0) {
        t.clear();
        return RT_OK;
    }
    if (n != n_list || n < 0) {
        rt_set_error("rt_scene_set_roughness: %d values for %d %ss (one per %s, or NULL / 0)", n, n_list, what, what);
        return RT_ERR_INVALID;
    }
    for (int i = 0; i < n; ++i) {
        if (!(rho[i] >= 0.f && rho[i] <= 1.f)) {
            rt_set_error("rt_scene_set_roughness: %s %d: roughness %g is not in [0, 1]", what, i, (double)rho[i]);
            return RT_ERR_INVALID;
        }
    }
    t.set(std::vector<float>(rho, rho + n));
    return RT_OK;
}

int rt_reflect_set_gloss_seed(RtReflect *r, unsigned seed)
{
    r->gloss_seed = seed;
    return RT_OK;
}

int rt_reflect_set_glass_model(RtReflect *r, int model)
{
    if (model != RT_GLASS_PLAIN && model != RT_GLASS_FRESNEL) {
        rt_set_error("rt_scene_set_glass_model: model %d is not RT_GLASS_PLAIN or RT_GLASS_FRESNEL", model);
        return RT_ERR_INVALID;
    }
    r->glass_model = model;
    return RT_OK;
}

int rt_reflect_set_scope(RtReflect *r, int scope)
{
    if (scope != RT_REFLECT_SPHERES && scope != RT_REFLECT_SCENE) {
        rt_set_error("rt_scene_set_reflect_scope: scope %d is not RT_REFLECT_SPHERES or RT_REFLECT_SCENE", scope);
        return RT_ERR_INVALID;
    }
    r->scope = scope;
    return RT_OK;
}

int rt_reflect_scope(const RtReflect *r) { return r->scope; }

int rt_reflect_set_samples(RtReflect *r, int mode)
{
    if (mode != RT_REFLECT_SAMPLES_ONE && mode != RT_REFLECT_SAMPLES_MANY) {
        rt_set_error("rt_scene_set_reflect_samples: mode %d is not RT_REFLECT_SAMPLES_ONE or RT_REFLECT_SAMPLES_MANY", mode);
        return RT_ERR_INVALID;
    }
    r->samples = mode;
    return RT_OK;
}

int rt_reflect_samples(const RtReflect *r) { return r->samples; }

bool rt_reflect_needs_upload(const RtReflect *r, unsigned long long sphere_gen, int n)
{
    // (the plane and cube tables count under either scope: the upload is due whenever they changed)
    return std::any_of(r->tab, r->tab + RF_TABLES, [](const RfTable &t) { return t.dirty; }) ||
           rt_sphere_bvh_stale(&r->bvh, sphere_gen, n);
}

// Brings materials and BVH up to date (the caller has waited for every frame that may read them) and makes sure the
// queues hold `npx` pixels (a supersampled frame: the pixel-samples of a group). rgba_scratch: set when the caller has
// no rgba buffer.
int rt_reflect_prepare(RtReflect *r, const float4 *h_spheres, int n, unsigned long long sphere_gen, int npx,
                       bool need_rgba, float **rgba_scratch, hipStream_t stream)
{
    {
        const int rc = rt_sphere_bvh_update(&r->bvh, h_spheres, n, sphere_gen, stream);
        if (rc != RT_OK) return rc;
    }
    for (RfTable &t : r->tab) RT_HIP(t.upload(stream));
    for (DevArray<QEntry> &q : r->d_q) RT_HIP(q.reserve((size_t)npx));
    RT_HIP(r->d_cnt.reserve(RT_REFLECT_MAX_GROUPS * (RT_MAX_REFLECT_DEPTH + 1)));   // one row per group
    *rgba_scratch = nullptr;
    if (need_rgba) {
        RT_HIP(r->d_rgba.reserve((size_t)npx));
        *rgba_scratch = reinterpret_cast<float *>(r->d_rgba.get());
    }
    return RT_OK;
}

// The scratch of a supersampled frame of `n` samples over `npx` band pixels (RtSamplesPlan, rt_internal.h).
// RT_ERR_CAPACITY when a group's pixel-samples do not fit the int of QEntry::pix (and of the bounces' grid stride).
int rt_reflect_samples_plan(const RtReflect *r, int n, int npx, RtSamplesPlan *plan)
{
    const int g = std::min(n, RT_REFLECT_SAMPLE_GROUP);
    const long long e = (long long)g * npx;
    if (e > 0x7fffffffLL - (long long)RT_BOUNCE_GRID * RT_REFLECT_BLOCK) {
        rt_set_error("rt_scene_render: %d samples of %d pixels per pass exceed the reflective queues' index range", g, npx);
        return RT_ERR_CAPACITY;
    }
    plan->entries = (int)e;
    plan->sum_px = n > g ? npx : 0;
    plan->grows = (size_t)e > r->d_slab.capacity() || (size_t)e > r->d_q[0].capacity() || (size_t)e > r->d_q[1].capacity() ||
                  (size_t)plan->sum_px > r->d_sum.capacity();
    return RT_OK;
}

// The slab and the running sum of a plan: after rt_reflect_prepare (the queues) and under its protocol -- after the
// frames in flight, and after a host wait when it re-allocates
int rt_reflect_prepare_samples(RtReflect *r, const RtSamplesPlan *plan)
{
    RT_HIP(r->d_slab.reserve((size_t)plan->entries));
    if (plan->sum_px > 0) RT_HIP(r->d_sum.reserve((size_t)plan->sum_px));
    return RT_OK;
}

// timing, per group (a one-sample frame: group 0): an event before the frame kernel(s) (slot 0), after them (1), after
// the primary pass (2), after bounce b (2 + b) and, a supersampled frame, after the resolve pass (depth + 3)
static hipError_t rf_mark(RtReflect *r, int group, int slot, hipStream_t stream)
{
    if (!r->timing) return hipSuccess;
    HipEvent &ev = r->ev[group][slot];
    const hipError_t e = ev.create(hipEventDefault);
    return e != hipSuccess ? e : hipEventRecord(ev.get(), stream);
}

// samples: 0 for a one-sample frame, else the samples of a supersampled one (rt_reflect_launch_samples)
int rt_reflect_begin_frame(RtReflect *r, int depth, int samples, hipStream_t stream)
{
    r->last_samples = samples > 0;
    r->last_groups = samples > 0 ? (samples + RT_REFLECT_SAMPLE_GROUP - 1) / RT_REFLECT_SAMPLE_GROUP : 1;
    RT_HIP(hipMemsetAsync(r->d_cnt.get(), 0, sizeof(int) * (size_t)r->last_groups * (RT_MAX_REFLECT_DEPTH + 1), stream));
    r->last_depth = depth;
    r->have_frame = true;
    r->timed = r->timing != 0;
    return RT_OK;
}

// Right before the frame kernel's launch (after anything else the frame enqueues, e.g. the tile-order sort).
int rt_reflect_mark_frame_start(RtReflect *r, hipStream_t stream)
{
    RT_HIP(rf_mark(r, 0, 0, stream));
    return RT_OK;
}

// What the passes of a frame read and which instantiations run them
struct RfPasses {
    RtReflectDev rd;
    RtKindsDev kd;
    bool glass, kinds, gloss, fresnel;
};

static RfPasses rf_passes(const RtReflect *r, const RtFrameConsts *fc, const float4 *d_spheres, int n, int depth, bool brute)
{
    RfPasses p{};
    RtReflectDev &rd = p.rd;
    rd.nodes = (!brute && r->bvh.ok) ? r->bvh.d_nodes.get() : nullptr;
    rd.lsph = r->bvh.d_lsph.get();
    rd.order = r->bvh.d_order.get();
    rd.spheres = d_spheres;
    rd.n = n;
    const RfTable *k = r->tab + RF_K, *rough = r->tab + RF_ROUGH;   // [0] sphere, [1] plane, [2] cube
    rd.k = k[0].dev();
    rd.depth = depth;
    rd.glass = reinterpret_cast<const float2 *>(r->tab[RF_GLASS].dev());
    p.glass = rd.glass != nullptr;   // mirror-only frames run the GLASS = false instantiations (today's code)
    // KINDS only where the scope is the scene and there is something besides spheres: every frame that rendered before
    // the scope existed runs the KINDS = false instantiations
    p.kinds = r->scope == RT_REFLECT_SCENE && (fc->n_planes > 0 || fc->n_cubes > 0 || fc->n_boxes > 0);
    p.kd.k_plane = p.kinds ? k[1].dev() : nullptr;
    p.kd.k_cube = p.kinds ? k[2].dev() : nullptr;
    // GLOSS only where a roughness table that this frame's scope reads holds a value > 0: every other frame runs the
    // GLOSS = false instantiations with the arguments it had before roughness existed (no table, seed 0)
    p.gloss = rough[0].pos_dev || (p.kinds && (rough[1].pos_dev || rough[2].pos_dev));
    // FRESNEL only under that model in a frame with glass; its draw needs the key, so it takes GLOSS along, with or
    // without a roughness table
    p.fresnel = p.glass && r->glass_model == RT_GLASS_FRESNEL;
    p.gloss = p.gloss || p.fresnel;
    if (p.gloss) {
        rd.rough = rough[0].dev();
        p.kd.rough_plane = p.kinds ? rough[1].dev() : nullptr;
        p.kd.rough_cube = p.kinds ? rough[2].dev() : nullptr;
        p.kd.gloss_seed = r->gloss_seed;
    }
    return p;
}

// The instantiations of the two passes for a frame's (glass, kinds, fresnel), at compile-time SAMPLES and GLOSS
template <bool SAMPLES, bool GLOSS>
static auto rf_primary_kernel(const RfPasses &p)
{
    if constexpr (GLOSS)   // (FRESNEL comes with GLASS and GLOSS only)
        if (p.fresnel)
            return p.kinds ? rt_reflect_primary<true, true, SAMPLES, true, true> : rt_reflect_primary<true, false, SAMPLES, true, true>;
    return p.kinds ? (p.glass ? rt_reflect_primary<true, true, SAMPLES, GLOSS, false> : rt_reflect_primary<false, true, SAMPLES, GLOSS, false>)
                   : (p.glass ? rt_reflect_primary<true, false, SAMPLES, GLOSS, false> : rt_reflect_primary<false, false, SAMPLES, GLOSS, false>);
}
template <bool GLOSS>
static auto rf_bounce_kernel(const RfPasses &p)
{
    if constexpr (GLOSS)
        if (p.fresnel) return p.kinds ? rt_reflect_bounce<true, true, true, true> : rt_reflect_bounce<true, false, true, true>;
    return p.kinds ? (p.glass ? rt_reflect_bounce<true, true, GLOSS, false> : rt_reflect_bounce<false, true, GLOSS, false>)
                   : (p.glass ? rt_reflect_bounce<true, false, GLOSS, false> : rt_reflect_bounce<false, false, GLOSS, false>);
}

// The primary pass over `threads` pixels (SAMPLES: pixel-samples) and the `depth` bounces of group `group`, with its
// counter row and its row of events
template <bool SAMPLES>
static int rf_run_passes(RtReflect *r, const RfPasses &p, const RtFrameConsts *fc, int threads, int depth, int group,
                         hipStream_t stream)
{
    int *const cnt = r->d_cnt.get() + group * (RT_MAX_REFLECT_DEPTH + 1);
    const auto primary = p.gloss ? rf_primary_kernel<SAMPLES, true>(p) : rf_primary_kernel<SAMPLES, false>(p);
    const auto bounce = p.gloss ? rf_bounce_kernel<true>(p) : rf_bounce_kernel<false>(p);
    r->dispatch = {p.glass, p.kinds, SAMPLES, p.gloss, p.fresnel, p.rd.nodes != nullptr, group + 1};
    hipLaunchKernelGGL(primary, dim3((threads + RT_REFLECT_BLOCK - 1) / RT_REFLECT_BLOCK), dim3(RT_REFLECT_BLOCK), 0,
                       stream, *fc, p.rd, r->d_q[0].get(), cnt, p.kd);
    RT_HIP(hipGetLastError());
    RT_HIP(rf_mark(r, group, 2, stream));
    for (int b = 1; b <= depth; ++b) {
        hipLaunchKernelGGL(bounce, dim3(RT_BOUNCE_GRID), dim3(RT_REFLECT_BLOCK), 0, stream, *fc, p.rd, b,
                           r->d_q[(b - 1) & 1].get(), cnt + (b - 1), r->d_q[b & 1].get(), cnt + b, p.kd);
        RT_HIP(hipGetLastError());
        RT_HIP(rf_mark(r, group, 2 + b, stream));
    }
    return RT_OK;
}

// The passes after the frame kernel (which has written fc->rgba).
int rt_reflect_launch(RtReflect *r, const RtFrameConsts *fc, const float4 *d_spheres, int n, int depth, bool brute,
                      hipStream_t stream)
{
    RT_HIP(rf_mark(r, 0, 1, stream));
    const RfPasses p = rf_passes(r, fc, d_spheres, n, depth, brute);
    const int rc = rf_run_passes<false>(r, p, fc, fc->width * fc->local_rows, depth, 0, stream);
    if (rc != RT_OK) return rc;
    RT_HIP(r->done.create());
    RT_HIP(hipEventRecord(r->done.get(), stream));
    return RT_OK;
}

// A supersampled frame, after rt_reflect_prepare_samples and rt_reflect_begin_frame. `fc`: the uniforms
// of one sample of the frame -- spp 1, no accumulate, no resolve, no packed output; its rgba and sample_base are set
// here. `out`: the caller's frame (rgba, packed, flags, spp, sample_base, sample_total), which only the resolve pass of
// the last group touches. Per group of at most RT_REFLECT_SAMPLE_GROUP samples: the frame kernel per sample into its
// slab, the primary pass over the group, the bounces, the resolve pass.
int rt_reflect_launch_samples(RtReflect *r, const RtFrameConsts *fc, const RtFrameConsts *out, const RtKernelChoice *kc,
                              const float4 *d_spheres, int n, int depth, hipStream_t stream)
{
    const int npx = fc->width * fc->local_rows;
    const int n_samples = out->spp, groups = r->last_groups;
    float4 *const slab = r->d_slab.get();
    for (int gi = 0; gi < groups; ++gi) {
        const int k0 = out->sample_base + gi * RT_REFLECT_SAMPLE_GROUP;
        const int g = std::min(RT_REFLECT_SAMPLE_GROUP, n_samples - gi * RT_REFLECT_SAMPLE_GROUP);
        RT_HIP(rf_mark(r, gi, 0, stream));
        RtFrameConsts f = *fc;
        for (int j = 0; j < g; ++j) {
            f.sample_base = k0 + j;
            f.rgba = reinterpret_cast<float *>(slab + (size_t)j * (size_t)npx);
            RT_HIP(rt_dev_launch_trace(&f, d_spheres, kc->tile, kc->cull, kc->mode, kc->feat, stream));
        }
        RT_HIP(rf_mark(r, gi, 1, stream));
        // the passes' view of the group: g samples from k0, the slab as their rgba, nothing packed
        f.spp = g;
        f.sample_base = k0;
        f.rgba = reinterpret_cast<float *>(slab);
        const RfPasses p = rf_passes(r, &f, d_spheres, n, depth, kc->cull == 0);
        const int rc = rf_run_passes<true>(r, p, &f, g * npx, depth, gi, stream);
        if (rc != RT_OK) return rc;
        hipLaunchKernelGGL(rt_reflect_resolve, dim3((npx + RT_REFLECT_BLOCK - 1) / RT_REFLECT_BLOCK), dim3(RT_REFLECT_BLOCK), 0,
                           stream, slab, npx, g, r->d_sum.get(), gi == 0 ? 1 : 0, gi == groups - 1 ? 1 : 0,
                           reinterpret_cast<float4 *>(out->rgba), out->packed, out->flags, (float)n_samples, out->sample_total);
        RT_HIP(hipGetLastError());
        RT_HIP(rf_mark(r, gi, depth + 3, stream));
    }
    RT_HIP(r->done.create());
    RT_HIP(hipEventRecord(r->done.get(), stream));
    return RT_OK;
}

int rt_reflect_set_timing(RtReflect *r, int on)
{
    r->timing = on ? 1 : 0;
    return RT_OK;
}

int rt_reflect_get_stats(RtReflect *r, rt_reflect_stats *out)
{
    memset(out, 0, sizeof *out);
    out->bvh_build_ms = r->bvh.build_ms;
    out->bvh_nodes = (int)r->bvh.nodes.size();
    out->bvh_depth = r->bvh.depth;
    out->bvh_leaves = r->bvh.leaves;
    if (!r->have_frame) return RT_OK;
    out->depth = r->last_depth;
    if (r->done.get()) RT_HIP(hipEventSynchronize(r->done.get()));   // the last frame only, not the whole device
    // (a supersampled frame: queue[] and pass_ms[] are summed over its groups, the resolve passes counted in the last
    // bounce's slot)
    int cnt[RT_REFLECT_MAX_GROUPS][RT_MAX_REFLECT_DEPTH + 1];
    RT_HIP(hipMemcpy(cnt, r->d_cnt.get(), sizeof(int) * (size_t)r->last_groups * (RT_MAX_REFLECT_DEPTH + 1), hipMemcpyDeviceToHost));
    for (int g = 0; g < r->last_groups; ++g)
        for (int b = 0; b <= RT_MAX_REFLECT_DEPTH; ++b) out->queue[b] += cnt[g][b];
    if (r->timed) {
        for (int g = 0; g < r->last_groups; ++g) {
            const HipEvent *ev = r->ev[g];
            for (int p = 0; p < r->last_depth + (r->last_samples ? 3 : 2); ++p) {
                float ms = 0.f;
                RT_HIP(hipEventElapsedTime(&ms, ev[p].get(), ev[p + 1].get()));
                out->pass_ms[std::min(p, r->last_depth + 1)] += ms;
            }
        }
        out->timed = 1;
    }
    return RT_OK;
}

// rt_debug_reflect_dispatch: out = {glass, kinds, samples, gloss, fresnel, bvh, groups} as rf_run_passes launched the
// last reflective frame; r null or no such frame yet: the flags -1 and groups 0
void rt_reflect_dispatch(const RtReflect *r, int out[RT_REFLECT_DISPATCH_FIELDS])
{
    static_assert(RT_REFLECT_DISPATCH_FIELDS == 7, "six flags and the group count");
    if (!r || r->dispatch.groups == 0) {
        std::fill(out, out + RT_REFLECT_DISPATCH_FIELDS - 1, -1);
        out[RT_REFLECT_DISPATCH_FIELDS - 1] = 0;
        return;
    }
    const auto &d = r->dispatch;
    const int v[RT_REFLECT_DISPATCH_FIELDS] = {d.glass, d.kinds, d.samples, d.gloss, d.fresnel, d.bvh, d.groups};
    std::copy(v, v + RT_REFLECT_DISPATCH_FIELDS, out);
}

// ---------------------------------------------------------------------------
// host-only debug entries (tests)
// ---------------------------------------------------------------------------
extern "C" int rt_debug_reflect(const rt_vec3 *I, const rt_vec3 *N, int n, rt_vec3 *out)
{
    if (!I || !N || !out || n < 0) {
        rt_set_error("rt_debug_reflect: invalid argument");
        return RT_ERR_INVALID;
    }
    for (int i = 0; i < n; ++i) rf_reflect(I[i].x, I[i].y, I[i].z, N[i].x, N[i].y, N[i].z, out[i].x, out[i].y, out[i].z);
    return RT_OK;
}

extern "C" int rt_debug_gloss(const rt_vec3 *R, const rt_vec3 *N, const float *rho, const unsigned *key, const int *b, int n,
                              rt_vec3 *out, int *what)
{
    if (!R || !N || !rho || !key || !b || !out || n < 0) {
        rt_set_error("rt_debug_gloss: invalid argument");
        return RT_ERR_INVALID;
    }
    for (int i = 0; i < n; ++i) {
        V3 o;
        const int w = rf_gloss(V3{R[i].x, R[i].y, R[i].z}, V3{N[i].x, N[i].y, N[i].z}, rho[i], key[i], (uint32_t)b[i], o);
        out[i].x = o.x; out[i].y = o.y; out[i].z = o.z;
        if (what) what[i] = w;
    }
    return RT_OK;
}

extern "C" int rt_debug_gloss_key(const unsigned *px, const unsigned *py, const unsigned *s, const unsigned *seed, int n,
                                  unsigned *key)
{
    if (!px || !py || !s || !seed || !key || n < 0) {
        rt_set_error("rt_debug_gloss_key: invalid argument");
        return RT_ERR_INVALID;
    }
    for (int i = 0; i < n; ++i) key[i] = rf_gloss_key(px[i], py[i], s[i], seed[i]);
    return RT_OK;
}

extern "C" int rt_debug_reflect_entry_size(void) { return (int)sizeof(QEntry); }

extern "C" int rt_debug_refract(const rt_vec3 *I, const rt_vec3 *N, const float *eta, int n, rt_vec3 *out)
{
    if (!I || !N || !eta || !out || n < 0) {
        rt_set_error("rt_debug_refract: invalid argument");
        return RT_ERR_INVALID;
    }
    for (int i = 0; i < n; ++i)
        rf_refract(I[i].x, I[i].y, I[i].z, N[i].x, N[i].y, N[i].z, eta[i], out[i].x, out[i].y, out[i].z);
    return RT_OK;
}

extern "C" int rt_debug_transmit(const rt_sphere *sphere, const float *ior, const rt_ray *rays, int n, rt_ray *out,
                                 int *entered)
{
    if (!sphere || !ior || !rays || !out || !entered || n < 0) {
        rt_set_error("rt_debug_transmit: invalid argument");
        return RT_ERR_INVALID;
    }
    const float4 v[1] = {make_float4(sphere->orgin.x, sphere->orgin.y, sphere->orgin.z, sphere->radius * sphere->radius)};
    for (int i = 0; i < n; ++i) {
        const V3 O{rays[i].Org.x, rays[i].Org.y, rays[i].Org.z}, D{rays[i].Dir.x, rays[i].Dir.y, rays[i].Dir.z};
        out[i] = rays[i];
        float t;
        if (!rf_intersect(O.x, O.y, O.z, D.x, D.y, D.z, v[0], t)) {
            entered[i] = -1;
            continue;
        }
        V3 normal, start, new_org, ro, rd;
        rf_hit_frame(O, D, t, v[0], normal, start, new_org);
        entered[i] = rf_transmit(D, normal, start, new_org, v[0], ior[i], ro, rd);
        out[i].Org.x = ro.x; out[i].Org.y = ro.y; out[i].Org.z = ro.z;
        out[i].Dir.x = rd.x; out[i].Dir.y = rd.y; out[i].Dir.z = rd.z;
    }
    return RT_OK;
}

extern "C" int rt_debug_fresnel(const float *c, const float *ior, int n, float *F)
{
    if (!c || !ior || !F || n < 0) {
        rt_set_error("rt_debug_fresnel: invalid argument");
        return RT_ERR_INVALID;
    }
    for (int i = 0; i < n; ++i) F[i] = rf_fresnel(c[i], ior[i]);
    return RT_OK;
}

extern "C" int rt_debug_glass_choice(const rt_sphere *sphere, const float *ior, const float *rho, const unsigned *key,
                                     const int *b, const rt_ray *rays, int n, rt_ray *out, int *choice, float *F, float *u,
                                     int *what)
{
    if (!sphere || !ior || !rho || !key || !b || !rays || !out || !choice || n < 0) {
        rt_set_error("rt_debug_glass_choice: invalid argument");
        return RT_ERR_INVALID;
    }
    const float4 v[1] = {make_float4(sphere->orgin.x, sphere->orgin.y, sphere->orgin.z, sphere->radius * sphere->radius)};
    for (int i = 0; i < n; ++i) {
        const V3 O{rays[i].Org.x, rays[i].Org.y, rays[i].Org.z}, D{rays[i].Dir.x, rays[i].Dir.y, rays[i].Dir.z};
        out[i] = rays[i];
        float t, Fi = 0.f, ui = 0.f;
        int wi = 0;
        if (!rf_intersect(O.x, O.y, O.z, D.x, D.y, D.z, v[0], t)) {
            choice[i] = -1;
        } else {
            V3 normal, start, new_org, ro, rd;
            rf_hit_frame(O, D, t, v[0], normal, start, new_org);
            choice[i] = rf_fresnel_continue(true, D, normal, start, new_org, v[0], ior[i], rho[i], key[i], (uint32_t)b[i], ro,
                                            rd, Fi, ui, wi);
            out[i].Org.x = ro.x; out[i].Org.y = ro.y; out[i].Org.z = ro.z;
            out[i].Dir.x = rd.x; out[i].Dir.y = rd.y; out[i].Dir.z = rd.z;
        }
        if (F) F[i] = Fi;
        if (u) u[i] = ui;
        if (what) what[i] = wi;
    }
    return RT_OK;
}
