// rt_bvh.h -- the sphere BVH and the per-ray pieces shared by the reflective passes (rt_reflect.hip) and the ray
// queries (rt_query.hip): sphere::intersect on a table entry, the exact BVH walk (nearest and any-hit), the sky
// lookup, the hit frame of a sphere hit and the primary ray of a pixel. Stands on rt_exact.h (V3, AuxPtr, the primitive tests) and
// takes neither the culling, the shadow chain nor the frame kernel: rt_sphere_bvh.cpp, a host unit, includes it.
//
// The BVH (host build in binary64, leaves of <= 4 spheres) is exact against the list: its traversal never drops a
// sphere that sphere::intersect reports as hit, and the nearest hit is the lexicographic minimum of (t, index) --
// what the reference's strict `t < nt` loop returns. The margin and the pruning rule are derived in DESIGN.md.
#pragma once
#include "rt_exact.h"
#include "rt_internal.h"

#include <vector>

#define RT_BVH_LEAF 4
#define RT_BVH_STACK 24        // traversal stack entries per lane (LDS, 24 KiB per workgroup); the host refuses a deeper
                               // tree (a median split of the library's 4 M spheres is 21 deep)
#define RT_BVH_PAD_REL 1.5e-2  // ray-dependent box padding: RT_BVH_PAD_REL * (L1 distance to the box's far corner + largest
#define RT_BVH_PAD_ABS 1.0e-16 // radius) + RT_BVH_PAD_ABS: twice the bound 7e-3 derived in DESIGN.md "Reflections" 

#define RT_BVH_BLOCK 256       // workgroup size of the kernels that walk the BVH (one stack column per thread)

struct BvhNode {   // 48 bytes; children of an inner node are `first` and `first + 1`
    float lo[3];
    float rmax;    // largest sphere radius below the node (rounded up)
    float hi[3];
    int first;     // inner: first child; leaf: first position in order[] / lsph[]
    int count;     // 0: inner node; else the leaf's sphere count
    int axis;      // inner: split axis (the first child holds the lower centres)
    int pad_[2];
};

struct RtReflectDev {              // the passes' uniforms (by value)
    const BvhNode *nodes;          // null: walk the whole list (brute force, or a scene the BVH does not cover)
    const float4 *lsph;            // spheres in leaf order
    const int *order;              // their list positions
    const float4 *spheres;         // the list
    int n;
    const float *k;                // reflectivness per sphere (null: all 0)
    int depth;
    const float2 *glass;           // (transperancy, ior) per sphere (null: no sphere has transperancy > 0)
    const float *rough;            // roughness per sphere (null: all 0); read by the GLOSS passes only
};

// ---------------------------------------------------------------------------
// host & device: sphere::intersect, the BVH walk
// ---------------------------------------------------------------------------
// sphere::intersect, kernel.cu:293-354, on a table entry {cx,cy,cz,radius*radius}: the operations of quadratic() and
// intersect_tail() in rt_exact.h, in the same order (this file is compiled without contraction, both sides).
__host__ __device__ __forceinline__ bool rf_intersect(float ox, float oy, float oz, float dx, float dy, float dz,
                                                      float4 s, float &t)
{
    const float ocx = ox - s.x, ocy = oy - s.y, ocz = oz - s.z;
    const float h = (dx * ocx + dy * ocy) + dz * ocz;
    const float B = 2.f * h;
    const float C = ((ocx * ocx + ocy * ocy) + ocz * ocz) - s.w;
    const float A = (dx * dx + dy * dy) + dz * dz;
    const float disc = B * B - (4.f * A) * C;
    const float sq = __builtin_sqrtf(disc);
    const float a2 = 2.f * ((dx * dx + dy * dy) + dz * dz);
    t = (-B + sq) / a2;
    if (t == 0.f) return true;
    if (t >= RT_T_MIN) {
        const float t2 = (-B - sq) / a2;
        if (t > t2) t = t2;
        return true;
    }
    return false;
}

// The traversal's preconditions: a finite origin within 1e15 of the world origin and a direction of
// squared length in [0.9, 1.1] (every ray here is a unit vector up to rounding). Other rays walk the list.
__host__ __device__ __forceinline__ bool rf_ray_ok(float ox, float oy, float oz, float dx, float dy, float dz)
{
    const double A = ((double)dx * dx + (double)dy * dy) + (double)dz * dz;
    return __builtin_fabs((double)ox) <= 1e15 && __builtin_fabs((double)oy) <= 1e15 && __builtin_fabs((double)oz) <= 1e15 &&
           A >= 0.9 && A <= 1.1;   // false for a NaN anywhere
}

// The integer mixer of every hashed draw (glossy reflections; the indirect pass, 6o): uint32 throughout
// (wrapping)
__host__ __device__ __forceinline__ uint32_t rf_mix(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// The key of pixel (px, py) of the full frame at absolute sample s under the scene's seed
__host__ __device__ __forceinline__ uint32_t rf_gloss_key(uint32_t px, uint32_t py, uint32_t s, uint32_t seed)
{
    return rf_mix(rf_mix(rf_mix(rf_mix(seed) ^ s) ^ py) ^ px);
}

struct RayD {
    double o[3], inv[3];
    float d[3];
};

// The node's box padded for this ray (any sphere of the node that intersect() reports as hit puts its
// returned t inside [tmin, tmax] of this padded box, and tmax >= 0). Binary64 slab test, unclamped tmin.
__host__ __device__ __forceinline__ bool rf_node_test(const BvhNode &nd, const RayD &r, double &tmin)
{
    double dsum = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double e0 = __builtin_fabs(r.o[a] - (double)nd.lo[a]), e1 = __builtin_fabs(r.o[a] - (double)nd.hi[a]);
        dsum += e0 > e1 ? e0 : e1;
    }
    const double pad = RT_BVH_PAD_REL * (dsum + (double)nd.rmax) + RT_BVH_PAD_ABS;
    double t0 = -__builtin_inf(), t1 = __builtin_inf();
    for (int a = 0; a < 3; ++a) {
        const double lo = (double)nd.lo[a] - pad, hi = (double)nd.hi[a] + pad;
        if (r.d[a] == 0.f) {
            if (r.o[a] < lo || r.o[a] > hi) return false;
        } else {
            double ta = (lo - r.o[a]) * r.inv[a], tb = (hi - r.o[a]) * r.inv[a];
            if (ta > tb) { const double x = ta; ta = tb; tb = x; }
            t0 = ta > t0 ? ta : t0;
            t1 = tb < t1 ? tb : t1;
        }
    }
    tmin = t0;
    return t0 <= t1 && t1 >= 0.0;
}

// Nearest hit (ANY = false: lexicographic minimum of (t, list index), -1 = none) or any-hit (ANY = true: returns 0 / 1).
// STK(i) is the lane's i-th stack slot.
template <bool ANY, class Stack>
__host__ __device__ __forceinline__ int rf_cast(const RtReflectDev &rd, float ox, float oy, float oz, float dx, float dy,
                                                float dz, float &t_best, Stack stk)
{
    int best = -1;
    float bt = __builtin_inff();
    if (!rd.nodes || !rf_ray_ok(ox, oy, oz, dx, dy, dz)) {
        for (int i = 0; i < rd.n; ++i) {
            float t;
            if (rf_intersect(ox, oy, oz, dx, dy, dz, rd.spheres[i], t)) {
                if (ANY) { t_best = t; return 1; }
                if (t < bt) { bt = t; best = i; }   // kernel.cu:1335: strict, the first index wins ties
            }
        }
        t_best = bt;
        return ANY ? 0 : best;
    }
    RayD r;
    r.o[0] = ox; r.o[1] = oy; r.o[2] = oz;
    r.d[0] = dx; r.d[1] = dy; r.d[2] = dz;
    r.inv[0] = 1.0 / (double)dx; r.inv[1] = 1.0 / (double)dy; r.inv[2] = 1.0 / (double)dz;
    int sp = 0;
    stk(sp++) = 0;
    while (sp > 0) {
        const BvhNode nd = rd.nodes[stk(--sp)];
        double tmin;
        if (!rf_node_test(nd, r, tmin)) continue;
        if (!ANY && tmin > (double)bt) continue;   // every hit inside has t >= tmin > bt (unclamped tmin: DESIGN.md)
        if (nd.count == 0) {
            // the nearer child last (popped first): the first child holds the lower centres along `axis`
            const bool up = (nd.axis == 0 ? r.d[0] : (nd.axis == 1 ? r.d[1] : r.d[2])) >= 0.f;   // (no dynamic index: scratch)
            stk(sp++) = up ? nd.first + 1 : nd.first;
            stk(sp++) = up ? nd.first : nd.first + 1;
            continue;
        }
        for (int p = nd.first; p < nd.first + nd.count; ++p) {
            float t;
            if (rf_intersect(ox, oy, oz, dx, dy, dz, rd.lsph[p], t)) {
                if (ANY) { t_best = t; return 1; }
                const int idx = rd.order[p];
                if (t < bt || (t == bt && idx < best)) { bt = t; best = idx; }
            }
        }
    }
    t_best = bt;
    return ANY ? 0 : best;
}

namespace {

struct LdsStack {
    int *base;   // this workgroup's stack array, slot i of thread tid at base[i * RT_BVH_BLOCK + tid]
    int tid;
    __device__ int &operator()(int i) const { return base[i * RT_BVH_BLOCK + tid]; }
};

// Append the wave's lanes with `push` set to a queue whose length is *count (one atomic per wave, the first such
// lane's): returns the lane's index in the queue, 0 without `push`. The ballot and the readlane are the wave's: every
// lane of the wave reaches the call, and in a loop a lane without an entry is switched off by its flag, never by
// leaving the loop.
__device__ __forceinline__ int rf_wave_append(bool push, int *count)
{
    const lmask m = ballot64(push);
    if (m == 0) return 0;
    const int leader = __builtin_ctzll(m);
    int b = 0;
    if ((int)(threadIdx.x & 63u) == leader) b = atomicAdd(count, __popcll(m));
    const int base = __builtin_amdgcn_readlane(b, leader);
    return push ? base + lane_prefix(m) : 0;
}

// skybox::getFColor, kernel.cu:1147-1166, as the frame kernel's brute-force instantiation evaluates it
__device__ __forceinline__ void rf_sky(AuxPtr ax, V3 O, V3 D, float &r, float &g, float &b)
{
    const RayK pr = make_ray(O, D);
    const float4 sk = make_float4(ax->sky_cx, ax->sky_cy, ax->sky_cz, ax->sky_r2);
    const Quad q = quadratic(pr, sk);
    float t;
    intersect_tail(pr, q, t);   // the boolean is ignored there, t is used as left
    const V3 hp{O.x + D.x * t, O.y + D.y * t, O.z + D.z * t};
    V3 nrm{hp.x - sk.x, hp.y - sk.y, hp.z - sk.z};
    normalise_inplace(nrm);
    const int sky_w = ax->sky_w, sky_h = ax->sky_h;
    const int ix = f2i((1.f + rtm::atan2f_rt(nrm.z, nrm.x) / 3.1415f) * 0.5f * (float)sky_w);
    const int iy = f2i(rtm::acosf_rt(nrm.y) / 3.1415f * (float)sky_h);
    int idx = iy * sky_w + ix;
    const int last = sky_w * sky_h - 1;
    idx = idx < 0 ? 0 : (idx > last ? last : idx);   // documented clamp (as the frame kernel)
    r = ax->sky_r[idx];
    g = ax->sky_g[idx];
    b = ax->sky_b[idx];
}

// normalise_inplace (rt_exact.h) for host and device: the same operations (the host debug entries run them)
__host__ __device__ __forceinline__ void rf_normalise(V3 &v)
{
    const float l = __builtin_sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z);
    if (l != 0.f) {
        v.x = v.x / l;
        v.y = v.y / l;
        v.z = v.z / l;
    }
}

// The hit point, normal and start_O of castRay's / rayTrace's sphere branch (kernel.cu:1398-1405, 1647)
__host__ __device__ __forceinline__ void rf_hit_frame(V3 O, V3 D, float nt, float4 s, V3 &normal, V3 &start, V3 &new_org)
{
    new_org = V3{O.x + D.x * nt, O.y + D.y * nt, O.z + D.z * nt};
    normal = V3{new_org.x - s.x, new_org.y - s.y, new_org.z - s.z};
    rf_normalise(normal);
    start = V3{normal.x * 0.00001f + new_org.x, normal.y * 0.00001f + new_org.y, normal.z * 0.00001f + new_org.z};
}
__host__ __device__ __forceinline__ void rf_hit_frame(V3 O, V3 D, float nt, float4 s, V3 &normal, V3 &start)
{
    V3 new_org;
    rf_hit_frame(O, D, nt, s, normal, start, new_org);
}

// The direction of the primary ray of band-local pixel `pix` (kernel.cu:1624-1631), as the frame kernel forms it for
// sample `sidx` of the tables' total (row sidx of dx_tab / dy_tab; 0: the only sample of a one-sample frame); its origin
// is {fc.org_x, fc.org_y, fc.org_z}
__device__ __forceinline__ V3 rf_primary_dir(const RtFrameConsts &fc, int pix, int sidx = 0)
{
    const int ly = pix / fc.width, px = pix - ly * fc.width;
    const int py = fc.y0 + ly;
    V3 dir{fc.dx_tab[sidx * fc.width + px], fc.dy_tab[sidx * fc.height + py], fc.eye_nz};
    normalise_inplace(dir);
    const float y = dir.y * fc.cos_pitch - dir.z * fc.sin_pitch;
    float z = dir.y * fc.sin_pitch + dir.z * fc.cos_pitch;
    const float x = dir.x * fc.cos_yaw + z * fc.sin_yaw;
    z = -dir.x * fc.sin_yaw + z * fc.cos_yaw;
    return V3{x, y, z};
}

}  // namespace

// The sphere BVH of the scene's list (host copy and device arrays), built once per sphere generation and shared by
// reflective frames and ray queries.
struct RtSphereBvh {
    unsigned long long gen = ~0ull;       // sphere_gen it was built from
    int n = -1;
    bool ok = false;                      // false: the list is walked (non-finite or huge data)
    std::vector<BvhNode> nodes;
    std::vector<float4> lsph;
    std::vector<int> order;
    DevArray<BvhNode> d_nodes;
    DevArray<float4> d_lsph;
    DevArray<int> d_order;
    int depth = 0, leaves = 0;
    double build_ms = 0.0;
};
// rt_sphere_bvh_stale: whether rt_sphere_bvh_update would rebuild it (the caller must first wait for every reader of the
// device arrays); rt_sphere_bvh_update: rebuild and upload on `stream` when stale (rt_sphere_bvh.cpp, declared in
// rt_internal.h)
