// rt_sphere_bvh.cpp -- the host side of the sphere BVH (rt_bvh.h) that reflective frames and ray queries share: the build
// (binary64 extents, binary32 boxes rounded outward, median split), the per-generation rebuild with its upload, and the
// host-only debug entries that walk a BVH on the host (rf_cast is host / device). No kernel is launched from here.
#include "rt_bvh.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

static int rf_build_rec(const std::vector<float4> &sph, std::vector<int> &idx, int lo, int hi, int node, int level,
                        RtSphereBvh *r)
{
    r->depth = level > r->depth ? level : r->depth;
    double blo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, bhi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    double clo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, chi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    double rmax = 0.0;
    for (int p = lo; p < hi; ++p) {
        const float4 s = sph[idx[p]];
        const double c[3] = {s.x, s.y, s.z};
        const double R = std::sqrt((double)s.w);   // intersect() squares the `radius` field: its radius is sqrt(w)
        rmax = R > rmax ? R : rmax;
        for (int a = 0; a < 3; ++a) {
            blo[a] = std::min(blo[a], c[a] - R);
            bhi[a] = std::max(bhi[a], c[a] + R);
            clo[a] = std::min(clo[a], c[a]);
            chi[a] = std::max(chi[a], c[a]);
        }
    }
    BvhNode &nd = r->nodes[node];
    for (int a = 0; a < 3; ++a) {   // rounded outward to binary32
        float l = (float)blo[a], h = (float)bhi[a];
        if ((double)l > blo[a]) l = std::nextafter(l, -HUGE_VALF);
        if ((double)h < bhi[a]) h = std::nextafter(h, HUGE_VALF);
        nd.lo[a] = l;
        nd.hi[a] = h;
    }
    float rm = (float)rmax;
    if ((double)rm < rmax) rm = std::nextafter(rm, HUGE_VALF);
    nd.rmax = rm;
    if (hi - lo <= RT_BVH_LEAF) {
        nd.first = lo;
        nd.count = hi - lo;
        nd.axis = 0;
        r->leaves++;
        return RT_OK;
    }
    int axis = 0;
    for (int a = 1; a < 3; ++a)
        if (chi[a] - clo[a] > chi[axis] - clo[axis]) axis = a;
    const int mid = lo + (hi - lo) / 2;   // median split: depth <= ceil(log2(n / 4)) + 1
    auto key = [&](int i) { const float4 s = sph[i]; return axis == 0 ? s.x : (axis == 1 ? s.y : s.z); };
    std::nth_element(idx.begin() + lo, idx.begin() + mid, idx.begin() + hi, [&](int a, int b) {
        const float ka = key(a), kb = key(b);
        return ka < kb || (ka == kb && a < b);
    });
    const int child = (int)r->nodes.size();
    r->nodes.resize(r->nodes.size() + 2);
    BvhNode &nd2 = r->nodes[node];   // (resize may move the array)
    nd2.first = child;
    nd2.count = 0;
    nd2.axis = axis;
    int rc = rf_build_rec(sph, idx, lo, mid, child, level + 1, r);
    if (rc != RT_OK) return rc;
    return rf_build_rec(sph, idx, mid, hi, child + 1, level + 1, r);
}

// Host build (binary64 extents, binary32 boxes rounded outward). ok = false when a sphere is non-finite or lies
// beyond 1e15 (the traversal's derivation assumes neither): every ray then walks the list.
static int rf_build(RtSphereBvh *r, const float4 *sph, int n)
{
    const auto t0 = std::chrono::steady_clock::now();
    r->nodes.clear();
    r->lsph.clear();
    r->order.clear();
    r->depth = 0;
    r->leaves = 0;
    r->ok = n > 0;
    for (int i = 0; i < n && r->ok; ++i) {
        const float4 s = sph[i];
        const double R = std::sqrt((double)s.w);
        if (!(std::fabs((double)s.x) + R <= 1e15 && std::fabs((double)s.y) + R <= 1e15 && std::fabs((double)s.z) + R <= 1e15))
            r->ok = false;   // (false for NaN / inf too)
    }
    if (r->ok) {
        std::vector<float4> v(sph, sph + n);
        std::vector<int> idx((size_t)n);
        for (int i = 0; i < n; ++i) idx[(size_t)i] = i;
        r->nodes.reserve((size_t)2 * n);
        r->nodes.resize(1);
        int rc = rf_build_rec(v, idx, 0, n, 0, 0, r);
        if (rc != RT_OK) return rc;
        if (r->depth + 2 > RT_BVH_STACK) {   // the stack holds at most depth + 1 entries (two pushed per inner node)
            rt_set_error("reflections: sphere BVH depth %d exceeds the traversal stack (%d)", r->depth, RT_BVH_STACK);
            return RT_ERR_CAPACITY;
        }
        r->order = idx;
        r->lsph.resize((size_t)n);
        for (int p = 0; p < n; ++p) r->lsph[(size_t)p] = v[(size_t)idx[(size_t)p]];
    }
    r->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return RT_OK;
}

bool rt_sphere_bvh_stale(const RtSphereBvh *b, unsigned long long sphere_gen, int n) { return b->gen != sphere_gen || b->n != n; }

int rt_sphere_bvh_update(RtSphereBvh *b, const float4 *h_spheres, int n, unsigned long long sphere_gen, hipStream_t stream)
{
    if (!rt_sphere_bvh_stale(b, sphere_gen, n)) return RT_OK;
    const int rc = rf_build(b, h_spheres, n);
    if (rc != RT_OK) return rc;
    if (b->ok) {
        RT_HIP(b->d_nodes.reserve(b->nodes.size()));
        RT_HIP(b->d_lsph.reserve((size_t)n));
        RT_HIP(b->d_order.reserve((size_t)n));
        RT_HIP(hipMemcpyAsync(b->d_nodes.get(), b->nodes.data(), sizeof(BvhNode) * b->nodes.size(), hipMemcpyHostToDevice, stream));
        RT_HIP(hipMemcpyAsync(b->d_lsph.get(), b->lsph.data(), sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, stream));
        RT_HIP(hipMemcpyAsync(b->d_order.get(), b->order.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, stream));
    }
    b->gen = sphere_gen;
    b->n = n;
    return RT_OK;
}

static RtReflectDev rf_host_view(const RtSphereBvh *r, const float4 *sph, int n, bool use_bvh)
{
    RtReflectDev rd{};
    rd.nodes = (use_bvh && r->ok) ? r->nodes.data() : nullptr;
    rd.lsph = r->lsph.data();
    rd.order = r->order.data();
    rd.spheres = sph;
    rd.n = n;
    return rd;
}

// ---------------------------------------------------------------------------
// host-only debug entries (tests)
// ---------------------------------------------------------------------------
static void pack_list(const rt_sphere *s, int n, std::vector<float4> &v)
{
    v.resize((size_t)n);
    for (int i = 0; i < n; ++i)
        v[(size_t)i] = make_float4(s[i].orgin.x, s[i].orgin.y, s[i].orgin.z, s[i].radius * s[i].radius);
}

extern "C" int rt_debug_sphere_bvh(const rt_sphere *spheres, int n, float *lohi, int *meta, int *order, int cap,
                                   int *n_nodes, int *depth)
{
    if (!spheres || n <= 0 || !lohi || !meta || !order || !n_nodes || !depth) {
        rt_set_error("rt_debug_sphere_bvh: invalid argument");
        return RT_ERR_INVALID;
    }
    std::vector<float4> v;
    pack_list(spheres, n, v);
    RtSphereBvh r;
    const int rc = rf_build(&r, v.data(), n);
    if (rc != RT_OK) return rc;
    if (!r.ok) {
        rt_set_error("rt_debug_sphere_bvh: the list has non-finite or huge spheres (no BVH: the list is walked)");
        return RT_ERR_UNSUPPORTED;
    }
    if ((int)r.nodes.size() > cap) {
        rt_set_error("rt_debug_sphere_bvh: %d nodes exceed cap %d", (int)r.nodes.size(), cap);
        return RT_ERR_CAPACITY;
    }
    for (size_t j = 0; j < r.nodes.size(); ++j) {
        for (int a = 0; a < 3; ++a) {
            lohi[6 * j + a] = r.nodes[j].lo[a];
            lohi[6 * j + 3 + a] = r.nodes[j].hi[a];
        }
        meta[2 * j] = r.nodes[j].first;
        meta[2 * j + 1] = r.nodes[j].count;
    }
    for (int p = 0; p < n; ++p) order[p] = r.order[(size_t)p];
    *n_nodes = (int)r.nodes.size();
    *depth = r.depth;
    return RT_OK;
}

extern "C" int rt_debug_bvh_cast(const rt_sphere *spheres, int n, const rt_ray *rays, int n_rays, int use_bvh,
                                 int *hit_index, float *t, int *any)
{
    if (!spheres || n <= 0 || !rays || n_rays < 0) {
        rt_set_error("rt_debug_bvh_cast: invalid argument");
        return RT_ERR_INVALID;
    }
    std::vector<float4> v;
    pack_list(spheres, n, v);
    RtSphereBvh r;
    int rc = RT_OK;
    if (use_bvh) rc = rf_build(&r, v.data(), n);
    if (rc != RT_OK) return rc;
    const RtReflectDev rd = rf_host_view(&r, v.data(), n, use_bvh != 0);
    int stack[RT_BVH_STACK];
    auto stk = [&stack](int i) -> int & { return stack[i]; };
    for (int i = 0; i < n_rays; ++i) {
        const rt_ray &ray = rays[i];
        if (hit_index || t) {
            float tb;
            const int h = rf_cast<false>(rd, ray.Org.x, ray.Org.y, ray.Org.z, ray.Dir.x, ray.Dir.y, ray.Dir.z, tb, stk);
            if (hit_index) hit_index[i] = h;
            if (t) t[i] = tb;
        }
        if (any) {
            float ta;
            any[i] = rf_cast<true>(rd, ray.Org.x, ray.Org.y, ray.Org.z, ray.Dir.x, ray.Dir.y, ray.Dir.z, ta, stk);
        }
    }
    return RT_OK;
}
