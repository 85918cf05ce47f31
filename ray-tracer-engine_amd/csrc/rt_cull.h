// rt_cull.h -- conservative culling: the beams that bound a tile's rays, the keep tests against them and the
// wave-cooperative list builders (build_list2, build_list_cand, build_box_list). Included by rt_shadow.h (and so by
// the frame kernel) and by rt_tables.hip, which builds the per-view candidate lists with the same code.
#pragma once
#include "rt_exact.h"

namespace {

// A ray that starts outside a sphere whose centre lies behind it has B > 0 and
// disc < B*B; then sqrt(disc) < B, t < 0 strictly and intersect() is false. The
// factor keeps sqrt(disc) below B even after rounding, so the `t == 0` clause
// (kernel.cu:338) cannot fire. Purely a shortcut: when in doubt the full tail runs.
#define RT_BEHIND_FACTOR 0.99999f

// ---------------------------------------------------------------------------
// conservative culling
// ---------------------------------------------------------------------------
struct Beam {        // all members wave-uniform
    float ax, ay, az;   // a point on the axis
    float ux, uy, uz;   // unit axis
    float smin;         // rays start at axial coordinate >= smin
    float smax;         // ... and <= smax (used only by the full-occluder test)
    float r0;           // ... within r0 of the axis
    float k;            // and spread with slope k = tan(theta)
};

// Keep sphere s unless no ray inside the beam can make intersect() return true.
// intersect() is true only if the float discriminant is >= 0, which (rounding
// included) needs the ray's line within sqrt(R^2 + eps*(1+|oc|^2)) of the centre
// (R^2 = s.w is the squared effective radius), and a far root >= 0.
__device__ __forceinline__ lmask beam_keeps(const Beam &b, float4 s)
{
    const float vx = s.x - b.ax, vy = s.y - b.ay, vz = s.z - b.az;
    const float vv = __builtin_fmaf(vx, vx, __builtin_fmaf(vy, vy, vz * vz));
    const float sa = __builtin_fmaf(vx, b.ux, __builtin_fmaf(vy, b.uy, vz * b.uz));
    const float d2 = __builtin_fmaxf(__builtin_fmaf(-sa, sa, vv), 0.f);
    // padded radius: rounding noise of the exact test + slack of this test
    const float rc2 = s.w + __builtin_fmaf(RT_PAD_REL, vv, RT_PAD_ABS);
    const float rc = __builtin_amdgcn_sqrtf(rc2) * 1.0001f;
    const float reach = sa + rc - b.smin;
    const float rad = __builtin_fmaf(b.k, __builtin_fmaxf(reach, 0.f), b.r0) + rc;
    return LM(reach >= 0.f) & LM(d2 <= rad * rad * 1.0005f);
}

// A block of the Morton-ordered table: {centre, radius} of a sphere containing all
// of its members (host side, rounded up). A member passes beam_keeps() only if
// the block passes this test: the block's padded radius covers the member's
// centre offset, its radius and its own padding sqrt(4e-5*|v|^2 + 1e-3)
// (<= 6.4e-3*|v| + 0.032 with |v| <= |v_block| + r_block).
__device__ __forceinline__ lmask beam_keeps_block(const Beam &b, float4 blk)
{
    const float vx = blk.x - b.ax, vy = blk.y - b.ay, vz = blk.z - b.az;
    const float vv = __builtin_fmaf(vx, vx, __builtin_fmaf(vy, vy, vz * vz));
    const float sa = __builtin_fmaf(vx, b.ux, __builtin_fmaf(vy, b.uy, vz * b.uz));
    const float d2 = __builtin_fmaxf(__builtin_fmaf(-sa, sa, vv), 0.f);
    const float dist = __builtin_amdgcn_sqrtf(vv) * 1.0001f;
    const float rc = __builtin_fmaf(RT_BLK_PAD_REL, dist + blk.w, blk.w) + RT_BLK_PAD_ABS;
    const float reach = sa + rc - b.smin;
    const float rad = __builtin_fmaf(b.k, __builtin_fmaxf(reach, 0.f), b.r0) + rc;
    return LM(!(reach < 0.f)) & LM(!(d2 > rad * rad * 1.0005f));   // NaN / inf bounds keep the block
}

// A column block of a light's table (RtFrameConsts::lsorted/lblocks): blkA = {point c on the
// column's axis, lateral radius rho}, blkB = {s_hi, r3d, -, -}. A member j passes
// beam_member_test() only if its block passes this test: its axial coordinate plus radius is
// at most (c - a).u + s_hi, its centre lies within rho - R_j of the column's axis, and its
// padding sqrt(4e-5 |v_j|^2 + 1e-3) <= 6.4e-3 |v_j| + 0.032 with |v_j| <= |c - a| + r3d.
// Only valid for beams whose axis is the light's u (all shadow beams are).
__device__ __forceinline__ lmask beam_keeps_column(const Beam &b, float4 blkA, float4 blkB)
{
    const float vx = blkA.x - b.ax, vy = blkA.y - b.ay, vz = blkA.z - b.az;
    const float vv = __builtin_fmaf(vx, vx, __builtin_fmaf(vy, vy, vz * vz));
    const float sa = __builtin_fmaf(vx, b.ux, __builtin_fmaf(vy, b.uy, vz * b.uz));
    const float d2 = __builtin_fmaxf(__builtin_fmaf(-sa, sa, vv), 0.f);
    const float dist = __builtin_amdgcn_sqrtf(vv) * 1.0001f;
    const float pad = __builtin_fmaf(RT_BLK_PAD_REL, dist + blkB.y, RT_BLK_PAD_ABS);
    const float reach = sa + blkB.x + pad - b.smin;
    const float rad = __builtin_fmaf(b.k, __builtin_fmaxf(reach, 0.f), b.r0) + blkA.w + pad;
    return LM(!(reach < 0.f)) & LM(!(d2 > rad * rad * 1.001f));   // NaN / inf bounds keep the block
}

// An entry of the list being walked: the wave's survivor list, or the whole table.
__device__ __forceinline__ float4 entry_at(bool use_list, const float4 *list, const float4 *__restrict__ gl_tab, int e)
{
    if (use_list) return list[e];
    return gl_tab[e];
}

// The member test of the culling loop: beam_keeps(), and with OCCL the question whether the
// sphere occludes the whole beam, in one straight line -- the two share |v|^2, the axial
// coordinate and the distance from the axis, and written with short-circuit conditions the
// compiler wraps every clause in its own exec-mask region (a third of the loop's instructions).
// `blocked`, only meaningful for kept entries:
// Sphere s certainly occludes EVERY ray of the beam: it lies entirely ahead of all
// ray origins, and the beam's cross-section at the centre's axial coordinate --
// radius r0 + k*(sa - smin) around the axis, both already padded -- sits inside
// the sphere shrunk by the same rounding allowance the cull test adds. Each ray
// then passes within that shrunken radius of the centre in its forward direction,
// so the exact float test has disc > 0 and h far below -h_sure: it returns true.
template <bool OCCL>
__device__ __forceinline__ lmask beam_member_test(const Beam &b, float4 s, lmask enable, lmask &blocked)
{
    const float vx = s.x - b.ax, vy = s.y - b.ay, vz = s.z - b.az;
    const float vv = __builtin_fmaf(vx, vx, __builtin_fmaf(vy, vy, vz * vz));
    const float sa = __builtin_fmaf(vx, b.ux, __builtin_fmaf(vy, b.uy, vz * b.uz));
    const float d2 = __builtin_fmaxf(__builtin_fmaf(-sa, sa, vv), 0.f);
    const float pad = __builtin_fmaf(RT_PAD_REL, vv, RT_PAD_ABS);
    const float rc = __builtin_amdgcn_sqrtf(s.w + pad) * 1.0001f;
    const float reach = sa + rc - b.smin;
    const float rad = __builtin_fmaf(b.k, __builtin_fmaxf(reach, 0.f), b.r0) + rc;
    const lmask keep = enable & LM(reach >= 0.f) & LM(d2 <= rad * rad * 1.0005f);
    if (OCCL) {
        const float r2b = s.w - pad;                                       // shrunken radius^2
        const float rr = __builtin_amdgcn_sqrtf(s.w);
        const lmask ahead = LM((sa - b.smax) >= __builtin_fmaf(rr, 1.001f, 0.01f));
        const float rho = __builtin_fmaf(b.k, sa - b.smin, b.r0);
        // (d2 = |v|^2 - (v.u)^2 carries a cancellation error of up to 3 eps |v|^2: its root is taken of an upper bound)
        const float lhs = __builtin_fmaf(__builtin_amdgcn_sqrtf(__builtin_fmaf(2.0e-7f, vv, d2)) + rho, 1.001f, 1.0e-4f);
        blocked |= keep & ahead & LM(r2b > 0.f) & LM(lhs * lhs <= r2b);
    }
    return keep;
}

// Two-level cull over an ordered copy of the table: the blocks of RT_BLOCK the beam can touch,
// then their members (64/RT_BLOCK blocks per step). Survivors come out in the table's order,
// which is fine for an any-hit; for the primary rays (ORDERED) their list positions are
// carried along in keys[] and the short list is re-ordered front to back (see below), ties
// between equal t being settled by those positions (kernel.cu:1335). Returns the survivor
// count (with OCCL, bit 30 flags "one sphere occludes the whole beam"); a count above
// RT_LIST_CAP tells the caller to walk the whole table instead.
// BLOCKS selects the first level: 0 = cubes of the 3-D order (fc.sorted/fc.blocks), 1 = a
// light's columns, 2 = eye cones (the last two: csorted/cblocks/corig, read from global memory).
template <int STATS, bool OCCL, bool ORDERED, int BLOCKS = 0, typename FC = RtFrameConsts>
__device__ __forceinline__ int build_list2(const FC &fc, int n, float4 *list, int *keys,
                                           int *blist, const Beam &b, int lane, unsigned long long &n_cull,
                                           const float4 *__restrict__ csorted = nullptr,
                                           const float4 *__restrict__ cblocks = nullptr,
                                           const int *__restrict__ corig = nullptr, bool stop_when_blocked = false)
{
    constexpr bool COLUMNS = BLOCKS != 0;   // two float4 per block, table in global memory
    const float4 *__restrict__ gsorted = COLUMNS ? csorted : reinterpret_cast<const float4 *>(fc.sorted);
    const float4 *__restrict__ gblocks = COLUMNS ? cblocks : reinterpret_cast<const float4 *>(fc.blocks);
    const int *__restrict__ gorig = COLUMNS ? corig : fc.orig_idx;
    // eye cones: cos and sin of the beam's own half-angle (slope padded as in the host's bound)
    float cone_cw = 1.f, cone_sw = 0.f;
    if (BLOCKS == 2) {
        const float kw = b.k * 1.001f;
        cone_cw = __builtin_amdgcn_rsqf(__builtin_fmaf(kw, kw, 1.f));
        cone_sw = kw * cone_cw;
    }
    const int nb = fc.n_blocks;
    int count = 0;
    lmask blk = 0;
    constexpr int G = 64 / RT_BLOCK;           // blocks examined side by side in one step
    const int grp = lane / RT_BLOCK, sub = lane % RT_BLOCK;
    for (int bbase = 0; bbase < nb; bbase += 64) {
        const int bi = bbase + lane;
        const int bc = bi < nb ? bi : nb - 1;
        lmask bm;
        if (BLOCKS == 2) {
            // angle(axis, beam axis) <= theta + theta_beam, both below pi (build_eye_cones)
            const float4 ba = gblocks[2 * bc], bbx = gblocks[2 * bc + 1];
            const float dotp = __builtin_fmaf(ba.x, b.ux, __builtin_fmaf(ba.y, b.uy, ba.z * b.uz));
            const float rhs = __builtin_fmaf(ba.w, cone_cw, -bbx.x * cone_sw) - 2.0e-5f;   // cos(theta + theta_beam)
            const lmask inside = LM(!(dotp < rhs));                                            // NaN keeps the block
            bm = LM(bi < nb) & LM(bbx.y >= 0.f) & (LM(bbx.y > 0.f) | inside);
        } else if (BLOCKS == 1) {
            const float4 ba = gblocks[2 * bc], bbx = gblocks[2 * bc + 1];
            bm = LM(bi < nb) & LM(!(ba.w < 0.f)) & beam_keeps_column(b, ba, bbx);
        } else {
            const float4 bb = gblocks[bc];
            bm = LM(bi < nb) & LM(!(bb.w < 0.f)) & beam_keeps_block(b, bb);   // w < 0: padding block
        }
        if (STATS == 1) n_cull += 64;
        // the marked blocks, compacted into the wave's block list; then G of them per step,
        // one per group of RT_BLOCK lanes (next step's block number read one step ahead)
        const int marked = __popcll(bm);
        if (lane_in(bm)) blist[lane_prefix(bm)] = bi;
        wave_lds_sync();
        int cur = (grp < marked) ? blist[grp] : -1;
        for (int t = 0; t < marked; t += G) {
            const int nslot = t + G + grp;
            const int nxt = (nslot < marked) ? blist[nslot] : -1;
            const int i = (cur < 0 ? 0 : cur) * RT_BLOCK + sub;   // inside the padded table
            const float4 s = gsorted[i];
            const lmask m = beam_member_test<OCCL>(b, s, LM(cur >= 0) & LM(i < n), blk);
            const int pos = count + lane_prefix(m);
            if (lane_in(m) && pos < RT_LIST_CAP) {
                list[pos] = s;
                if (ORDERED) keys[pos] = gorig[i];
            }
            count += __popcll(m);
            if (STATS == 1) n_cull += 64;
            cur = nxt;
            // the caller only wants to know whether one sphere occludes the whole beam, and one does:
            // the rest of the list is of no interest (the light adds nothing)
            if (OCCL && stop_when_blocked && blk != 0) {
                wave_lds_sync();
                return count | 0x40000000;
            }
        }
        if (bbase + 64 < nb) wave_lds_sync();   // the next 64 blocks reuse the block list
    }
    wave_lds_sync();
    if (ORDERED) {
        if (count > 64) {
            count = RT_LIST_CAP + 1;     // too long to reorder in one step: caller walks the table
        } else if (count > 1) {
            // Front to back: the list is ordered by a LOWER BOUND of any t the entry can return
            // to a ray from the apex (|D| = 1): dist - R outside the sphere, -(dist + R) inside
            // (the near root is what intersect() returns), less an allowance for the float
            // evaluation. That allowance is set by grazing rays: B^2 - 4AC is formed with an
            // absolute error of about 12 ulp(dist^2) = 3e-6 dist^2, so sqrt(disc) -- and with it
            // the near root -- can be off by sqrt(7.5e-7) dist = 8.7e-4 dist where the exact
            // discriminant vanishes (where it does not, the error is far smaller and the exact
            // root exceeds dist - R by up to R): 1e-3 + 1.5e-3 (dist + R) covers both cases.
            // The caller stops as soon as every lane's nearest hit lies
            // strictly below the next entry's bound; ties between equal t are resolved by the
            // list positions in keys[] (first index wins, kernel.cu:1335), so the order of
            // evaluation does not matter. The bounds go where the block list was (<= 64 entries).
            float *lbs = reinterpret_cast<float *>(blist);
            float4 e = make_float4(0.f, 0.f, 0.f, 0.f);
            int key = 0, rank = 0;
            float lb = 0.f;
            if (lane < count) {
                e = list[lane];
                key = keys[lane];
                const float vx = e.x - b.ax, vy = e.y - b.ay, vz = e.z - b.az;
                const float vv = __builtin_fmaf(vx, vx, __builtin_fmaf(vy, vy, vz * vz));
                const float dist = __builtin_amdgcn_sqrtf(vv), rr = __builtin_amdgcn_sqrtf(e.w);
                const float slack = __builtin_fmaf(1.5e-3f, dist + rr, 1.0e-3f);
                lb = (vv > e.w * 1.001f + 1.0e-6f) ? (dist - rr) - slack : -(dist + rr) - slack;
                lb = (lb == lb) ? lb : -__builtin_inff();   // non-finite entries first: they never end the walk early
                lbs[lane] = lb;
            }
            wave_lds_sync();
            for (int j = 0; j < count; ++j) {
                const float lj = lbs[j];
                // (ties go to the lower slot: `j < lane` is the scalar mask of the lanes above j)
                rank += lane_in(LM(lj < lb) | (LM(lj == lb) & (~1ull << j))) ? 1 : 0;
            }
            wave_lds_sync();
            if (lane < count) {
                list[rank] = e;
                keys[rank] = key;
                lbs[rank] = lb;
            }
            wave_lds_sync();
        }
    }
    if (OCCL && blk != 0) count |= 0x40000000;
    return count;
}

// The cull of a light's table for a group of pixels whose closest hit is ONE sphere S: the entries that a shadow ray
// from S can hit at all were listed when the scene or the light last changed (RtFrameAux::cand_hdr / cand_ent,
// rt_tables.hip: rt_occluder_lists_kernel -- a beam of slope kcap from a ball around S; the caller has checked its own
// slope against kcap), in table order, and only those are put to the member test -- one step per 64 of them, where the walk over the light's column blocks takes
// a block pass and three or four member steps. Same result convention as build_list2<OCCL = true>.
template <int STATS>
__device__ __forceinline__ int build_list_cand(const float4 *__restrict__ ents, int n, float4 *list, const Beam &b, int lane,
                                               unsigned long long &n_cull, bool stop_when_blocked)
{
    int count = 0;
    lmask blk = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const float4 s = ents[i];                       // the entry array is padded to whole steps
        const lmask m = beam_member_test<true>(b, s, LM(i < n), blk);
        const int pos = count + lane_prefix(m);
        if (lane_in(m) && pos < RT_LIST_CAP) list[pos] = s;
        count += __popcll(m);
        if (STATS == 1) n_cull += 64;
        if (stop_when_blocked && blk != 0) {
            wave_lds_sync();
            return count | 0x40000000;
        }
    }
    wave_lds_sync();
    if (blk != 0) count |= 0x40000000;
    return count;
}

// One triangle of a leaf against the beam, by its bounding sphere ts = {centre, radius} and tn = {unit normal, kappa}
// (host side: rt_scene_set_mesh). Moller-Trumbore (kernel.cu:1024-1059) accepts a ray when its computed barycentrics
// lie in the unit simplex. Their rounding errors are those of two 3x3 determinants (absolute error <= gamma |s| |e|,
// gamma ~ 10 eps, |s| the distance from the ray origin to the first vertex) divided by a = D . (e2 x e1) =
// |e1| |e2| sin(phi0) cos(theta_n), theta_n the angle between the ray and the normal: in the triangle's plane they
// displace the hit point by at most 2 gamma (|s| + |e|) / (sigma |cos(theta_n)|), sigma the smallest corner sine. For a
// ray with |cos(theta_n)| >= kappa = 3e-3 / sigma that is below 4e-4 (|s| + |e|), inside pad = 2e-3 + 1e-3 (dist + r)
// (|s| <= dist + r, |e| <= 2 r): such a ray can only be accepted if its line comes within pad of the triangle, hence
// of its bounding sphere. A ray that GRAZES the triangle's plane is another matter: the error grows like
// 1 / cos(theta_n) (float Moller-Trumbore does accept rays that pass the sphere at several radii once cos(theta_n)
// drops below 3e-4: tools/mt_grazing.py), so a triangle is only culled when every ray of the beam keeps
// |cos(theta_n)| >= kappa, i.e. |n . u| >= (kappa + k)(1 + k) for the beam's axis u and slope k. A well-shaped
// triangle is "edge-on" to 0.5 % of the directions, a sliver (sigma -> 0, kappa >= 1; also anything degenerate or
// non-finite: normal 0) to all of them: never culled.
__device__ __forceinline__ bool beam_keeps_triangle(const Beam &b, float4 ts, float4 tn)
{
    const float vx = ts.x - b.ax, vy = ts.y - b.ay, vz = ts.z - b.az;
    const float vv = __builtin_fmaf(vx, vx, __builtin_fmaf(vy, vy, vz * vz));
    const float sa = __builtin_fmaf(vx, b.ux, __builtin_fmaf(vy, b.uy, vz * b.uz));
    const float d2 = __builtin_fmaxf(__builtin_fmaf(-sa, sa, vv), 0.f);
    const float dist = __builtin_amdgcn_sqrtf(vv) * 1.0001f;
    const float rc = __builtin_fmaf(1.0e-3f, dist + ts.w, ts.w + 2.0e-3f) * 1.0001f;
    const float reach = sa + rc - b.smin;
    const float rad = __builtin_fmaf(b.k, __builtin_fmaxf(reach, 0.f), b.r0) + rc;
    const float nu = __builtin_fabsf(__builtin_fmaf(tn.x, b.ux, __builtin_fmaf(tn.y, b.uy, tn.z * b.uz)));
    const bool facing = nu >= (tn.w + b.k) * (1.f + b.k);              // false for a NaN anywhere
    return !facing | (!(reach < 0.f) & !(d2 > rad * rad * 1.0005f));   // NaN / inf keep the triangle
}

// Leaf boxes of the mesh that the beam can touch, as indices in leaf order. A ray
// tests a leaf's triangles only after passing the leaf's slab test, i.e. only if
// it crosses the box, hence its bounding sphere: the sphere test with the usual
// padding is conservative. Order is kept (first triangle wins ties, kernel.cu:1309):
// two levels as for the spheres, but over blocks of RT_BLOCK CONSECUTIVE leaves (the host
// appends their bounding spheres after the leaf spheres), marked blocks and their members
// both taken in increasing order.
__device__ __forceinline__ int build_box_list(const float4 *__restrict__ bsph, int nb, int *list, int *blist, const Beam &b,
                                              int lane)
{
    const int nb_pad = (nb + RT_BLOCK - 1) / RT_BLOCK * RT_BLOCK, nblk = nb_pad / RT_BLOCK;
    const float4 *__restrict__ blocks = bsph + nb_pad;
    constexpr int G = 64 / RT_BLOCK;
    const int grp = lane / RT_BLOCK, sub = lane % RT_BLOCK;
    int count = 0;
    for (int bbase = 0; bbase < nblk; bbase += 64) {
        const int bi = bbase + lane;
        const float4 bb = blocks[bi < nblk ? bi : nblk - 1];
        const lmask bm = LM(bi < nblk) & beam_keeps_block(b, bb);
        const int marked = __popcll(bm);
        if (lane_in(bm)) blist[lane_prefix(bm)] = bi;
        wave_lds_sync();
        for (int t = 0; t < marked; t += G) {
            const int slot = t + grp;
            const int blk = (slot < marked) ? blist[slot] : -1;
            const int i = (blk < 0 ? 0 : blk) * RT_BLOCK + sub;
            const float4 s = bsph[i];
            const lmask m = LM(blk >= 0) & LM(i < nb) & beam_keeps(b, s);
            const int pos = count + lane_prefix(m);
            if (lane_in(m) && pos < RT_BOX_CAP) list[pos] = i;
            count += __popcll(m);
        }
        if (bbase + 64 < nblk) wave_lds_sync();
    }
    wave_lds_sync();
    return count;
}

}  // namespace
