// rt_stages.h -- the frame kernel's configuration record (TraceCfg), four helpers that stand for blocks the kernel held
// twice or more, and those of its steps that could be cut out without moving the product kernels' machine code:
// __forceinline__ functions that take values and return values, under the phase of the tuning build's stamps they
// belong to. Included by rt_trace.inc and by nothing else: the other passes take the device library (rt_wave.h ...
// rt_shadow.h). The derivation comments stand beside the code they derive; DESIGN.md section 4 has the map of the
// steps and says what was tried for those that stay inline.
#pragma once
#include "rt_shadow.h"

// Timing experiments (RT_ABLATE) exist in tuning builds only (make EXTRA=-DRT_TUNING, tools/variants.sh):
// the product kernel has no such switch and the product library reads no environment.
#ifdef RT_TUNING
#define RT_ABL(bits) ((fc.ablate & (bits)) != 0)
#else
#define RT_ABL(bits) false
#endif

namespace {

// ---------------------------------------------------------------------------
// the configuration: every switch the kernel and its stages read, derived once
// ---------------------------------------------------------------------------
// MODE, FEAT: RtTraceMode and RtTraceFeat (rt_device.h), which say what each value is.
// MULTI: the launch may take several samples per pixel (rt_launch_opts.spp > 1). The
// one-sample kernel has no sample loop: 74 -> 22 spilled scalars and 15 fewer vector registers.
template <int TW_, bool CULL_, int MODE_, int FEAT_, bool MULTI_>
struct TraceCfg {
    static constexpr int TW = TW_, MODE = MODE_, FEAT = FEAT_;
    static constexpr bool CULL = CULL_, MULTI = MULTI_;
    static constexpr int STATS = (MODE == RT_MODE_STATS) ? 1 : (MODE == RT_MODE_PHASES) ? 2 : 0;
    static constexpr bool force_slow = (MODE == RT_MODE_FORCE_SLOW);
    static constexpr bool FAST = (MODE == RT_MODE_FAST);    // rt_launch_opts.fast: approximate arithmetic, never the default
    static constexpr bool AOV = (MODE == RT_MODE_AOV);     // rt_frame_desc.aov_*: the product kernel plus the G-buffer stores after the texel fetch
    static constexpr bool MESH = (FEAT == RT_FEAT_MESH);
    static constexpr bool PRIMS = (FEAT == RT_FEAT_PRIMS || FEAT == RT_FEAT_MESH);   // cubes and planes may be present
    // the culling kernels take every exactness-preserving shortcut (lean normalise/sqrt, fast
    // texel index); the brute-force and force-slow ones evaluate everything the long way
#ifdef RT_NO_LEAN
    static constexpr int LEAN = 0;
#else
    static constexpr int LEAN = (CULL && !force_slow) ? 1 : 0;   // precision class of normalise_t & co. (FAST: primary rays, normal and toL stay exact)
#endif
    // the lean tail of intersect(): for the primary rays; for the shadow rays it costs the one-sample
    // kernel two spilled registers at its 6-waves-per-SIMD budget (measured: profiles/r02_variants.txt)
#ifdef RT_NO_LEAN_PRIMARY_TAIL
    static constexpr int LEAN_PRIMARY_TAIL = 0;
#else
    static constexpr int LEAN_PRIMARY_TAIL = LEAN;
#endif
#ifdef RT_LEAN_SHADOW_TAIL
    static constexpr int LEAN_SHADOW_TAIL = LEAN;
#else
    static constexpr int LEAN_SHADOW_TAIL = FAST ? 2 : 0;
#endif
    static constexpr int TH = 64 / TW;
    // Light verdicts (RtFrameConsts::rest_rd / rest_wr). RT_MODE_REST_READ: the tile's word of an earlier launch of
    // bit-identical inputs is asked for at the head (lanes 0 and 1, a dword each, by the tile's frame coordinates), parked in
    // the wave's LDS ahead of the light loop and consumed there two bits at a time. RT_MODE_REST_WRITE: the word this launch finds
    // is gathered in the same place and stored at the write-back. Nothing of it is held in a register across the light
    // loop, whose scalar and vector files are full.
    static constexpr bool COMPACT = (MODE == RT_MODE_REST_COMPACT);   // the reader with the compact launch's head (step 5e)
    static constexpr bool VD_USE = (MODE == RT_MODE_REST_READ || COMPACT), VD_REC = (MODE == RT_MODE_REST_WRITE), VERD = VD_USE || VD_REC;
    static_assert(!VERD || (CULL && FEAT == RT_FEAT_SPHERES), "light verdicts: the sphere-only culling kernels");
    // A reading launch forms a group's ball (g_r2, the check against its sphere's ball: two wave reductions) only where a
    // light of the group culls at all: 3.4 % of the 0.136 lights per tile that it still walks at C3. (RT_EAGER_BALL: the
    // variant it was measured against, profiles/primary_records_ab.json.)
#ifdef RT_EAGER_BALL
    static constexpr bool LAZY_BALL = false;
#else
    static constexpr bool LAZY_BALL = VD_USE;
#endif
    // (RT_EAGER_REST_LOADS: the other order of a reading launch's head -- word, tags and primary records asked for before
    // the summary is known and dropped by a settled tile -- which the order of the kernel's head was measured against,
    // profiles/settled_tiles_ab.json.)
#ifdef RT_EAGER_REST_LOADS
    static constexpr bool REST_EAGER = true;
#else
    static constexpr bool REST_EAGER = false;
#endif
    // The view list of the block of the frame a tile lies in (RtFrameConsts::view_lists) stands in for the primary cull
    static constexpr bool VIEW = CULL && !force_slow;
    // waves per SIMD the register budget is cut to (__launch_bounds__)
    static constexpr int MIN_WAVES = (FEAT == RT_FEAT_MESH) ? (MODE == RT_MODE_STATS ? 3 : MULTI ? RT_MIN_WAVES_MESH_MULTI : RT_MIN_WAVES_MESH) : (MODE == RT_MODE_STATS) ? 4 : (MODE == RT_MODE_REST_WRITE) ? RT_MIN_WAVES_PER_SIMD : !MULTI ? RT_MIN_WAVES_ONE_SAMPLE : RT_MIN_WAVES_PER_SIMD;
};

// ---------------------------------------------------------------------------
// what several steps share
// ---------------------------------------------------------------------------
// The kernel-argument pointer again, behind an opaque copy: what is read through it is loaded at the point of use, not
// merged with the loads at the kernel's entry and held in scalar registers from there (the write-back of rt_trace_tiles says what that costs).
__device__ __forceinline__ FcPtr kargs_again()
{
    FcPtr k = (FcPtr)__builtin_amdgcn_kernarg_segment_ptr();   // the frame constants are the first kernel argument
    asm volatile("" : "+s"(k));                                // opaque: not merged with the loads at the entry
    return k;
}

// documented clamp of a texel index (the reference is UB there)
__device__ __forceinline__ int clamp_texel(int idx, int last)
{
    return idx < 0 ? 0 : (idx > last ? last : idx);
}

// the exact texture coordinates of a sphere / cube hit, kernel.cu:1402-1403: the literals 1, 3.1415, 0.5 make these
// binary64 expressions; "/ 3.1415" in binary64 through div_by_3p1415 (same bits)
__device__ __forceinline__ void exact_uv(const V3 &normal, const double *myatan, float &tx, float &ty)
{
    tx = (float)((1.0 + rtm::div_by_3p1415((double)rtm::atan2f_rt(normal.z, normal.x, myatan))) * 0.5);
    ty = (float)rtm::div_by_3p1415((double)rtm::acosf_rt(normal.y, myatan));
}

// mean over the frame's samples (x/1.0f is exact, so 1 spp is the
// reference's rgbToInt(fr*254, fg*254, fb*254), kernel.cu:1682/1688)
__device__ __forceinline__ unsigned resolve_pixel(float acc_r, float acc_g, float acc_b, float o_total)
{
    float mr = acc_r, mg = acc_g, mb = acc_b;
    if (o_total != 1.f) {   // wave-uniform; three IEEE divisions saved at 1 spp
        mr = acc_r / o_total;
        mg = acc_g / o_total;
        mb = acc_b / o_total;
    }
    return rgb_to_int(f2i(mr * 254.f), f2i(mg * 254.f), f2i(mb * 254.f));
}

// ---------------------------------------------------------------------------
// the compact reading launch: a run of streamable tiles (step 5e)
// ---------------------------------------------------------------------------
// Entries [first, first + count) of the table's run list `list` (count <= RT_REST_LIST_RUN_MAX, wave-uniform), each of them a
// settled tile that needs neither the full path nor a table staged. Per tile what a settled tile's wave does in
// rt_trace_tiles, by the same expressions: its place, the valid lanes, the sample's sum (0 for a hit lane, the sky texel
// on record through the clamp for a miss lane), one write-back, its own duration into tile_cost. The entries and their
// summaries are asked for once for the whole run, a lane each. No LDS; the frame uniforms of the write-back come from
// the kernel-argument segment here, so that the one-wave path beside this one holds none of them.
template <class Cfg>
__device__ __forceinline__ void stream_settled_run(const RtFrameConsts &fc, AuxPtr ax, const unsigned *list, int lane, unsigned first, unsigned count)
{
    const unsigned s_tiles_x = (unsigned)(fc.width + Cfg::TW - 1) / (unsigned)Cfg::TW;
    const unsigned s_tiles = s_tiles_x * rt_rest_tiles_y(fc.local_rows, Cfg::TW);
    unsigned my_p = 0, my_ts = 0;
    if ((unsigned)lane < count) {
        my_p = list[first + (unsigned)lane];
        my_ts = reinterpret_cast<const unsigned *>(fc.rest_rd)[RT_REST_SUMMARY_DWORD(s_tiles, (my_p >> 16) * s_tiles_x + (my_p & 0xffffu))];
    }
    FcPtr kargs = kargs_again();
    float *const o_rgba = kargs->rgba;
    uint32_t *const o_packed = kargs->packed, *const o_packed24 = kargs->packed24;
    unsigned *const o_cost = kargs->tile_cost;
    const int o_flags = kargs->flags;
    const float o_total = kargs->sample_total;
    const int il_sh = __builtin_ctz((unsigned)fc.il_rows);
    // (The other tile shapes' readers are the sample-loop kernels, MULTI, and a launch that reads a table takes one sample:
    // the count is 1 in every launch there is. It is spelt as the kernel spells it so that the two cannot drift apart.)
    const int n_samples = Cfg::MULTI ? fc.spp : 1;
    for (unsigned r = 0; r < count; ++r) {
        const unsigned t_start = o_cost ? (unsigned)__builtin_amdgcn_s_memtime() : 0u;
        const unsigned p = (unsigned)__builtin_amdgcn_readlane((int)my_p, (int)r), ts = (unsigned)__builtin_amdgcn_readlane((int)my_ts, (int)r);
        const unsigned blk_x = p & 0xffffu, blk_y = p >> 16;
        const int ly = (int)blk_y * Cfg::TH + (lane / Cfg::TW);
        const int px = (int)blk_x * Cfg::TW + (lane % Cfg::TW);
        const int py = fc.y0 + ((((ly >> il_sh) * fc.il_count + fc.il_index) << il_sh) | (ly & (fc.il_rows - 1)));
        const lmask valid_m = LM(px < fc.width) & LM(ly < fc.local_rows) & LM(py < fc.y1);
        if (valid_m == 0) continue;   // (as its own wave such a tile stores nothing either, its duration included: the kernel returns before)
        const bool valid = lane_in(valid_m);
        float fr = 0.f, fg = 0.f, fb = 0.f;
        if ((ts & RT_TILE_NO_MISS) == 0) {   // wave-uniform
            const unsigned pr_rec = reinterpret_cast<const unsigned *>(fc.rest_rd + RT_REST_PRIMARY_OFFSET(s_tiles))[(size_t)(blk_y * s_tiles_x + blk_x) * (RT_REST_PRIMARY_BYTES / 4u) + lane];
            if (valid && (pr_rec & 0xffu) == RT_PRIMARY_MISS) {
                const int idx = clamp_texel((int)(pr_rec >> 8), ax->sky_w * ax->sky_h - 1);
                fr = ax->sky_r[idx];
                fg = ax->sky_g[idx];
                fb = ax->sky_b[idx];
            }
        }
        float acc_r = 0.f, acc_g = 0.f, acc_b = 0.f;
        for (int sample = 0; sample < n_samples; ++sample)   // (a settled tile's samples are all this one)
            if (valid) {
                acc_r = acc_r + fr;
                acc_g = acc_g + fg;
                acc_b = acc_b + fb;
            }
        // the write-back of rt_trace_tiles
        const unsigned out_idx = (unsigned)ly * (unsigned)fc.width + (unsigned)px;   // band-local pixel index
        if (valid) {
            const size_t o = out_idx;
            float w = (float)n_samples;
            if (o_rgba) {
                float4 *dst = reinterpret_cast<float4 *>(o_rgba) + o;
                if (o_flags & RT_FLAG_ACCUMULATE) {
                    const float4 old = *dst;
                    acc_r = old.x + acc_r;
                    acc_g = old.y + acc_g;
                    acc_b = old.z + acc_b;
                    w = old.w + w;
                }
                *dst = make_float4(acc_r, acc_g, acc_b, w);
            }
            if (o_packed && (o_flags & RT_FLAG_RESOLVE)) o_packed[o] = resolve_pixel(acc_r, acc_g, acc_b, o_total);
        }
        if (o_packed24 && (o_flags & RT_FLAG_RESOLVE)) {   // wave-uniform; all lanes take part in the quad exchange
            const unsigned q = resolve_pixel(acc_r, acc_g, acc_b, o_total);
            const unsigned qn = (unsigned)__builtin_amdgcn_update_dpp(0, (int)q, 0xF9 /* quad_perm [1,2,3,3] */, 0xf, 0xf, true);
            const int i = lane & 3;
            const unsigned w24 = (q >> (8 * i)) | (qn << (24 - 8 * i));
            if (valid && i < 3) o_packed24[(size_t)(out_idx >> 2) * 3 + (size_t)i] = w24;
        }
        if (o_cost) {
            const unsigned dt = (unsigned)__builtin_amdgcn_s_memtime() - t_start;
            if (lane == 0) o_cost[blk_y * s_tiles_x + blk_x] = dt;
        }
    }
}

// ---------------------------------------------------------------------------
// phase 3: the primary record, the G-buffer, the parked verdicts
// ---------------------------------------------------------------------------
// The recording launch: every lane's primary record, one coalesced 256-byte store per wave. A tile that walked
// no view list (an overflowed block or one without cone, a tile shape that does not nest, a scene below 64
// spheres, the switch off) says so in all its lanes, and so does every tile when a texture's texel indices
// do not fit 24 bits -- decided here from the launch's own uniforms, wave-uniformly.
// Returns the tile's summary before its groups are known.
template <class Cfg>
__device__ __forceinline__ unsigned store_primary_record(AuxPtr ax, int lane, unsigned blk_x, unsigned blk_y, bool v_use, bool hit, int hent,
                                                         int pr_tex, lmask valid_m, lmask hit_m)
{
    FcPtr kp = kargs_again();
    const bool fits = (unsigned)(kp->tex_w * kp->tex_h) <= (unsigned)RT_PRIMARY_TEXELS && (unsigned)(ax->sky_w * ax->sky_h) <= (unsigned)RT_PRIMARY_TEXELS;
    unsigned d = RT_PRIMARY_NONE;
    if (v_use && fits) d = (hit ? (unsigned)hent : RT_PRIMARY_MISS) | ((unsigned)pr_tex << 8);
    const unsigned p_tiles_x = rt_rest_tiles_x(kp->width, Cfg::TW);
    const unsigned p_tiles = p_tiles_x * rt_rest_tiles_y(kp->local_rows, Cfg::TW);   // = the grid
    unsigned *const o_prim = reinterpret_cast<unsigned *>(kp->rest_wr + RT_REST_PRIMARY_OFFSET(p_tiles));
    o_prim[(size_t)(blk_y * p_tiles_x + blk_x) * (RT_REST_PRIMARY_BYTES / 4u) + lane] = d;
    // The tile's summary (step 5d) so far: it can be settled at all -- it has a record, and every light has its
    // bits in the word --, and whether a valid lane is a miss. Parked behind the tile index by park_verdicts; the groups
    // have their say behind the light loop.
    return ((v_use && fits && kp->n_lights <= RT_VERDICT_LIGHTS) ? RT_TILE_SETTLED : 0u) | ((valid_m & ~hit_m) == 0 ? RT_TILE_NO_MISS : 0u);
}

// ================= G-buffer (rt_frame_desc.aov_*) =================
// Every value is live here and nothing new is held across the light loop, whose register peak is
// what the budget is cut to: the output pointers come from the kernel-argument segment at this point,
// and the pixel's place is formed again as the write-back forms it.
template <class Cfg>
__device__ __forceinline__ void store_gbuffer(AuxPtr ax, int lane, int wave, bool valid, bool hit, float nt, const V3 &normal, int hkind, int htri,
                                              int hprim, int holder, float tr, float tg, float tb, float fr, float fg, float fb)
{
    FcPtr ka = kargs_again();
    float *const o_depth = ka->aov_depth, *const o_normal = ka->aov_normal, *const o_albedo = ka->aov_albedo;
    int *const o_id = ka->aov_id;
    unsigned a_x = blockIdx.x, a_y = blockIdx.y;
    const unsigned a_tiles_x = (unsigned)(ka->width + Cfg::TW - 1) / (unsigned)Cfg::TW;
    if (ka->tile_perm) {
        const unsigned p = ka->tile_perm[blockIdx.y * a_tiles_x + blockIdx.x];
        a_x = p & 0xffffu;
        a_y = p >> 16;
    }
    const size_t o = (size_t)((unsigned)((a_y + wave) * Cfg::TH + lane / Cfg::TW) * (unsigned)ka->width + (unsigned)(a_x * Cfg::TW + lane % Cfg::TW));
    if (valid) {
        if (o_depth) o_depth[o] = nt;   // +inf on a miss
        if (o_normal)
            reinterpret_cast<float4 *>(o_normal)[o] = hit ? make_float4(normal.x, normal.y, normal.z, 0.f)
                                                          : make_float4(0.f, 0.f, 0.f, 0.f);
        if (o_id) {
            int idx = -1;
            if (hit) idx = (Cfg::MESH && hkind == 0) ? ax->tri_idx[htri] : (Cfg::PRIMS && hkind >= 2) ? hprim : holder;
            reinterpret_cast<int2 *>(o_id)[o] = make_int2(hit ? hkind : -1, idx);
        }
        if (o_albedo)
            reinterpret_cast<float4 *>(o_albedo)[o] = hit ? make_float4(tr, tg, tb, 1.f) : make_float4(fr, fg, fb, 1.f);
    }
}

// the tile's word: the verdicts it was handed (RT_MODE_REST_READ), or those it finds (RT_MODE_REST_WRITE: none so far)
template <class Cfg>
__device__ __forceinline__ void park_verdicts(unsigned *myvd, int lane, unsigned vd_ld, unsigned ts_pre)
{
    if (lane < 4) myvd[lane] = vd_ld;
    if (Cfg::VD_REC && lane == 4) myvd[4] = ts_pre;
    wave_lds_sync();
}

// ---------------------------------------------------------------------------
// the group loop's head: group ids
// ---------------------------------------------------------------------------
// A tile that straddles a silhouette sees several spheres at different
// depths; one beam around all of their shadow rays would be fat and its
// survivor list long. So the hit lanes are processed in groups that share
// the closest sphere (3.5 % of the 8x8 tiles at 4K see more than one):
// each group's origins lie on one small patch, its beam is thin, its
// list short -- and no wave runs orders of magnitude longer than the rest.
// group ids first (the sphere centres / kinds they are derived from are
// not needed afterwards, which frees four registers for the light loop)
// Returns the number of groups; gid_out takes the lane's (-1 where nothing was hit).
template <class Cfg>
__device__ __forceinline__ int form_groups(lmask hit_m, float hcx, float hcy, float hcz, int hkind, int &gid_out)
{
    int gid = -1, n_groups = 0;
    {
        lmask rem = hit_m;
        while (rem) {
            const int first = __builtin_ctzll(rem);
            const float gx = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, hcx), first));
            const float gy = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, hcy), first));
            const float gz = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, hcz), first));
            const int gk = __builtin_amdgcn_readlane(hkind, first);
            const lmask in = rem & ((1ull << first) | ((Cfg::PRIMS ? LM(hkind == gk) : ~0ull) & LM(hcx == gx) & LM(hcy == gy) & LM(hcz == gz)));
            if (lane_in(in)) gid = n_groups;
            rem &= ~in;
            ++n_groups;
        }
    }
    gid_out = gid;
    return n_groups;
}

// ---------------------------------------------------------------------------
// phase 7: a walked light's record; the tile's summary
// ---------------------------------------------------------------------------
// The recording launch: a light that was walked to the end (not clear, not dark) takes the tile's next free
// record -- every lane's count as a byte, 64 in a row -- and lane 0 notes whose it is in the tag dword.
template <class Cfg>
__device__ __forceinline__ void record_counts(unsigned *myvd, int g, int li, int lane, unsigned us)
{
    const unsigned tg = (unsigned)__builtin_amdgcn_readfirstlane((int)myvd[2]);
    int slot = -1;
#pragma unroll
    for (int r = RT_SHADOW_RECORDS - 1; r >= 0; --r)
        if (((tg >> (8 * r)) & 0xffu) == 0u) slot = r;
    if (slot >= 0) {
        FcPtr kg = kargs_again();
        const unsigned tiles = rt_rest_tiles(kg->width, kg->local_rows, Cfg::TW);
        const unsigned tile = (unsigned)__builtin_amdgcn_readfirstlane((int)myvd[3]);
        unsigned char *rec = kg->rest_wr + RT_REST_COUNTS_OFFSET(tiles) + ((size_t)tile * RT_SHADOW_RECORDS + (size_t)slot) * RT_REST_RECORD_BYTES;
        rec[lane] = (unsigned char)(us >> 16);
        if (lane == 0)
            (void)__hip_atomic_fetch_or(&myvd[2], RT_SHADOW_TAG(g, li) << (8 * slot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        wave_lds_sync();
    }
}

// Settled (step 5d): every iteration the tile has left its code RT_VERDICT_NOTHING in the word -- lane 0
// made every note, so it reads its own -- and the word holds them all. What the word must then be: code
// 1 for each of the n_lights lights in each of the n_groups 16-bit fields, 0 elsewhere. (Lane 0 of the recording launch.)
// (reads no switch of the configuration: not a template)
__device__ __forceinline__ void tile_summary(const RtFrameConsts &fc, unsigned *myvd, int n_groups)
{
    bool all_nothing = n_groups <= RT_VERDICT_GROUPS && fc.n_lights <= RT_VERDICT_LIGHTS;
    if (all_nothing) {
        const unsigned pat = 0x5555u & ((1u << (2 * fc.n_lights)) - 1u);
        const unsigned lo = (n_groups > 0 ? pat : 0u) | (n_groups > 1 ? pat << 16 : 0u);
        const unsigned hi = (n_groups > 2 ? pat : 0u) | (n_groups > 3 ? pat << 16 : 0u);
        all_nothing = myvd[0] == lo && myvd[1] == hi;
    }
    myvd[4] = (myvd[4] & (all_nothing ? (RT_TILE_SETTLED | RT_TILE_NO_MISS) : RT_TILE_NO_MISS)) |
                ((unsigned)(n_groups < 255 ? n_groups : 255) << RT_TILE_GROUPS_SHIFT);
}

}  // namespace
