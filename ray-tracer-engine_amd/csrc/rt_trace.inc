// rt_trace.inc -- the frame kernel rt_trace_tiles for gfx950 (MI355X), the table of its instantiations
// (trace_exists, the trace_fn_* ladders) and the declarations of the table's three parts. Included by the units that
// instantiate the kernel and by no other: rt_kernels.hip (default tile, culling kernels, plus the launch
// configuration and the diagnostics), rt_kernels_brute.hip (the same tile, brute-force loops) and
// rt_kernels_tiles.hip (the other tile shapes) -- one code object, compiled in parallel. The configuration record
// the kernel reads its switches from (TraceCfg), four helpers for blocks it held twice and the steps that stand on
// their own are in rt_stages.h, which only this file includes. DESIGN.md section 4 maps the steps and says, for each
// block that is still inline here, what cutting it out was measured to cost. The
// device library both stand on is in four headers, each including the one before it: rt_wave.h (pointer types, V3,
// wave helpers), rt_exact.h (exact and lean arithmetic, primitive tests), rt_cull.h (beams, list builders) and
// rt_shadow.h (ShadowChain, shadow_test, the sample pre-pass). The other passes take those headers, never these two files.
//
// What is computed is the reference's `rayTrace` kernel (kernel.cu:1614-1690 and callees: castRay :1287-1431,
// castLightRay :1432-1544, sphere::intersect :292-354, skybox::getFColor :1146-1166, rgbToInt :546-556). How it is
// computed is not the reference's one-thread-per-pixel brute force:
//
//   * one wave64 owns a TW x (64/TW) pixel tile and is its own workgroup; the sphere
//     tables {cx,cy,cz,radius^2} stay in global memory (L2-resident) and only the
//     tile's culled lists live in LDS;
//   * per tile the wave cooperatively culls the table against a conservative
//     bound of the tile's rays (a cone for the primary rays, a cone-capped beam
//     for each light's shadow rays), ballot-compacts the survivors IN LIST
//     ORDER into a per-wave LDS list, and only those are tested; every lane
//     reads the same list entry (LDS broadcast);
//   * every value that decides a pixel (the quadratic, sqrt, divisions, the
//     shadow-sample construction) is evaluated with exactly the reference's
//     IEEE binary32/binary64 operations -- the library is compiled with
//     -ffp-contract=off and correctly rounded divide/sqrt; only the culling
//     bounds use fast approximate math, and they are padded so that a culled
//     sphere is one whose exact test would have returned false;
//   * shadow rays leave their loop through a wave-wide "all lanes occluded".
//
// A sphere skipped by culling can never change the closest hit (it is not hit)
// nor an any-hit result, and survivors keep their list order, so first-index-
// wins ties (kernel.cu:1335) resolve identically: the output is bit-identical
// to the brute-force loops (template CULL=false), which tests check.
#pragma once
#include "rt_stages.h"

namespace {

// ---------------------------------------------------------------------------
// the frame kernel
// ---------------------------------------------------------------------------
// The template parameters are TraceCfg's (rt_stages.h), which derives every switch from them.
template <int TW, bool CULL, int MODE, int FEAT = RT_FEAT_SPHERES, bool MULTI = true>
__global__ __launch_bounds__(64, (TraceCfg<TW, CULL, MODE, FEAT, MULTI>::MIN_WAVES)) void rt_trace_tiles(const RtFrameConsts fc,
                                                                     const float4 *__restrict__ spheres)
{
    using Cfg = TraceCfg<TW, CULL, MODE, FEAT, MULTI>;
    // One wave per workgroup: with the tables in global memory nothing is shared between waves, and one-wave
    // workgroups fill the SIMDs best (0.68 vs 0.71 ms at C3) and need no barrier.
    extern __shared__ float4 lds[];

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;   // always 0 (one-wave workgroups); kept for code generation only: the
                                         // wave's LDS and the tile rows below say why
    const int n = fc.n_spheres;
    const AuxPtr ax = (AuxPtr)(uintptr_t)fc.aux;   // lights, sample constants, sky, planes/cubes, mesh (device memory)

    // The wave's LDS, by the layout block of rt_device.h (RT_LDS_*), which also sizes the launch. The `wave` terms are
    // zero, but with them the compiler holds these addresses in registers; as plain constants it re-materialises them
    // inside the loops, and the product kernel's code grows by 8 %.
// (plain locals: held in one record handed to the steps by reference, the null test of the arctangent table is no
// longer folded and the code grows by 8 %; formed again at each use, the tuning build's reading kernel spills 8 vector registers for 1)
    float4 *mylist = lds + wave * RT_LIST_CAP;
    int *mykeys = reinterpret_cast<int *>(lds + RT_LIST_CAP) + RT_LDS_KEYS + wave * RT_LIST_CAP;   // list positions (primary order)
    // b after n float+=double steps of 0.1 (brightness_steps), one 16-entry copy per wave: a
    // per-lane n then costs one LDS read instead of a ten-deep select chain per light
    float *mybtab = reinterpret_cast<float *>(lds + RT_LIST_CAP) + RT_LDS_BTAB + wave * 16;
    // marked blocks of one culling pass (at most 64 at a time)
    int *myblks = reinterpret_cast<int *>(lds + RT_LIST_CAP) + RT_LDS_BLKS + wave * 64;
    // rtm::atan_eighth(0..8) for the binary64 arctangent (one LDS read instead of a select chain)
    double *myatan = reinterpret_cast<double *>(reinterpret_cast<int *>(lds + RT_LIST_CAP) + RT_LDS_ATAN) + wave * 16;
    // the pixels' texel colours wait here for the shading at the end of a light (three registers that are live across
    // the whole light loop for one use per lit light; the compiler put them in scratch memory -- 0.4 GB per frame)
    float *mytex = reinterpret_cast<float *>(reinterpret_cast<int *>(lds + RT_LIST_CAP) + RT_LDS_TEX) + wave * 192;
    int *myboxes = reinterpret_cast<int *>(lds + RT_LIST_CAP) + RT_LDS_TAIL + wave * RT_LDS_MESH_DWORDS;   // the mesh's tail: + marked leaf blocks + 64 staged floats
    float *mytri = reinterpret_cast<float *>(myboxes + RT_LDS_MESH_TRI);   // staged vertices of a leaf (MESH launches only)
    // Tile summaries (step 5d, RT_MODE_REST_READ): the tile's dword of the resting-view table is asked for first of all -- one scalar
    // load by the tile's frame coordinates, formed here as below. A settled tile (RT_TILE_SETTLED) stages no table,
    // loads no word, tag, list or ray table and, where no valid lane is a miss (RT_TILE_NO_MISS), no primary record:
    // the head of the sample loop sends it to the write-back. The others go on from here as they always did, with the
    // summary's latency in front of their loads: the flag is known before anything else is asked for.
    unsigned ts = 0;
    if (Cfg::VD_USE) {
        // The compact launch (step 5e, RT_MODE_REST_COMPACT): a 1-D grid over the table's run list. n_unsettled workgroups take
        // their tile from it wherever this kernel forms a tile's place -- tile_perm points at the list so that their
        // blockIdx.x finds their entry -- and go on below as ever; each of the others streams a run of R settled tiles and
        // ends here. The runs lie behind the one-wave tiles, or (n_ahead > 0) all of them ahead.
        if (Cfg::COMPACT) {
            const unsigned *c_hdr = reinterpret_cast<const unsigned *>(fc.rest_rd + RT_REST_LIST_OFFSET(rt_rest_tiles(fc.width, fc.local_rows, Cfg::TW)));
            const unsigned n_unsettled = c_hdr[0], n_ahead = c_hdr[3];
            if (blockIdx.x < n_ahead || blockIdx.x >= n_ahead + n_unsettled) {
                const unsigned c_end = n_unsettled + c_hdr[1], c_run = c_hdr[2];
                const unsigned c_first = n_unsettled + (blockIdx.x < n_ahead ? blockIdx.x : blockIdx.x - n_unsettled) * c_run;
                if (c_first < c_end) stream_settled_run<Cfg>(fc, ax, c_hdr + RT_REST_LIST_HEADER, lane, c_first, c_end - c_first < c_run ? c_end - c_first : c_run);
                return;
            }
        }
        // (the tile's place is formed four times -- here, below, at the G-buffer and at the write-back: as one function it
        // changed 8 lines of the product kernel's machine code and 50 of the reading kernel's)
        unsigned h_x = blockIdx.x, h_y = blockIdx.y;
        const unsigned h_tiles_x = (unsigned)(fc.width + Cfg::TW - 1) / (unsigned)Cfg::TW;
        if (fc.tile_perm) {
            const unsigned p = fc.tile_perm[blockIdx.y * h_tiles_x + blockIdx.x];
            h_x = p & 0xffffu;
            h_y = p >> 16;
        }
        ts = reinterpret_cast<const unsigned *>(fc.rest_rd)[RT_REST_SUMMARY_DWORD(h_tiles_x * rt_rest_tiles_y(fc.local_rows, Cfg::TW), h_y * h_tiles_x + h_x)];
    }
    bool settled = Cfg::VD_USE && (ts & RT_TILE_SETTLED) != 0;   // wave-uniform
    if (!Cfg::VD_USE || !settled) {
        // (twice, here and where a settled tile falls back: as one function of (mybtab, myatan, lane) it changed 12 lines of the
        // product kernel's machine code and 22 of the multi-sample kernel's)
        if (lane < 16) {
            mybtab[lane] = kBrightnessSteps[lane];   // same values as brightness_steps()
            myatan[lane] = kAtanEighth[lane];
        }
        wave_lds_sync();
    }

    // which tile: the workgroup's own, or the one the frame's tile order puts at this place
    unsigned blk_x = blockIdx.x, blk_y = blockIdx.y;
    unsigned t_start = 0;
    const unsigned tiles_x = (unsigned)(fc.width + Cfg::TW - 1) / (unsigned)Cfg::TW;   // = gridDim.x
    if (fc.tile_perm) {
        const unsigned p = fc.tile_perm[blockIdx.y * tiles_x + blockIdx.x];
        blk_x = p & 0xffffu;
        blk_y = p >> 16;
    }
    if (fc.tile_cost) t_start = (unsigned)__builtin_amdgcn_s_memtime();
    // Shadow counts (step 5b) go the same way: the tile's tag dword is asked for by lane 2 and parked behind the word,
    // and behind that the tile's index, which the light loop needs for a record's address and must not hold in a register.
    unsigned *myvd = reinterpret_cast<unsigned *>(reinterpret_cast<int *>(lds + RT_LIST_CAP) + RT_LDS_TAIL) + wave * RT_LDS_REST_DWORDS;   // word, tags, tile index, summary (RT_MODE_REST_WRITE), in the tail's place
    unsigned vd_ld = 0;
    unsigned pr_rec = RT_PRIMARY_NONE;
    if (Cfg::VERD) {
        const unsigned vd_tile = blk_y * tiles_x + blk_x, vd_tiles = tiles_x * rt_rest_tiles_y(fc.local_rows, Cfg::TW);   // T = the grid
        // (a dword each: the word's halves, the tag)
        if (Cfg::VD_USE && (Cfg::REST_EAGER || !settled) && lane < 3) vd_ld = reinterpret_cast<const unsigned *>(fc.rest_rd)[lane < 2 ? RT_REST_WORD_DWORD(vd_tile) + lane : RT_REST_TAG_DWORD(vd_tiles, vd_tile)];
        if (lane == 3) vd_ld = vd_tile;
        // Primary records (step 5c): the lane's dword -- which entry of the tile's view list is its closest hit, and its
        // texel -- asked for here beside the word and used after the ray arithmetic. (A settled tile without a miss lane
        // has no use for them; one with miss lanes tells hit from miss by them and takes the sky texel.)
        if (Cfg::VD_USE && (Cfg::REST_EAGER || (ts & (RT_TILE_SETTLED | RT_TILE_NO_MISS)) != (RT_TILE_SETTLED | RT_TILE_NO_MISS))) pr_rec = reinterpret_cast<const unsigned *>(fc.rest_rd + RT_REST_PRIMARY_OFFSET(vd_tiles))[(size_t)vd_tile * (RT_REST_PRIMARY_BYTES / 4u) + lane];
    }
    const int tile_x = blk_x * Cfg::TW;
    // local row -> global row: a contiguous band, or row blocks dealt round-robin
    // to the ranks of a multi-GPU frame (il_rows is a multiple of the tile rows a
    // workgroup covers, so a tile never straddles two blocks)
    // (`+ wave` adds 0; without it the 64x1-tile kernels compile to different code, the others do not change)
    const int ly = (blk_y + wave) * Cfg::TH + (lane / Cfg::TW);
    const int px = tile_x + (lane % Cfg::TW);
    // (il_rows is a power of two -- the host checks -- and il_count = 1, il_index = 0 for a contiguous band: shifts and a
    // mask, where a division by a run-time il_rows is thirty vector instructions at the head of every wave)
    const int il_sh = __builtin_ctz((unsigned)fc.il_rows);
    const int py = fc.y0 + ((((ly >> il_sh) * fc.il_count + fc.il_index) << il_sh) | (ly & (fc.il_rows - 1)));   // blocks are dealt from the band's first row
    const lmask valid_m = LM(px < fc.width) & LM(ly < fc.local_rows) & LM(py < fc.y1);
    if (valid_m == 0) return;   // wave-uniform
    const bool valid = lane_in(valid_m);

// (plain locals: as one record with phase() and the flushes as members they moved registers and spills of the
// work-counter mesh kernels and the phase-stamp kernels, 119 -> 135 vector registers in one; a run-time-indexed hist[] member put the record in scratch)
    unsigned long long st_primary = 0, st_shadow = 0, st_cull = 0, st_slots = 0, st_entries = 0,
                       st_overflow = 0, st_hits = 0, st_unshadowed = 0, st_clusters = 0;

    unsigned long long hist[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long st_walks = 0, st_walks_no_penumbra = 0, st_pen_lanes = 0, st_walk_lanes = 0, st_pre = 0;
    unsigned long long st_walks_all_dark = 0, st_walks_all_lit = 0;
    unsigned long long sm_plisted = 0, sm_pleaf = 0, sm_ptri = 0, sm_slisted = 0, sm_sslab = 0, sm_stri = 0;   // mesh work (STATS, MESH)
    unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long t_prev = 0;
    const bool span_only = RT_ABL(512);   // no inner stamps: near-real wave durations
    const unsigned long long rt_begin = (Cfg::STATS == 2) ? __builtin_amdgcn_s_memrealtime() : 0ull;   // 100 MHz
    auto phase = [&](int k, bool last = false) {   // charge the cycles since the previous stamp to phase k
        if (Cfg::STATS == 2 && (k < 0 || last || !span_only)) {
            __builtin_amdgcn_sched_barrier(0);
            const unsigned long long now = __builtin_amdgcn_s_memtime();
            __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): s_memtime returns through it
            __builtin_amdgcn_sched_barrier(0);
            if (k >= 0) ph[k] += now - t_prev;
            t_prev = now;
        }
    };
    phase(-1);

    float acc_r = 0.f, acc_g = 0.f, acc_b = 0.f;

    // The view list of the block of the frame this tile lies in (RtFrameConsts::view_lists), by the tile's frame
    // coordinates alone: what the primary cull below would compute, built once per view (rt_tables.hip).
    const float4 *vslot = nullptr;
    if (Cfg::VIEW && fc.view_lists) {
        const int ly0 = (int)blk_y * Cfg::TH;
        const int py0 = fc.y0 + ((((ly0 >> il_sh) * fc.il_count + fc.il_index) << il_sh) | (ly0 & (fc.il_rows - 1)));
        const int vblk = __builtin_amdgcn_readfirstlane((py0 >> (fc.view_shift >> 8)) * fc.view_nbx + (tile_x >> (fc.view_shift & 255)));
        vslot = reinterpret_cast<const float4 *>(fc.view_lists) + (size_t)vblk * RT_VIEW_SLOT;
    }

    const int n_samples = Cfg::MULTI ? fc.spp : 1;
    for (int sample = 0; sample < n_samples; ++sample) {
        float fr = 0.f, fg = 0.f, fb = 0.f;   // this sample's colour (sky texel on a miss)
        do {   // (left at its head by a settled tile, step 5d; by every other at its end)
        if (Cfg::VD_USE && settled) {
            // A settled tile: by the verdicts on record no light adds to any of its pixels, so a hit lane's colour is
            // the 0 it starts with and a miss lane's the sky texel of its record, through the clamp as ever. No ray, list,
            // normal, texel or group is formed: none of them has a consumer left. Everything from here to the sample's
            // sum and the write-back is wave-uniformly skipped.
            const bool no_miss = (ts & RT_TILE_NO_MISS) != 0;
            if (no_miss || (valid_m & LM((pr_rec & 0xffu) == RT_PRIMARY_NONE)) == 0) {
                if (!no_miss && valid && (pr_rec & 0xffu) == RT_PRIMARY_MISS) {
                    const int idx = clamp_texel((int)(pr_rec >> 8), ax->sky_w * ax->sky_h - 1);
                    fr = ax->sky_r[idx];
                    fg = ax->sky_g[idx];
                    fb = ax->sky_b[idx];
                }
                break;
            }
            // A valid lane without a record (the setters only): the full path. The tables the head left out are staged
            // here; the word and the tags it did not ask for stay 0, "evaluate" and "no record" for every light, which
            // is the plain kernel's frame. (Asking for them again here costs the kernel a spilled vector register.)
            settled = false;
            if (lane < 16) {
                mybtab[lane] = kBrightnessSteps[lane];
                myatan[lane] = kAtanEighth[lane];
            }
            wave_lds_sync();
        }
        // header (a scalar load) and this lane's entry of the block's list: asked for here, ahead of the ray
        // arithmetic, and consumed after it. The slot is whole whatever its count, so the entry does not wait for the
        // header. A multi-sample launch fetches the list again for every sample (the light loop re-uses its LDS).
        int v_count = 0;
        bool v_use = false;
        float4 v_ent = make_float4(0.f, 0.f, 0.f, 0.f);
        int v_key = 0;
        float v_lb = 0.f;
        if (Cfg::VIEW && vslot) {
            const ConstIntPtr vh = (ConstIntPtr)(uintptr_t)vslot;
            v_count = vh[0];
            v_use = vh[1] == 0;
            v_ent = vslot[1 + lane];
            v_key = reinterpret_cast<const int *>(vslot + 1 + RT_VIEW_CAP)[lane];
            v_lb = reinterpret_cast<const float *>(vslot + 1 + RT_VIEW_CAP + RT_VIEW_CAP / 4)[lane];
        }
        // (inline: as a function returning D it changed 6 lines of the product kernel's machine code)
        // ================= primary ray, kernel.cu:1624-1631 =================
        // dx, dy of kernel.cu:1624-1625 (binary64 expressions of the column resp. the row) come
        // from the frame's tables, evaluated by the host with the reference's operations; lanes
        // beyond the frame edge read the last column / row (their pixels are never stored)
        const int sidx = fc.sample_base + sample;
        const float dx = fc.dx_tab[sidx * fc.width + (px < fc.width ? px : fc.width - 1)];
        const float dy = fc.dy_tab[sidx * fc.height + (py < fc.height ? py : fc.height - 1)];
        V3 dir{dx, dy, fc.eye_nz};   // (dx,dy,0) - (0,0,-1/aspect)
        normalise_t<Cfg::LEAN>(dir);
        // camera::rotateDir, kernel.cu:252-257 (cos/sin hoisted to the host)
        V3 D;
        {
            const float y = dir.y * fc.cos_pitch - dir.z * fc.sin_pitch;
            float z = dir.y * fc.sin_pitch + dir.z * fc.cos_pitch;
            const float x = dir.x * fc.cos_yaw + z * fc.sin_yaw;
            z = -dir.x * fc.sin_yaw + z * fc.cos_yaw;
            D = V3{x, y, z};
        }
        const V3 O{fc.org_x, fc.org_y, fc.org_z};
        const RayK pr = make_ray(O, D);

        phase(0);
        // ================= castRay, sphere branch =================
        bool p_use_list = false;   // false: walk the whole table
        int pcount = n;
        bool pb_use_list = false;  // leaf boxes of the mesh: false = all of them
        int pbcount = Cfg::MESH ? fc.n_boxes : 0;
        Beam pbeam;                // the tile's primary beam, kept for the per-triangle cull of the mesh leaves
        bool pbeam_ok = false;
        if (Cfg::CULL) {
            Beam b;
            bool ok = false;
            if (!v_use || Cfg::MESH) {
                // cone around the tile's mean direction, apex at the (shared) origin
                float sx = D.x, sy = D.y, sz = D.z;
                wave_sum3(sx, sy, sz);
                const float inv = __builtin_amdgcn_rsqf(__builtin_fmaf(sx, sx, __builtin_fmaf(sy, sy, sz * sz)));
                b.ux = uniform(sx * inv); b.uy = uniform(sy * inv); b.uz = uniform(sz * inv);
                const float cx = D.y * b.uz - D.z * b.uy, cy = D.z * b.ux - D.x * b.uz, cz = D.x * b.uy - D.y * b.ux;
                float s2 = wave_max(__builtin_fmaf(cx, cx, __builtin_fmaf(cy, cy, cz * cz)));
                s2 = uniform(s2);
                // s2 is sin^2 of the largest deviation (|D| = 1 up to rounding)
                ok = (s2 < 0.25f);   // NaN or a degenerate tile: do not cull
                const float sn = __builtin_amdgcn_sqrtf(s2) * 1.01f + 1.0e-5f;
                b.k = sn * __builtin_amdgcn_rsqf(1.f - sn * sn);
                b.ax = O.x; b.ay = O.y; b.az = O.z;
                b.smin = 0.f;
                b.smax = 0.f;
                b.r0 = 1.0e-4f;
            }
            if (v_use) {
                // the block's list as it stands: a superset of what this tile's own cull would keep, in the order and
                // with the positions and bounds the walk below expects (no block pass, no member step, no sort)
                // (filtering it first with the tile's own beam -- one member test, ballot compaction -- costs the beam
                // it was meant to save: 0.202 against 0.194 ms at C3, profiles/view_lists_ab.json)
                mylist[lane] = v_ent;
                mykeys[lane] = v_key;
                reinterpret_cast<float *>(myblks)[lane] = v_lb;
                wave_lds_sync();
                p_use_list = true;
                pcount = v_count;
                if (Cfg::STATS == 1) st_entries += (unsigned long long)v_count;
            } else if (ok) {
                // eye cones when the scene has them and the tile's beam is within their slope limit
                const float4 *csorted = reinterpret_cast<const float4 *>(fc.csorted);
                const int c = (csorted && b.k <= fc.cone_kcap)
                                  ? build_list2<Cfg::STATS, false, true, 2>(fc, n, mylist, mykeys, myblks, b, lane, st_cull,
                                                                              csorted, reinterpret_cast<const float4 *>(fc.cblocks),
                                                                              fc.corig)
                                  : build_list2<Cfg::STATS, false, true>(fc, n, mylist, mykeys, myblks, b, lane, st_cull);
                if (c <= RT_LIST_CAP) {
                    p_use_list = true;
                    pcount = c;
                } else if (Cfg::STATS == 1) {
                    st_overflow += 1;
                }
                if (Cfg::STATS == 1) st_entries += (unsigned long long)(c <= RT_LIST_CAP ? c : n);
            }
            if (Cfg::MESH && ok) {
                const int cb = build_box_list(reinterpret_cast<const float4 *>(ax->box_spheres), fc.n_boxes, myboxes, myboxes + RT_LDS_MESH_BLKS, b, lane);
                if (cb <= RT_BOX_CAP) {
                    pb_use_list = true;
                    pbcount = cb;
                }
                pbeam = b;
                pbeam_ok = !Cfg::force_slow;
                if (Cfg::STATS == 1) sm_plisted += (unsigned long long)pbcount;
            }
        }

        phase(1);
        float nt = __builtin_inff();
        float hcx = 0.f, hcy = 0.f, hcz = 0.f;   // centre of the closest sphere
        int hkind = 1;                           // 0 triangle, 1 sphere, 2 plane, 3 cube (kernel.cu:1376)
        int htri = 0;
        int hprim = 0;                           // list position of the closest plane or cube (AOV only)
        if (Cfg::MESH) {
            // triangles through the flat list of leaf boxes, kernel.cu:1293-1328 (before
            // the spheres, as there): a lane tests a leaf's triangles iff its ray hits the box
            const V3 inv{1.f / D.x, 1.f / D.y, 1.f / D.z};
            for (int jj = 0; jj < (RT_ABL(2048) ? 0 : pbcount); ++jj) {
                const int j = pb_use_list ? myboxes[jj] : jj;
                const RtBoxDev bx = ax->boxes[j];
                const bool bh = box_intersect(bx, O, inv);
                if (any64(bh) && !RT_ABL(1024)) {
                    if (Cfg::STATS == 1) sm_pleaf += 1;
                    // which of the leaf's triangles the tile's beam can touch at all (a leaf of the reference's
                    // ten-pass split holds triangles far larger than a tile: about a third survive), 63 triangles
                    // -- nine loads of seven -- at a time: the split leaves a few leaves of a hundred and more
                    for (int c0 = 0; c0 < bx.len; c0 += 63) {
                        const int clen = bx.len - c0 < 63 ? bx.len - c0 : 63;
                        unsigned long long tmask = ~0ull;
                        if (Cfg::CULL && pbeam_ok) {
                            const int ti = bx.start + c0 + (lane < clen ? lane : 0);
                            const float4 ts = reinterpret_cast<const float4 *>(ax->tri_bs)[ti];
                            const float4 tn = reinterpret_cast<const float4 *>(ax->tri_nrm)[ti];
                            tmask = ballot64(lane < clen && beam_keeps_triangle(pbeam, ts, tn));
                            if (tmask == 0) continue;
                        }
                        // the leaf's vertices, seven triangles (63 floats) per coalesced load, staged in LDS
                        // and broadcast from there: one memory round trip per seven triangles instead of
                        // two dependent scalar loads per triangle
                        for (int base = 0; base < clen; base += 7) {
                            const int cnt = clen - base < 7 ? clen - base : 7;
                            if (((tmask >> base) & 0x7full) == 0) continue;
                            mytri[lane] = ax->tri9[(size_t)(bx.start + c0 + base) * 9 + lane];   // the array is padded by 64 floats
                            wave_lds_sync();
                            for (int i = 0; i < cnt; ++i) {
                                if (!((tmask >> (base + i)) & 1ull)) continue;
                                const float *tv = mytri + 9 * i;
                                float t, u, v;
                                if (Cfg::STATS == 1) sm_ptri += 1;
                                if (bh && tri_intersect(O, D, tv, tv + 3, tv + 6, t, u, v) && t < nt) {
                                    nt = t;
                                    htri = bx.start + c0 + base + i;   // position in tri_idx; resolved when shading (u, v too)
                                    hkind = 0;
                                }
                            }
                            wave_lds_sync();
                        }
                    }
                }
            }
        }
        // without a list the table is walked in list order, from global memory
        auto primary_entry = [&](int e) -> float4 {
            if (Cfg::CULL) return p_use_list ? mylist[e] : spheres[e];
            return spheres[e];
        };
        // A culled list comes front to back (build_list2): entry e carries its list position in
        // mykeys[e] and a lower bound of its t in the block-list slot e. `holder` is the list
        // position of the sphere that currently holds nt (-1: none, e.g. a triangle does), so
        // that "first index wins ties" (kernel.cu:1335) holds in any order of evaluation.
        const float *plbs = reinterpret_cast<const float *>(myblks);
        const bool p_front_to_back = Cfg::CULL && p_use_list && pcount > 1;
        int holder = -1;
        int hent = 0;   // (RT_MODE_REST_WRITE) the list entry that holds nt
        // Primary records (step 5c): a reading launch whose tile has a record does not walk. Which entry each lane ends on
        // is what the recording launch decided from the same list and the same rays; the lane evaluates that one entry, by
        // the walk's own gate, functions and operands, and so arrives at the same nt, holder and centre. A lane on record
        // as a miss keeps nt = +inf; the record is not trusted beyond that: hit_m below is formed from nt as ever.
        // (wave-uniform: the tile read a view list, and no valid lane's record says "none")
        const bool pr_use = Cfg::VD_USE && v_use && (valid_m & LM((pr_rec & 0xffu) == RT_PRIMARY_NONE)) == 0;
        if (Cfg::VD_USE && pr_use) {
            const unsigned e = pr_rec & 0xffu;
            if (valid && e < (unsigned)RT_VIEW_CAP) {
                const float4 s = mylist[e];
                const int pos = mykeys[e];
                const Quad q = quadratic(pr, s);
                const bool need = q.disc >= 0.f && !(q.h > 0.f && q.disc < q.BB * RT_BEHIND_FACTOR);
                float t;
                if (need && intersect_tail_t<Cfg::LEAN_PRIMARY_TAIL>(pr, q, t) && t < nt) {
                    nt = t;
                    holder = pos;
                    hcx = s.x; hcy = s.y; hcz = s.z;
                }
            }
        }
        float4 pcur = pcount > 0 ? primary_entry(0) : make_float4(0.f, 0.f, 0.f, 0.f);
        for (int e = 0; !(Cfg::VD_USE && pr_use) && e < ((RT_ABL(262144) && pcount > 1) ? 1 : pcount); ++e) {   // (262144: the price of the walk -- entry 0 for every lane)
            const float4 s = pcur;
            const int pos = (Cfg::CULL && p_use_list) ? mykeys[e] : e;
            pcur = primary_entry(e + 1 < pcount ? e + 1 : e);   // one entry in flight
            const Quad q = quadratic(pr, s);
            lmask need = LM(q.disc >= 0.f);
            if (!Cfg::force_slow) need &= ~(LM(q.h > 0.f) & LM(q.disc < q.BB * RT_BEHIND_FACTOR));
            if (Cfg::force_slow) need = ~0ull;
            if (need != 0) {
                if (lane_in(need)) {
                    float t;
                    if (intersect_tail_t<Cfg::LEAN_PRIMARY_TAIL>(pr, q, t)) {
                        // strict, and among equal t the lower list position: first index wins ties
                        if (t < nt || (t == nt && holder >= 0 && pos < holder)) {
                            nt = t;
                            holder = pos;
                            if (Cfg::VD_REC) hent = e;
                            hcx = s.x; hcy = s.y; hcz = s.z;
                            if (Cfg::MESH) hkind = 1;
                        }
                    }
                }
            }
            if (Cfg::STATS == 1) { st_primary += __popcll(valid_m); st_slots += 64; }
            // every remaining entry returns t >= its bound >= the next entry's bound
            if (p_front_to_back && e + 1 < pcount && !Cfg::force_slow) {
                const float lb_next = plbs[e + 1];
                if ((valid_m & ~LM(nt < lb_next)) == 0) break;
            }
        }
        if (Cfg::CULL) wave_lds_sync();   // the list is rebuilt below
        // cubes (kernel.cu:1344-1356) then planes (:1359-1372): few, tested exhaustively;
        // for a plane hit hc* carries the plane's normal instead of a centre
        if (Cfg::PRIMS && fc.n_cubes > 0) {
            const V3 inv{1.f / D.x, 1.f / D.y, 1.f / D.z};
            for (int i = 0; i < fc.n_cubes; ++i) {
                const RtCubeDev c = ax->cubes[i];
                float t;
                if (cube_intersect(c, O, inv, t) && t < nt) {
                    nt = t;
                    hkind = 3;
                    hcx = c.cx; hcy = c.cy; hcz = c.cz;
                    if (Cfg::AOV) hprim = i;
                }
            }
        }
        for (int i = 0; i < (Cfg::PRIMS ? fc.n_planes : 0); ++i) {
            const RtPlaneDev p = ax->planes[i];
            float t;
            if (plane_intersect(p, O, D, t) && t < nt) {
                nt = t;
                hkind = 2;
                hcx = p.nx; hcy = p.ny; hcz = p.nz;
                if (Cfg::AOV) hprim = i;
            }
        }
        phase(2);

        const lmask hit_m = valid_m & LM(nt != __builtin_inff());   // kernel.cu:1374
        const bool hit = lane_in(hit_m);

        // ================= miss: skybox::getFColor, kernel.cu:1147-1166 =================
        int sky_idx = -1;
        int pr_tex = 0;   // (RT_MODE_REST_WRITE) the lane's clamped texel index, sky or object texture
        if (Cfg::VD_USE && pr_use) {
            // the sky texel on record: no sky-sphere intersection, no normalise, no uv chain; the clamp stays
            if (valid && !hit) {
                sky_idx = clamp_texel((int)(pr_rec >> 8), ax->sky_w * ax->sky_h - 1);
            }
        } else if (valid && !hit) {
            const float4 sk = make_float4(ax->sky_cx, ax->sky_cy, ax->sky_cz, ax->sky_r2);
            const Quad q = quadratic(pr, sk);
            float t;
            intersect_tail_t<Cfg::LEAN_PRIMARY_TAIL>(pr, q, t);   // the boolean is ignored there, t is used as left
            const V3 hp{O.x + D.x * t, O.y + D.y * t, O.z + D.z * t};
            V3 nrm{hp.x - sk.x, hp.y - sk.y, hp.z - sk.z};
            normalise_t<Cfg::LEAN>(nrm);
            const int sky_w = ax->sky_w, sky_h = ax->sky_h;
            int ix, iy;
            int sky_fast = -1;
            if (Cfg::FAST) {
                float ux, uy;
                approx_sphere_uv(nrm, ux, uy);
                ix = f2i(ux * (float)sky_w);
                iy = f2i(uy * (float)sky_h);
            } else {
                if (Cfg::LEAN) {
                    // the same certainty test as for the object texture (approx_sphere_uv / sure_texel above); here
                    // the exact expressions are binary32 chains of their own -- atan2f and acosf rounded to float, a
                    // float division, 1.f + ..., two products -- which stay within 1.7e-7 of the real value, so the
                    // margin is size * (1e-6 + 2^-22): 5e-7 approximation budget + that + both product roundings
                    float ux, uy;
                    approx_sphere_uv(nrm, ux, uy);
                    sky_fast = sure_texel(ux, uy, sky_w, sky_h, ax->sky_mu_x, ax->sky_mu_y);
                }
                ix = iy = 0;
                if (__builtin_expect(sky_fast < 0, 0)) {
                    ix = f2i((1.f + rtm::atan2f_rt(nrm.z, nrm.x, myatan) / 3.1415f) * 0.5f * (float)sky_w);
                    iy = f2i(rtm::acosf_rt(nrm.y, myatan) / 3.1415f * (float)sky_h);
                }
            }
            sky_idx = clamp_texel(sky_fast >= 0 ? sky_fast : iy * sky_w + ix, sky_w * sky_h - 1);   // documented clamp (reference is UB there)
            if (Cfg::VD_REC) pr_tex = sky_idx;
        }

        // ================= hit: shade, kernel.cu:1396-1405, 1643-1677 =================
        V3 start{0.f, 0.f, 0.f}, normal{0.f, 1.f, 0.f};
        float tr = 0.f, tg = 0.f, tb = 0.f;
        if (hit) {
            // the texture's uniforms: read from the kernel-argument segment here (see the write-back), not carried through
            // the primary cull and tests
            FcPtr kt = kargs_again();
            const int t_w = kt->tex_w, t_h = kt->tex_h;
            const V3 new_org{O.x + D.x * nt, O.y + D.y * nt, O.z + D.z * nt};
            float tx = 0.5f, ty = 0.5f;   // plane, kernel.cu:1413-1414
            int ci_fast = -1;             // texel index already known for sure (sphere / cube hits of the culling kernels)
            V3 hp = new_org;              // what start_O is offset from
            if (Cfg::MESH && hkind == 0) {     // triangle, kernel.cu:1378-1393
                const RtTriDev *tp = ax->tris + ax->tri_idx[htri];
                // the barycentrics of the winning triangle: the same operations on the same operands as
                // in the loop above (which does not carry them along)
                float hnt, hnu = 0.f, hnv = 0.f;
                (void)tri_intersect(O, D, tp->p0, tp->p1, tp->p2, hnt, hnu, hnv);
                const float w0 = 1 - hnu - hnv;
                if (fc.flags & RT_FLAG_MESH_NORMALS) {
                    normal = V3{(tp->vn[0] * w0 + tp->vn[3] * hnu) + tp->vn[6] * hnv,
                                (tp->vn[1] * w0 + tp->vn[4] * hnu) + tp->vn[7] * hnv,
                                (tp->vn[2] * w0 + tp->vn[5] * hnu) + tp->vn[8] * hnv};
                    normalise_t<Cfg::LEAN>(normal);
                } else {
                    normal = V3{tp->n[0], tp->n[1], tp->n[2]};
                }
                tx = (w0 * tp->vt[0]) + (hnu * tp->vt[2]) + (hnv * tp->vt[4]);
                ty = (w0 * tp->vt[1]) + (hnu * tp->vt[3]) + (hnv * tp->vt[5]);
                // new_org = add(normal, add(Org, Dir * nt)): displaced by the whole normal
                hp = V3{normal.x + new_org.x, normal.y + new_org.y, normal.z + new_org.z};
                hcx = hcy = hcz = 0.f;    // one group for all triangle hits of the tile
            } else if (Cfg::PRIMS && hkind == 2) {      // plane, kernel.cu:1407-1416: the normal as stored
                normal = V3{hcx, hcy, hcz};
            } else {                      // sphere / cube, kernel.cu:1396-1405, 1418-1425
                normal = V3{new_org.x - hcx, new_org.y - hcy, new_org.z - hcz};
                normalise_t<Cfg::LEAN>(normal);
                if (RT_ABL(8)) {
                    tx = normal.x; ty = normal.y;
                } else if (Cfg::VD_USE && pr_use) {
                    ci_fast = (int)(pr_rec >> 8);       // the texel on record (24 bits: never negative); clamped below
                } else if (Cfg::FAST) {
                    approx_sphere_uv(normal, tx, ty);   // no certainty test: a texel now and then is the neighbour
                } else if (Cfg::LEAN && !RT_ABL(4096)) {
                    float ux, uy;
                    approx_sphere_uv(normal, ux, uy);
                    ci_fast = sure_texel(ux, uy, t_w, t_h, kt->tex_mu_x, kt->tex_mu_y);
                    if (__builtin_expect(ci_fast < 0, 0)) exact_uv(normal, myatan, tx, ty);
                } else {
                    exact_uv(normal, myatan, tx, ty);
                }
            }
            int ci = f2i(ty * (float)t_h) * t_w + f2i(tx * (float)t_w);
            if (ci_fast >= 0) ci = ci_fast;
            ci = clamp_texel(ci, t_w * t_h - 1);       // documented clamp
            if (Cfg::VD_REC) pr_tex = ci;
            tr = kt->tex_r[ci];
            tg = kt->tex_g[ci];
            tb = kt->tex_b[ci];
            // start_O = normal * 0.00001 + new_org, kernel.cu:1647
            start = V3{normal.x * 0.00001f + hp.x, normal.y * 0.00001f + hp.y, normal.z * 0.00001f + hp.z};
            if (Cfg::STATS == 1) st_hits += 1;
        }
        unsigned ts_pre = 0;   // (RT_MODE_REST_WRITE) the tile's summary before its groups are known
        if (Cfg::VD_REC) ts_pre = store_primary_record<Cfg>(ax, lane, blk_x, blk_y, v_use, hit, hent, pr_tex, valid_m, hit_m);

        phase(3);
        // finite: x - x is 0 (inf - inf and NaN - NaN are NaNs); written as a comparison of its own -- `fabs(x) < inf` becomes
        // a class test, whose ballot goes through a 0/1 register
        const lmask tex_fin_m = LM(tr - tr == 0.f) & LM(tg - tg == 0.f) & LM(tb - tb == 0.f);
        mytex[lane] = tr;
        mytex[64 + lane] = tg;
        mytex[128 + lane] = tb;
        if (sky_idx >= 0) {
            fr = ax->sky_r[sky_idx];
            fg = ax->sky_g[sky_idx];
            fb = ax->sky_b[sky_idx];
        }
        if (Cfg::AOV) store_gbuffer<Cfg>(ax, lane, wave, valid, hit, nt, normal, hkind, htri, hprim, holder, tr, tg, tb, fr, fg, fb);
        if (Cfg::VERD) park_verdicts<Cfg>(myvd, lane, vd_ld, ts_pre);
        if (hit_m != 0 && !RT_ABL(16)) {
            int gid = -1;
            const int n_groups = form_groups<Cfg>(hit_m, hcx, hcy, hcz, hkind, gid);
            for (int g = 0; g < n_groups; ++g) {
            const lmask inc_m = LM(gid == g);   // (gid is -1 where nothing was hit)
            const bool inc = lane_in(inc_m);
            if (Cfg::STATS == 1) st_clusters += 1;
            // The group's ray origins, bounded once for all lights: a ball around the first
            // member's `start`. (Per-light axial and perpendicular extents would be a little
            // tighter, for three more wave reductions per light; the patch a tile sees of one
            // primitive is small against the spheres it is culled against.)
            float g_ax = 0.f, g_ay = 0.f, g_az = 0.f, g_r2 = 0.f;
            int g_sphere = -1;     // list position of the sphere the group lies on (-1: a plane, cube or triangle)
            if (Cfg::CULL) {
                const int glead = __builtin_ctzll(inc_m);
                g_sphere = __builtin_amdgcn_readlane(holder, glead);
                if (Cfg::PRIMS && __builtin_amdgcn_readlane(hkind, glead) != 1) g_sphere = -1;
                // (Groups are formed by the CENTRE of the closest sphere, so two concentric spheres would share one. They
                // never do where it matters: intersect() returns the near root even when it is negative, and of two
                // concentric spheres the larger has the smaller C, hence the larger discriminant and the smaller near
                // root for every ray whose line meets the smaller one -- wherever the camera is, only the largest of a
                // concentric family is ever a closest hit; radii so close that the roots round to the same float differ
                // by far less than the 1e-3 by which the list's ball exceeds its sphere; a non-finite entry anywhere in
                // the table switches the lists off. tests/test_gpu_scenarios.py renders the camera-in-between case.)
                g_ax = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, start.x), glead));
                g_ay = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, start.y), glead));
                g_az = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, start.z), glead));
                if (!Cfg::LAZY_BALL) {
                // (twice, here and at LAZY_BALL's first culling light: as one function with g_r2 and g_sphere by reference it moved four
                // kernels' spilled scalars, 11 -> 14 in the product one; as two that return them, 24 lines of its machine code)
                const float ox = start.x - g_ax, oy = start.y - g_ay, oz = start.z - g_az;
                g_r2 = uniform(wave_max(inc ? __builtin_fmaf(ox, ox, __builtin_fmaf(oy, oy, oz * oz)) : 0.f));
                // The sphere's occluder lists and its kbeam (rt_tables.hip) hold for starts inside the ball of radius
                // R 1.001 + 1e-3 around its centre. A start is a float hit point: at a grazing primary ray the rounding of
                // the discriminant moves it along the ray by up to ~1e-3 of the camera's distance, far outside that ball
                // (tests/test_margins_cpu.py). So the ball is checked, every start of the group against it, in float
                // with 1e-5 relative to spare (|start - c|^2 and the radius carry a few ulp each); a group that has a
                // start outside takes neither the list nor kbeam and culls as a group on a plane does.
                if (g_sphere >= 0) {
                    const float4 sc = spheres[g_sphere];
                    const float cx = start.x - sc.x, cy = start.y - sc.y, cz = start.z - sc.z;
                    const float ball = __builtin_amdgcn_sqrtf(sc.w) * 1.001f + 1.0e-3f;
                    const float far2 = uniform(wave_max(inc ? __builtin_fmaf(cx, cx, __builtin_fmaf(cy, cy, cz * cz)) : 0.f));
                    if (!(far2 <= ball * ball * 0.99999f)) g_sphere = -1;   // (also for a NaN)
                }
                }
            }
            bool ball_done = !Cfg::LAZY_BALL;   // (LAZY_BALL: the two reductions wait for the group's first light that culls at all)
            for (int li = 0; li < fc.n_lights; ++li) {
                // An earlier launch of the same inputs left this iteration by one of the three exits marked below:
                // so would this one, having added nothing -- the iteration is skipped whole.
                // (groups beyond RT_VERDICT_GROUPS and lights beyond RT_VERDICT_LIGHTS have no bits: always evaluated)
                const bool vd_has = Cfg::VERD && g < RT_VERDICT_GROUPS && li < RT_VERDICT_LIGHTS;
                const int vd_sh = 16 * (g & 1) + 2 * li;
                unsigned vd = 0;
                if (Cfg::VD_USE && vd_has) vd = ((unsigned)__builtin_amdgcn_readfirstlane((int)myvd[g >> 1]) >> vd_sh) & 3u;
                if (Cfg::VD_USE && vd == RT_VERDICT_NOTHING) continue;
                auto vd_note = [&](unsigned code) {
                    if (Cfg::VD_REC && vd_has && lane == 0)
                        (void)__hip_atomic_fetch_or(&myvd[g >> 1], code << vd_sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                };
                // Shadow counts: a light that the recording launch walked to the end (code 0) and gave a record. Its lanes'
                // numbers of unshadowed samples are what this launch would count again from the same bits, so the
                // iteration takes the all-clear path -- the facing test (lit_m is still needed), then the chain's begin and
                // settle for toL, no list header, beam, cull, all-clear test, list order, pre-pass or sample -- and the
                // shading reads the lane's count from the record instead of RT_SHADOW_SAMPLES.
                if (Cfg::VD_USE && vd_has && vd == 0) {
                    const unsigned tg = (unsigned)__builtin_amdgcn_readfirstlane((int)myvd[2]);
#pragma unroll
                    for (int r = 0; r < RT_SHADOW_RECORDS; ++r)
                        if (((tg >> (8 * r)) & 0xffu) == RT_SHADOW_TAG(g, li)) vd = 4u + r;   // (neither code: record r)
                }
                const bool sc_use = Cfg::VD_USE && vd >= 4u;
                const RtLightDev L = ax->lights[li];
                const V3 lpos{L.px, L.py, L.pz};

                // toL = normalise(l.pos - start), kernel.cu:1438 -- here only to ~1e-6 (fast
                // reciprocal square root): it feeds the facing test and the beam bound, both of
                // which carry margins; the exact value is formed by ShadowChain::begin when the
                // samples are actually constructed.
                V3 toL{lpos.x - start.x, lpos.y - start.y, lpos.z - start.z};
                {
                    const float inv = __builtin_amdgcn_rsqf(__builtin_fmaf(toL.x, toL.x, __builtin_fmaf(toL.y, toL.y, toL.z * toL.z)));
                    toL.x *= inv; toL.y *= inv; toL.z *= inv;
                }

                // A surface that faces away from the light gets b *= 0 at kernel.cu:1542
                // whatever its ten shadow samples say, and fr + (0*l.r)*r leaves fr
                // untouched. The reference's `a` uses toL after its in-place
                // re-normalisations, which move it by an ulp or two, so only a clearly
                // negative normal.toL (and finite factors, so that 0*x is 0) counts.
                // Such lanes take no part in this light; if the whole group faces away
                // the light is skipped. (Not applied in the brute-force build, which
                // runs the reference's loops as written and is what tests compare with.)
                lmask lit_m = inc_m;
                lmask zero_ok_m = 0;   // brightness 0 adds exactly nothing for this lane
                if (Cfg::CULL && !Cfg::force_slow) {
                    const float a0 = dot3(normal, toL);
                    // (0 * l.r) * r is 0 iff the light's colour (frame constant, checked by the host) and the
                    // texel (checked once per pixel) are finite
                    zero_ok_m = (L.fin != 0.f) ? (tex_fin_m & LM(__builtin_fabsf(a0) < 1.0e30f)) : 0ull;
                    lit_m = inc_m & ~(LM(a0 < -1.0e-4f) & zero_ok_m);   // (facing away: takes no part)
                    if (lit_m == 0) {
                        vd_note(RT_VERDICT_NOTHING);
                        continue;
                    }
                }
                const bool lit = lane_in(lit_m);
                const bool all_zero_ok = (lit_m & ~zero_ok_m) == 0;   // every lit pixel may take a zero brightness as "adds nothing"

                // ---------- conservative beam for this light's 10 x 64 rays ----------
                bool s_use_list = false;
                int scount = n;
                bool sb_use_list = false;
                int sbcount = Cfg::MESH ? fc.n_boxes : 0;
                float beam_k = 0.f;   // slope of the light's beam (valid when s_use_list)
                // (a light whose all-clear test held for these inputs needs neither its list nor the test again)
                // (nor does a light whose counts are on record)
                if (Cfg::CULL && !(Cfg::VD_USE && vd == RT_VERDICT_CLEAR) && !sc_use) {
                    if (Cfg::LAZY_BALL && !ball_done) {   // the group's ball, as above
                        const float ox = start.x - g_ax, oy = start.y - g_ay, oz = start.z - g_az;
                        g_r2 = uniform(wave_max(inc ? __builtin_fmaf(ox, ox, __builtin_fmaf(oy, oy, oz * oz)) : 0.f));
                        if (g_sphere >= 0) {
                            const float4 sc = spheres[g_sphere];
                            const float cx = start.x - sc.x, cy = start.y - sc.y, cz = start.z - sc.z;
                            const float ball = __builtin_amdgcn_sqrtf(sc.w) * 1.001f + 1.0e-3f;
                            const float far2 = uniform(wave_max(inc ? __builtin_fmaf(cx, cx, __builtin_fmaf(cy, cy, cz * cz)) : 0.f));
                            if (!(far2 <= ball * ball * 0.99999f)) g_sphere = -1;
                        }
                        ball_done = true;
                    }
                    bool ok = true;
                    Beam b;
                    b.ux = L.ux; b.uy = L.uy; b.uz = L.uz;
                    // How far this light's sample directions can stray from its axis u = l.pos/|l.pos|, per lane, from the
                    // approximate toL (fast math; the allowance is RT_SPREAD_*). A sample direction is w_j = l.pos - r_j with
                    // r_j = x_j R0 + y_j R1 + z_j R2 = M^T v_j (Ri: rows of the matrix of kernel.cu:1267-1277, built from
                    // toL with az = 0), v_j = (sqrt(1 - z_j^2) (cos phi_j, sin phi_j), z_j), |v_j| <= 1. Its deviation:
                    // sin = |w x u| / |w| = |r x u| / |w| (l.pos x u = 0), |w| >= |l.pos| - |r| >= |l.pos| - ||M||_F, and
                    // |r x u| = |E^T r| for an orthonormal pair E = [e1 e2] across u (host: RtLightDev): E^T r = (M E)^T v,
                    // whose supremum over |v| <= 1 is the larger singular value of the 3 x 2 matrix M E (column k =
                    // (R0.ek, R1.ek, R2.ek)) = the root of the larger eigenvalue of the 2 x 2 Gram matrix of its columns.
                    // That is the EXACT supremum over the unit ball (round 2 bounded (x, y) and z separately: up to a
                    // quarter more, and a launch's work grows by a third when the beams are twice as wide). A NaN or inf
                    // anywhere makes smax2 a NaN, which switches culling off below; toL within 0.6 degrees of +-z, where
                    // the axis (0,0,1) x toL is all rounding, takes a bound that holds for every axis: ||M||_F^2 <= 6 < 8.
                    // ... unless the group lies on a sphere whose header carries the bound for ANY start on it (kbeam:
                    // rt_tables.hip, rt_sphere_beam_slope -- the same supremum over the whole cone of toL the sphere's
                    // surface subtends, evaluated once per sphere and light in binary64): the hundred instructions
                    // below are then not executed at all
#ifdef RT_NO_CAND
                    const RtCandHdr *chdr = nullptr;
#else
                    const RtCandHdr *chdr = ax->cand_hdr[li];
#endif
                    RtCandHdr ch{0, -1, 0.f, -1.f};
                    if (!RT_ABL(65536) && chdr && g_sphere >= 0) ch = chdr[g_sphere];
                    const bool own_bound = !(ch.kbeam > 0.f) || RT_ABL(524288);
                    float smax2 = 0.f;
                    if (!own_bound) {
                        b.k = ch.kbeam;
                    } else {
                    if (RT_ABL(32)) smax2 = 0.01f;
                    else {
                        const float c = toL.z;
                        const float sn = __builtin_amdgcn_sqrtf(__builtin_fmaxf(1.f - c * c, 0.f));
                        const float q2 = toL.x * toL.x + toL.y * toL.y;
                        const float rq = q2 > 0.f ? __builtin_amdgcn_rsqf(q2) : 0.f;
                        const float ax = -toL.y * rq, ay = toL.x * rq;   // axis = (0,0,1) x toL, az = 0
                        const float omc = 1.f - c;
                        // rotate(nAngle, axis), kernel.cu:1267-1277, with az = 0
                        const float m00 = c + ax * ax, m01 = ax * ay * omc, m02 = -ay * sn;
                        const float m10 = m01, m11 = c + ay * ay * omc, m12 = -ax * sn;
                        const float m20 = -ay * sn, m21 = ax * sn, m22 = c;
                        const float p0 = __builtin_fmaf(m00, L.e1x, __builtin_fmaf(m01, L.e1y, m02 * L.e1z));
                        const float p1 = __builtin_fmaf(m10, L.e1x, __builtin_fmaf(m11, L.e1y, m12 * L.e1z));
                        const float p2 = __builtin_fmaf(m20, L.e1x, __builtin_fmaf(m21, L.e1y, m22 * L.e1z));
                        const float q0 = __builtin_fmaf(m00, L.e2x, __builtin_fmaf(m01, L.e2y, m02 * L.e2z));
                        const float q1 = __builtin_fmaf(m10, L.e2x, __builtin_fmaf(m11, L.e2y, m12 * L.e2z));
                        const float q2_ = __builtin_fmaf(m20, L.e2x, __builtin_fmaf(m21, L.e2y, m22 * L.e2z));
                        const float h11 = __builtin_fmaf(p0, p0, __builtin_fmaf(p1, p1, p2 * p2));
                        const float h22 = __builtin_fmaf(q0, q0, __builtin_fmaf(q1, q1, q2_ * q2_));
                        const float h12 = __builtin_fmaf(p0, q0, __builtin_fmaf(p1, q1, p2 * q2_));
                        const float hd = 0.5f * (h11 - h22);
                        float kmax2 = (0.5f * (h11 + h22) + __builtin_amdgcn_sqrtf(hd * hd + h12 * h12)) * 1.001f;
                        float frob2 = __builtin_fmaf(m00, m00, __builtin_fmaf(m01, m01, m02 * m02)) +
                                      __builtin_fmaf(m10, m10, __builtin_fmaf(m11, m11, m12 * m12)) +
                                      __builtin_fmaf(m20, m20, __builtin_fmaf(m21, m21, m22 * m22));
                        const bool polar = q2 < 1.0e-4f;     // not for a NaN: that one must reach smax2
                        kmax2 = polar ? 8.f : kmax2;         // (8 rather than 6: an inline constant of the instruction set, where
                        frob2 = polar ? 8.f : frob2;         // any other literal in a select occupies a register across the loops)
                        const float den = L.pos_len - __builtin_amdgcn_sqrtf(frob2) * 1.001f;
                        // a light closer to the origin than the matrix can reach has no usable bound
                        const float rden = __builtin_amdgcn_rcpf(den);
                        smax2 = (den > 0.05f * L.pos_len) ? kmax2 * rden * rden * 1.0001f : __builtin_nanf("");
                    }
                    if (!lit || smax2 < 0.f) smax2 = 0.f;   // (the wave maximum compares bit patterns; a NaN passes through)
                    ok = (lit_m & ~LM(smax2 < 0.25f)) == 0;
                    const float s2w = uniform(wave_max(smax2));
                    const float snw = __builtin_amdgcn_sqrtf(s2w) * RT_SPREAD_MUL + RT_SPREAD_ADD;
                    b.k = snw * __builtin_amdgcn_rsqf(__builtin_fmaxf(1.f - snw * snw, 0.05f));
                    }
                    // origins: the group's ball (see above), centred on the axis
                    b.ax = g_ax; b.ay = g_ay; b.az = g_az;
                    ok = ok && (g_r2 < RT_R0_CAP * RT_R0_CAP * 0.99f);   // (false for a NaN; the paddings assume r0 <= RT_R0_CAP)
                    b.r0 = __builtin_amdgcn_sqrtf(g_r2) * 1.001f + RT_ORIGIN_ADD;
                    b.smin = -b.r0;
                    b.smax = b.r0;
                    phase(4);
                    if (RT_ABL(4)) { ok = false; scount = 0; }
                    if (ok) {
                        // One sphere in front of the whole beam shadows all 10 samples of
                        // every lit lane: unshadowed = 0, b = 0, and the light adds exactly
                        // nothing -- the sample construction and the tests are skipped.
                        const bool may_skip = !Cfg::force_slow && !RT_ABL(64) && all_zero_ok;
                        const float4 *lsorted = reinterpret_cast<const float4 *>(ax->lsorted[li]);
                        // the fallback culls read the table pointers and block count from the kernel-argument segment
                        // HERE (see the write-back): they are rarely needed once the occluder lists exist, and held in
                        // scalar registers from the kernel's entry they are spilled around every loop in between
                        FcPtr kl = kargs_again();
                        // the group's own sphere has a list of what can shadow it from this light: cull that
                        int cand_n = ch.count;
                        const int cand_off = ch.offset;
                        if (!(uniform(b.k) <= ch.kcap)) cand_n = -1;   // (also for a NaN)
                        const int cb = cand_n >= 0 ? build_list_cand<Cfg::STATS>(reinterpret_cast<const float4 *>(ax->cand_ent[li]) + cand_off, cand_n,
                                                                            mylist, b, lane, st_cull, may_skip)
                                     : lsorted ? build_list2<Cfg::STATS, true, false, 1>(
                                                     *kl, n, mylist, mykeys, myblks, b, lane, st_cull, lsorted,
                                                     reinterpret_cast<const float4 *>(ax->lblocks[li]), nullptr, may_skip)
                                               : build_list2<Cfg::STATS, true, false>(*kl, n, mylist, mykeys, myblks, b,
                                                                                         lane, st_cull, nullptr, nullptr, nullptr, may_skip);
                        const int c = cb & 0x3fffffff;
                        if (may_skip && (cb & 0x40000000)) {
                            if (Cfg::STATS == 1) hist[7] += 1;
                            wave_lds_sync();
                            vd_note(RT_VERDICT_NOTHING);
                            continue;
                        }
                        if (Cfg::MESH && RT_ABL(32768)) {
                            sb_use_list = true;
                            sbcount = 0;
                        } else if (Cfg::MESH) {
                            const int cbx = build_box_list(reinterpret_cast<const float4 *>(ax->box_spheres), fc.n_boxes, myboxes, myboxes + RT_LDS_MESH_BLKS, b, lane);
                            if (cbx <= RT_BOX_CAP) {
                                sb_use_list = true;
                                sbcount = cbx;
                            }
                        }
                        if (c <= RT_LIST_CAP) {
                            s_use_list = true;
                            scount = c;
                            beam_k = b.k;
                        } else if (Cfg::STATS == 1) {
                            st_overflow += 1;
                        }
                        if (Cfg::STATS == 1) st_entries += (unsigned long long)(c <= RT_LIST_CAP ? c : n);
                        if (Cfg::STATS == 1) {
                            const int bin = c <= 1 ? 0 : c <= 2 ? 1 : c <= 4 ? 2 : c <= 8 ? 3 : c <= 16 ? 4 : c <= RT_LIST_CAP ? 5 : 6;
                            hist[bin] += 1;
                        }
                    }
                }

                phase(5);
                // ---------- the 10 samples, kernel.cu:1442-1540 (exact) ----------
                ShadowChain<Cfg::LEAN> chain;
                // one register for both: bits 0..15 = samples left to the exact chain (pre-pass), bits 16.. = unshadowed samples so far
                unsigned us = 0;
                // (inline: as a function returning all_clear this test moved the spilled-scalar counts of four kernels, 14 -> 18 in the reading one)
                // A short list whose every sphere lies behind every ray of the beam (for
                // each lit lane: start outside the sphere by more than the `behind`
                // shortcut needs, C > 2e-5*|oc|^2, and the whole cone of directions on the
                // far side, cos(u,oc) > sin(u,oc)*tan(theta) + 0.02) leaves all ten samples
                // unshadowed without constructing one of them: only toL's evolution is
                // needed for kernel.cu:1541. Typically the list is just the sphere the
                // tile itself lies on.
                bool all_clear = (Cfg::VD_USE && vd == RT_VERDICT_CLEAR) || sc_use;   // (sc_use: no walk either; the counts differ)
                if (Cfg::CULL && (!Cfg::MESH || (sb_use_list && sbcount == 0)) && s_use_list && scount <= 4 && !Cfg::force_slow &&
                    !RT_ABL(128) && (!Cfg::PRIMS || (fc.n_planes | fc.n_cubes) == 0)) {
                    lmask clear = ~0ull;
                    for (int e = 0; e < scount; ++e) {
                        const float4 sp = mylist[e];
                        const float ocx = start.x - sp.x, ocy = start.y - sp.y, ocz = start.z - sp.z;
                        const float q = ocx * ocx + ocy * ocy + ocz * ocz;
                        const float C = q - sp.w;
                        const float cu = (ocx * L.ux + ocy * L.uy + ocz * L.uz) * __builtin_amdgcn_rsqf(q);
                        const float su = __builtin_amdgcn_sqrtf(__builtin_fmaxf(1.f - cu * cu, 0.f));
                        clear &= LM(C > 2.0e-5f * q) & LM(cu > su * beam_k + 0.02f);
                    }
                    all_clear = (lit_m & ~clear) == 0;
                }
                // (the chain begins after the pre-pass below, which borrows its registers for the approximate frame)
                const bool will_prepass = Cfg::CULL && !Cfg::force_slow && !Cfg::FAST && Cfg::FEAT == RT_FEAT_SPHERES && !all_clear && s_use_list && !RT_ABL(131072);
                if (!will_prepass) chain.begin(lpos, start);
                if (all_clear) {
                    chain.settle();
                    us = (unsigned)RT_SHADOW_SAMPLES << 16;
                    vd_note(RT_VERDICT_CLEAR);
                    if (Cfg::STATS == 1) hist[6] += 1;
                }
                // (inline: as a function of the list, the group's origin and the light it changed 13 lines of the product kernel's machine
                // code and 31 of the multi-sample kernel's)
                // The samples will be walked: put the likeliest occluders first -- the spheres that
                // reach farthest across the beam's axis (distance from the axis minus radius) -- so
                // that the any-hit loops end sooner. An any-hit does not depend on the order.
                if (Cfg::CULL && s_use_list && !all_clear && scount > 2 && scount <= 64 && !Cfg::force_slow &&
                    !RT_ABL(256)) {
                    float *kbuf = reinterpret_cast<float *>(myblks);
                    float4 e = make_float4(0.f, 0.f, 0.f, 0.f);
                    float key = 0.f;
                    int rank = 0;
                    if (lane < scount) {
                        e = mylist[lane];
                        const float vx = e.x - g_ax, vy = e.y - g_ay, vz = e.z - g_az;
                        const float vv = __builtin_fmaf(vx, vx, __builtin_fmaf(vy, vy, vz * vz));
                        const float sa = __builtin_fmaf(vx, L.ux, __builtin_fmaf(vy, L.uy, vz * L.uz));
                        key = __builtin_amdgcn_sqrtf(__builtin_fmaxf(__builtin_fmaf(-sa, sa, vv), 0.f)) - __builtin_amdgcn_sqrtf(e.w);
                        key = (key == key) ? key : __builtin_inff();
                        kbuf[lane] = key;
                    }
                    wave_lds_sync();
                    for (int jj = 0; jj < scount; ++jj) {
                        const float kj = kbuf[jj];
                        rank += lane_in(LM(kj < key) | (LM(kj == key) & (~1ull << jj))) ? 1 : 0;
                    }
                    wave_lds_sync();
                    if (lane < scount) mylist[rank] = e;
                    wave_lds_sync();
                }
                if (Cfg::FAST && !all_clear) {   // toL as the reference leaves it (exact), then the sample frame once, approximately
                    chain.settle();
                    chain.setup_fast(L, start);
                }
                // ---------- pre-pass: the ten samples with approximate directions and margins ----------
                // Most of a walked light's cost is the exact construction of its sample directions (binary64 acos / sincos,
                // five normalisations per evaluation, a normalise per sample) -- and for most lanes and samples the answer
                // does not hang on the last bits of a direction: a ray that hits a listed sphere squarely, or misses all
                // of them clearly, does so for every direction within 1e-5 of it. So the ten directions are first formed
                // approximately (setup_approx / direction_approx: binary32, hardware rsq, the approximate toL of the facing
                // test) and every lit lane's ray is classified against the list by presure_test: `shadowed for sure`,
                // `unshadowed for sure`, or undecided. Only samples with an undecided lane are then evaluated by the exact
                // chain, and only the undecided lanes take its result; the toL the brightness needs (kernel.cu:1541) comes
                // from the chain's evolution alone (advance()). Error budget of an approximate direction, |v| <= 1,
                // |w| = |l.pos - M^T v| >= 18 in the guard range: toL from a reciprocal square root against the chain's
                // re-normalised toL, 5e-7, amplified by the frame's sensitivity K = 4/q + 3 <= 83 for q >= 0.05: 4.2e-5 on M,
                // 2.3e-6 on the direction; `angle` (cosine of twice a dot product of two such vectors) 2e-6, through
                // z = jf (1 - angle) + angle into sqrt(1 - z^2) with slope <= 20 (guard: sqrt >= 0.05): 4e-5 on (x, y), 2.2e-6;
                // cos/sin(acos z) against z, sqrt(1 - z^2) and the roundings of either evaluation: below 1e-6. Together
                // below 6e-6 < RT_PRE_DELTA. Sphere scenes only (a lane that misses every sphere could still hit a
                // triangle, plane or cube).
                bool prepass = false, dark = false;
                if (will_prepass) {
                    prepass = true;
                    // (the bookkeeping in wave masks -- scalar registers and scalar instructions: as `bool`s carried around the
                    // loops the flags live in vector registers as 0/1, a select and a compare per use)
                    const lmask ok_m = chain.setup_approx(L, start, toL);
                    // RT_PRE_GROUP samples per pass over the list: what a test forms from the entry and the pixel alone serves all
                    // of them (the last pass takes what is left of the ten)
                    int n_single = 0;   // (STATS) samples for which ONE entry is hit for sure by every lit pixel
                    auto group = [&](auto n_tag, int j0) {
                        constexpr int N = decltype(n_tag)::value;
                        V3 d[N];
                        lmask dok = ok_m;
                        lmask dir_m[N], h[N], m[N];
#pragma unroll
                        for (int i = 0; i < N; ++i) {
                            bool okd;
                            d[i] = chain.direction_approx(ax, L, j0 + i, okd);
                            dir_m[i] = LM(okd);
                            h[i] = 0;
                            m[i] = ~0ull;
                        }
                        int e = 0;
                        bool broke = false;
                        for (; e < scount; ++e) {
                            const PreSure<N> r = presure_test<N>(start, d, mylist[e]);
                            lmask all_hit = ~0ull;
#pragma unroll
                            for (int i = 0; i < N; ++i) {
                                if (Cfg::STATS == 1 && (lit_m & ~h[i]) != 0 && (lit_m & ~r.hit[i]) == 0) n_single += 1;
                                h[i] |= r.hit[i];
                                m[i] &= r.miss[i];
                                all_hit &= h[i];
                            }
                            if (Cfg::STATS == 1) { st_shadow += N * __popcll(lit_m); st_slots += 64 * N; }
                            if ((lit_m & ~all_hit) == 0) { broke = true; break; }
                        }
                        // the entry that completed "every lit pixel hit" goes to the front: the next samples' rays are
                        // neighbours of these, and an any-hit does not depend on the order
                        if (broke && e > 0) {
                            if (lane == 0) {
                                const float4 a = mylist[0], b = mylist[e];
                                mylist[0] = b;
                                mylist[e] = a;
                            }
                            wave_lds_sync();
                        }
#pragma unroll
                        for (int i = 0; i < N; ++i) {
                            const lmask dec = dok & dir_m[i] & (h[i] | m[i]);
                            if (lane_in(lit_m & dec & ~h[i])) us += 1u << 16;
                            if (lane_in(lit_m & ~dec)) us |= 1u << (j0 + i);
                        }
                    };
                    {
                        constexpr int G = RT_PRE_GROUP, R = RT_SHADOW_SAMPLES % G;
                        int j = 0;
#pragma unroll 1
                        for (; j + G <= RT_SHADOW_SAMPLES; j += G) group(std::integral_constant<int, G>{}, j);
                        if constexpr (R != 0) group(std::integral_constant<int, R>{}, j);
                    }
                    if (Cfg::STATS == 1) {   // pre-pass outcome: walks that need the exact chain, and how many of their samples
                        unsigned long long need = 0;
                        for (int j = 0; j < RT_SHADOW_SAMPLES; ++j) need += any64((us >> j) & 1u) ? 1 : 0;
                        st_pre += need + ((need ? 1ull : 0ull) << 24) + ((n_single == RT_SHADOW_SAMPLES ? 1ull : 0ull) << 44);
                    }
                    // Every lit pixel settled, all ten samples of each shadowed (half of the walked lights end so), and a
                    // zero brightness adds exactly nothing for all of them (finite light, texel and normal.toL: the
                    // condition of the full-occluder skip): b = 0 whatever toL turns out to be -- no chain at all.
                    dark = !RT_ABL(2097152) && all_zero_ok && (lit_m & ~LM(us == 0u)) == 0;
                    if (dark) vd_note(RT_VERDICT_NOTHING);
                    if (!dark) {
                        chain.begin(lpos, start);   // toL = normalise(l.pos - start), kernel.cu:1438: the exact chain starts here
                        if (!any64((us & 0xffffu) != 0)) chain.settle();
                    }
                }
                phase(6);   // (all-clear test, list order, pre-pass, settle)
#pragma unroll 1
                for (int j = 0; j < ((all_clear || (prepass && !any64((us & 0xffffu) != 0))) ? 0 : RT_SHADOW_SAMPLES); ++j) {
                    lmask want_m = lit_m;       // lanes whose result of this sample is still open
                    if (prepass) {
                        want_m = lit_m & LM(((us >> j) & 1u) != 0);
                        if (want_m == 0) {      // nobody needs this sample's direction: only toL moves on
                            chain.advance();
                            continue;
                        }
                    }
                    const bool want = lane_in(want_m);
                    const V3 new_dir = RT_ABL(2) ? chain.toL
                                       : Cfg::FAST   ? chain.direction_fast(ax, L, j)
                                                : chain.direction(ax, Cfg::force_slow, L, start, j, myatan);
                    const RayK sr = make_ray(start, new_dir);
                    phase(6);
                    // any-hit over the list, kernel.cu:1501-1510
                    bool shadowed = !want;   // lanes outside the group, unlit or already decided are simply done
                    const int scount_j = RT_ABL(1) ? 0 : scount;
                    if (scount_j > 0) {
                        FcPtr kg = kargs_again();
                        const float4 *gtab = Cfg::CULL ? reinterpret_cast<const float4 *>(kg->sorted) : spheres;
                        // (no entry kept in flight: at 7 waves per SIMD the LDS latency is covered by the other
                        // waves, and the four registers are what lets the kernel run at 7)
                        for (int e = 0; e < scount_j; ++e) {
                            const float4 cur = entry_at(s_use_list, mylist, gtab, e);
                            shadow_test<Cfg::LEAN_SHADOW_TAIL>(sr, cur, shadowed, Cfg::force_slow);
                            if (Cfg::STATS == 1) { st_shadow += __popcll(ballot64(lit)); st_slots += 64; }
                            if (all64(shadowed)) break;
                        }
                    }
                    // triangles, kernel.cu:1475-1497 (the reference tests them first; an
                    // any-hit does not depend on the order)
                    if (Cfg::MESH && !all64(shadowed) && !RT_ABL(8192)) {
                        const V3 inv{1.f / new_dir.x, 1.f / new_dir.y, 1.f / new_dir.z};
                        for (int bjj = 0; bjj < sbcount; ++bjj) {
                            const int bj = sb_use_list ? myboxes[bjj] : bjj;
                            const RtBoxDev bx = ax->boxes[bj];
                            const bool bh = !shadowed && box_intersect(bx, start, inv);
                            if (Cfg::STATS == 1) sm_sslab += 1;
                            if (any64(bh) && !RT_ABL(16384)) {
                                // (a per-triangle cull against the light's beam, as for the primary rays, was measured:
                                // -1.7 % at 4K, +2.8 % at 1080p, one more spilled register -- not kept)
                                for (int base = 0; base < bx.len; base += 7) {
                                    const int cnt = bx.len - base < 7 ? bx.len - base : 7;
                                    mytri[lane] = ax->tri9[(size_t)(bx.start + base) * 9 + lane];
                                    wave_lds_sync();
                                    for (int i = 0; i < cnt; ++i) {
                                        const float *tv = mytri + 9 * i;
                                        float t, u, v;
                                        if (Cfg::STATS == 1) sm_stri += 1;
                                        if (bh && !shadowed && tri_intersect(start, new_dir, tv, tv + 3, tv + 6, t, u, v))
                                            shadowed = true;
                                    }
                                    wave_lds_sync();
                                }
                                if (all64(shadowed)) break;
                            }
                        }
                    }
                    // planes (kernel.cu:1511-1523) then cubes (:1524-1536), any-hit
                    if (Cfg::PRIMS && (fc.n_planes | fc.n_cubes) != 0 && !all64(shadowed)) {
                        for (int i = 0; i < fc.n_planes; ++i) {
                            float t;
                            if (!shadowed && plane_intersect(ax->planes[i], start, new_dir, t)) shadowed = true;
                            if (all64(shadowed)) break;
                        }
                        if (fc.n_cubes > 0 && !all64(shadowed)) {
                            const V3 inv{1.f / new_dir.x, 1.f / new_dir.y, 1.f / new_dir.z};
                            for (int i = 0; i < fc.n_cubes; ++i) {
                                float t;
                                if (!shadowed && cube_intersect(ax->cubes[i], start, inv, t)) shadowed = true;
                                if (all64(shadowed)) break;
                            }
                        }
                    }
                    if (!shadowed) us += 1u << 16;   // b += 0.1, kernel.cu:1537-1539
                    phase(7);
                }
                if (Cfg::CULL) wave_lds_sync();
                if (Cfg::VD_REC && vd_has && !all_clear && !dark) record_counts<Cfg>(myvd, g, li, lane, us);
                if (Cfg::STATS == 1 && Cfg::MESH && !all_clear) sm_slisted += (unsigned long long)sbcount;
                if (Cfg::STATS == 1 && !all_clear) {   // how many of the walked lights had a lane in a penumbra at all
                    const int unshadowed = (int)(us >> 16);
                    const bool pen = lit && unshadowed != 0 && unshadowed != RT_SHADOW_SAMPLES;
                    st_walks += 1;
                    st_walks_no_penumbra += any64(pen) ? 0 : 1;
                    st_walks_all_dark += any64(lit && unshadowed != 0) ? 0 : 1;
                    st_walks_all_lit += any64(lit && unshadowed != RT_SHADOW_SAMPLES) ? 0 : 1;
                    st_pen_lanes += (unsigned long long)__popcll(ballot64(pen));
                    st_walk_lanes += (unsigned long long)__popcll(ballot64(lit));
                }

                if (lit && !dark) {   // unlit lanes would add (0 * l.r) * r = +0, and so does a light that is dark for all of them
                    // b after `unshadowed` float+=double steps, then b *= max(normal.toL, 0)
                    int unshadowed = (int)(us >> 16);
                    // A light on record: the lane's count. The address is formed here, from the kernel-argument segment and
                    // the tile index parked in LDS, so that nothing of it lives across the loop; and the load is issued
                    // here, where the fewest registers are live -- asked for ahead of begin and settle, so that the chain
                    // covers its latency, it costs the kernel four spilled vector registers and its scratch-free frame.
                    if (sc_use) {
                        FcPtr kg = kargs_again();
                        const unsigned tiles = rt_rest_tiles(kg->width, kg->local_rows, Cfg::TW);
                        const unsigned tile = (unsigned)__builtin_amdgcn_readfirstlane((int)myvd[3]);
                        const unsigned char *rec = kg->rest_rd + RT_REST_COUNTS_OFFSET(tiles) + ((size_t)tile * RT_SHADOW_RECORDS + (size_t)(vd - 4u)) * RT_REST_RECORD_BYTES;
                        // (a scalar base and a lane index formed on the spot, both opaque, and a global load said to be one:
                        // as plain expressions the compiler keeps parts of the address in vector registers -- four spills)
                        asm volatile("" : "+s"(rec));
                        int sc_lane = (int)(threadIdx.x & 63u);
                        asm volatile("" : "+v"(sc_lane));
                        unshadowed = (int)((const __attribute__((address_space(1))) unsigned char *)rec)[sc_lane];
                    }
                    float bsum = mybtab[unshadowed];
                    const float a = dot3(normal, chain.toL);                    // kernel.cu:1541
                    bsum = bsum * (a > 0.f ? a : 0.f);
                    fr = fr + bsum * L.r * mytex[lane];                         // kernel.cu:1673-1675
                    fg = fg + bsum * L.g * mytex[64 + lane];
                    fb = fb + bsum * L.b * mytex[128 + lane];
                    if (Cfg::STATS == 1) st_unshadowed += (unsigned long long)unshadowed;
                }
            }
            }   // groups
            if (Cfg::VD_REC && lane == 0) tile_summary(fc, myvd, n_groups);
        }
        } while (false);
        if (valid) {
            acc_r = acc_r + fr;
            acc_g = acc_g + fg;
            acc_b = acc_b + fb;
        }
    }

    // (inline: as a function of (myvd, lane, wave, valid, t_start, acc, n_samples) it changed 38 lines of the product kernel's
    // machine code and 40 of the multi-sample kernel's; with it and the five blocks marked likewise above cut out, the multi-sample
    // frame measured 0.7777 ms against the parent's 0.7760, every round above every round of the parent's)
    // ================= write-back =================
    // The frame uniforms of this part -- output pointers, flags, the divisor -- are read from the kernel-argument
    // segment HERE: taken from `fc` they are loaded at the kernel's entry and held in scalar registers across the whole
    // kernel, whose scalar file is full (each one more is a v_writelane / v_readlane pair in the loops above).
    FcPtr kargs = kargs_again();
    float *const o_rgba = kargs->rgba;
    uint32_t *const o_packed = kargs->packed, *const o_packed24 = kargs->packed24;
    unsigned *const o_cost = kargs->tile_cost;
    const int o_flags = kargs->flags;
    const float o_total = kargs->sample_total;
    // The tile's place in the frame, formed AGAIN here (same expressions as at the kernel's entry, behind opaque copies of
    // their inputs so that the compiler does not simply keep the first results): pixel column, local row and tile
    // coordinates are then dead between the primary ray and this point instead of occupying vector registers -- or a
    // scratch slot -- across the light loop, whose register peak is what the seven-waves-per-SIMD budget is cut to.
    unsigned wb_x = blockIdx.x, wb_y = blockIdx.y;
    const unsigned wb_tiles_x = (unsigned)(kargs->width + Cfg::TW - 1) / (unsigned)Cfg::TW;
    const uint32_t *perm = kargs->tile_perm;
    if (perm) {
        const unsigned p = perm[blockIdx.y * wb_tiles_x + blockIdx.x];
        wb_x = p & 0xffffu;
        wb_y = p >> 16;
    }
    int wb_lane = (int)(threadIdx.x & 63u);
    asm volatile("" : "+v"(wb_lane));
    const int wb_px = (int)(wb_x * Cfg::TW) + (wb_lane % Cfg::TW);
    const int wb_ly = (int)((wb_y + wave) * Cfg::TH) + (wb_lane / Cfg::TW);
    const unsigned out_idx = (unsigned)wb_ly * (unsigned)kargs->width + (unsigned)wb_px;   // band-local pixel index
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
        if (o_packed && (o_flags & RT_FLAG_RESOLVE)) {
            o_packed[o] = resolve_pixel(acc_r, acc_g, acc_b, o_total);
        }
    }
    if (o_packed24 && (o_flags & RT_FLAG_RESOLVE)) {   // wave-uniform; all lanes take part in the quad exchange
        const unsigned p = resolve_pixel(acc_r, acc_g, acc_b, o_total);
        // the next pixel of the quad (lanes 4q..4q+3 hold four consecutive pixels of a row)
        const unsigned pn = (unsigned)__builtin_amdgcn_update_dpp(0, (int)p, 0xF9 /* quad_perm [1,2,3,3] */, 0xf, 0xf, true);
        const int i = lane & 3;
        // bytes B,G,R of pixel k at 3k..3k+2: dword i of the quad's three
        const unsigned w24 = (p >> (8 * i)) | (pn << (24 - 8 * i));
        if (valid && i < 3) o_packed24[(size_t)(out_idx >> 2) * 3 + (size_t)i] = w24;
    }

    if (Cfg::VD_REC) {   // the tile's light verdicts as this launch found them (an all-sky tile: 0)
        unsigned *const o_rest = reinterpret_cast<unsigned *>(kargs->rest_wr);
        wave_lds_sync();
        if (wb_lane < 2) o_rest[RT_REST_WORD_DWORD(wb_y * wb_tiles_x + wb_x) + wb_lane] = myvd[wb_lane];
        if (wb_lane == 2) o_rest[RT_REST_TAG_DWORD(rt_rest_tiles(kargs->width, kargs->local_rows, Cfg::TW), wb_y * wb_tiles_x + wb_x)] = myvd[2];   // the tags of its records
        if (wb_lane == 3) o_rest[RT_REST_SUMMARY_DWORD(rt_rest_tiles(kargs->width, kargs->local_rows, Cfg::TW), wb_y * wb_tiles_x + wb_x)] = myvd[4];   // its summary
    }
    if (o_cost) {   // this tile's wave duration, for the order of later frames (a plain store: an atomic maximum
        // per block of tiles here, 256 waves ending together on one address, slowed the whole launch down by 3 %)
        const unsigned dt = (unsigned)__builtin_amdgcn_s_memtime() - t_start;
        if (wb_lane == 0) o_cost[wb_y * wb_tiles_x + wb_x] = dt;
    }

    phase(3, true);
    if (Cfg::STATS == 2 && fc.stats) {
        if (lane == 0) {
            unsigned long long tot = 0;
            for (int k = 0; k < 8; ++k) {
                atomicAdd(&fc.stats[8 + k], ph[k]);
                tot += ph[k];
            }
            // wave durations (constant 100 MHz clock), octaves: [<5, <10, <20, <40, <80, <160, >=160] us
            const unsigned long long span = __builtin_amdgcn_s_memrealtime() - rt_begin;
            int bin = 0;
            while (bin < 6 && span >= (500ull << bin)) ++bin;
            atomicAdd(&fc.stats[17 + bin], 1ull);
            (void)tot;
        }
    }
    if (Cfg::STATS == 1 && fc.stats) {
        // per-lane counters were kept wave-uniform except hits/unshadowed
        const unsigned long long h = (unsigned long long)wave_sum((float)st_hits);
        const unsigned long long u = (unsigned long long)wave_sum((float)st_unshadowed);
        if (lane == 0) {
            atomicAdd(&fc.stats[0], st_primary);
            atomicAdd(&fc.stats[1], st_shadow);
            atomicAdd(&fc.stats[2], st_cull);
            atomicAdd(&fc.stats[3], h);
            atomicAdd(&fc.stats[4], u);
            atomicAdd(&fc.stats[5], st_slots);
            atomicAdd(&fc.stats[6], st_entries);
            atomicAdd(&fc.stats[7], st_overflow);
            for (int k = 0; k < 8; ++k) atomicAdd(&fc.stats[8 + k], hist[k]);
            atomicAdd(&fc.stats[17], st_walks);               // (slots 17.. hold the wave-duration histogram in RT_MODE_PHASES)
            if (Cfg::MESH) {   // mesh launches: the mesh's work instead of the penumbra counters (tools/mesh_stats.py)
                atomicAdd(&fc.stats[18], sm_plisted);
                atomicAdd(&fc.stats[19], sm_pleaf);
                atomicAdd(&fc.stats[20], sm_ptri);
                atomicAdd(&fc.stats[21], sm_slisted);
                atomicAdd(&fc.stats[22], sm_sslab);
                atomicAdd(&fc.stats[23], sm_stri);
            } else {
                atomicAdd(&fc.stats[18], st_walks_no_penumbra);
                atomicAdd(&fc.stats[19], st_pen_lanes);
                atomicAdd(&fc.stats[20], st_walk_lanes);
                atomicAdd(&fc.stats[21], st_walks_all_dark);
                atomicAdd(&fc.stats[22], st_walks_all_lit);
                atomicAdd(&fc.stats[23], st_pre);
            }
            atomicAdd(&fc.stats[16], st_clusters);
        }
    }
}


typedef void (*RtTraceFn)(const RtFrameConsts, const float4 *);

// Which (mode, feat) exist for a tile / cull / MULTI combination. The default tile has them all; the other tile
// widths are test dimensions of the exact kernels (the product and force-slow modes on sphere scenes, the product mode with cubes / planes / a
// mesh, the work counters on sphere scenes only): what no test, tool or bench launches is not compiled (build time
// and code-object size, profiles/r03_build_and_first_launch.json). A missing combination makes the launch fail with
// hipErrorNotSupported.
template <int TW, bool CULL, bool MULTI, int MODE, int FEAT>
static constexpr bool trace_exists()
{
#ifdef RT_QUICK   // kernel experiments (tools/variants.sh): the product instantiation and its brute-force twin only
    if (TW != 8 || FEAT != RT_FEAT_SPHERES || (MODE != RT_MODE_PRODUCT && MODE != RT_MODE_STATS && MODE != RT_MODE_REST_READ && MODE != RT_MODE_REST_COMPACT && MODE != RT_MODE_REST_WRITE) || (MULTI && MODE != RT_MODE_PRODUCT)) return false;
#endif
    if (MODE == RT_MODE_REST_READ || MODE == RT_MODE_REST_COMPACT || MODE == RT_MODE_REST_WRITE) return CULL && FEAT == RT_FEAT_SPHERES && MULTI == (TW != 8);   // light verdicts: the one-sample kernel (other tiles: the sample loop, one pass)
    if (MODE == RT_MODE_FAST) return TW == 8 && CULL && FEAT != RT_FEAT_MESH;   // fast mode: the product configuration only
    if (MODE == RT_MODE_AOV) return TW == 8 && !MULTI;   // G-buffer: the one-sample kernels of the default tile
    if (TW != 8 && FEAT != RT_FEAT_SPHERES && MODE != RT_MODE_PRODUCT) return false;
#ifndef RT_TUNING
    if (MODE == RT_MODE_PHASES) return false;
#endif
    return true;
}

template <int TW, bool CULL, bool MULTI, int MODE, int FEAT>
static RtTraceFn trace_fn_one()
{
    if constexpr (trace_exists<TW, CULL, MULTI, MODE, FEAT>()) return rt_trace_tiles<TW, CULL, MODE, FEAT, MULTI>;
    else return nullptr;
}

template <int TW, bool CULL, bool MULTI, int MODE>
static RtTraceFn trace_fn_feat(int feat)
{
    switch (feat) {
    case RT_FEAT_SPHERES: return trace_fn_one<TW, CULL, MULTI, MODE, RT_FEAT_SPHERES>();
    case RT_FEAT_PRIMS: return trace_fn_one<TW, CULL, MULTI, MODE, RT_FEAT_PRIMS>();
    case RT_FEAT_MESH: return trace_fn_one<TW, CULL, MULTI, MODE, RT_FEAT_MESH>();
    default: return nullptr;
    }
}

template <int TW, bool CULL, bool MULTI>
static RtTraceFn trace_fn_mode_feat(int mode, int feat)
{
    switch (mode) {
    case RT_MODE_PRODUCT: return trace_fn_feat<TW, CULL, MULTI, RT_MODE_PRODUCT>(feat);
    case RT_MODE_STATS: return trace_fn_feat<TW, CULL, MULTI, RT_MODE_STATS>(feat);
    case RT_MODE_FORCE_SLOW: return trace_fn_feat<TW, CULL, MULTI, RT_MODE_FORCE_SLOW>(feat);
    case RT_MODE_PHASES: return trace_fn_feat<TW, CULL, MULTI, RT_MODE_PHASES>(feat);
    case RT_MODE_FAST: return trace_fn_feat<TW, CULL, MULTI, RT_MODE_FAST>(feat);
    case RT_MODE_AOV: return trace_fn_feat<TW, CULL, MULTI, RT_MODE_AOV>(feat);
    case RT_MODE_REST_READ: return feat == RT_FEAT_SPHERES ? trace_fn_one<TW, CULL, MULTI, RT_MODE_REST_READ, RT_FEAT_SPHERES>() : nullptr;
    case RT_MODE_REST_COMPACT: return feat == RT_FEAT_SPHERES ? trace_fn_one<TW, CULL, MULTI, RT_MODE_REST_COMPACT, RT_FEAT_SPHERES>() : nullptr;
    case RT_MODE_REST_WRITE: return feat == RT_FEAT_SPHERES ? trace_fn_one<TW, CULL, MULTI, RT_MODE_REST_WRITE, RT_FEAT_SPHERES>() : nullptr;
    default: return nullptr;
    }
}

}  // namespace

// the parts of the instantiation table (one translation unit each)
RtTraceFn rt_trace_fn_cull8(int mode, int feat, int multi);                 // rt_kernels.hip
RtTraceFn rt_trace_fn_brute8(int mode, int feat, int multi);                // rt_kernels_brute.hip
RtTraceFn rt_trace_fn_tiles(int tile_w, int cull, int mode, int feat);      // rt_kernels_tiles.hip
