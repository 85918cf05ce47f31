// rt_scene.h -- struct rt_scene and what its own translation units share (rt_scene.cpp, rt_scene_tables.cpp,
// rt_scene_rest.cpp, rt_render.cpp, rt_post.cpp, rt_shim.cpp, rt_debug.cpp). Everything else goes through the functions of
// rt_internal.h.
//
// Frames in flight and the buffers they read. A frame is asynchronous work on the caller's stream; the scene's device
// buffers may be read by frames on several streams at once (two frames in flight, a replaying graph). Whoever is about
// to overwrite or free such a buffer first waits for the frames launched so far -- not for the whole device:
//   * every launch records an event into a ring of RT_RING slots; before a slot is re-used the launching stream waits
//     on the event it held, so "the ring's events are done" implies "every earlier frame is done";
//   * rare mutations (sphere list, lights, textures, resolution) wait on the host for the ring (rt_scene_quiesce) and
//     then change the buffers in place;
//   * the per-frame mutations, the eye-cone table and the view lists of a moving camera, never wait on the host: each
//     rotates through a few RtTableSlot buffers and is handed over by the four functions below.
//
// The hand-over of a cached table (rt_scene_begin_build / end_build / order_reader / note_launch). The contract:
//   (a) builds run on the scene's table stream, never on the frame's -- beside frame k's kernel, not in front of frame
//       k+1's. The exception is the host build of an eye-cone table beyond RT_EYE_DEVICE_MAX, which quiesces, uploads
//       blocking on the caller's stream and leaves nothing pending;
//   (b) a view-list build follows the cone build it reads because both are on the table stream, or because the host
//       build has finished;
//   (c) a reader waits on the build event on the device only; the host never waits for a build, except in
//       rt_scene_view_lists_info;
//   (d) rt_scene_quiesce waits for the ring, then the table stream, then every post pass's event (rt_scene::post_event);
//   (e) the tile order keeps one event for all layouts; a new layout or a re-sort first makes the launching stream
//       wait for every ring event;
//   (f) every post pass's event is recorded also after a launch that failed half-way, and a pass host-waits for it
//       before it grows or rewrites the scratch the event guards (rt_post.cpp, PostCall);
//   (g) whatever rewrites or re-allocates a buffer a recorded graph may point into bumps `epoch`, and nothing else
//       does: of the hand-over functions only an rt_scene_begin_build whose buffer re-allocates;
//   (h) a resting-view table is written by a frame launch on the frame's own stream, not by a build on the table
//       stream: that stream is ordered behind the slot's last reader (through the frame ring) and its last writer, the
//       slot's `built` is the writing launch's event, and readers on other streams wait for it on the device. Its
//       buffer is in no graph, so growing it (after a quiesce) bumps no epoch.
#pragma once
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "rt_internal.h"
#include "rt_tables.h"

#define RT_RING 4
#define RT_CONE_SLOTS 3
#define RT_VIEW_SLOTS 4
#define RT_REST_SLOTS 4

// One cached device table of a few: built on the table stream after the slot's last reader (through the frame ring),
// read after `built` (on the device).
struct RtTableSlot {
    DevArray<float4> buf;
    bool valid = false;
    bool used = false;                    // read by some launch since it was built
    unsigned long long last_use = 0;      // ring sequence number of the last launch that read it
    HipPendingEvent built;                // the build on the scene's table stream
};
struct ConeSlot : RtTableSlot {
    float org[3] = {0, 0, 0};
    unsigned long long gen = ~0ull;       // sphere_gen the table was built from
};
// View lists (RtFrameConsts::view_lists, rt_tables.hip): one table per recent view, built after the eye-cone table it reads.
struct ViewSlot : RtTableSlot {
    unsigned key[18] = {};                // compared by bits: sphere_gen, origin, rotation, eye_nz, aspect, frame size, sample total, block shape
    int nbx = 0, nby = 0, bw = 0, bh = 0;
};

// Resting-view tables (RtFrameConsts::rest_rd): one per recent (view, layout), written by a
// frame launch itself -- `built` is that launch's event on ITS stream -- and read by later launches of the same key.
struct RtRestKey {
    RtFrameConsts fc;                     // every field the kernel reads; outputs, tile order and the table pointers zeroed
    unsigned long long epoch = 0;         // generation of every table behind fc's pointers that quiesce-and-rewrite mutations touch
    unsigned long long sphere_gen = 0;    // ... and of the sphere list (tables built from it: cones, view lists, light tables)
    int tile = 0, cull = 0, mode = 0, feat = 0;
};
// The run list of a compact reading launch (the table's list section) is built by rt_rest_list_launch on the stream of the
// reading launch that finds it stale -- never built, or built from another order than the launch's (list_perm,
// list_order_serial) or with another R, or from sections a setter has rewritten since -- behind every frame launched so
// far, as a tile-order sort is; `list_done` is that build, and compact launches on other streams wait for it on the
// device. The host needs the list's two counts for the grid. They depend on the summaries and records alone -- another
// order re-orders the list and leaves them as they are --, so they are fetched once per content of those sections:
// the build copies the header into `list_counts` (pinned), and the first launch that finds list_done complete adopts
// them; no launch waits for that on the host, and until then reading launches keep the full grid and do not look at the list.
struct RestSlot : RtTableSlot {          // buf: RT_REST_TABLE_BYTES(tiles), the layout of rt_device.h
    RtRestKey key;
    int tiles_x = 0, tiles_y = 0;
    bool list_built = false;              // a build from the table's present sections is enqueued or done
    bool list_adopted = false;            // the counts of the table's present sections are in list_n
    const unsigned *list_perm = nullptr;  // the order the list was built from (null: grid order)
    unsigned long long list_order_serial = 0;   // TileOrder::serial of that order at that build
    unsigned list_run = 0;                // R of that build
    unsigned list_ahead = 0;              // ... and where it put the runs (RtRestListParams::ahead)
    unsigned list_n[2] = {0, 0};          // n_unsettled, n_streamed
    PinnedArray<unsigned> list_counts;    // RT_REST_LIST_HEADER dwords, copied behind every build
    DevArray<unsigned> list_scratch;      // the builder's (rt_rest_list_scratch)
    HipPendingEvent list_done;            // the last build and its copy
};
// What the last launch's geometry was (rt_debug_compact_launch).
struct RtCompactLast {
    int compact = 0, ahead = 0;
    unsigned n_unsettled = 0, n_streamed = 0, run = 0, workgroups = 0;
};

// The slot a new table replaces: a free one (is_free: it holds nothing a frame could ask for) before an occupied one;
// among occupied ones a never-read one before a read one; then the least recently read.
template <typename Slot, size_t N, typename IsFree>
Slot &rt_slot_victim(Slot (&slots)[N], IsFree is_free)
{
    Slot *v = &slots[0];
    for (Slot &c : slots) {
        const bool c_free = is_free(c), v_free = is_free(*v);
        if ((c_free && !v_free) || (c_free == v_free && (!c.used || (v->used && c.last_use < v->last_use)))) v = &c;
    }
    return *v;
}

struct RtReflectDeleter {
    void operator()(RtReflect *r) const { rt_reflect_destroy(r); }
};

#define RT_COMPACT_RUN 64           // settled tiles per workgroup of a compact reading launch, and (RT_COMPACT_AHEAD) those
#define RT_COMPACT_MIN_PERCENT 25   // ... and only where at least this share of the tiles is streamed (C3: 68 %, 18 % faster; C5: 8 %, 3.5 % slower)
#define RT_COMPACT_AHEAD 1          // workgroups ahead of the one-wave tiles': both by measurement, DESIGN.md 4, step 5e
#define RT_ORDER_SLOTS 4
#define RT_ORDER_EVERY 32            // an unchanged view: the order is sorted again from fresh durations every so many launches
#ifndef RT_ORDER_MOVING
#define RT_ORDER_MOVING 3            // a view that keeps changing: every so many
#endif
struct TileOrder {
    int key[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // tile width, frame width / height, y0, y1, local rows, interleave
                                                  // count / index / rows, and which kernel: cull, mode, samples
    RtTileOrderBuf buf;                          // empty: the slot has had no layout yet
    RtTileGrid grid = {};
    float view[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // camera and sphere list the last launch saw
    int same_view = 0;                           // consecutive launches of that view so far
    int since_sort = 0;                          // launches (all of which recorded durations) since the order was sorted / reset
    bool have_perm = false;
    unsigned long long last_use = 0;
    unsigned long long serial = 0;               // of its last sort or reset: a run list built from an earlier one is stale
};

// One kind's emission table: what the host last set, and a device copy that changes only in an indirect call, behind
// the calls that may still read it (the protocol of rt_reflect.hip's RfTable, with the indirect pass's event for the
// frame ring).
// The passes are pointed by what the device holds (v_dev), never by v.
struct RtEmitTable {
    std::vector<float4> v;               // (r, g, b, 0) per primitive; empty = no table
    std::vector<float4> v_dev;           // what the device copy holds
    bool dirty = false;                  // v changed since the last upload
    DevArray<float4> d;
    const float4 *dev() const { return v_dev.empty() ? nullptr : d.get(); }
};

// The post passes (rt_post.cpp). Every owner of scratch has one event, which orders the scene's calls of that pass on
// the device, whatever their streams, and which rt_scene_quiesce waits for; every timed entry has a timer of its own.
// The two denoisers share their scratch, so their event. A new pass: one value in each enum, one line in the map.
enum RtPostOwner { RT_OWNER_ATROUS, RT_OWNER_TEMPORAL, RT_OWNER_UPSAMPLE, RT_OWNER_DISPLAY, RT_OWNER_BLOOM, RT_OWNER_INDIRECT, RT_POST_OWNERS };
enum RtPostEntry { RT_POST_DENOISE, RT_POST_VDENOISE, RT_POST_TEMPORAL, RT_POST_UPSAMPLE, RT_POST_DISPLAY, RT_POST_BLOOM, RT_POST_INDIRECT, RT_POST_ENTRIES };
constexpr RtPostOwner kPostOwner[RT_POST_ENTRIES] = {RT_OWNER_ATROUS, RT_OWNER_ATROUS, RT_OWNER_TEMPORAL, RT_OWNER_UPSAMPLE,
                                                     RT_OWNER_DISPLAY, RT_OWNER_BLOOM, RT_OWNER_INDIRECT};
// One cap for every entry's events (a HipEvent is made on first use: a spare slot costs nothing). The denoisers: one
// event per iteration, and before the first launch, after the pack, after the variance's spatial estimate.
#define RT_POST_MAX_EVENTS RT_INDIRECT_MAX_EVENTS
static_assert(RT_DENOISE_MAX_ITERATIONS + 3 <= RT_POST_MAX_EVENTS, "the denoisers' events");
static_assert(2 <= RT_POST_MAX_EVENTS, "the temporal pass's and the upsampler's events");
static_assert(RT_DISPLAY_MAX_EVENTS <= RT_POST_MAX_EVENTS, "the display transform's events");
static_assert(RT_BLOOM_MAX_EVENTS + 1 <= RT_POST_MAX_EVENTS, "the bloom pass's events");
struct RtPostTimer {
    HipEvent ev[RT_POST_MAX_EVENTS];
    bool on = false;                     // rt_scene_set_*_timing
    int timed = 0;                       // events the entry's last timed call recorded
};

// A pass's own ray tables at one sample, dx[w] then dy[h]: its own, so that a call at another size than the frames'
// (half resolution) does not rebuild their d_raygen.
struct RtRayTables {
    DevArray<float> tab;
    int w = 0, h = 0;
    float aspect = 0.f;                  // compared by bits
    // The tables of this size and aspect; if they are others, new ones after the host has seen `done`, the pass's last call, end
    int prepare(HipPendingEvent &done, int width, int height, float aspect_);
    const float *dx() const { return tab.get(); }
    const float *dy() const { return tab.get() + w; }
};

struct rt_scene {
    DevArray<float4> d_spheres;      // [n] list order | [n_pad] Morton order | [n_blocks] block bounds | [n_pad] ints
    int n_spheres = 0;
    int n_blocks = 0;
    std::vector<float4> h_prev;      // what was uploaded last (skip identical re-mirrors)
    PinnedArray<float4> h_stage;     // staging for asynchronous re-uploads
    HipPendingEvent stage_done;      // the last upload out of h_stage
    DevArray<float> d_tex[3];
    int tex_w = 0, tex_h = 0;
    DevArray<float> d_sky[3];
    int sky_w = 0, sky_h = 0;
    float sky_c[3] = {0, 0, 0};
    float sky_radius = 0;        // the sphere's `radius` field (already r*r)
    bool have_sky = false;
    rt_light lights[RT_MAX_LIGHTS];
    int n_lights = 0;
    DevArray<RtPlaneDev> d_planes;
    DevArray<RtCubeDev> d_cubes;
    int n_planes = 0, n_cubes = 0;
    DevArray<RtTriDev> d_tris;
    DevArray<RtBoxDev> d_boxes;
    DevArray<int> d_tri_idx;
    DevArray<float> d_box_spheres, d_tri9, d_tri_bs, d_tri_nrm;
    int n_boxes = 0, n_tris = 0, mesh_has_normals = 0;
    // per-light column blocks (see RtFrameAux::lsorted): one allocation, rebuilt when the
    // sphere list or a light's position changes
    DevArray<float4> d_light_tabs;
    // per-light occluder lists (rt_build_occluder_lists): [n_lights][n] headers, then the lights' entry arrays
    DevArray<char> d_cand;
    size_t cand_ent_off[RT_MAX_LIGHTS] = {};   // byte offset of light i's entries in d_cand (headers: i * n * 16)
    bool cand_valid[RT_MAX_LIGHTS] = {};
    float cand_pos[RT_MAX_LIGHTS][3];    // light position each list set was built for
    unsigned long long cand_gen = ~0ull;
    int cand_n_lights = 0;
    unsigned long long sphere_gen = 0;   // bumped whenever the mirrored sphere list changes
    unsigned long long ltab_gen = ~0ull; // sphere_gen the light tables were built from
    int ltab_n_lights = 0;
    float ltab_axis[RT_MAX_LIGHTS][3];   // axis each table was built for
    bool ltab_valid[RT_MAX_LIGHTS] = {};
    // eye cones for the primary rays (see RtFrameConsts::csorted), one table per recent ray origin
    ConeSlot cones[RT_CONE_SLOTS];
    // dx / dy of the primary rays per column / row and sample (RtFrameConsts::dx_tab)
    DevArray<float> d_raygen;
    int rg_w = 0, rg_h = 0, rg_total = 0;
    float rg_aspect = 0.f;
    // RtFrameAux as uploaded last
    RtFrameAux h_aux;
    DevArray<RtFrameAux> d_aux;
    bool aux_valid = false;
    // where the slots' builds run: beside the frames, not in front of them
    HipStream table_stream;
    // frames in flight
    HipEvent ring[RT_RING];
    bool ring_used[RT_RING] = {};
    unsigned long long ring_seq = 0;     // sequence number of the next launch
    // bumped whenever a buffer a recorded graph may point into is rewritten or re-allocated
    unsigned long long epoch = 0;
    // order of the tiles within a launch (RtFrameConsts::tile_perm / tile_cost, rt_tables.hip): per launch
    // layout (which rows of which frame, tile shape) the tiles' wave durations as the frame kernel records
    // them and, rebuilt from those every RT_ORDER_EVERY launches, the order that starts the longest first
    TileOrder orders[RT_ORDER_SLOTS];
    unsigned long long order_clock = 0;      // for least-recently-used replacement
    int tile_order_mode = 1;                 // rt_scene_set_tile_order
    HipPendingEvent order_built;             // the last rebuild; launches on other streams wait for it on the device
    unsigned long long order_serial = 0;     // counts the sorts and resets of all orders; TileOrder::serial takes its values
    unsigned long long order_cur_serial = 0; // the serial of the order the launch being prepared starts its tiles in
    // per-view candidate lists of the primary rays
    ViewSlot views[RT_VIEW_SLOTS];
    int view_lists_mode = 1;                 // rt_scene_set_view_lists
    int view_last = -1;                      // the slot the last launch read, -1: it read none
    // the tables of a resting view: light verdicts, shadow counts, primary records
    RestSlot rest[RT_REST_SLOTS];
    int light_verdicts_mode = 1;             // rt_scene_set_light_verdicts
    RtRestKey rest_seen[RT_REST_SLOTS];      // keys of recent launches that found no table and wrote none, a ring:
    bool rest_seen_valid[RT_REST_SLOTS] = {};   // a key leaves it when its table is written or the ring comes round
    int rest_seen_next = 0;                  // the entry the next such key replaces
    int rest_last = -1;                      // the slot the last launch wrote or read, -1: neither
    int rest_last_wrote = 0;                 // 1: it wrote it
    int compact_mode = 1;                    // rt_scene_set_compact_launch
    unsigned compact_run = RT_COMPACT_RUN;   // R of the lists built from now on (rt_debug_set_compact_run)
    unsigned compact_min_percent = RT_COMPACT_MIN_PERCENT;   // ... and the share of streamed tiles below which a launch keeps the full grid
    unsigned compact_ahead = RT_COMPACT_AHEAD;   // ... and the runs' place: 0 behind the one-wave tiles, 1 ahead of them
    unsigned long long list_rebuilds = 0;    // run lists built so far, all slots
    RtCompactLast compact_last;              // the last frame launch's geometry
    // mirror reflections (rt_reflect.hip): materials, sphere BVH, queues; created on first use
    std::unique_ptr<RtReflect, RtReflectDeleter> refl;
    // the post passes: what orders each one's calls, and each timed entry's timing state (guided upsampling,
    // rt_upsample.hip, has no more than these); below, each pass's scratch
    HipPendingEvent post_event[RT_POST_OWNERS];
    RtPostTimer post_timer[RT_POST_ENTRIES];
    // the two denoisers' scratch (rt_denoise.hip): two irradiance buffers and the packed guides, grown on demand
    DevArray<float4> dn_col[2], dn_guide;
    DevArray<int> dn_key;
    // the variance-guided denoiser uses the scratch above, plus two variance arrays
    DevArray<float> vd_var[2];
    // temporal accumulation (rt_temporal.hip): the ray tables of the view its last call reprojected from
    RtRayTables tp_rays;
    // the display transform (rt_display.hip): the histogram's RT_DISPLAY_BINS counters and, behind them, the 256
    // thresholds of the sRGB encoding, uploaded when the buffer is made
    DevArray<uint32_t> dp_scratch;
    // the bloom pass (rt_bloom.hip): the pyramid's levels one behind the other, grown on demand and never shrunk
    DevArray<float4> bl_pyramid;
    // the indirect pass (rt_indirect.hip): ray tables of its own, as the temporal pass has, and the product's scratch,
    // grown on demand
    RtRayTables ind_rays;
    DevArray<float4> ind_slab, ind_queue, ind_sum;
    DevArray<int> ind_count;
    DevArray<float4> ind_queue2;                     // bounces > 1: the second of the two queues
    int ind_counts = 0, ind_bounces = 1;             // the last call's counters (groups * bounces; plain: 0) and bounces
    // emission per primitive of a kind (rt_scene_set_emission; [kind - RT_HIT_SPHERE]): host state, which
    // the next indirect call uploads on its stream behind the pass's event -- the indirect calls are the tables' only readers
    RtEmitTable emit[3];
#ifdef RT_TUNING
    int tune_no_eye_cones = 0, tune_no_light_columns = 0, tune_ablate = 0;
#endif
};

// rt_scene.cpp
int rt_scene_wait_all_frames(rt_scene *s, hipStream_t stream);   // `stream` waits for every frame launched so far (no host wait)
// Begin a build into slot c of `total` float4: quiesces before the buffer is freed (it grows; epoch++) or written from
// the host (on_host); otherwise orders the table stream after the slot's last reader and an upload in flight, and the
// caller launches the build there. End it: records the build. A reader's stream: ordered behind the build.
int rt_scene_begin_build(rt_scene *s, RtTableSlot &c, size_t total, bool on_host);
int rt_scene_end_build(rt_scene *s, RtTableSlot &c, bool on_host);
inline hipError_t rt_scene_order_reader(RtTableSlot &c, hipStream_t stream) { return c.built.order(stream); }
RtReflect *rt_scene_reflect(rt_scene *s);   // created on first use
void rt_pack_spheres(const rt_sphere *src, int n, float4 *dst);
// rt_scene_tables.cpp: each finds or builds what the frame reads; the slot index comes back (-1: the frame reads none)
int rt_scene_prepare_eye(rt_scene *s, const float org[3], hipStream_t stream, int *slot_out);
int rt_scene_prepare_view(rt_scene *s, const rt_frame_desc *fd, const RtKernelChoice &kc, int cone_slot, RtFrameConsts *fc,
                          hipStream_t stream, int *view_out);
int rt_scene_prepare_tile_order(rt_scene *s, const RtKernelChoice &kc, RtFrameConsts *fc, hipStream_t stream);
// rt_scene_rest.cpp: the resting-view table of a launch whose uniforms are otherwise complete. `eligible`: it runs the one-sample sphere-only
// product kernel. Points fc at the table it reads or writes (slot index in *slot_out, -1: neither); after the launch
// rt_scene_end_rest records a written table.
// *workgroups_out: the 1-D grid of a compact reading launch (fc then carries RT_FLAG_COMPACT and the run list in tile_perm), 0: the full grid.
int rt_scene_prepare_rest(rt_scene *s, const RtKernelChoice &kc, RtFrameConsts *fc, bool eligible, hipStream_t stream, int *slot_out, unsigned *workgroups_out);
int rt_scene_end_rest(rt_scene *s, int slot, hipStream_t stream);
int rt_scene_prepare_raygen(rt_scene *s, int width, int height, float aspect, int total);
void rt_raygen_fill(int width, int height, float aspect, int total, float *h);   // the tables' values (host)
void rt_build_frame_aux(const rt_scene *s, RtFrameAux *ax);
int rt_scene_sync_aux(rt_scene *s);
void rt_view_params_from_consts(const RtFrameConsts &fc, float aspect, RtViewParams *p);
void rt_view_lists_summary(const float4 *slots, int blocks, rt_view_lists_info *out);
// rt_render.cpp
void rt_view_rotation(const rt_frame_desc *fd, RtFrameConsts *fc);

// For the entry points of rt_render.cpp and rt_post.cpp. A caller's versioned struct in this build's layout: what its
// struct_size (0: `size0`) does not cover reads as 0. Returns the bytes taken from the caller.
template <typename T>
size_t as_built(const T *in, T *out, size_t size0 = sizeof(T))
{
    memset(out, 0, sizeof *out);
    const size_t sz = std::min<size_t>(in->struct_size ? in->struct_size : size0, sizeof *out);
    memcpy(out, in, sz);
    out->struct_size = (uint32_t)sizeof *out;
    return sz;
}
inline bool stream_capturing(hipStream_t stream)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (stream) (void)hipStreamIsCapturing(stream, &cs);
    return cs != hipStreamCaptureStatusNone;
}

// margin of the fast texel-index path for a texture dimension of `size` texels (rt_kernels.hip:
// sure_texel): approximation error RT_UV_DELTA plus the rounding of the two float products
inline float rt_texel_margin(int size, float delta) { return (float)size * (delta + 0x1.0p-22f) * 1.01f; }
