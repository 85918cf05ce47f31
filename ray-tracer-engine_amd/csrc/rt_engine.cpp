// rt_engine.cpp -- host side of the C ABI (include/rt_engine.h): device-resident
// scene, frame-uniform hoisting, kernel launch, the rayTrace launch shim and the
// memManager surface.
//
// Reference interfaces replaced here:
//   memManager / check_cuda      /root/reference/memManager.h:11-18, memManager.cpp:3-22
//   rayTrace<<<...>>> launch     /root/reference/kernel.cu:1615, 1780-1783
//   object / sprite / skybox     /root/reference/kernel.cu:1116-1244, sprite.h:11-47
//
// There is no CPU fallback: every render entry point needs a gfx950 device and
// fails with RT_ERR_NO_DEVICE / RT_ERR_HIP otherwise.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <memory>
#include <utility>
#include <vector>

#include "../../include/rt_engine.h"
#include "rt_device.h"
#include "rt_internal.h"
#include "rt_math.h"
#include "rt_tables.h"

// launchers defined in rt_kernels.hip
extern "C" hipError_t rt_dev_launch_dbg_shortcuts(int what, unsigned seed, long long n, unsigned long long *out, hipStream_t stream);
extern "C" hipError_t rt_dev_launch_dbg_math(int op, const float *a, const float *b, float *out, int n,
                                             hipStream_t stream);
extern "C" hipError_t rt_dev_launch_dbg_intersect(const float4 *tab, const float *rays, int n, int *hit,
                                                  float *t, hipStream_t stream);
extern "C" hipError_t rt_dev_launch_dbg_light(const RtFrameConsts *fc, const float4 *tab, const float *starts,
                                              const float *normals, int light_index, int n, float *dirs,
                                              float *bright, float *adirs, int *aok, hipStream_t stream);

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
static char g_last_error[512] = "";
static int g_soft_errors = 0;

void rt_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_error, sizeof g_last_error, fmt, ap);
    va_end(ap);
}

int rt_hip_fail(hipError_t e, const char *expr, const char *file, int line)
{
    rt_set_error("HIP error = %u (%s) at %s:%d '%s'", (unsigned)e, hipGetErrorString(e), file, line, expr);
    (void)hipGetLastError();   // clear the sticky error so later calls can proceed
    return (e == hipErrorNoDevice || e == hipErrorInvalidDevice) ? RT_ERR_NO_DEVICE : RT_ERR_HIP;
}

extern "C" const char *rt_last_error(void) { return g_last_error; }
extern "C" int rt_abi_version(void) { return RT_ABI_VERSION; }
extern "C" int rt_set_soft_errors(int on)
{
    const int old = g_soft_errors;
    g_soft_errors = on ? 1 : 0;
    return old;
}
extern "C" int rt_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

// check_cuda, memManager.cpp:3-11
extern "C" void rt_check(int err, const char *expr, const char *file, int line)
{
    if (err) {
        fprintf(stderr, "HIP error = %u at %s:%d '%s' \n", (unsigned)err, file, line, expr);
        rt_set_error("HIP error = %u at %s:%d '%s'", (unsigned)err, file, line, expr);
        if (g_soft_errors) return;
        (void)hipDeviceReset();
        exit(99);
    }
}
#define checkHipErrors(val) rt_check((int)(val), #val, __FILE__, __LINE__)

// memManager::operator new / delete, memManager.cpp:12-22
extern "C" void *rt_managed_alloc(size_t len)
{
    void *ptr = nullptr;
    checkHipErrors(hipMallocManaged(&ptr, len ? len : 1));
    checkHipErrors(hipDeviceSynchronize());
    return ptr;
}
static void shim_forget(const void *ptr);
extern "C" void rt_managed_free(void *ptr)
{
    if (!ptr) return;
    shim_forget(ptr);   // a sprite / mesh re-created at the same address must be uploaded again
    checkHipErrors(hipDeviceSynchronize());
    (void)hipFree(ptr);
}

// ---------------------------------------------------------------------------
// device-resident scene
// ---------------------------------------------------------------------------
// Frames in flight and the buffers they read. A frame is asynchronous work on the caller's
// stream; the scene's device buffers may be read by frames on several streams at once (two
// frames in flight, a replaying graph). Whoever is about to overwrite or free such a buffer
// first waits for the frames launched so far -- not for the whole device:
//   * every launch records an event into a ring of RT_RING slots; before a slot is re-used the
//     launching stream waits on the event it held, so "the ring's events are done" implies
//     "every earlier frame is done";
//   * rare mutations (sphere list, lights, textures, resolution) wait on the host for the ring
//     (rt_scene_quiesce) and then change the buffers in place;
//   * the one per-frame mutation, the eye-cone table of a moving camera, never waits on the
//     host: it rotates through RT_CONE_SLOTS device buffers, the build kernel is ordered after
//     the slot's last reader with hipStreamWaitEvent, and runs on the frame's own stream.
#define RT_RING 4
#define RT_CONE_SLOTS 3

struct ConeSlot {
    DevArray<float4> buf;
    float org[3] = {0, 0, 0};
    unsigned long long gen = ~0ull;       // sphere_gen the table was built from
    bool valid = false;
    bool used = false;                    // read by some frame since it was built
    unsigned long long last_use = 0;      // ring sequence number of the last frame that read it
    HipEvent built;                       // the build on the scene's table stream
    bool build_pending = false;           // `built` not yet seen complete: readers wait on it (on the device)
};

// View lists (RtFrameConsts::view_lists, rt_tables.hip): one table per recent view, built on the table stream after the
// eye-cone table it reads and handed over exactly as that one is -- after the slot's last reader through the frame ring,
// before its first reader through `built`; a camera move costs no host wait.
#define RT_VIEW_SLOTS 4
struct ViewSlot {
    DevArray<float4> buf;
    unsigned key[18] = {};                // compared by bits: sphere_gen, origin, rotation, eye_nz, aspect, frame size, sample total, block shape
    bool valid = false;
    bool used = false;
    unsigned long long last_use = 0;
    HipEvent built;
    bool build_pending = false;
    int nbx = 0, nby = 0, bw = 0, bh = 0;
};

struct RtReflectDeleter {
    void operator()(RtReflect *r) const { rt_reflect_destroy(r); }
};

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
};

struct rt_scene {
    DevArray<float4> d_spheres;      // [n] list order | [n_pad] Morton order | [n_blocks] block bounds | [n_pad] ints
    int n_spheres = 0;
    int n_blocks = 0;
    std::vector<float4> h_prev;      // what was uploaded last (skip identical re-mirrors)
    PinnedArray<float4> h_stage;     // staging for asynchronous re-uploads
    HipEvent stage_done;             // the last upload out of h_stage
    bool stage_busy = false;
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
    // where the eye-cone builds run: beside the frames, not in front of them
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
    // per-view candidate lists of the primary rays
    ViewSlot views[RT_VIEW_SLOTS];
    int view_lists_mode = 1;                 // rt_scene_set_view_lists
    int view_last = -1;                      // the slot the last launch read, -1: it read none
    HipEvent order_built;                    // the last rebuild; launches on other streams wait for it on the device
    bool order_pending = false;
    // mirror reflections (rt_reflect.hip): materials, sphere BVH, queues; created on first use
    std::unique_ptr<RtReflect, RtReflectDeleter> refl;
    // the denoiser's scratch (rt_denoise.hip): two irradiance buffers and the packed guides, grown on demand; `dn_done`
    // orders the scene's denoise calls on the device, whatever their streams
    DevArray<float4> dn_col[2], dn_guide;
    DevArray<int> dn_key;
    HipEvent dn_done;
    bool dn_used = false;
    HipEvent dn_ev[RT_DENOISE_MAX_ITERATIONS + 2];   // rt_scene_set_denoise_timing
    bool dn_timing = false;
    int dn_timed = 0;                                // events the last timed call recorded
#ifdef RT_TUNING
    int tune_no_eye_cones = 0, tune_no_light_columns = 0, tune_ablate = 0;
#endif
};

static const int kMaxSpheres = 1 << 22;
static const int kMaxSpheresOccluders = 8192;    // the per-sphere occluder lists take n * 128 entries (2 KiB per sphere) per light

extern "C" rt_scene *rt_scene_create(void)
{
    rt_scene *s = new rt_scene();
    memset(&s->h_aux, 0, sizeof s->h_aux);
#ifdef RT_TUNING
    // tuning builds (make EXTRA=-DRT_TUNING, tools/variants.sh) read their switches once per scene;
    // the product library reads no environment
    if (const char *e = getenv("RT_NO_EYE_CONES")) s->tune_no_eye_cones = atoi(e);
    if (const char *e = getenv("RT_NO_LIGHT_COLUMNS")) s->tune_no_light_columns = atoi(e);
    if (const char *e = getenv("RT_ABLATE")) s->tune_ablate = atoi(e);
#endif
    return s;
}

// Wait (on the host) for every frame launched on this scene so far.
int rt_scene_quiesce(rt_scene *s)
{
    for (int i = 0; i < RT_RING; ++i)
        if (s->ring_used[i]) RT_HIP(hipEventSynchronize(s->ring[i].get()));
    if (s->table_stream.get()) RT_HIP(hipStreamSynchronize(s->table_stream.get()));   // a table build still reading the list
    if (s->dn_used) RT_HIP(hipEventSynchronize(s->dn_done.get()));                     // a denoise call still using the scratch
    return RT_OK;
}

// Make `stream` wait for every frame launched on this scene so far (no host wait).
static int stream_wait_all_frames(rt_scene *s, hipStream_t stream)
{
    for (int i = 0; i < RT_RING; ++i)
        if (s->ring_used[i]) RT_HIP(hipStreamWaitEvent(stream, s->ring[i].get(), 0));
    return RT_OK;
}

// A frame has just been enqueued on `stream`: give it the next ring slot. `cone_slot` >= 0:
// the eye-cone table the frame reads.
int rt_scene_note_launch(rt_scene *s, hipStream_t stream, int cone_slot)
{
    const int k = (int)(s->ring_seq % RT_RING);
    RT_HIP(s->ring[k].create());
    // chain: whoever sees this slot's new event done has also seen the one it replaces
    if (s->ring_used[k]) RT_HIP(hipStreamWaitEvent(stream, s->ring[k].get(), 0));
    RT_HIP(hipEventRecord(s->ring[k].get(), stream));
    s->ring_used[k] = true;
    if (cone_slot >= 0) {
        s->cones[cone_slot].used = true;
        s->cones[cone_slot].last_use = s->ring_seq;
    }
    s->ring_seq++;
    return RT_OK;
}

extern "C" void rt_scene_destroy(rt_scene *s)
{
    if (!s) return;
    (void)rt_scene_quiesce(s);   // then nothing reads what the members release
    delete s;
}

// {cx, cy, cz, radius*radius}: the only four numbers sphere::intersect reads
// (kernel.cu:332-334); radius*radius is the same binary32 product either way.
static void pack_spheres(const rt_sphere *src, int n, float4 *dst)
{
    for (int i = 0; i < n; ++i)
        dst[i] = make_float4(src[i].orgin.x, src[i].orgin.y, src[i].orgin.z, src[i].radius * src[i].radius);
}

// ---------------------------------------------------------------------------
// eye cones: which table a frame with ray origin `org` reads, building it if need be
// ---------------------------------------------------------------------------
static bool eye_cones_wanted(const rt_scene *s, const float org[3])
{
#ifdef RT_TUNING
    if (s->tune_no_eye_cones) return false;
#endif
    return s->n_spheres >= 64 && s->h_prev.size() == (size_t)s->n_spheres && std::isfinite(org[0]) &&
           std::isfinite(org[1]) && std::isfinite(org[2]);
}

// Fill `buf` (rt_eye_cones_size(n) float4) for `org`: on the device, on `stream`, when the list
// fits the one-workgroup builder; else on the host with a blocking upload (the caller has made
// sure nothing reads `buf`).
static int build_eye_cones_into(rt_scene *s, const float org[3], float4 *buf, hipStream_t stream)
{
    const int n = s->n_spheres;
    if (((n + 63) & ~63) <= RT_EYE_DEVICE_MAX) {
        RT_HIP(rt_eye_cones_launch(s->d_spheres.get(), n, org, buf, 1024, stream));
        return RT_OK;
    }
    const int n_pad = (n + 63) & ~63, nb = n_pad / RT_BLOCK;
    std::vector<float4> h(rt_eye_cones_size(n));
    rt_build_eye_cones_host(s->h_prev.data(), n, org, h.data(), h.data() + n_pad, reinterpret_cast<int *>(h.data() + n_pad + 2 * nb));
    RT_HIP(hipMemcpyAsync(buf, h.data(), sizeof(float4) * h.size(), hipMemcpyHostToDevice, stream));
    RT_HIP(hipStreamSynchronize(stream));   // `h` goes out of scope
    return RT_OK;
}

// Returns the slot whose table is current for `org` (building it on `stream` if none is), or
// -1 when the scene renders without eye cones. Not inside a stream capture.
static int rt_scene_prepare_eye(rt_scene *s, const float org[3], hipStream_t stream, int *slot_out)
{
    *slot_out = -1;
    if (!eye_cones_wanted(s, org)) return RT_OK;
    for (int i = 0; i < RT_CONE_SLOTS; ++i) {
        const ConeSlot &c = s->cones[i];
        if (c.valid && c.gen == s->sphere_gen && memcmp(org, c.org, sizeof c.org) == 0) {
            *slot_out = i;
            return RT_OK;
        }
    }
    // victim: an unused or stale slot, else the one read longest ago
    int v = 0;
    for (int i = 0; i < RT_CONE_SLOTS; ++i) {
        const ConeSlot &c = s->cones[i], &b = s->cones[v];
        const bool c_free = !c.valid || c.gen != s->sphere_gen, b_free = !b.valid || b.gen != s->sphere_gen;
        if ((c_free && !b_free) || (c_free == b_free && (!c.used || (b.used && c.last_use < b.last_use)))) v = i;
    }
    ConeSlot &c = s->cones[v];
    const size_t total = rt_eye_cones_size(s->n_spheres);
    const bool host_build = ((s->n_spheres + 63) & ~63) > RT_EYE_DEVICE_MAX;
    if (total > c.buf.capacity() || host_build) {
        const int rc = rt_scene_quiesce(s);   // nothing may still read the buffer that is freed / overwritten from the host
        if (rc != RT_OK) return rc;
    }
    c.valid = false;
    bool grew;
    RT_HIP(c.buf.reserve(total, &grew));
    if (grew) s->epoch++;
    if (host_build) {
        const int rc = build_eye_cones_into(s, org, c.buf.get(), stream);
        if (rc != RT_OK) return rc;
        c.build_pending = false;
    } else {
        // On the scene's table stream, so that the build of frame k+1's table runs beside frame
        // k's kernel instead of in front of frame k+1's (one small workgroup; a moving camera
        // then costs the frames nothing but an event wait). Ordered, on the device only, after
        // the last frame that read this slot and after a sphere-table upload still in flight.
        if (!s->table_stream.get()) {
            int lo = 0, hi = 0;
            (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
            RT_HIP(s->table_stream.create(hipStreamNonBlocking, hi));
        }
        const hipStream_t ts = s->table_stream.get();
        RT_HIP(c.built.create());
        if (c.used) {
            if (s->ring_seq - c.last_use <= RT_RING) RT_HIP(hipStreamWaitEvent(ts, s->ring[c.last_use % RT_RING].get(), 0));
            else {
                const int rc = stream_wait_all_frames(s, ts);
                if (rc != RT_OK) return rc;
            }
        }
        if (s->stage_busy) RT_HIP(hipStreamWaitEvent(ts, s->stage_done.get(), 0));
        RT_HIP(rt_eye_cones_launch(s->d_spheres.get(), s->n_spheres, org, c.buf.get(), 256, ts));
        RT_HIP(hipEventRecord(c.built.get(), ts));
        c.build_pending = true;
    }
    memcpy(c.org, org, sizeof c.org);
    c.gen = s->sphere_gen;
    c.valid = true;
    c.used = false;
    *slot_out = v;
    return RT_OK;
}

// ---------------------------------------------------------------------------
// per-light column tables (host build: lights and the list rarely change)
// ---------------------------------------------------------------------------
static int rt_scene_prepare_lights(rt_scene *s, hipStream_t stream)
{
    const int n = s->n_spheres;
    const int n_pad = (n + 63) & ~63, nb = n_pad / RT_BLOCK;
    bool want = n >= 64 && s->h_prev.size() == (size_t)n;
#ifdef RT_TUNING
    if (s->tune_no_light_columns) want = false;
#endif
    if (!want) {
        for (int i = 0; i < RT_MAX_LIGHTS; ++i) s->ltab_valid[i] = false;
        s->ltab_gen = ~0ull;
        return RT_OK;
    }
    const size_t per_light = (size_t)n_pad + 2 * (size_t)nb;   // float4 units
    float axis[RT_MAX_LIGHTS][3];
    bool usable[RT_MAX_LIGHTS];
    bool same = (s->ltab_gen == s->sphere_gen) && (s->ltab_n_lights == s->n_lights);
    for (int i = 0; i < s->n_lights; ++i) {
        const rt_light &l = s->lights[i];
        const float len = std::sqrt(l.pos.x * l.pos.x + l.pos.y * l.pos.y + l.pos.z * l.pos.z);   // as rt_build_frame_consts
        usable[i] = len > 0 && std::isfinite(len);
        axis[i][0] = usable[i] ? l.pos.x / len : 0.f;
        axis[i][1] = usable[i] ? l.pos.y / len : 0.f;
        axis[i][2] = usable[i] ? l.pos.z / len : 0.f;
        usable[i] = usable[i] && std::isfinite(axis[i][0]) && std::isfinite(axis[i][1]) && std::isfinite(axis[i][2]);
        same = same && (usable[i] == s->ltab_valid[i]) &&
               (!usable[i] || memcmp(axis[i], s->ltab_axis[i], sizeof axis[i]) == 0);
    }
    if (same) return RT_OK;
    // frames still in flight (another stream, a replaying graph) may be reading the old tables
    int rc = rt_scene_quiesce(s);
    if (rc != RT_OK) return rc;
    const size_t total = per_light * (size_t)std::max(1, s->n_lights);
    RT_HIP(s->d_light_tabs.reserve(total));
    std::vector<float4> h(total);
    for (int i = 0; i < s->n_lights; ++i) {
        s->ltab_valid[i] = usable[i];
        memcpy(s->ltab_axis[i], axis[i], sizeof axis[i]);
        if (usable[i])
            rt_build_light_columns(s->h_prev.data(), n, axis[i], h.data() + per_light * i, h.data() + per_light * i + n_pad);
    }
    for (int i = s->n_lights; i < RT_MAX_LIGHTS; ++i) s->ltab_valid[i] = false;
    RT_HIP(hipMemcpyAsync(s->d_light_tabs.get(), h.data(), sizeof(float4) * total, hipMemcpyHostToDevice, stream));
    RT_HIP(hipStreamSynchronize(stream));   // rare (scene or light change): `h` goes out of scope
    s->ltab_gen = s->sphere_gen;
    s->ltab_n_lights = s->n_lights;
    s->epoch++;
    return RT_OK;
}

// Per-light occluder lists (rt_tables.hip): which spheres a shadow ray from each sphere's surface can hit at all. Built
// on the DEVICE (one wave per sphere and light, from the list-order table that is already there) when the list or a
// light's position changes; the host waits for the build (rare, ~0.1 ms) so that frames on any stream may follow.
static int rt_scene_prepare_occluders(rt_scene *s, hipStream_t stream)
{
    const int n = s->n_spheres;
    bool want = n >= 64 && n <= kMaxSpheresOccluders && s->h_prev.size() == (size_t)n && s->d_spheres.get();
#ifdef RT_TUNING
    if (s->tune_no_light_columns) want = false;
#endif
    if (!want) {
        for (int i = 0; i < RT_MAX_LIGHTS; ++i) s->cand_valid[i] = false;
        s->cand_gen = ~0ull;
        return RT_OK;
    }
    bool same = (s->cand_gen == s->sphere_gen) && (s->cand_n_lights == s->n_lights);
    for (int i = 0; i < s->n_lights && same; ++i) {
        const float p[3] = {s->lights[i].pos.x, s->lights[i].pos.y, s->lights[i].pos.z};
        same = memcmp(p, s->cand_pos[i], sizeof p) == 0;
    }
    if (same) return RT_OK;
    int rc = rt_scene_quiesce(s);   // frames in flight may be reading the old lists
    if (rc != RT_OK) return rc;
    const size_t hdr_bytes = sizeof(RtCandHdr) * (size_t)n, ent_bytes = sizeof(float4) * (size_t)n * RT_CAND_CAP;
    const size_t bytes = (hdr_bytes + ent_bytes) * (size_t)s->n_lights;
    bool grew;
    RT_HIP(s->d_cand.reserve(bytes, &grew));
    // a wave reads whole steps of 64 from a slot and masks what lies past the count: let that be zeros, once
    if (grew) RT_HIP(hipMemsetAsync(s->d_cand.get(), 0, bytes, stream));
    if (s->stage_busy) RT_HIP(hipStreamWaitEvent(stream, s->stage_done.get(), 0));   // the table the build reads may still be on its way
    for (int i = 0; i < s->n_lights; ++i) {
        const float p[3] = {s->lights[i].pos.x, s->lights[i].pos.y, s->lights[i].pos.z};
        memcpy(s->cand_pos[i], p, sizeof p);
        s->cand_ent_off[i] = hdr_bytes * (size_t)s->n_lights + ent_bytes * (size_t)i;
        RT_HIP(rt_occluder_lists_launch(s->d_spheres.get(), n, p, reinterpret_cast<RtCandHdr *>(s->d_cand.get() + hdr_bytes * (size_t)i),
                                        reinterpret_cast<float4 *>(s->d_cand.get() + s->cand_ent_off[i]), stream));
        s->cand_valid[i] = true;
    }
    for (int i = s->n_lights; i < RT_MAX_LIGHTS; ++i) s->cand_valid[i] = false;
    RT_HIP(hipStreamSynchronize(stream));
    s->cand_gen = s->sphere_gen;
    s->cand_n_lights = s->n_lights;
    s->epoch++;
    return RT_OK;
}

int rt_scene_set_spheres_async(rt_scene *s, const rt_sphere *host_spheres, int n, hipStream_t stream)
{
    if (!s || n < 0 || (n > 0 && !host_spheres)) {
        rt_set_error("rt_scene_set_spheres: invalid argument");
        return RT_ERR_INVALID;
    }
    if (n > kMaxSpheres) {
        rt_set_error("rt_scene_set_spheres: %d spheres exceed the limit of %d", n, kMaxSpheres);
        return RT_ERR_CAPACITY;
    }
    const int n_pad = (n + 63) & ~63, nb = n_pad / RT_BLOCK;
    const size_t total = (size_t)n + (size_t)n_pad + (size_t)nb + ((size_t)n_pad + 3) / 4;   // in float4 units
    std::vector<float4> packed((size_t)n);
    if (n > 0) {
        pack_spheres(host_spheres, n, packed.data());
        if (s->n_spheres == n && s->h_prev.size() == (size_t)n && total <= s->d_spheres.capacity() &&
            memcmp(s->h_prev.data(), packed.data(), sizeof(float4) * (size_t)n) == 0)
            return RT_OK;   // unchanged since the last mirror: the device copy is current
    }
    // the table changes: frames in flight on ANY stream may still be reading the device copy
    // (two frames in flight, a replaying graph), so wait for them before it is overwritten or freed
    {
        const int rc = rt_scene_quiesce(s);
        if (rc != RT_OK) return rc;
    }
    bool grew;
    RT_HIP(s->d_spheres.reserve(total, &grew));
    if (grew) s->h_prev.clear();
    if (total > s->h_stage.capacity() && s->stage_busy) RT_HIP(hipEventSynchronize(s->stage_done.get()));   // before it is freed
    RT_HIP(s->h_stage.reserve(total));
    if (n > 0) {
        // the staging buffer is reused: wait for the previous upload to have left it
        RT_HIP(s->stage_done.create());
        if (s->stage_busy) RT_HIP(hipEventSynchronize(s->stage_done.get()));
        float4 *h_orig = s->h_stage.get(), *h_sorted = h_orig + n, *h_blocks = h_sorted + n_pad;
        int *h_idx = reinterpret_cast<int *>(h_blocks + nb);
        memcpy(h_orig, packed.data(), sizeof(float4) * (size_t)n);
        rt_build_sorted_blocks(packed.data(), n, h_sorted, h_blocks, h_idx);
        RT_HIP(hipMemcpyAsync(s->d_spheres.get(), s->h_stage.get(), sizeof(float4) * total, hipMemcpyHostToDevice, stream));
        RT_HIP(hipEventRecord(s->stage_done.get(), stream));
        s->stage_busy = true;
        s->h_prev.swap(packed);
    } else {
        s->h_prev.clear();
    }
    s->sphere_gen++;
    s->epoch++;
    s->n_blocks = nb;
    if (s->refl) rt_reflect_spheres_changed(s->refl.get(), s->n_spheres, n);
    s->n_spheres = n;
    return RT_OK;
}

extern "C" int rt_scene_set_spheres(rt_scene *s, const rt_sphere *host_spheres, int n)
{
    const int rc = rt_scene_set_spheres_async(s, host_spheres, n, nullptr);
    if (rc != RT_OK) return rc;
    RT_HIP(hipStreamSynchronize(nullptr));
    return RT_OK;
}

extern "C" int rt_scene_set_planes(rt_scene *s, const rt_plane *host_planes, int n)
{
    if (!s || n < 0 || (n > 0 && !host_planes)) {
        rt_set_error("rt_scene_set_planes: invalid argument");
        return RT_ERR_INVALID;
    }
    if (n > RT_MAX_PLANES) {
        rt_set_error("rt_scene_set_planes: %d planes > RT_MAX_PLANES %d", n, RT_MAX_PLANES);
        return RT_ERR_CAPACITY;
    }
    { const int rc = rt_scene_quiesce(s); if (rc != RT_OK) return rc; }
    RT_HIP(s->d_planes.reserve(RT_MAX_PLANES));
    std::vector<RtPlaneDev> tmp(n ? n : 1);
    for (int i = 0; i < n; ++i)
        tmp[i] = RtPlaneDev{host_planes[i].orgin.x, host_planes[i].orgin.y, host_planes[i].orgin.z,
                            host_planes[i].normal.x, host_planes[i].normal.y, host_planes[i].normal.z, 0.f, 0.f};
    if (n) RT_HIP(hipMemcpy(s->d_planes.get(), tmp.data(), sizeof(RtPlaneDev) * n, hipMemcpyHostToDevice));
    s->n_planes = n;
    s->epoch++;
    return RT_OK;
}

extern "C" int rt_scene_set_cubes(rt_scene *s, const rt_cube *host_cubes, int n)
{
    if (!s || n < 0 || (n > 0 && !host_cubes)) {
        rt_set_error("rt_scene_set_cubes: invalid argument");
        return RT_ERR_INVALID;
    }
    if (n > RT_MAX_CUBES) {
        rt_set_error("rt_scene_set_cubes: %d cubes > RT_MAX_CUBES %d", n, RT_MAX_CUBES);
        return RT_ERR_CAPACITY;
    }
    { const int rc = rt_scene_quiesce(s); if (rc != RT_OK) return rc; }
    RT_HIP(s->d_cubes.reserve(RT_MAX_CUBES));
    std::vector<RtCubeDev> tmp(n ? n : 1);
    for (int i = 0; i < n; ++i) {
        const rt_cube &c = host_cubes[i];
        tmp[i] = RtCubeDev{c.bounds[0].x, c.bounds[0].y, c.bounds[0].z, c.bounds[1].x, c.bounds[1].y, c.bounds[1].z,
                           c.orgin.x, c.orgin.y, c.orgin.z, 0.f, 0.f, 0.f};
    }
    if (n) RT_HIP(hipMemcpy(s->d_cubes.get(), tmp.data(), sizeof(RtCubeDev) * n, hipMemcpyHostToDevice));
    s->n_cubes = n;
    s->epoch++;
    return RT_OK;
}

// Flatten the reference-layout mesh (triangles, leaf boxes with their own index
// arrays) into three device arrays: triangles, boxes {bounds, start, len}, indices.
extern "C" int rt_scene_set_mesh(rt_scene *s, const rt_mesh *mesh)
{
    if (!s) {
        rt_set_error("rt_scene_set_mesh: null scene");
        return RT_ERR_INVALID;
    }
    { const int rc = rt_scene_quiesce(s); if (rc != RT_OK) return rc; }
    s->epoch++;
    RT_HIP(s->d_tris.reset());
    RT_HIP(s->d_boxes.reset());
    RT_HIP(s->d_tri_idx.reset());
    RT_HIP(s->d_box_spheres.reset());
    RT_HIP(s->d_tri9.reset());
    RT_HIP(s->d_tri_bs.reset());
    RT_HIP(s->d_tri_nrm.reset());
    s->n_boxes = s->n_tris = 0;
    if (!mesh || mesh->bvhbox_count == 0) return RT_OK;
    if (mesh->poly_count <= 0 || mesh->bvhbox_count < 0 || !mesh->d_tri_arr || !mesh->d_box) {
        rt_set_error("rt_scene_set_mesh: malformed mesh (poly_count=%d bvhbox_count=%d)", mesh->poly_count,
                     mesh->bvhbox_count);
        return RT_ERR_INVALID;
    }
    std::vector<RtTriDev> tris((size_t)mesh->poly_count);
    for (int i = 0; i < mesh->poly_count; ++i) {
        const rt_triangle &t = mesh->d_tri_arr[i];
        RtTriDev &d = tris[i];
        memset(&d, 0, sizeof d);
        memcpy(d.p0, &t.points[0], 12); memcpy(d.p1, &t.points[1], 12); memcpy(d.p2, &t.points[2], 12);
        memcpy(d.n, &t.normal, 12);
        memcpy(d.vn, t.vecNormal, 36);
        memcpy(d.vt, t.vt, 24);
    }
    std::vector<RtBoxDev> boxes((size_t)mesh->bvhbox_count);
    std::vector<float> bsph((size_t)mesh->bvhbox_count * 4);   // bounding sphere of each leaf (for beam culling)
    std::vector<int> idx;
    for (int j = 0; j < mesh->bvhbox_count; ++j) {
        const rt_bvhbox &b = mesh->d_box[j];
        const rt_cube *c = b.d_bvhbox ? b.d_bvhbox : b.bvhbox;
        if (!c || !b.d_indexes || b.length < 0) {
            rt_set_error("rt_scene_set_mesh: leaf %d is incomplete", j);
            return RT_ERR_INVALID;
        }
        RtBoxDev &d = boxes[j];
        d.lo[0] = c->bounds[0].x; d.lo[1] = c->bounds[0].y; d.lo[2] = c->bounds[0].z;
        d.hi[0] = c->bounds[1].x; d.hi[1] = c->bounds[1].y; d.hi[2] = c->bounds[1].z;
        {
            const double cx = 0.5 * ((double)d.lo[0] + d.hi[0]), cy = 0.5 * ((double)d.lo[1] + d.hi[1]),
                         cz = 0.5 * ((double)d.lo[2] + d.hi[2]);
            const double hx = 0.5 * std::fabs((double)d.hi[0] - d.lo[0]), hy = 0.5 * std::fabs((double)d.hi[1] - d.lo[1]),
                         hz = 0.5 * std::fabs((double)d.hi[2] - d.lo[2]);
            bsph[4 * j + 0] = (float)cx; bsph[4 * j + 1] = (float)cy; bsph[4 * j + 2] = (float)cz;
            bsph[4 * j + 3] = (float)((hx * hx + hy * hy + hz * hz) * 1.001 + 1e-6);   // radius^2, rounded up
        }
        d.start = (int)idx.size();
        d.len = b.length;
        for (int i = 0; i < b.length; ++i) {
            if (b.d_indexes[i] < 0 || b.d_indexes[i] >= mesh->poly_count) {
                rt_set_error("rt_scene_set_mesh: leaf %d references triangle %d of %d", j, b.d_indexes[i], mesh->poly_count);
                return RT_ERR_INVALID;
            }
            idx.push_back(b.d_indexes[i]);
        }
    }
    RT_HIP(s->d_tris.reserve(tris.size()));
    RT_HIP(s->d_boxes.reserve(boxes.size()));
    RT_HIP(s->d_tri_idx.reserve(idx.size() ? idx.size() : 1));
    {   // blocks of RT_BLOCK consecutive leaves (leaf order is kept: it decides ties between triangles),
        // each with a sphere around its members' spheres, appended after the (padded) leaf spheres
        const int nb = mesh->bvhbox_count, nb_pad = (nb + RT_BLOCK - 1) / RT_BLOCK * RT_BLOCK, nblk = nb_pad / RT_BLOCK;
        bsph.resize((size_t)(nb_pad + nblk) * 4, 0.f);
        for (int j = nb; j < nb_pad; ++j) bsph[4 * (size_t)j + 3] = -1.f;
        for (int k = 0; k < nblk; ++k) {
            const int j0 = k * RT_BLOCK, j1 = std::min(nb, j0 + RT_BLOCK);
            double cx = 0, cy = 0, cz = 0;
            for (int j = j0; j < j1; ++j) { cx += bsph[4 * (size_t)j]; cy += bsph[4 * (size_t)j + 1]; cz += bsph[4 * (size_t)j + 2]; }
            const double inv = 1.0 / std::max(1, j1 - j0);
            const float cf[3] = {(float)(cx * inv), (float)(cy * inv), (float)(cz * inv)};
            double r = 0;
            for (int j = j0; j < j1; ++j) {
                const double dx = bsph[4 * (size_t)j] - (double)cf[0], dy = bsph[4 * (size_t)j + 1] - (double)cf[1],
                             dz = bsph[4 * (size_t)j + 2] - (double)cf[2];
                const double d = std::sqrt(dx * dx + dy * dy + dz * dz) + std::sqrt(std::max(0.0, (double)bsph[4 * (size_t)j + 3]));
                r = (d > r || d != d) ? d : r;   // a NaN sticks
            }
            float rf = (float)(r * 1.001 + 1e-3);
            const bool fin = std::isfinite(cf[0]) && std::isfinite(cf[1]) && std::isfinite(cf[2]) && rf == rf;
            float *o = &bsph[4 * (size_t)(nb_pad + k)];
            o[0] = fin ? cf[0] : 0.f; o[1] = fin ? cf[1] : 0.f; o[2] = fin ? cf[2] : 0.f;
            o[3] = fin ? rf : INFINITY;
        }
    }
    RT_HIP(s->d_box_spheres.reserve(bsph.size()));
    RT_HIP(hipMemcpy(s->d_box_spheres.get(), bsph.data(), sizeof(float) * bsph.size(), hipMemcpyHostToDevice));
    RT_HIP(hipMemcpy(s->d_tris.get(), tris.data(), sizeof(RtTriDev) * tris.size(), hipMemcpyHostToDevice));
    RT_HIP(hipMemcpy(s->d_boxes.get(), boxes.data(), sizeof(RtBoxDev) * boxes.size(), hipMemcpyHostToDevice));
    if (!idx.empty()) RT_HIP(hipMemcpy(s->d_tri_idx.get(), idx.data(), sizeof(int) * idx.size(), hipMemcpyHostToDevice));
    {   // vertices per (leaf, triangle) pair, de-indexed and padded by 64 floats so that a full-wave load stays inside
        std::vector<float> t9(idx.size() * 9 + 64, 0.f);
        for (size_t k = 0; k < idx.size(); ++k) {
            memcpy(&t9[9 * k + 0], tris[idx[k]].p0, 12);
            memcpy(&t9[9 * k + 3], tris[idx[k]].p1, 12);
            memcpy(&t9[9 * k + 6], tris[idx[k]].p2, 12);
        }
        RT_HIP(s->d_tri9.reserve(t9.size()));
        RT_HIP(hipMemcpy(s->d_tri9.get(), t9.data(), sizeof(float) * t9.size(), hipMemcpyHostToDevice));
        // bounding sphere of every (leaf, triangle) pair for the per-triangle beam cull (beam_keeps_triangle):
        // centre = centroid, radius = farthest vertex, rounded up; with it the unit normal and kappa, the least
        // |cos| between a ray and the normal for which the cull is valid (slivers and anything non-finite: radius
        // +inf, normal 0, kappa 2 -- never culled)
        std::vector<float> bs(idx.size() * 4 + 4 * 64, 0.f);
        std::vector<float> bn(idx.size() * 4 + 4 * 64, 0.f);   // unit normals (zero = "always edge-on" for degenerate ones)
        for (size_t k = 0; k < idx.size(); ++k) {
            const float *p = &t9[9 * k];
            double c[3], r = 0, e[3][3], len[3];
            for (int a = 0; a < 3; ++a) c[a] = ((double)p[a] + p[3 + a] + p[6 + a]) / 3.0;
            for (int v = 0; v < 3; ++v) {
                double d2 = 0;
                for (int a = 0; a < 3; ++a) d2 += ((double)p[3 * v + a] - c[a]) * ((double)p[3 * v + a] - c[a]);
                r = std::max(r, std::sqrt(d2));
            }
            for (int v = 0; v < 3; ++v) {   // edge v: from vertex v to vertex (v+1)%3
                len[v] = 0;
                for (int a = 0; a < 3; ++a) {
                    e[v][a] = (double)p[3 * ((v + 1) % 3) + a] - p[3 * v + a];
                    len[v] += e[v][a] * e[v][a];
                }
                len[v] = std::sqrt(len[v]);
            }
            const double cx = e[0][1] * e[1][2] - e[0][2] * e[1][1], cy = e[0][2] * e[1][0] - e[0][0] * e[1][2],
                         cz = e[0][0] * e[1][1] - e[0][1] * e[1][0];
            const double area2 = std::sqrt(cx * cx + cy * cy + cz * cz);   // |e0 x e1| = twice the area
            double min_sin = INFINITY;
            for (int v = 0; v < 3; ++v) min_sin = std::min(min_sin, area2 / (len[v] * len[(v + 2) % 3]));
            // kappa = 3e-3 / (smallest corner sine), see beam_keeps_triangle; >= 1 means "never culled"
            const bool good = std::isfinite(r) && std::isfinite(c[0] + c[1] + c[2]) && min_sin > 3.0e-3 && min_sin == min_sin &&
                              area2 > 0 && std::isfinite(area2);
            bs[4 * k + 0] = (float)c[0]; bs[4 * k + 1] = (float)c[1]; bs[4 * k + 2] = (float)c[2];
            bs[4 * k + 3] = good ? (float)(r * 1.001 + 1e-6) : INFINITY;
            if (good) {
                bn[4 * k + 0] = (float)(cx / area2); bn[4 * k + 1] = (float)(cy / area2); bn[4 * k + 2] = (float)(cz / area2);
                bn[4 * k + 3] = (float)(3.0e-3 / min_sin * 1.001);
            } else {
                bn[4 * k + 3] = 2.f;
            }
        }
        RT_HIP(s->d_tri_bs.reserve(bs.size()));
        RT_HIP(hipMemcpy(s->d_tri_bs.get(), bs.data(), sizeof(float) * bs.size(), hipMemcpyHostToDevice));
        RT_HIP(s->d_tri_nrm.reserve(bn.size()));
        RT_HIP(hipMemcpy(s->d_tri_nrm.get(), bn.data(), sizeof(float) * bn.size(), hipMemcpyHostToDevice));
    }
    s->n_boxes = mesh->bvhbox_count;
    s->n_tris = mesh->poly_count;
    s->mesh_has_normals = mesh->has_normals ? 1 : 0;
    return RT_OK;
}

static int upload_planes(DevArray<float> dst[3], const float *r, const float *g, const float *b, int w, int h)
{
    const float *src[3] = {r, g, b};
    const size_t count = (size_t)w * (size_t)h;
    for (int i = 0; i < 3; ++i) (void)dst[i].reset();
    for (int i = 0; i < 3; ++i) {
        RT_HIP(dst[i].reserve(count));
        RT_HIP(hipMemcpy(dst[i].get(), src[i], sizeof(float) * count, hipMemcpyDefault));
    }
    return RT_OK;
}

extern "C" int rt_scene_set_texture(rt_scene *s, const float *r, const float *g, const float *b, int w, int h)
{
    if (!s || !r || !g || !b || w <= 0 || h <= 0) {
        rt_set_error("rt_scene_set_texture: invalid argument");
        return RT_ERR_INVALID;
    }
    int rc = rt_scene_quiesce(s);
    if (rc != RT_OK) return rc;
    s->epoch++;
    rc = upload_planes(s->d_tex, r, g, b, w, h);
    if (rc != RT_OK) return rc;
    s->tex_w = w;
    s->tex_h = h;
    return RT_OK;
}

extern "C" int rt_scene_set_sky(rt_scene *s, const rt_sphere *box, const float *r, const float *g,
                                const float *b, int w, int h)
{
    if (!s || !box || !r || !g || !b || w <= 0 || h <= 0) {
        rt_set_error("rt_scene_set_sky: invalid argument");
        return RT_ERR_INVALID;
    }
    int rc = rt_scene_quiesce(s);
    if (rc != RT_OK) return rc;
    s->epoch++;
    rc = upload_planes(s->d_sky, r, g, b, w, h);
    if (rc != RT_OK) return rc;
    s->sky_w = w;
    s->sky_h = h;
    s->sky_c[0] = box->orgin.x;
    s->sky_c[1] = box->orgin.y;
    s->sky_c[2] = box->orgin.z;
    s->sky_radius = box->radius;
    s->have_sky = true;
    return RT_OK;
}

extern "C" int rt_scene_set_lights(rt_scene *s, const rt_light *lights, int n)
{
    if (!s || n < 0 || (n > 0 && !lights)) {
        rt_set_error("rt_scene_set_lights: invalid argument");
        return RT_ERR_INVALID;
    }
    if (n > RT_MAX_LIGHTS) {
        rt_set_error("rt_scene_set_lights: light_size %d > RT_MAX_LIGHTS %d", n, RT_MAX_LIGHTS);
        return RT_ERR_CAPACITY;
    }
    // a frame graph holds the lights (its uniforms, RtFrameAux, the tables keyed on them): other lights rebuild it. The
    // drop-in boundary sets the same lights every frame, which must not.
    const bool same = n == s->n_lights && (n == 0 || memcmp(s->lights, lights, sizeof(rt_light) * (size_t)n) == 0);
    for (int i = 0; i < n; ++i) s->lights[i] = lights[i];
    s->n_lights = n;
    if (!same) s->epoch++;
    return RT_OK;
}


// ---------------------------------------------------------------------------
// sample positions (build-defined extension; n = 1 is the reference's +0.5)
// ---------------------------------------------------------------------------
extern "C" int rt_sample_offset(int k, int n, double *ox, double *oy)
{
    if (n < 1 || k < 0 || k >= n || !ox || !oy) return RT_ERR_INVALID;
    int g = 1;
    while (g * g < n) ++g;   // stratified g x g grid, cell centres
    *ox = ((double)(k % g) + 0.5) / (double)g;
    *oy = ((double)(k / g) + 0.5) / (double)g;
    return RT_OK;
}

extern "C" float rt_default_aspect(void)
{
    return (float)std::tan((90 * 0.5 * 3.1415) / 180);   // kernel.cu:1701
}

// ---------------------------------------------------------------------------
// frame uniforms: everything the reference recomputes per pixel from
// frame-constant inputs, evaluated once with the same operations.
// ---------------------------------------------------------------------------
// eyePos + cam.Org, kernel.cu:1629-1631: the origin of every primary ray of the frame
void rt_ray_origin(const rt_frame_desc *fd, float org[3])
{
    const float ez = -1.f / fd->aspect;
    org[0] = 0.f + fd->cam.Org.x;
    org[1] = 0.f + fd->cam.Org.y;
    org[2] = ez + fd->cam.Org.z;
}

// dx and dy of kernel.cu:1624-1625 for every column, row and sample of a frame:
//   dx = aspect*(2*(x+0.5)/(float)width) - 1,  dy = aspect*(2*(y+0.5)/(float)height)*((float)height/width) - 1
// binary64 expressions (the literal 0.5) narrowed to float on assignment. They depend on the
// camera in no way, so a moving camera re-uses them; a new size, aspect or sample count
// rebuilds them (host, W + H divisions per sample) after waiting for the frames in flight.
static int rt_scene_prepare_raygen(rt_scene *s, int width, int height, float aspect, int total)
{
    if (s->d_raygen.get() && s->rg_w == width && s->rg_h == height && s->rg_total == total &&
        memcmp(&s->rg_aspect, &aspect, sizeof aspect) == 0)
        return RT_OK;
    const int rc = rt_scene_quiesce(s);
    if (rc != RT_OK) return rc;
    const size_t need = (size_t)total * ((size_t)width + (size_t)height);
    RT_HIP(s->d_raygen.reserve(need));
    std::vector<float> h(need);
    const double aspect_d = (double)aspect;
    const double width_d = (double)(float)width, height_d = (double)(float)height;
    const double hw_d = (double)((float)height / (float)width);
    for (int k = 0; k < total; ++k) {
        double ox, oy;
        rt_sample_offset(k, total, &ox, &oy);
        float *dx = h.data() + (size_t)k * width, *dy = h.data() + (size_t)total * width + (size_t)k * height;
        for (int x = 0; x < width; ++x) {
            const double tx_d = (2.0 * ((double)x + ox)) / width_d;
            dx[x] = (float)(aspect_d * tx_d - 1.0);
        }
        for (int y = 0; y < height; ++y) {
            const double ty_d = (2.0 * ((double)y + oy)) / height_d;
            dy[y] = (float)((aspect_d * ty_d) * hw_d - 1.0);
        }
    }
    RT_HIP(hipMemcpy(s->d_raygen.get(), h.data(), sizeof(float) * need, hipMemcpyHostToDevice));
    s->rg_w = width;
    s->rg_h = height;
    s->rg_total = total;
    s->rg_aspect = aspect;
    s->epoch++;
    return RT_OK;
}

// margin of the fast texel-index path for a texture dimension of `size` texels (rt_kernels.hip:
// sure_texel): approximation error RT_UV_DELTA plus the rounding of the two float products
static float texel_margin(int size, float delta)
{
    return (float)size * (delta + 0x1.0p-22f) * 1.01f;
}

// Everything of the frame that lives in RtFrameAux (device memory): pure host computation.
static void rt_build_frame_aux(const rt_scene *s, RtFrameAux *ax)
{
    memset(ax, 0, sizeof *ax);
    // castLightRay sample constants, kernel.cu:1453-1454, 1462-1463
    for (int j = 0; j < RT_SHADOW_SAMPLES; ++j) {
        const float jf = (float)j / 10;
        const float phi = jf * 2.f * 3.1415f;
        ax->jf[j] = jf;
        ax->jcos[j] = rtm::cosf_rt(phi);
        ax->jsin[j] = rtm::sinf_rt(phi);
    }
    for (int i = 0; i < s->n_lights; ++i) {
        const rt_light &l = s->lights[i];
        RtLightDev &d = ax->lights[i];
        d.px = l.pos.x; d.py = l.pos.y; d.pz = l.pos.z;
        d.size = l.size;
        d.r = l.r; d.g = l.g; d.b = l.b;
        const float len = std::sqrt(l.pos.x * l.pos.x + l.pos.y * l.pos.y + l.pos.z * l.pos.z);
        d.pos_len = len;
        d.fin = (std::isfinite(l.r) && std::isfinite(l.g) && std::isfinite(l.b)) ? 1.f : 0.f;
        // a light at the origin has no beam axis: NaN makes the kernel skip culling
        d.ux = len > 0 ? l.pos.x / len : NAN;
        d.uy = len > 0 ? l.pos.y / len : NAN;
        d.uz = len > 0 ? l.pos.z / len : NAN;
        // e1 = the coordinate axis least aligned with u, made orthogonal to it; e2 = u x e1 (binary64, rounded once)
        {
            const double u[3] = {d.ux, d.uy, d.uz};
            const int k = (std::fabs(u[0]) <= std::fabs(u[1]) && std::fabs(u[0]) <= std::fabs(u[2])) ? 0 : (std::fabs(u[1]) <= std::fabs(u[2]) ? 1 : 2);
            double t[3] = {0, 0, 0};
            t[k] = 1;
            const double dt = u[k];
            double e1[3] = {t[0] - dt * u[0], t[1] - dt * u[1], t[2] - dt * u[2]};
            const double l1 = std::sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
            for (double &v : e1) v /= l1;   // NaN for a light at the origin: culling is off for it anyway
            const double e2[3] = {u[1] * e1[2] - u[2] * e1[1], u[2] * e1[0] - u[0] * e1[2], u[0] * e1[1] - u[1] * e1[0]};
            d.e1x = (float)e1[0]; d.e1y = (float)e1[1]; d.e1z = (float)e1[2];
            d.e2x = (float)e2[0]; d.e2y = (float)e2[1]; d.e2z = (float)e2[2];
            d.pad0_ = d.pad1_ = 0.f;
        }
    }
    {
        const int n_pad = (s->n_spheres + 63) & ~63;
        const size_t per_light = (size_t)n_pad + 2 * (size_t)s->n_blocks;
        const bool current = s->d_light_tabs.get() && s->ltab_gen == s->sphere_gen && s->ltab_n_lights == s->n_lights;
        for (int i = 0; i < RT_DEV_MAX_LIGHTS; ++i) {
            const bool on = current && i < s->n_lights && s->ltab_valid[i];
            ax->lsorted[i] = on ? reinterpret_cast<const float *>(s->d_light_tabs.get() + per_light * i) : nullptr;
            ax->lblocks[i] = on ? reinterpret_cast<const float *>(s->d_light_tabs.get() + per_light * i + n_pad) : nullptr;
            const bool con = s->d_cand.get() && s->cand_gen == s->sphere_gen && s->cand_n_lights == s->n_lights && i < s->n_lights && s->cand_valid[i];
            ax->cand_hdr[i] = con ? reinterpret_cast<const RtCandHdr *>(s->d_cand.get() + sizeof(RtCandHdr) * (size_t)s->n_spheres * (size_t)i) : nullptr;
            ax->cand_ent[i] = con ? reinterpret_cast<const float *>(s->d_cand.get() + s->cand_ent_off[i]) : nullptr;
        }
    }
    ax->sky_r = s->d_sky[0].get(); ax->sky_g = s->d_sky[1].get(); ax->sky_b = s->d_sky[2].get();
    ax->sky_w = s->sky_w; ax->sky_h = s->sky_h;
    ax->sky_cx = s->sky_c[0]; ax->sky_cy = s->sky_c[1]; ax->sky_cz = s->sky_c[2];
    ax->sky_r2 = s->sky_radius * s->sky_radius;
    ax->sky_mu_x = texel_margin(s->sky_w, 1.0e-6f);
    ax->sky_mu_y = texel_margin(s->sky_h, 1.0e-6f);
    ax->planes = s->d_planes.get();
    ax->cubes = s->d_cubes.get();
    ax->tris = s->d_tris.get();
    ax->boxes = s->d_boxes.get();
    ax->tri_idx = s->d_tri_idx.get();
    ax->box_spheres = s->d_box_spheres.get();
    ax->tri9 = s->d_tri9.get();
    ax->tri_bs = s->d_tri_bs.get();
    ax->tri_nrm = s->d_tri_nrm.get();
}

// Bring the device copy of RtFrameAux up to date (a camera move never changes it).
static int rt_scene_sync_aux(rt_scene *s)
{
    RtFrameAux ax;
    rt_build_frame_aux(s, &ax);
    if (s->aux_valid && memcmp(&ax, &s->h_aux, sizeof ax) == 0) return RT_OK;
    const int rc = rt_scene_quiesce(s);
    if (rc != RT_OK) return rc;
    RT_HIP(s->d_aux.reserve(1));
    RT_HIP(hipMemcpy(s->d_aux.get(), &ax, sizeof ax, hipMemcpyHostToDevice));
    s->h_aux = ax;
    s->aux_valid = true;
    s->epoch++;
    return RT_OK;
}

// camera::rotateDir, kernel.cu:249-250
static void view_rotation(const rt_frame_desc *fd, RtFrameConsts *fc)
{
    const float yawRad = (float)(fd->cam.Camyaw * (3.1415 / 180));
    const float pitchRad = (float)(fd->cam.Campitch * (3.1415 / 180));
    fc->cos_pitch = rtm::cosf_rt(pitchRad);
    fc->sin_pitch = rtm::sinf_rt(pitchRad);
    fc->cos_yaw = rtm::cosf_rt(yawRad);
    fc->sin_yaw = rtm::sinf_rt(yawRad);
}

// The by-value frame uniforms. Pure host computation: no device call, the scene is not
// changed. `cones`: the eye-cone table the frame reads (its org must be the frame's), or null.
int rt_build_frame_consts(const rt_scene *s, const rt_frame_desc *fd, const float4 *cones, RtFrameConsts *fc)
{
    if (!s || !fd) {
        rt_set_error("rt_scene_render: null scene or frame");
        return RT_ERR_INVALID;
    }
    if (fd->width <= 0 || fd->height <= 0) {
        rt_set_error("rt_scene_render: width/height must be positive (%d x %d)", fd->width, fd->height);
        return RT_ERR_INVALID;
    }
    const rt_launch_opts &o = fd->opts;
    int y0 = o.y0, y1 = o.y1;
    if (y0 == 0 && y1 == 0) y1 = fd->height;
    if (y0 < 0 || y1 > fd->height || y0 >= y1) {
        rt_set_error("rt_scene_render: bad row band [%d,%d) for height %d", y0, y1, fd->height);
        return RT_ERR_INVALID;
    }
    const int spp = o.spp > 0 ? o.spp : 1;
    const int total = o.sample_total > 0 ? o.sample_total : spp;
    if (spp > RT_MAX_SPP || total > RT_MAX_SPP || o.sample_base < 0 || o.sample_base + spp > total) {
        rt_set_error("rt_scene_render: bad sample range base=%d spp=%d total=%d (max %d)", o.sample_base, spp,
                     total, RT_MAX_SPP);
        return RT_ERR_INVALID;
    }
    if ((s->n_spheres > 0 || s->n_planes > 0 || s->n_cubes > 0 || s->n_boxes > 0) && (!s->d_tex[0].get() || s->tex_w <= 0)) {
        rt_set_error("rt_scene_render: scene has primitives but no object texture");
        return RT_ERR_INVALID;
    }
    if (!s->have_sky) {
        rt_set_error("rt_scene_render: scene has no skybox");
        return RT_ERR_INVALID;
    }
    {
        bool owns_rows = true;
        if (o.interleave_count > 1) {
            const int b = o.interleave_rows > 0 ? o.interleave_rows : 16;
            owns_rows = b > 0 && (long long)o.interleave_index * b < (y1 - y0);
        }
        if (owns_rows && !fd->pixels && !o.rgba && !o.packed24 && !rt_fd_aov_field(fd)) {
            rt_set_error("rt_scene_render: no output buffer (pixels, opts.rgba, opts.packed24 and aov_* are all null)");
            return RT_ERR_INVALID;
        }
    }

    memset(fc, 0, sizeof *fc);
    fc->width = fd->width;
    fc->height = fd->height;
    fc->y0 = y0;
    fc->y1 = y1;
    fc->n_spheres = s->n_spheres;
    fc->n_lights = s->n_lights;
    fc->spp = spp;
    fc->sample_base = o.sample_base;
    fc->sample_total = (float)total;
    fc->flags = (o.accumulate ? RT_FLAG_ACCUMULATE : 0) |
                (((fd->pixels || o.packed24) && o.resolve >= 0) ? RT_FLAG_RESOLVE : 0) |
                (o.force_slow_path ? RT_FLAG_FORCE_SLOW : 0) | (s->mesh_has_normals ? RT_FLAG_MESH_NORMALS : 0);
    fc->local_rows = y1 - y0;
    fc->il_count = 1;      // a contiguous band is the interleave of one rank (the kernel has one row formula)
    fc->il_index = 0;
    fc->il_rows = 16;
    if (o.interleave_count > 1) {
        const int b = o.interleave_rows > 0 ? o.interleave_rows : 16;
        // with a row band the blocks are dealt from the band's first row (which must start a block)
        if (b < 16 || (b & (b - 1)) != 0 || y0 % b != 0 || o.interleave_index < 0 || o.interleave_index >= o.interleave_count) {
            rt_set_error("rt_scene_render: bad interleave (count=%d index=%d rows=%d: a power of two >= 16; y0=%d must be a multiple of rows)",
                         o.interleave_count, o.interleave_index, b, y0);
            return RT_ERR_INVALID;
        }
        fc->il_count = o.interleave_count;
        fc->il_index = o.interleave_index;
        fc->il_rows = b;
        const int band = y1 - y0;
        int rows = 0;   // rows of the blocks this rank owns
        for (int k = o.interleave_index; k * b < band; k += o.interleave_count)
            rows += (band - k * b < b) ? band - k * b : b;
        fc->local_rows = rows;   // may be 0 (more ranks than row blocks): the launch is then skipped
    }
    fc->n_planes = s->n_planes;
    fc->n_cubes = s->n_cubes;
    fc->n_boxes = s->n_boxes;
#ifdef RT_TUNING
    fc->ablate = s->tune_ablate;   // timing experiments only: output is wrong when set
#endif

    // kernel.cu:1624-1625 through the raygen tables; :1629-1631: eyePos = (0,0,-1/aspect); dir - eyePos; eyePos + cam.Org
    const bool rg = s->d_raygen.get() && s->rg_w == fd->width && s->rg_h == fd->height && s->rg_total == total &&
                    memcmp(&s->rg_aspect, &fd->aspect, sizeof(float)) == 0;
    fc->dx_tab = rg ? s->d_raygen.get() : nullptr;
    fc->dy_tab = rg ? s->d_raygen.get() + (size_t)total * fd->width : nullptr;
    const float ez = -1.f / fd->aspect;
    fc->eye_nz = 0.f - ez;
    float org[3];
    rt_ray_origin(fd, org);
    fc->org_x = org[0];
    fc->org_y = org[1];
    fc->org_z = org[2];
    view_rotation(fd, fc);

    fc->tex_r = s->d_tex[0].get(); fc->tex_g = s->d_tex[1].get(); fc->tex_b = s->d_tex[2].get();
    fc->tex_w = s->tex_w; fc->tex_h = s->tex_h;
    fc->tex_mu_x = texel_margin(s->tex_w, 5.0e-7f);   // RT_UV_DELTA of rt_kernels.hip
    fc->tex_mu_y = texel_margin(s->tex_h, 5.0e-7f);
    {
        const int n_pad = (s->n_spheres + 63) & ~63;
        const float4 *base = s->d_spheres.get();
        fc->sorted = base ? reinterpret_cast<const float *>(base + s->n_spheres) : nullptr;
        fc->blocks = base ? reinterpret_cast<const float *>(base + s->n_spheres + n_pad) : nullptr;
        fc->orig_idx = base ? reinterpret_cast<const int *>(base + s->n_spheres + n_pad + s->n_blocks) : nullptr;
        fc->n_blocks = s->n_blocks;
        fc->csorted = cones ? reinterpret_cast<const float *>(cones) : nullptr;
        fc->cblocks = cones ? reinterpret_cast<const float *>(cones + n_pad) : nullptr;
        fc->corig = cones ? reinterpret_cast<const int *>(cones + n_pad + 2 * (size_t)s->n_blocks) : nullptr;
        fc->cone_kcap = (float)RT_CONE_KCAP;
    }
    fc->aux = s->d_aux.get();
    fc->rgba = o.rgba;
    fc->packed = fd->pixels;
    fc->packed24 = (uint32_t *)o.packed24;
    if (o.packed24 && fd->width % 4 != 0) {
        rt_set_error("rt_scene_render: packed24 needs a frame width that is a multiple of 4 (got %d)", fd->width);
        return RT_ERR_INVALID;
    }
    fc->stats = (unsigned long long *)o.stats;
    fc->aov_depth = fd->aov_depth;
    fc->aov_normal = fd->aov_normal;
    fc->aov_id = fd->aov_id;
    fc->aov_albedo = fd->aov_albedo;
    return RT_OK;
}

static int tile_from_opts(const rt_launch_opts &o, int *tile)
{
    const int t = o.tile ? o.tile : 8;
    if (t != 8 && t != 16 && t != 32 && t != 64) {
        rt_set_error("rt_scene_render: tile width %d not in {8,16,32,64}", t);
        return RT_ERR_INVALID;
    }
    *tile = t;
    return RT_OK;
}

// Which instantiation renders this frame (rt_kernels.hip: TW, CULL, MODE, FEAT).
int rt_frame_kernel_choice(const rt_scene *s, const rt_frame_desc *fd, RtKernelChoice *kc)
{
    int rc = tile_from_opts(fd->opts, &kc->tile);
    if (rc != RT_OK) return rc;
    kc->cull = (fd->opts.cull == 0) ? 0 : 1;
    kc->mode = fd->opts.stats ? (fd->opts.profile ? 3 : 1) : (fd->opts.force_slow_path ? 2 : 0);
    kc->feat = s->n_boxes > 0 ? 2 : ((s->n_planes > 0 || s->n_cubes > 0) ? 1 : 0);
    // the opt-in approximate mode exists for the product configuration only; anything else renders exactly
    // (a reflective frame is exact: `fast` is ignored there -- its L feeds the bounces; and so is
    // a launch with the table_lds field set: include/rt_engine.h)
    if (fd->opts.fast == 1 && fd->opts.reflect_depth == 0 && kc->mode == 0 && kc->cull && kc->tile == 8 && kc->feat < 2 &&
        fd->opts.table_lds != 1)
        kc->mode = 4;
#ifndef RT_TUNING
    if (kc->mode == 3) {
        rt_set_error("rt_scene_render: opts.profile (phase stamps) needs a tuning build of the library (make EXTRA=-DRT_TUNING)");
        return RT_ERR_UNSUPPORTED;
    }
#endif
    if (fd->opts.stats && fd->opts.force_slow_path) {
        rt_set_error("rt_scene_render: stats and force_slow_path exclude each other");
        return RT_ERR_UNSUPPORTED;
    }
    // the G-buffer kernel: the product kernel plus its stores (aov_supported has refused what it does not cover;
    // `fast` is ignored, as for reflective frames)
    if (rt_fd_aov_field(fd)) kc->mode = 5;
    return RT_OK;
}

// Everything a frame needs on the device that is NOT the eye-cone table: per-light tables,
// raygen tables, RtFrameAux. Host waits happen here, and only when something changed.
int rt_scene_prepare_static(rt_scene *s, const rt_frame_desc *fd, hipStream_t stream)
{
    if (!s || !fd || fd->width <= 0 || fd->height <= 0) {
        rt_set_error("rt_scene_render: null scene or bad frame");
        return RT_ERR_INVALID;
    }
    int rc = RT_OK;
    if (fd->opts.cull != 0) {
        rc = rt_scene_prepare_lights(s, stream);
        if (rc != RT_OK) return rc;
        rc = rt_scene_prepare_occluders(s, stream);
        if (rc != RT_OK) return rc;
    }
    const int spp = fd->opts.spp > 0 ? fd->opts.spp : 1;
    const int total = fd->opts.sample_total > 0 ? fd->opts.sample_total : spp;
    if (total < 1 || total > RT_MAX_SPP) {
        rt_set_error("rt_scene_render: bad sample total %d (max %d)", total, RT_MAX_SPP);
        return RT_ERR_INVALID;
    }
    rc = rt_scene_prepare_raygen(s, fd->width, fd->height, fd->aspect, total);
    if (rc != RT_OK) return rc;
    return rt_scene_sync_aux(s);
}

// The frame kernel records every tile's wave duration (two s_memtime and one store per wave: free). From the
// previous launch's durations the blocks of 16 x 16 tiles are sorted "longest tile first" (one workgroup on the
// launching stream, rt_tables.hip) and the launches start their tiles in that order: sorted again after 2, 4, 8, 16,
// 32, 64, 96, ... launches of an unchanged view (camera, sphere list), every RT_ORDER_MOVING launches while the view
// keeps changing. Scheduling only -- every tile is rendered once, by the same instructions. Ordering against frames
// in flight: the sort waits (on the device) for every frame launched so far, which read the old order; frames launched
// afterwards on other streams wait for the sort's event.
static int rt_scene_prepare_tile_order(rt_scene *s, const RtKernelChoice &kc, RtFrameConsts *fc, hipStream_t stream)
{
    const RtTileGrid grid = rt_tile_grid(kc.tile, fc->width, fc->local_rows);
    if (!grid.ok) return RT_OK;   // grid order
    const int key[12] = {kc.tile, fc->width, fc->height, fc->y0, fc->y1, fc->local_rows, fc->il_count, fc->il_index, fc->il_rows,
                         kc.cull, kc.mode, fc->spp};
    // what the durations depend on from frame to frame: the view and the sphere list
    const float view[8] = {fc->org_x, fc->org_y, fc->org_z, fc->cos_pitch, fc->sin_pitch, fc->cos_yaw, fc->sin_yaw,
                           (float)(s->sphere_gen & 0xffffff)};
    TileOrder *t = nullptr, *lru = &s->orders[0];
    for (TileOrder &o : s->orders) {
        if (o.buf.cap && memcmp(o.key, key, sizeof key) == 0) t = &o;
        if (o.last_use < lru->last_use) lru = &o;
    }
    if (s->order_pending) {   // an order being sorted (any layout: one event) precedes this launch
        if (hipEventQuery(s->order_built.get()) == hipSuccess) s->order_pending = false;
        else RT_HIP(hipStreamWaitEvent(stream, s->order_built.get(), 0));
        (void)hipGetLastError();
    }
    if (!t) {                 // a new layout takes the least recently used slot
        t = lru;
        int rc = stream_wait_all_frames(s, stream);   // frames that still write into the slot's old arrays
        if (rc != RT_OK) return rc;
        if (!t->buf.fits(grid)) {
            rc = rt_scene_quiesce(s);                  // re-allocation: nothing may still use the old arrays
            if (rc != RT_OK) return rc;
        }
        RT_HIP(t->buf.reserve(grid));
        RT_HIP(hipMemsetAsync(t->buf.cost(), 0, sizeof(unsigned) * t->buf.cap, stream));
        memcpy(t->key, key, sizeof key);
        memcpy(t->view, view, sizeof view);
        t->grid = grid;
        t->same_view = 0;
        t->since_sort = 0;
        t->have_perm = false;
        RT_HIP(s->order_built.create());
        RT_HIP(hipEventRecord(s->order_built.get(), stream));   // launches on other streams: after the reset
        s->order_pending = true;
    } else {
        if (memcmp(t->view, view, sizeof view) != 0) {
            memcpy(t->view, view, sizeof view);
            t->same_view = 0;
        }
        // launches of this view so far: t->same_view; launches since the last sort: t->since_sort (all recorded durations)
        const int k = t->same_view;
        const bool due = k == 0 ? t->since_sort >= (t->have_perm ? RT_ORDER_MOVING : 1)                 // a view that changes
                                : (k >= 2 && ((k & (k - 1)) == 0 || k % RT_ORDER_EVERY == 0)) || !t->have_perm;
        if (due && t->since_sort >= 1) {
            int rc = stream_wait_all_frames(s, stream);
            if (rc != RT_OK) return rc;
            RT_HIP(rt_tile_order_launch(t->buf.cost(), t->buf.key(), t->buf.start(), t->buf.perm(), t->grid.tiles_x, t->grid.tiles_y,
                                        stream));
            RT_HIP(s->order_built.create());
            RT_HIP(hipEventRecord(s->order_built.get(), stream));
            s->order_pending = true;
            t->have_perm = true;
            t->since_sort = 0;
        }
    }
    t->since_sort++;
    t->same_view++;
    t->last_use = ++s->order_clock;
    fc->tile_cost = t->buf.cost();
    fc->tile_perm = t->have_perm ? t->buf.perm() : nullptr;
    return RT_OK;
}

// The view of a frame as the view-list builders take it (block shape by rt_view_block_shape; tab, cones, out left null).
static void view_params_from_consts(const RtFrameConsts &fc, float aspect, RtViewParams *p)
{
    memset(p, 0, sizeof *p);
    p->n = fc.n_spheres;
    p->n_blocks = fc.n_blocks;
    p->org[0] = fc.org_x; p->org[1] = fc.org_y; p->org[2] = fc.org_z;
    p->cos_pitch = fc.cos_pitch; p->sin_pitch = fc.sin_pitch; p->cos_yaw = fc.cos_yaw; p->sin_yaw = fc.sin_yaw;
    p->eye_nz = fc.eye_nz;
    p->aspect = aspect;
    p->width = fc.width;
    p->height = fc.height;
    rt_view_block_shape(fc.width, fc.height, &p->bw, &p->bh);
    p->nbx = (fc.width + (1 << p->bw) - 1) >> p->bw;
    p->nby = (fc.height + (1 << p->bh) - 1) >> p->bh;
}

// Do whole tiles of this launch nest in the view's blocks? Tiles start at multiples of their width and, counted from
// the band's first row y0 (interleaved row blocks are multiples of 16 rows from there), of their height.
static bool view_tiles_nest(const RtViewParams &p, const RtFrameConsts &fc, int tile_w)
{
    const int th = 64 / tile_w;
    return (1 << p.bw) >= tile_w && (1 << p.bh) >= th && fc.y0 % th == 0;
}

// The view lists of a culled frame whose eye-cone table is cones[cone_slot]: finds or builds them and points fc at them.
// Leaves fc without lists (every tile culls for itself) when the switch is off or the launch's tiles do not nest.
static int rt_scene_prepare_view(rt_scene *s, const rt_frame_desc *fd, const RtKernelChoice &kc, int cone_slot, RtFrameConsts *fc,
                                 hipStream_t stream, int *view_out)
{
    *view_out = -1;
    if (!s->view_lists_mode || cone_slot < 0 || !kc.cull || kc.mode == 2) return RT_OK;
    RtViewParams p;
    view_params_from_consts(*fc, fd->aspect, &p);
    if (!view_tiles_nest(p, *fc, kc.tile)) return RT_OK;
    unsigned key[18];
    {
        const float f[10] = {p.org[0], p.org[1], p.org[2], p.cos_pitch, p.sin_pitch, p.cos_yaw, p.sin_yaw, p.eye_nz, p.aspect, fc->sample_total};
        memcpy(key, f, sizeof f);
        key[10] = (unsigned)s->sphere_gen; key[11] = (unsigned)(s->sphere_gen >> 32);
        key[12] = (unsigned)p.width; key[13] = (unsigned)p.height; key[14] = (unsigned)p.bw; key[15] = (unsigned)p.bh;
        key[16] = (unsigned)p.n; key[17] = 0;
    }
    int v = -1;
    for (int i = 0; i < RT_VIEW_SLOTS; ++i)
        if (s->views[i].valid && memcmp(s->views[i].key, key, sizeof key) == 0) v = i;
    if (v < 0) {
        // victim: a slot that holds nothing, else the one read longest ago
        v = 0;
        for (int i = 1; i < RT_VIEW_SLOTS; ++i) {
            const ViewSlot &c = s->views[i], &b = s->views[v];
            if (b.valid && (!c.valid || !c.used || (b.used && c.last_use < b.last_use))) v = i;
        }
        ViewSlot &c = s->views[v];
        const size_t total = rt_view_lists_size(p.nbx, p.nby);
        c.valid = false;
        if (total > c.buf.capacity()) {
            const int rc = rt_scene_quiesce(s);   // nothing may still read the buffer that is freed
            if (rc != RT_OK) return rc;
            RT_HIP(c.buf.reserve(total));
            s->epoch++;
        }
        if (!s->table_stream.get()) {
            int lo = 0, hi = 0;
            (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
            RT_HIP(s->table_stream.create(hipStreamNonBlocking, hi));
        }
        // on the table stream: behind the build of the eye-cone table it reads (same stream, or finished on the host),
        // after the last frame that read this slot and after a sphere-table upload still in flight
        const hipStream_t ts = s->table_stream.get();
        RT_HIP(c.built.create());
        if (c.used) {
            if (s->ring_seq - c.last_use <= RT_RING) RT_HIP(hipStreamWaitEvent(ts, s->ring[c.last_use % RT_RING].get(), 0));
            else {
                const int rc = stream_wait_all_frames(s, ts);
                if (rc != RT_OK) return rc;
            }
        }
        if (s->stage_busy) RT_HIP(hipStreamWaitEvent(ts, s->stage_done.get(), 0));
        p.tab = s->d_spheres.get();
        p.cones = s->cones[cone_slot].buf.get();
        p.out = c.buf.get();
        RT_HIP(rt_view_lists_launch(p, ts));
        RT_HIP(hipEventRecord(c.built.get(), ts));
        c.build_pending = true;
        memcpy(c.key, key, sizeof key);
        c.nbx = p.nbx; c.nby = p.nby; c.bw = p.bw; c.bh = p.bh;
        c.valid = true;
        c.used = false;
    }
    ViewSlot &c = s->views[v];
    if (c.build_pending) {   // the build precedes its readers
        if (hipEventQuery(c.built.get()) == hipSuccess) c.build_pending = false;
        else RT_HIP(hipStreamWaitEvent(stream, c.built.get(), 0));
        (void)hipGetLastError();
    }
    fc->view_lists = reinterpret_cast<const float *>(c.buf.get());
    fc->view_nbx = c.nbx;
    fc->view_shift = c.bw | (c.bh << 8);
    *view_out = v;
    return RT_OK;
}

// The layout before rt_launch_opts.reflect_depth was appended: what struct_size 0 reads as.
static const size_t kOptsSizeV1 = offsetof(rt_launch_opts, reflect_depth);
static const size_t kFrameSizeV1 = offsetof(rt_frame_desc, opts) + kOptsSizeV1;

// A frame description as this build lays it out, from a caller's that may be older (shorter): what the caller's
// struct_size fields do not cover reads as 0.
void normalise_frame_desc(const rt_frame_desc *fd, rt_frame_desc *out)
{
    memset(out, 0, sizeof *out);
    size_t fsz = fd->struct_size ? fd->struct_size : kFrameSizeV1;
    if (fsz > sizeof *out) fsz = sizeof *out;
    memcpy(out, fd, fsz);
    const size_t have = fsz > offsetof(rt_frame_desc, opts) ? fsz - offsetof(rt_frame_desc, opts) : 0;
    size_t osz = out->opts.struct_size ? out->opts.struct_size : kOptsSizeV1;
    if (osz > have) osz = have;
    if (osz < sizeof out->opts) memset(reinterpret_cast<char *>(&out->opts) + osz, 0, sizeof out->opts - osz);
    out->struct_size = (uint32_t)sizeof *out;
    out->opts.struct_size = (uint32_t)sizeof out->opts;
}

const char *rt_fd_aov_field(const rt_frame_desc *fd)
{
    if (fd->aov_depth) return "aov_depth";
    if (fd->aov_normal) return "aov_normal";
    if (fd->aov_id) return "aov_id";
    if (fd->aov_albedo) return "aov_albedo";
    return nullptr;
}

const char *rt_frame_aov_field(const rt_frame_desc *fd)
{
    if (!fd) return nullptr;
    rt_frame_desc f;
    normalise_frame_desc(fd, &f);
    return rt_fd_aov_field(&f);
}

// What a frame with G-buffer outputs (fd->aov_*) does not support; RT_OK when the frame may run (or sets none).
static int aov_supported(const rt_frame_desc *fd)
{
    const rt_launch_opts &o = fd->opts;
    const char *field = rt_fd_aov_field(fd);
    if (!field) return RT_OK;
    if (((uintptr_t)fd->aov_depth & 3u) || ((uintptr_t)fd->aov_normal & 15u) || ((uintptr_t)fd->aov_id & 7u) ||
        ((uintptr_t)fd->aov_albedo & 15u)) {
        rt_set_error("rt_scene_render: aov_normal and aov_albedo must be 16-byte aligned, aov_id 8-byte, aov_depth 4-byte");
        return RT_ERR_INVALID;
    }
    const char *why = nullptr;
    if (o.spp > 1 || o.sample_total > 1) why = "more than one sample per pixel";
    else if (o.tile != 0 && o.tile != 8) why = "a tile other than 8";
    else if (o.stats) why = "stats";
    else if (o.profile) why = "profile";
    else if (o.force_slow_path) why = "force_slow_path";
    if (why) {
        rt_set_error("rt_scene_render: %s (G-buffer outputs) does not support %s (one sample, the product kernel)", field, why);
        return RT_ERR_UNSUPPORTED;
    }
    return RT_OK;
}

int rt_frame_reflect_depth(const rt_frame_desc *fd)
{
    if (!fd) return 0;
    rt_frame_desc f;
    normalise_frame_desc(fd, &f);
    return f.opts.reflect_depth;
}

// What a reflective frame (opts.reflect_depth > 0) does not support; RT_OK when the frame may run.
static int reflect_supported(const rt_scene *s, const rt_frame_desc *fd)
{
    const rt_launch_opts &o = fd->opts;
    if (o.reflect_depth < 0 || o.reflect_depth > RT_MAX_REFLECT_DEPTH) {
        rt_set_error("rt_scene_render: reflect_depth %d not in [0, %d]", o.reflect_depth, RT_MAX_REFLECT_DEPTH);
        return RT_ERR_INVALID;
    }
    const char *why = nullptr;
    if (s->n_planes > 0 || s->n_cubes > 0 || s->n_boxes > 0) why = "planes, cubes or a mesh in the scene";
    else if (o.spp > 1 || o.sample_base != 0 || o.sample_total > 1) why = "more than one sample per pixel";
    else if (o.accumulate) why = "accumulate";
    else if (o.interleave_count > 1 || o.interleave_index != 0 || o.interleave_rows != 0) why = "interleave_*";
    else if (o.packed24) why = "packed24";
    else if (o.table_lds) why = "table_lds";
    else if (o.profile) why = "profile";
    if (why) {
        rt_set_error("rt_scene_render: reflect_depth > 0 does not support %s (spheres only, one sample, plain outputs)", why);
        return RT_ERR_UNSUPPORTED;
    }
    return RT_OK;
}

static RtReflect *scene_reflect(rt_scene *s)   // created on first use
{
    if (!s->refl) s->refl.reset(rt_reflect_create());
    return s->refl.get();
}

extern "C" int rt_scene_set_materials(rt_scene *s, const rt_material *per_sphere, int n)
{
    if (!s) {
        rt_set_error("rt_scene_set_materials: null scene");
        return RT_ERR_INVALID;
    }
    // frames in flight may read the device copy: rt_reflect_prepare re-uploads it before the next reflective frame,
    // after those frames (rt_scene_render waits for them when anything changed)
    return rt_reflect_set_materials(scene_reflect(s), per_sphere, n, s->n_spheres);
}

extern "C" int rt_scene_set_materials_ex(rt_scene *s, const rt_material_ex *per_sphere, int n)
{
    if (!s) {
        rt_set_error("rt_scene_set_materials_ex: null scene");
        return RT_ERR_INVALID;
    }
    // (as rt_scene_set_materials: the next reflective frame uploads after the frames in flight)
    return rt_reflect_set_materials_ex(scene_reflect(s), per_sphere, n, s->n_spheres);
}

extern "C" int rt_scene_set_reflect_timing(rt_scene *s, int on)
{
    if (!s) {
        rt_set_error("rt_scene_set_reflect_timing: null scene");
        return RT_ERR_INVALID;
    }
    return rt_reflect_set_timing(scene_reflect(s), on);
}

extern "C" int rt_scene_reflect_stats(rt_scene *s, rt_reflect_stats *out)
{
    if (!s || !out) {
        rt_set_error("rt_scene_reflect_stats: null argument");
        return RT_ERR_INVALID;
    }
    return rt_reflect_get_stats(scene_reflect(s), out);
}

// A sphere-table upload enqueued on some stream: order what `stream` does next after it.
static hipError_t order_after_upload(rt_scene *s, hipStream_t stream)
{
    if (s->stage_busy) {
        if (hipEventQuery(s->stage_done.get()) == hipSuccess) s->stage_busy = false;
        else {
            const hipError_t e = hipStreamWaitEvent(stream, s->stage_done.get(), 0);
            if (e != hipSuccess) return e;
        }
        (void)hipGetLastError();   // hipEventQuery reports "not ready" as an error
    }
    return hipSuccess;
}

static bool stream_capturing(hipStream_t stream)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (stream) (void)hipStreamIsCapturing(stream, &cs);
    return cs != hipStreamCaptureStatusNone;
}

extern "C" int rt_scene_render(rt_scene *s, const rt_frame_desc *fd_in, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!s || !fd_in) {
        rt_set_error("rt_scene_render: null scene or frame");
        return RT_ERR_INVALID;
    }
    rt_frame_desc fd_local;
    normalise_frame_desc(fd_in, &fd_local);
    const rt_frame_desc *fd = &fd_local;
    const int reflect_depth = fd->opts.reflect_depth;
    if (reflect_depth != 0) {
        const int rc = reflect_supported(s, fd);
        if (rc != RT_OK) return rc;
    }
    {
        const int rc = aov_supported(fd);
        if (rc != RT_OK) return rc;
    }
    {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (stream) (void)hipStreamIsCapturing(stream, &cs);
        if (cs != hipStreamCaptureStatusNone) {
            rt_set_error("rt_scene_render: the stream is being captured; use rt_graph_capture, which records the frame as graph nodes");
            return RT_ERR_UNSUPPORTED;
        }
    }
    RT_HIP(order_after_upload(s, stream));
    int rc = rt_scene_prepare_static(s, fd, stream);
    if (rc != RT_OK) return rc;
    int slot = -1;
    if (fd->opts.cull != 0) {
        float org[3];
        rt_ray_origin(fd, org);
        rc = rt_scene_prepare_eye(s, org, stream, &slot);
        if (rc != RT_OK) return rc;
    }
    if (slot >= 0 && s->cones[slot].build_pending) {   // the table's build (table stream) precedes its readers
        ConeSlot &c = s->cones[slot];
        if (hipEventQuery(c.built.get()) == hipSuccess) c.build_pending = false;
        else RT_HIP(hipStreamWaitEvent(stream, c.built.get(), 0));
        (void)hipGetLastError();
    }
    RtFrameConsts fc;
    rc = rt_build_frame_consts(s, fd, slot >= 0 ? s->cones[slot].buf.get() : nullptr, &fc);
    if (rc != RT_OK) return rc;
    RtKernelChoice kc;
    rc = rt_frame_kernel_choice(s, fd, &kc);
    if (rc != RT_OK) return rc;
    if (fc.local_rows == 0) return RT_OK;   // this rank owns no rows of the frame
    int view = -1;
    rc = rt_scene_prepare_view(s, fd, kc, slot, &fc, stream, &view);
    if (rc != RT_OK) return rc;
    if (reflect_depth > 0) {
        // the queues, the BVH and the materials are the scene's: after every frame launched so far (a host wait only
        // when the BVH or the materials change)
        RtReflect *refl = scene_reflect(s);
        if (rt_reflect_needs_upload(refl, s->sphere_gen, s->n_spheres)) {
            rc = rt_scene_quiesce(s);
            if (rc != RT_OK) return rc;
        }
        rc = stream_wait_all_frames(s, stream);
        if (rc != RT_OK) return rc;
        float *scratch = nullptr;
        rc = rt_reflect_prepare(refl, s->h_prev.data(), s->n_spheres, s->sphere_gen, fc.width * fc.local_rows,
                                fc.rgba == nullptr, &scratch, stream);
        if (rc != RT_OK) return rc;
        if (!fc.rgba) fc.rgba = scratch;
        rc = rt_reflect_begin_frame(refl, reflect_depth, stream);
        if (rc != RT_OK) return rc;
    }
    if (s->tile_order_mode != 0) {
        rc = rt_scene_prepare_tile_order(s, kc, &fc, stream);
        if (rc != RT_OK) return rc;
    }
    if (reflect_depth > 0) {
        rc = rt_reflect_mark_frame_start(s->refl.get(), stream);
        if (rc != RT_OK) return rc;
    }
    RT_HIP(rt_dev_launch_trace(&fc, s->d_spheres.get(), kc.tile, kc.cull, kc.mode, kc.feat, stream));
    if (reflect_depth > 0) {
        rc = rt_reflect_launch(s->refl.get(), &fc, s->d_spheres.get(), s->n_spheres, reflect_depth, kc.cull == 0, stream);
        if (rc != RT_OK) return rc;
    }
    s->view_last = view;
    if (view >= 0) {
        s->views[view].used = true;
        s->views[view].last_use = s->ring_seq;   // the ring slot this launch is about to take
    }
    return rt_scene_note_launch(s, stream, slot);
}

// ---------------------------------------------------------------------------
// ray queries (rt_query.hip)
// ---------------------------------------------------------------------------
extern "C" int rt_scene_trace_rays(rt_scene *s, const rt_ray_query *q_in, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!s || !q_in) {
        rt_set_error("rt_scene_trace_rays: null scene or query");
        return RT_ERR_INVALID;
    }
    rt_ray_query q;   // in this build's layout: what the caller's struct_size does not cover reads as 0
    memset(&q, 0, sizeof q);
    size_t sz = q_in->struct_size ? q_in->struct_size : sizeof q;
    if (sz > sizeof q) sz = sizeof q;
    memcpy(&q, q_in, sz);
    q.struct_size = (uint32_t)sizeof q;
    const char *bad = nullptr;
    if (q.mode != RT_QUERY_NEAREST && q.mode != RT_QUERY_OCCLUDED && q.mode != RT_QUERY_SHADE) bad = "mode is not an RT_QUERY_* value";
    else if (q.n < 0 || q.n > RT_MAX_QUERY_RAYS) bad = "n is not in [0, RT_MAX_QUERY_RAYS]";
    else if (q.cull < -1 || q.cull > 1) bad = "cull is not -1, 0 or 1";
    else if (q.n > 0 && !q.rays) bad = "rays is NULL";
    else if (q.mode == RT_QUERY_NEAREST && !q.hits) bad = "NEAREST needs hits";
    else if (q.mode == RT_QUERY_OCCLUDED && !q.occluded) bad = "OCCLUDED needs occluded";
    else if (q.mode == RT_QUERY_SHADE && !q.rgba && !q.packed) bad = "SHADE needs rgba or packed";
    else if ((((uintptr_t)q.rays | (uintptr_t)q.hits | (uintptr_t)q.occluded | (uintptr_t)q.packed) & 3u) || ((uintptr_t)q.rgba & 15u))
        bad = "rgba must be 16-byte aligned (one float4 store per ray), the other pointers 4-byte aligned";
    else if (q.mode == RT_QUERY_SHADE && !s->have_sky) bad = "SHADE needs the scene's sky";
    else if (q.mode == RT_QUERY_SHADE && (s->n_spheres > 0 || s->n_planes > 0 || s->n_cubes > 0 || s->n_boxes > 0) &&
             (!s->d_tex[0].get() || s->tex_w <= 0))
        bad = "SHADE needs the scene's texture";
    if (bad) {
        rt_set_error("rt_scene_trace_rays: %s (mode %d, n %d, cull %d)", bad, q.mode, q.n, q.cull);
        return RT_ERR_INVALID;
    }
    if (stream_capturing(stream)) {
        rt_set_error("rt_scene_trace_rays: the stream is being captured (queries are not recorded into graphs)");
        return RT_ERR_UNSUPPORTED;
    }
    if (q.n == 0) return RT_OK;
    RT_HIP(order_after_upload(s, stream));
    int rc = rt_scene_sync_aux(s);
    if (rc != RT_OK) return rc;
    const RtSphereBvh *bvh = nullptr;
    if (q.cull != 0 && s->n_spheres > 0) {
        // the BVH is shared with reflective frames: rebuilt (after a host wait for every reader) only when the list
        // changed, and read after whatever frame uploaded it last
        RtSphereBvh *b = rt_reflect_bvh(scene_reflect(s));
        if (rt_sphere_bvh_stale(b, s->sphere_gen, s->n_spheres)) {
            rc = rt_scene_quiesce(s);
            if (rc != RT_OK) return rc;
            rc = rt_sphere_bvh_update(b, s->h_prev.data(), s->n_spheres, s->sphere_gen, stream);
            if (rc != RT_OK) return rc;
        }
        rc = stream_wait_all_frames(s, stream);
        if (rc != RT_OK) return rc;
        bvh = b;
    }
    RtFrameConsts fc;
    memset(&fc, 0, sizeof fc);
    fc.n_spheres = s->n_spheres;
    fc.n_lights = s->n_lights;
    fc.n_planes = s->n_planes;
    fc.n_cubes = s->n_cubes;
    fc.n_boxes = s->n_boxes;
    fc.flags = s->mesh_has_normals ? RT_FLAG_MESH_NORMALS : 0;
    fc.tex_r = s->d_tex[0].get(); fc.tex_g = s->d_tex[1].get(); fc.tex_b = s->d_tex[2].get();
    fc.tex_w = s->tex_w; fc.tex_h = s->tex_h;
    fc.aux = s->d_aux.get();
    rc = rt_query_launch(&fc, bvh, s->d_spheres.get(), s->n_spheres, &q, stream);
    if (rc != RT_OK) return rc;
    return rt_scene_note_launch(s, stream, -1);   // a query in flight counts as a frame
}

extern "C" int rt_scene_primary_rays(rt_scene *s, const rt_frame_desc *fd_in, rt_ray *rays_dev, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!s || !fd_in || !rays_dev) {
        rt_set_error("rt_scene_primary_rays: null scene, frame or ray buffer");
        return RT_ERR_INVALID;
    }
    rt_frame_desc fd;
    normalise_frame_desc(fd_in, &fd);
    // one sample, a contiguous band; the frame's outputs are not used (rt_build_frame_consts wants one: the rays)
    rt_launch_opts &o = fd.opts;
    o.spp = 1; o.sample_base = 0; o.sample_total = 0; o.accumulate = 0; o.reflect_depth = 0;
    o.interleave_count = 0; o.interleave_index = 0; o.interleave_rows = 0;
    o.rgba = nullptr; o.packed24 = nullptr; o.stats = nullptr;
    fd.aov_depth = nullptr; fd.aov_normal = nullptr; fd.aov_id = nullptr; fd.aov_albedo = nullptr;
    fd.pixels = reinterpret_cast<uint32_t *>(rays_dev);
    if (stream_capturing(stream)) {
        rt_set_error("rt_scene_primary_rays: the stream is being captured");
        return RT_ERR_UNSUPPORTED;
    }
    RtFrameConsts fc;
    int rc = rt_build_frame_consts(s, &fd, nullptr, &fc);   // validates size, band, texture and sky first
    if (rc != RT_OK) return rc;
    rc = rt_scene_prepare_raygen(s, fd.width, fd.height, fd.aspect, 1);
    if (rc != RT_OK) return rc;
    rc = rt_build_frame_consts(s, &fd, nullptr, &fc);       // now with the raygen tables
    if (rc != RT_OK) return rc;
    rc = rt_query_launch_primary(&fc, rays_dev, stream);
    if (rc != RT_OK) return rc;
    return rt_scene_note_launch(s, stream, -1);   // it reads the raygen tables
}

// ---------------------------------------------------------------------------
// the G-buffer-guided denoiser (rt_denoise.hip)
// ---------------------------------------------------------------------------
extern "C" void rt_denoise_desc_init(rt_denoise_desc *d)
{
    if (!d) return;
    memset(d, 0, sizeof *d);
    d->struct_size = (uint32_t)sizeof *d;
    d->iterations = 4;
    d->normal_shift = 5;
    d->sigma_depth = 0.05f;
    d->sigma_colour = 0.f;
    d->demodulate = 1;
}

extern "C" int rt_scene_denoise(rt_scene *s, const rt_denoise_desc *d_in, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!s || !d_in) {
        rt_set_error("rt_scene_denoise: null scene or description");
        return RT_ERR_INVALID;
    }
    rt_denoise_desc d;   // in this build's layout: what the caller's struct_size does not cover reads as 0
    memset(&d, 0, sizeof d);
    size_t sz = d_in->struct_size ? d_in->struct_size : sizeof d;
    if (sz > sizeof d) sz = sizeof d;
    memcpy(&d, d_in, sz);
    d.struct_size = (uint32_t)sizeof d;
    const char *bad = nullptr;
    if (d.width <= 0 || d.height <= 0 || d.width > RT_DENOISE_MAX_SIZE || d.height > RT_DENOISE_MAX_SIZE)
        bad = "width and height must be in [1, RT_DENOISE_MAX_SIZE]";
    else if (!d.rgba_in || !d.depth || !d.normal || !d.id || !d.rgba_out) bad = "rgba_in, depth, normal, id and rgba_out must not be NULL";
    else if (d.demodulate && !d.albedo) bad = "demodulate needs albedo";
    else if ((((uintptr_t)d.rgba_in | (uintptr_t)d.normal | (uintptr_t)d.albedo | (uintptr_t)d.rgba_out) & 15u) ||
             ((uintptr_t)d.id & 7u) || (((uintptr_t)d.depth | (uintptr_t)d.pixels) & 3u))
        bad = "rgba_in, normal, albedo and rgba_out must be 16-byte aligned, id 8-byte, depth and pixels 4-byte";
    else if (d.iterations < 1 || d.iterations > RT_DENOISE_MAX_ITERATIONS) bad = "iterations is not in [1, RT_DENOISE_MAX_ITERATIONS]";
    else if (d.normal_shift < 0 || d.normal_shift > RT_DENOISE_MAX_NORMAL_SHIFT) bad = "normal_shift is not in [0, RT_DENOISE_MAX_NORMAL_SHIFT]";
    else if (!(d.sigma_depth > 0.f) || !std::isfinite(d.sigma_depth)) bad = "sigma_depth is not finite and > 0";
    else if (!std::isfinite(d.sigma_colour)) bad = "sigma_colour is not finite";
    else if (d.variant < 0 || d.variant > 2) bad = "variant is not 0, 1 or 2";
    if (bad) {
        rt_set_error("rt_scene_denoise: %s (%d x %d, iterations %d, normal_shift %d, variant %d)", bad, d.width, d.height,
                     d.iterations, d.normal_shift, d.variant);
        return RT_ERR_INVALID;
    }
    if (stream_capturing(stream)) {
        rt_set_error("rt_scene_denoise: the stream is being captured (the denoiser is not recorded into graphs)");
        return RT_ERR_UNSUPPORTED;
    }
    const size_t npx = (size_t)d.width * d.height;
    if (npx > s->dn_col[0].capacity() || npx > s->dn_col[1].capacity() ||
        (d.variant != 1 && (npx > s->dn_guide.capacity() || npx > s->dn_key.capacity()))) {
        // growing releases the old buffers: after the host has seen the last call that used them end
        if (s->dn_used) RT_HIP(hipEventSynchronize(s->dn_done.get()));
        RT_HIP(s->dn_col[0].reserve(npx));
        RT_HIP(s->dn_col[1].reserve(npx));
        if (d.variant != 1) {
            RT_HIP(s->dn_guide.reserve(npx));
            RT_HIP(s->dn_key.reserve(npx));
        }
    }
    RT_HIP(s->dn_done.create());
    if (s->dn_used) RT_HIP(hipStreamWaitEvent(stream, s->dn_done.get(), 0));   // one scratch: one call at a time
    hipEvent_t ev[RT_DENOISE_MAX_ITERATIONS + 2];
    s->dn_timed = 0;
    if (s->dn_timing) {
        for (int i = 0; i < RT_DENOISE_MAX_ITERATIONS + 2; ++i) {
            RT_HIP(s->dn_ev[i].create(hipEventDefault));
            ev[i] = s->dn_ev[i].get();
        }
    }
    const int rc = rt_denoise_launch(&d, s->dn_col[0].get(), s->dn_col[1].get(), s->dn_guide.get(), s->dn_key.get(),
                                     s->dn_timing ? ev : nullptr, stream);
    // also after a launch that failed half way: what was enqueued uses the scratch
    RT_HIP(hipEventRecord(s->dn_done.get(), stream));
    s->dn_used = true;
    if (rc == RT_OK && s->dn_timing) s->dn_timed = d.iterations + (d.variant == 1 ? 1 : 2);
    return rc;
}

extern "C" int rt_scene_set_denoise_timing(rt_scene *s, int on)
{
    if (!s) {
        rt_set_error("rt_scene_set_denoise_timing: null scene");
        return RT_ERR_INVALID;
    }
    s->dn_timing = on != 0;
    return RT_OK;
}

extern "C" int rt_scene_denoise_times(rt_scene *s, float *ms, int cap, int *n)
{
    if (!s || !ms || !n || cap < 0) {
        rt_set_error("rt_scene_denoise_times: null argument");
        return RT_ERR_INVALID;
    }
    *n = 0;
    if (s->dn_timed < 2) return RT_OK;
    RT_HIP(hipEventSynchronize(s->dn_done.get()));
    for (int i = 0; i + 1 < s->dn_timed && i < cap; ++i) {
        RT_HIP(hipEventElapsedTime(&ms[i], s->dn_ev[i].get(), s->dn_ev[i + 1].get()));
        *n = i + 1;
    }
    return RT_OK;
}

int rt_scene_tile_order_mode(const rt_scene *s) { return s->tile_order_mode; }

extern "C" int rt_scene_set_tile_order(rt_scene *s, int mode)
{
    if (!s || (mode != 0 && mode != 1)) {
        rt_set_error("rt_scene_set_tile_order: null scene or mode %d not in {0, 1}", mode);
        return RT_ERR_INVALID;
    }
    s->tile_order_mode = mode;
    return RT_OK;
}

// For rt_graph.cpp: the scene's buffers a graph node needs.
const float4 *rt_scene_sphere_table(const rt_scene *s) { return s->d_spheres.get(); }
int rt_scene_sphere_count(const rt_scene *s) { return s->n_spheres; }
unsigned long long rt_scene_epoch(const rt_scene *s) { return s->epoch; }
int rt_scene_view_lists_mode(const rt_scene *s) { return s->view_lists_mode; }

extern "C" int rt_scene_set_view_lists(rt_scene *s, int mode)
{
    if (!s || (mode != 0 && mode != 1)) {
        rt_set_error("rt_scene_set_view_lists: null scene or mode %d not in {0, 1}", mode);
        return RT_ERR_INVALID;
    }
    s->view_lists_mode = mode;
    return RT_OK;
}

static void view_lists_summary(const float4 *slots, int blocks, rt_view_lists_info *out)
{
    long long sum = 0;
    for (int b = 0; b < blocks; ++b) {
        int hdr[4];
        memcpy(hdr, slots + (size_t)b * RT_VIEW_SLOT, sizeof hdr);
        if (hdr[1] & RT_VIEW_OVERFLOW) out->overflowed++;
        if (hdr[1] & RT_VIEW_NOT_BUILT) out->not_built++;
        if (hdr[0] > out->longest) out->longest = hdr[0];
        sum += hdr[0];
    }
    out->blocks = blocks;
    out->mean = blocks > 0 ? (float)((double)sum / blocks) : 0.f;
}

// What the last launch on this scene read (waits for that view's build); out->read = 0: it read no lists. `slots`
// (optional, `cap` float4): a copy of the lists themselves.
extern "C" int rt_scene_view_lists_info(rt_scene *s, rt_view_lists_info *out, float *slots, size_t cap)
{
    if (!s || !out) {
        rt_set_error("rt_scene_view_lists_info: null argument");
        return RT_ERR_INVALID;
    }
    memset(out, 0, sizeof *out);
    if (s->view_last < 0) return RT_OK;
    const ViewSlot &c = s->views[s->view_last];
    RT_HIP(hipEventSynchronize(c.built.get()));
    const size_t total = rt_view_lists_size(c.nbx, c.nby);
    std::vector<float4> h(total);
    RT_HIP(hipMemcpy(h.data(), c.buf.get(), sizeof(float4) * total, hipMemcpyDeviceToHost));
    out->read = 1;
    out->block_w = 1 << c.bw; out->block_h = 1 << c.bh;
    out->blocks_x = c.nbx; out->blocks_y = c.nby;
    view_lists_summary(h.data(), c.nbx * c.nby, out);
    if (slots) {
        if (cap < total) {
            rt_set_error("rt_scene_view_lists_info: room for %zu float4, the lists take %zu", cap, total);
            return RT_ERR_INVALID;
        }
        memcpy(slots, h.data(), sizeof(float4) * total);
    }
    return RT_OK;
}

// The host builder for a sphere list and a frame description, no device involved (tests): the summary, and into `slots`
// (optional, `cap` float4) the lists. beams (optional): {ux, uy, uz, k or -1} per block.
extern "C" int rt_debug_view_lists_host(const rt_sphere *spheres, int n, const rt_frame_desc *fd_in, rt_view_lists_info *out,
                                        float *slots, size_t cap, float *beams)
{
    if (!spheres || n < 1 || !fd_in || !out) {
        rt_set_error("rt_debug_view_lists_host: bad argument");
        return RT_ERR_INVALID;
    }
    rt_frame_desc fd;
    normalise_frame_desc(fd_in, &fd);
    RtFrameConsts fc;
    memset(&fc, 0, sizeof fc);
    fc.n_spheres = n;
    fc.width = fd.width; fc.height = fd.height;
    fc.eye_nz = 0.f - (-1.f / fd.aspect);
    float org[3];
    rt_ray_origin(&fd, org);
    fc.org_x = org[0]; fc.org_y = org[1]; fc.org_z = org[2];
    view_rotation(&fd, &fc);
    RtViewParams p;
    view_params_from_consts(fc, fd.aspect, &p);
    std::vector<float4> tab((size_t)n);
    pack_spheres(spheres, n, tab.data());
    const size_t total = rt_view_lists_size(p.nbx, p.nby);
    std::vector<float4> h(total);
    p.out = h.data();
    rt_build_view_lists_host(tab.data(), p, h.data());
    memset(out, 0, sizeof *out);
    out->block_w = 1 << p.bw; out->block_h = 1 << p.bh;
    out->blocks_x = p.nbx; out->blocks_y = p.nby;
    view_lists_summary(h.data(), p.nbx * p.nby, out);
    if (slots) {
        if (cap < total) {
            rt_set_error("rt_debug_view_lists_host: room for %zu float4, the lists take %zu", cap, total);
            return RT_ERR_INVALID;
        }
        memcpy(slots, h.data(), sizeof(float4) * total);
    }
    if (beams)
        for (int b = 0; b < p.nbx * p.nby; ++b) {
            const RtViewBeam vb = rt_view_block_beam(p, b % p.nbx, b / p.nbx);
            beams[4 * b + 0] = vb.ux; beams[4 * b + 1] = vb.uy; beams[4 * b + 2] = vb.uz; beams[4 * b + 3] = vb.ok ? vb.k : -1.f;
        }
    return RT_OK;
}

// for a graph's own lists (rt_graph.cpp)
int rt_view_params_for_frame(const rt_scene *s, const RtFrameConsts *fc, float aspect, int tile_w, int cull, int mode, RtViewParams *p)
{
    view_params_from_consts(*fc, aspect, p);
    return s->view_lists_mode && cull && mode != 2 && view_tiles_nest(*p, *fc, tile_w);
}

bool rt_scene_wants_eye_cones(const rt_scene *s, const float org[3]) { return eye_cones_wanted(s, org); }
int rt_scene_build_eye_cones_host(rt_scene *s, const float org[3], float4 *buf, hipStream_t stream)
{
    return build_eye_cones_into(s, org, buf, stream);
}

// ---------------------------------------------------------------------------
// rayTrace launch shim (kernel.cu:1615, 1780-1783): same argument list, the
// object / skybox graphs are read on the host and mirrored to the device.
// ---------------------------------------------------------------------------
struct ShimCache {
    rt_scene *scene = nullptr;
    const rt_mesh *mesh_key = nullptr;
    int mesh_polys = -1, mesh_boxes = -1;
    const float *tex_key[3] = {nullptr, nullptr, nullptr};
    int tex_w = 0, tex_h = 0;
    const float *sky_key[3] = {nullptr, nullptr, nullptr};
    int sky_w = 0, sky_h = 0;
    float sky_c[3] = {0, 0, 0};
    float sky_radius = -1;
};
static ShimCache g_shim;

// memManager::operator delete on something the shim has mirrored: the next launch re-uploads.
static void shim_forget(const void *ptr)
{
    for (int i = 0; i < 3; ++i) {
        if (ptr == g_shim.tex_key[i]) g_shim.tex_key[0] = g_shim.tex_key[1] = g_shim.tex_key[2] = nullptr;
        if (ptr == g_shim.sky_key[i]) g_shim.sky_key[0] = g_shim.sky_key[1] = g_shim.sky_key[2] = nullptr;
    }
    if (ptr == g_shim.mesh_key) {
        g_shim.mesh_key = nullptr;
        g_shim.mesh_polys = g_shim.mesh_boxes = -1;
    }
}

extern "C" void rt_invalidate_textures(void)
{
    g_shim.mesh_key = nullptr;
    g_shim.mesh_polys = g_shim.mesh_boxes = -1;
    g_shim.tex_key[0] = g_shim.tex_key[1] = g_shim.tex_key[2] = nullptr;
    g_shim.sky_key[0] = g_shim.sky_key[1] = g_shim.sky_key[2] = nullptr;
}

static bool sprite_ok(const rt_sprite *t)
{
    return t && t->rBuff && t->gBuff && t->bBuff && t->rBuff->data && t->gBuff->data && t->bBuff->data &&
           t->width > 0 && t->height > 0;
}

extern "C" int rt_launch_raytrace_ex(uint32_t *pixels, int width, int height, float aspect,
                                     const rt_object *objs, const rt_light *lights, int light_size,
                                     rt_camera cam, const rt_skybox *sky, void *stream,
                                     const rt_launch_opts *opts)
{
    if (!objs || !sky || (!lights && light_size > 0)) {
        rt_set_error("rt_launch_raytrace: null objs/lights/sky");
        return RT_ERR_INVALID;
    }
    if (objs->cube_count < 0 || objs->plane_count < 0 || (objs->cube_count > 0 && !objs->d_cubes) ||
        (objs->plane_count > 0 && !objs->d_planes)) {
        rt_set_error("rt_launch_raytrace: bad cube/plane list");
        return RT_ERR_INVALID;
    }
    if (objs->sphere_count < 0 || (objs->sphere_count > 0 && !objs->d_spheres)) {
        rt_set_error("rt_launch_raytrace: bad sphere list");
        return RT_ERR_INVALID;
    }
    if (!sky->box || !sprite_ok(sky->skyboxTex)) {
        rt_set_error("rt_launch_raytrace: skybox needs a box sphere and a texture");
        return RT_ERR_INVALID;
    }
    if ((objs->sphere_count > 0 || objs->cube_count > 0 || objs->plane_count > 0 || objs->mesh1) &&
        !sprite_ok(objs->texture)) {
        rt_set_error("rt_launch_raytrace: object texture missing");
        return RT_ERR_INVALID;
    }
    if (!g_shim.scene) g_shim.scene = rt_scene_create();
    rt_scene *s = g_shim.scene;
    int rc;
    // textures: uploaded once per (planes, size); see rt_invalidate_textures()
    if (objs->sphere_count > 0 || objs->cube_count > 0 || objs->plane_count > 0 || objs->mesh1) {
        const rt_sprite *t = objs->texture;
        if (t->rBuff->data != g_shim.tex_key[0] || t->gBuff->data != g_shim.tex_key[1] ||
            t->bBuff->data != g_shim.tex_key[2] || t->width != g_shim.tex_w || t->height != g_shim.tex_h) {
            rc = rt_scene_set_texture(s, t->rBuff->data, t->gBuff->data, t->bBuff->data, t->width, t->height);
            if (rc != RT_OK) return rc;
            g_shim.tex_key[0] = t->rBuff->data; g_shim.tex_key[1] = t->gBuff->data; g_shim.tex_key[2] = t->bBuff->data;
            g_shim.tex_w = t->width; g_shim.tex_h = t->height;
        }
    }
    {
        const rt_sprite *t = sky->skyboxTex;
        if (t->rBuff->data != g_shim.sky_key[0] || t->gBuff->data != g_shim.sky_key[1] ||
            t->bBuff->data != g_shim.sky_key[2] || t->width != g_shim.sky_w || t->height != g_shim.sky_h ||
            sky->box->orgin.x != g_shim.sky_c[0] || sky->box->orgin.y != g_shim.sky_c[1] ||
            sky->box->orgin.z != g_shim.sky_c[2] || sky->box->radius != g_shim.sky_radius) {
            rc = rt_scene_set_sky(s, sky->box, t->rBuff->data, t->gBuff->data, t->bBuff->data, t->width, t->height);
            if (rc != RT_OK) return rc;
            g_shim.sky_key[0] = t->rBuff->data; g_shim.sky_key[1] = t->gBuff->data; g_shim.sky_key[2] = t->bBuff->data;
            g_shim.sky_w = t->width; g_shim.sky_h = t->height;
            g_shim.sky_c[0] = sky->box->orgin.x; g_shim.sky_c[1] = sky->box->orgin.y; g_shim.sky_c[2] = sky->box->orgin.z;
            g_shim.sky_radius = sky->box->radius;
        }
    }
    // the mesh is uploaded once per (pointer, counts), like the textures
    {
        const rt_mesh *m = (objs->mesh1 && objs->mesh1->bvhbox_count > 0) ? objs->mesh1 : nullptr;
        const int polys = m ? m->poly_count : 0, boxes = m ? m->bvhbox_count : 0;
        if (m != g_shim.mesh_key || polys != g_shim.mesh_polys || boxes != g_shim.mesh_boxes) {
            rc = rt_scene_set_mesh(s, m);
            if (rc != RT_OK) return rc;
            g_shim.mesh_key = m;
            g_shim.mesh_polys = polys;
            g_shim.mesh_boxes = boxes;
        }
    }
    // spheres and lights are small and may change every frame: re-mirror them
    rc = rt_scene_set_spheres_async(s, objs->d_spheres, objs->sphere_count, (hipStream_t)stream);
    if (rc != RT_OK) return rc;
    rc = rt_scene_set_lights(s, lights, light_size);
    if (rc != RT_OK) return rc;
    if (objs->plane_count > 0 || s->n_planes > 0) {
        rc = rt_scene_set_planes(s, objs->d_planes, objs->plane_count);
        if (rc != RT_OK) return rc;
    }
    if (objs->cube_count > 0 || s->n_cubes > 0) {
        rc = rt_scene_set_cubes(s, objs->d_cubes, objs->cube_count);
        if (rc != RT_OK) return rc;
    }
    // the reference's object-wide material (object::mat) on every sphere, for a reflective launch only
    if (opts && opts->struct_size >= offsetof(rt_launch_opts, reflect_depth) + sizeof(int) && opts->reflect_depth > 0) {
        {
            std::vector<rt_material> mats;
            if (objs->mat) mats.assign((size_t)objs->sphere_count, *static_cast<const rt_material *>(objs->mat));
            rc = rt_scene_set_materials(s, mats.empty() ? nullptr : mats.data(), (int)mats.size());
            if (rc != RT_OK) return rc;
        }
    }

    rt_frame_desc fd;
    memset(&fd, 0, sizeof fd);
    fd.struct_size = sizeof fd;
    fd.width = width;
    fd.height = height;
    fd.aspect = aspect;
    fd.cam = cam;
    fd.pixels = pixels;
    if (opts) {
        const size_t nbytes = opts->struct_size < sizeof fd.opts ? opts->struct_size : sizeof fd.opts;
        memcpy(&fd.opts, opts, nbytes);
        fd.opts.struct_size = (uint32_t)sizeof fd.opts;
    } else {
        fd.opts.cull = -1;
    }
    return rt_scene_render(s, &fd, stream);
}

extern "C" int rt_launch_raytrace(uint32_t *pixels, int width, int height, float aspect,
                                  const rt_object *objs, const rt_light *lights, int light_size,
                                  rt_camera cam, const rt_skybox *sky, void *stream)
{
    return rt_launch_raytrace_ex(pixels, width, height, aspect, objs, lights, light_size, cam, sky, stream, nullptr);
}

// ---------------------------------------------------------------------------
// diagnostics: device evaluation of scalar building blocks (host arrays in/out)
// ---------------------------------------------------------------------------
extern "C" int rt_debug_math(int op, const float *a, const float *b, float *out, int n)
{
    if (n <= 0 || !a || !out || op < 0 || op > 5 || (op == 3 && !b)) return RT_ERR_INVALID;
    DevArray<float> da, db, dout;
    RT_HIP(da.reserve(n));
    RT_HIP(db.reserve(n));
    RT_HIP(dout.reserve(n));
    RT_HIP(hipMemcpy(da.get(), a, sizeof(float) * n, hipMemcpyHostToDevice));
    RT_HIP(hipMemcpy(db.get(), b ? b : a, sizeof(float) * n, hipMemcpyHostToDevice));
    RT_HIP(rt_dev_launch_dbg_math(op, da.get(), db.get(), dout.get(), n, nullptr));
    RT_HIP(hipMemcpy(out, dout.get(), sizeof(float) * n, hipMemcpyDeviceToHost));
    return RT_OK;
}

extern "C" int rt_debug_shortcuts(int what, unsigned seed, long long n, unsigned long long out[4])
{
    if (what < 0 || what > 2 || !out || n < 0) return RT_ERR_INVALID;
    DevArray<unsigned long long> d;
    RT_HIP(d.reserve(4));
    RT_HIP(hipMemset(d.get(), 0, sizeof(unsigned long long) * 4));
    RT_HIP(rt_dev_launch_dbg_shortcuts(what, seed, n, d.get(), nullptr));
    RT_HIP(hipMemcpy(out, d.get(), sizeof(unsigned long long) * 4, hipMemcpyDeviceToHost));
    return RT_OK;
}

// The occluder lists of one light (rt_build_occluder_lists; host only, no GPU): counts[i] = entries of sphere i's list
// (-1: none), kcaps[i] = the beam slope it holds for, members: n x cap ints, the list positions of the first `cap`
// members of every list (an entry is identified by its four floats: the first sphere of the table with those).
extern "C" int rt_debug_occluder_lists_ex(const rt_sphere *spheres, int n, const rt_light *light, int *counts, float *kcaps, int *members, int cap,
                                          int *offsets, int *entries_allocated)
{
    if (n <= 0 || !spheres || !light || !counts || !kcaps || (cap > 0 && !members)) return RT_ERR_INVALID;
    std::vector<float4> tab((size_t)n);
    pack_spheres(spheres, n, tab.data());
    std::vector<RtCandHdr> hdr;
    std::vector<float4> ent;
    const float p[3] = {light->pos.x, light->pos.y, light->pos.z};
    rt_build_occluder_lists(tab.data(), n, p, hdr, ent);
    if (entries_allocated) *entries_allocated = (int)ent.size();
    for (int i = 0; i < n; ++i) {
        counts[i] = hdr[(size_t)i].count;
        kcaps[i] = hdr[(size_t)i].kcap;
        if (offsets) offsets[i] = hdr[(size_t)i].offset;
        for (int k = 0; k < cap; ++k) members[(size_t)i * cap + k] = -1;
        for (int k = 0; k < hdr[(size_t)i].count && k < cap; ++k) {
            const float4 e = ent[(size_t)hdr[(size_t)i].offset + k];
            for (int j = 0; j < n; ++j)
                if (memcmp(&tab[(size_t)j], &e, sizeof e) == 0) { members[(size_t)i * cap + k] = j; break; }
        }
    }
    return RT_OK;
}

// The per-sphere beam slopes (RtCandHdr::kbeam; -1: none) as the host builder (host_kbeam, or NULL) and the device builder
// (device_kbeam, or NULL: no GPU needed then) compute them, and the pieces of the bound for tests: the spread at ONE start.
extern "C" int rt_debug_sphere_beam_slopes(const rt_sphere *spheres, int n, const rt_light *light, float *host_kbeam, float *device_kbeam)
{
    if (n <= 0 || !spheres || !light) return RT_ERR_INVALID;
    std::vector<float4> tab((size_t)n);
    pack_spheres(spheres, n, tab.data());
    const float p[3] = {light->pos.x, light->pos.y, light->pos.z};
    if (host_kbeam) {
        std::vector<RtCandHdr> hdr;
        std::vector<float4> ent;
        rt_build_occluder_lists(tab.data(), n, p, hdr, ent);
        for (int i = 0; i < n; ++i) host_kbeam[i] = hdr[(size_t)i].kbeam;
    }
    if (device_kbeam) {
        DevArray<float4> dtab, dent;
        DevArray<RtCandHdr> dhdr;
        RT_HIP(dtab.reserve((size_t)n));
        RT_HIP(dent.reserve((size_t)n * RT_CAND_CAP));
        RT_HIP(dhdr.reserve((size_t)n));
        RT_HIP(hipMemcpy(dtab.get(), tab.data(), sizeof(float4) * (size_t)n, hipMemcpyHostToDevice));
        RT_HIP(rt_occluder_lists_launch(dtab.get(), n, p, dhdr.get(), dent.get(), nullptr));
        std::vector<RtCandHdr> hdr((size_t)n);
        RT_HIP(hipMemcpy(hdr.data(), dhdr.get(), sizeof(RtCandHdr) * (size_t)n, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) device_kbeam[i] = hdr[(size_t)i].kbeam;
    }
    return RT_OK;
}
extern "C" double rt_debug_sphere_beam_slope(const double lpos[3], const double centre[3], double r0)
{
    return rt_sphere_beam_slope(lpos, centre, r0);
}
extern "C" double rt_debug_beam_sine(const double lpos[3], const double start[3], double *sigma, double *frob, double m9[9])
{
    return rt_beam_sine_at_start(lpos, start, sigma, frob, m9);
}

// The same lists as the DEVICE builds them (rt_occluder_lists_launch: what the scene uses), downloaded: counts, kcaps and
// the first `cap` members of every list as list positions (device order = table order).
extern "C" int rt_debug_occluder_lists_device(const rt_sphere *spheres, int n, const rt_light *light, int *counts, float *kcaps, int *members, int cap)
{
    if (n <= 0 || !spheres || !light || !counts || !kcaps || (cap > 0 && !members)) return RT_ERR_INVALID;
    std::vector<float4> tab((size_t)n);
    pack_spheres(spheres, n, tab.data());
    DevArray<float4> dtab, dent;
    DevArray<RtCandHdr> dhdr;
    RT_HIP(dtab.reserve((size_t)n));
    RT_HIP(dent.reserve((size_t)n * RT_CAND_CAP));
    RT_HIP(dhdr.reserve((size_t)n));
    RT_HIP(hipMemcpy(dtab.get(), tab.data(), sizeof(float4) * (size_t)n, hipMemcpyHostToDevice));
    RT_HIP(hipMemset(dent.get(), 0, sizeof(float4) * (size_t)n * RT_CAND_CAP));
    const float p[3] = {light->pos.x, light->pos.y, light->pos.z};
    RT_HIP(rt_occluder_lists_launch(dtab.get(), n, p, dhdr.get(), dent.get(), nullptr));
    std::vector<RtCandHdr> hdr((size_t)n);
    std::vector<float4> ent((size_t)n * RT_CAND_CAP);
    RT_HIP(hipMemcpy(hdr.data(), dhdr.get(), sizeof(RtCandHdr) * (size_t)n, hipMemcpyDeviceToHost));
    RT_HIP(hipMemcpy(ent.data(), dent.get(), sizeof(float4) * ent.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {
        counts[i] = hdr[(size_t)i].count;
        kcaps[i] = hdr[(size_t)i].kcap;
        for (int k = 0; k < cap; ++k) members[(size_t)i * cap + k] = -1;
        for (int k = 0; k < hdr[(size_t)i].count && k < cap; ++k) {
            const float4 e = ent[(size_t)hdr[(size_t)i].offset + k];
            for (int j = 0; j < n; ++j)
                if (memcmp(&tab[(size_t)j], &e, sizeof e) == 0) { members[(size_t)i * cap + k] = j; break; }
        }
    }
    return RT_OK;
}

extern "C" int rt_debug_occluder_lists(const rt_sphere *spheres, int n, const rt_light *light, int *counts, float *kcaps, int *members, int cap)
{
    return rt_debug_occluder_lists_ex(spheres, n, light, counts, kcaps, members, cap, nullptr, nullptr);
}

extern "C" int rt_debug_intersect(const rt_sphere *spheres, const rt_ray *rays, int n, int *hit, float *t)
{
    if (n <= 0 || !spheres || !rays || !hit || !t) return RT_ERR_INVALID;
    std::vector<float4> tab(n);
    pack_spheres(spheres, n, tab.data());
    DevArray<float4> dtab;
    DevArray<float> drays, dt;
    DevArray<int> dhit;
    RT_HIP(dtab.reserve(n));
    RT_HIP(drays.reserve(6 * (size_t)n));
    RT_HIP(dt.reserve(n));
    RT_HIP(dhit.reserve(n));
    RT_HIP(hipMemcpy(dtab.get(), tab.data(), sizeof(float4) * n, hipMemcpyHostToDevice));
    RT_HIP(hipMemcpy(drays.get(), rays, sizeof(float) * 6 * n, hipMemcpyHostToDevice));
    RT_HIP(rt_dev_launch_dbg_intersect(dtab.get(), drays.get(), n, dhit.get(), dt.get(), nullptr));
    RT_HIP(hipMemcpy(hit, dhit.get(), sizeof(int) * n, hipMemcpyDeviceToHost));
    RT_HIP(hipMemcpy(t, dt.get(), sizeof(float) * n, hipMemcpyDeviceToHost));
    return RT_OK;
}

static int debug_light_impl(const rt_sphere *spheres, int n_spheres, const rt_vec3 *start,
                            const rt_vec3 *normal, const rt_light *light, int n, float *dirs,
                            float *brightness, float *approx_dirs, int *approx_ok)
{
    if (n <= 0 || n_spheres < 0 || !start || !normal || !light || !dirs || !brightness) return RT_ERR_INVALID;
    rt_scene sc;
    sc.lights[0] = *light;
    sc.n_lights = 1;
    RtFrameAux ax;
    rt_build_frame_aux(&sc, &ax);
    DevArray<RtFrameAux> dax;
    RT_HIP(dax.reserve(1));
    RT_HIP(hipMemcpy(dax.get(), &ax, sizeof ax, hipMemcpyHostToDevice));
    RtFrameConsts fc;
    memset(&fc, 0, sizeof fc);
    fc.n_lights = 1;
    fc.aux = dax.get();
    fc.n_spheres = n_spheres;
    std::vector<float4> tab(n_spheres ? n_spheres : 1);
    if (n_spheres) pack_spheres(spheres, n_spheres, tab.data());
    DevArray<float4> dtab;
    DevArray<float> dstart, dnormal, ddirs, dbright, dadirs;
    DevArray<int> daok;
    RT_HIP(dtab.reserve(tab.size()));
    RT_HIP(dstart.reserve(3 * (size_t)n));
    RT_HIP(dnormal.reserve(3 * (size_t)n));
    RT_HIP(ddirs.reserve(30 * (size_t)n));
    RT_HIP(dbright.reserve(n));
    RT_HIP(hipMemcpy(dtab.get(), tab.data(), sizeof(float4) * tab.size(), hipMemcpyHostToDevice));
    RT_HIP(hipMemcpy(dstart.get(), start, sizeof(float) * 3 * n, hipMemcpyHostToDevice));
    RT_HIP(hipMemcpy(dnormal.get(), normal, sizeof(float) * 3 * n, hipMemcpyHostToDevice));
    if (approx_dirs) {
        RT_HIP(dadirs.reserve(30 * (size_t)n));
        RT_HIP(daok.reserve(10 * (size_t)n));
    }
    RT_HIP(rt_dev_launch_dbg_light(&fc, dtab.get(), dstart.get(), dnormal.get(), 0, n, ddirs.get(), dbright.get(), approx_dirs ? dadirs.get() : nullptr,
                                   approx_dirs ? daok.get() : nullptr, nullptr));
    RT_HIP(hipMemcpy(dirs, ddirs.get(), sizeof(float) * 30 * n, hipMemcpyDeviceToHost));
    RT_HIP(hipMemcpy(brightness, dbright.get(), sizeof(float) * n, hipMemcpyDeviceToHost));
    if (approx_dirs) {
        RT_HIP(hipMemcpy(approx_dirs, dadirs.get(), sizeof(float) * 30 * n, hipMemcpyDeviceToHost));
        RT_HIP(hipMemcpy(approx_ok, daok.get(), sizeof(int) * 10 * n, hipMemcpyDeviceToHost));
    }
    return RT_OK;
}

extern "C" int rt_debug_light(const rt_sphere *spheres, int n_spheres, const rt_vec3 *start,
                              const rt_vec3 *normal, const rt_light *light, int n, float *dirs,
                              float *brightness)
{
    return debug_light_impl(spheres, n_spheres, start, normal, light, n, dirs, brightness, nullptr, nullptr);
}

// The exact sample directions next to the pre-pass's approximate ones (frame kernel: setup_approx / direction_approx)
// and the pre-pass's guard flags, for the error bound RT_PRE_DELTA (tests only).
extern "C" int rt_debug_light_prepass(const rt_vec3 *start, const rt_light *light, int n, float *dirs, float *approx_dirs, int *approx_ok)
{
    if (!approx_dirs || !approx_ok || n <= 0) return RT_ERR_INVALID;
    std::vector<rt_vec3> normal((size_t)n, rt_vec3{0.f, 1.f, 0.f});
    std::vector<float> bright((size_t)n);
    return debug_light_impl(nullptr, 0, start, normal.data(), light, n, dirs, bright.data(), approx_dirs, approx_ok);
}
