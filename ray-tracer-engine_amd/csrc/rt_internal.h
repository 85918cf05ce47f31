// rt_internal.h -- helpers shared by the host translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/rt_engine.h"
#include "rt_device.h"

void rt_set_error(const char *fmt, ...);
int rt_hip_fail(hipError_t e, const char *expr, const char *file, int line);

// For int-returning entry points: report, never exit.
#define RT_HIP(expr)                                                        \
    do {                                                                    \
        hipError_t rt_e_ = (expr);                                          \
        if (rt_e_ != hipSuccess) return rt_hip_fail(rt_e_, #expr, __FILE__, __LINE__); \
    } while (0)

// Owners of the host side's device buffers, pinned buffers, events and streams: each releases its resource when it is
// destroyed or reset. None of them waits for the device: whoever releases something a frame in flight may still use
// waits first, at the call site. They can be moved from but not assigned to (no release hides in an assignment), and
// nothing with static storage duration holds one (it would be released after the HIP runtime has gone).
template <typename T, bool Pinned>
class HipArray {
public:
    HipArray() = default;
    HipArray(HipArray &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    ~HipArray() { (void)reset(); }
    T *get() const { return p_; }
    size_t capacity() const { return cap_; }   // elements
    // Room for n elements: re-allocates only when n exceeds the capacity, and then keeps none of the old contents.
    // *grew (if given): whether it re-allocated.
    hipError_t reserve(size_t n, bool *grew = nullptr)
    {
        if (grew) *grew = false;
        if (n <= cap_) return hipSuccess;
        hipError_t e = reset();
        if (e == hipSuccess)
            e = Pinned ? hipHostMalloc((void **)&p_, sizeof(T) * n, hipHostMallocDefault) : hipMalloc((void **)&p_, sizeof(T) * n);
        if (e != hipSuccess) {
            p_ = nullptr;
            return e;
        }
        cap_ = n;
        if (grew) *grew = true;
        return hipSuccess;
    }
    hipError_t reset()
    {
        T *p = p_;
        p_ = nullptr;
        cap_ = 0;
        return p ? (Pinned ? hipHostFree(p) : hipFree(p)) : hipSuccess;
    }

private:
    T *p_ = nullptr;
    size_t cap_ = 0;
};
template <typename T> using DevArray = HipArray<T, false>;      // hipMalloc
template <typename T> using PinnedArray = HipArray<T, true>;    // hipHostMalloc

// An event or stream, made by the first create() (later calls do nothing).
template <typename H, hipError_t (*Destroy)(H)>
class HipHandle {
public:
    HipHandle() = default;
    HipHandle(HipHandle &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    ~HipHandle() { reset(); }
    H get() const { return h_; }
    void reset()
    {
        if (h_) (void)Destroy(h_);
        h_ = nullptr;
    }

protected:
    H h_ = nullptr;
};
struct HipEvent : HipHandle<hipEvent_t, hipEventDestroy> {
    hipError_t create(unsigned flags = hipEventDisableTiming) { return h_ ? hipSuccess : hipEventCreateWithFlags(&h_, flags); }
};
struct HipStream : HipHandle<hipStream_t, hipStreamDestroy> {
    hipError_t create(unsigned flags) { return h_ ? hipSuccess : hipStreamCreateWithFlags(&h_, flags); }
    hipError_t create(unsigned flags, int priority) { return h_ ? hipSuccess : hipStreamCreateWithPriority(&h_, flags, priority); }
};

// An event that may still be pending: recorded on one stream, and whatever must follow it -- on any stream, or on the
// host -- asks this owner instead of keeping a flag beside the event. Once the event has been seen complete nobody
// waits on it again.
class HipPendingEvent {
public:
    hipError_t record(hipStream_t stream)   // created on first use
    {
        hipError_t e = ev_.create();
        if (e == hipSuccess) e = hipEventRecord(ev_.get(), stream);
        if (e == hipSuccess) pending_ = true;
        return e;
    }
    // What `stream` does next follows the last record(): a device-side wait, and none once the event is complete.
    hipError_t order(hipStream_t stream)
    {
        if (!pending_) return hipSuccess;
        if (hipEventQuery(ev_.get()) == hipSuccess) {
            pending_ = false;
            return hipSuccess;
        }
        (void)hipGetLastError();   // "not ready" is reported as an error
        return hipStreamWaitEvent(stream, ev_.get(), 0);
    }
    hipError_t host_wait()
    {
        const hipError_t e = pending_ ? hipEventSynchronize(ev_.get()) : hipSuccess;
        if (e == hipSuccess) pending_ = false;
        return e;
    }
    bool pending() const { return pending_; }
    // *done: whether the last record() has completed; never waits. "Not ready" is the only answer taken for "no":
    // any other error of the query (or an earlier asynchronous one it reports) is returned.
    hipError_t complete(bool *done)
    {
        if (pending_) {
            const hipError_t e = hipEventQuery(ev_.get());
            if (e == hipSuccess) pending_ = false;
            else if (e == hipErrorNotReady) (void)hipGetLastError();
            else return e;
        }
        *done = !pending_;
        return hipSuccess;
    }

private:
    HipEvent ev_;
    bool pending_ = false;
};

struct rt_scene;
struct RtTableSlot;   // rt_scene.h

// which instantiation of the frame kernel renders a frame (rt_trace.inc: TW, CULL; rt_device.h: RtTraceMode, RtTraceFeat)
struct RtKernelChoice {
    int tile, cull, mode, feat;
};

int rt_scene_set_spheres_async(rt_scene *s, const rt_sphere *host_spheres, int n, hipStream_t stream);
// per-light tables, raygen tables, RtFrameAux: everything but the eye cones (may wait for frames in flight)
int rt_scene_prepare_static(rt_scene *s, const rt_frame_desc *fd, hipStream_t stream);
// pure host computation of the by-value uniforms; `cones`: the eye-cone table the frame reads, or null
int rt_build_frame_consts(const rt_scene *s, const rt_frame_desc *fd, const float4 *cones, RtFrameConsts *fc);
int rt_frame_kernel_choice(const rt_scene *s, const rt_frame_desc *fd, RtKernelChoice *kc);
void rt_ray_origin(const rt_frame_desc *fd, float org[3]);
// frames in flight (rt_scene.cpp): host wait for all of them; bookkeeping after a launch that read the scene's cached
// eye-cone table `cones`, view lists `views` and resting-view table `rest` (null: it read none of its own)
int rt_scene_quiesce(rt_scene *s);
int rt_scene_note_launch(rt_scene *s, hipStream_t stream, RtTableSlot *cones, RtTableSlot *views, RtTableSlot *rest);
// what a graph node needs from the scene
const float4 *rt_scene_sphere_table(const rt_scene *s);
int rt_scene_sphere_count(const rt_scene *s);
unsigned long long rt_scene_epoch(const rt_scene *s);
bool rt_scene_wants_eye_cones(const rt_scene *s, const float org[3]);
int rt_scene_tile_order_mode(const rt_scene *s);   // rt_scene_set_tile_order
// The view (block shape included) of a frame with uniforms fc, for the view-list builders; returns whether a launch of
// that tile width / cull / mode reads view lists at all (rt_scene_set_view_lists, nesting tiles).
struct RtViewParams;
int rt_view_params_for_frame(const rt_scene *s, const RtFrameConsts *fc, float aspect, int tile_w, int cull, int mode, RtViewParams *p);
int rt_scene_build_eye_cones_host(rt_scene *s, const float org[3], float4 *buf, hipStream_t stream);

// rt_shim.cpp: memManager::operator delete on something the shim has mirrored
void rt_shim_forget(const void *ptr);

// rt_mesh.cpp: the reference-layout mesh (triangles, leaf boxes with their own index arrays) flattened into the arrays
// the device reads -- pure host computation, validation of the leaves included
struct RtFlatMesh {
    std::vector<RtTriDev> tris;
    std::vector<RtBoxDev> boxes;     // {bounds, start, len} into idx
    std::vector<int> idx;
    std::vector<float> box_spheres;  // leaf spheres, padded to RT_BLOCK, then one per block of leaves
    std::vector<float> tri9;         // vertices per (leaf, triangle) pair, padded by 64 floats
    std::vector<float> tri_bs, tri_nrm;   // per pair: bounding sphere; unit normal and kappa
};
int rt_mesh_flatten(const rt_mesh *mesh, RtFlatMesh *out);

// launchers of rt_kernels.hip
extern "C" hipError_t rt_dev_trace_config(const RtFrameConsts *fc, int tile_w, int cull, int mode, int feat,
                                          const void **func, dim3 *grid, dim3 *block, unsigned *lds_bytes);
extern "C" hipError_t rt_dev_launch_trace(const RtFrameConsts *fc, const float4 *spheres, int tile_w, int cull, int mode,
                                          int feat, hipStream_t stream);
// ... with the 1-D grid of a compact reading launch (workgroups > 0: fc carries RT_FLAG_COMPACT and a table with a run
// list; rt_dev_trace_config knows no list and always gives the full grid)
extern "C" hipError_t rt_dev_launch_trace_grid(const RtFrameConsts *fc, const float4 *spheres, int tile_w, int cull, int mode,
                                               int feat, unsigned workgroups, hipStream_t stream);

// rt_sphere_bvh.cpp: the scene's sphere BVH (rt_bvh.h), shared by reflective frames and ray queries
struct RtSphereBvh;
bool rt_sphere_bvh_stale(const RtSphereBvh *b, unsigned long long sphere_gen, int n);
int rt_sphere_bvh_update(RtSphereBvh *b, const float4 *h_spheres, int n, unsigned long long sphere_gen, hipStream_t stream);

// rt_reflect.hip: mirror reflections (rt_launch_opts.reflect_depth) -- materials, queues, passes; it owns the scene's BVH
struct RtReflect;
RtReflect *rt_reflect_create();
void rt_reflect_destroy(RtReflect *r);
void rt_reflect_spheres_changed(RtReflect *r, int n_old, int n_new);
int rt_reflect_set_materials(RtReflect *r, const rt_material *m, int n, int n_spheres);
int rt_reflect_set_materials_ex(RtReflect *r, const rt_material_ex *m, int n, int n_spheres);
int rt_reflect_set_kind_materials(RtReflect *r, int which, const rt_material *m, int n, int n_list);   // which: 0 planes, 1 cubes
void rt_reflect_kind_list_changed(RtReflect *r, int which, int n_old, int n_new);
int rt_reflect_set_roughness(RtReflect *r, int kind, const float *rho, int n, int n_list);   // kind: RT_HIT_SPHERE / PLANE / CUBE
int rt_reflect_set_gloss_seed(RtReflect *r, unsigned seed);
int rt_reflect_set_glass_model(RtReflect *r, int model);   // RT_GLASS_PLAIN / RT_GLASS_FRESNEL
int rt_reflect_set_scope(RtReflect *r, int scope);
int rt_reflect_scope(const RtReflect *r);
int rt_reflect_set_samples(RtReflect *r, int mode);
int rt_reflect_samples(const RtReflect *r);
bool rt_reflect_needs_upload(const RtReflect *r, unsigned long long sphere_gen, int n);
int rt_reflect_prepare(RtReflect *r, const float4 *h_spheres, int n, unsigned long long sphere_gen, int npx,
                       bool need_rgba, float **rgba_scratch, hipStream_t stream);
// the scratch of a supersampled frame (rt_scene_set_reflect_samples): the pixel-samples of its largest group, which the
// queues and the slab must hold; the pixels of the running sum (0: one group, no sum); whether a buffer would be
// re-allocated for it
struct RtSamplesPlan {
    int entries, sum_px;
    bool grows;
};
int rt_reflect_samples_plan(const RtReflect *r, int n, int npx, RtSamplesPlan *plan);
int rt_reflect_prepare_samples(RtReflect *r, const RtSamplesPlan *plan);
int rt_reflect_begin_frame(RtReflect *r, int depth, int samples, hipStream_t stream);
int rt_reflect_mark_frame_start(RtReflect *r, hipStream_t stream);
int rt_reflect_launch(RtReflect *r, const RtFrameConsts *fc, const float4 *d_spheres, int n, int depth, bool brute,
                      hipStream_t stream);
int rt_reflect_launch_samples(RtReflect *r, const RtFrameConsts *fc, const RtFrameConsts *out, const RtKernelChoice *kc,
                              const float4 *d_spheres, int n, int depth, hipStream_t stream);
int rt_reflect_set_timing(RtReflect *r, int on);
int rt_reflect_get_stats(RtReflect *r, rt_reflect_stats *out);
enum { RT_REFLECT_DISPATCH_FIELDS = 7 };
void rt_reflect_dispatch(const RtReflect *r, int out[RT_REFLECT_DISPATCH_FIELDS]);   // r may be null
RtSphereBvh *rt_reflect_bvh(RtReflect *r);

// rt_query.hip: ray queries (q: validated, in this build's layout; bvh: null or current -- the list is walked then)
int rt_query_launch(const RtFrameConsts *fc, const RtSphereBvh *bvh, const float4 *d_spheres, int n_spheres,
                    const rt_ray_query *q, hipStream_t stream);
int rt_query_launch_primary(const RtFrameConsts *fc, rt_ray *rays, hipStream_t stream);

// opts.reflect_depth of a frame description, honouring the struct sizes (0 where the caller's structs end before it)
int rt_frame_reflect_depth(const rt_frame_desc *fd);
// the first G-buffer output (aov_*) a frame sets, by field name, or null: of a frame description in this build's
// layout, and of a caller's (honouring its struct sizes)
const char *rt_fd_aov_field(const rt_frame_desc *fd);
const char *rt_frame_aov_field(const rt_frame_desc *fd);
// a caller's frame description in this build's layout (what its struct_size fields do not cover reads as 0)
void normalise_frame_desc(const rt_frame_desc *fd, rt_frame_desc *out);

// rt_denoise.hip: the two a-trous denoisers, one set of kernels. Both public descriptions in one layout:
// rt_vdenoise_desc's fields, which rt_denoise_desc's are among, and which filter. `plain`: rt_scene_denoise's (a uniform
// colour threshold sigma_colour, none if it is <= 0; moments, variance_out, sigma_floor, min_history and spatial_boost
// are not read).
struct RtAtrousDesc : rt_vdenoise_desc {
    bool plain;
};
// d: validated; the scene's scratch, room for width * height pixels each; ev: null, or iterations + 2 timing events
int rt_denoise_launch(const RtAtrousDesc *d, float4 *col0, float4 *col1, float4 *guide, int *key, hipEvent_t *ev,
                      hipStream_t stream);
// the variance-guided one: lds16: step 16 runs the LDS-staged kernel; ev: null, or iterations + 3 timing events
int rt_vdenoise_launch(const RtAtrousDesc *d, float4 *col0, float4 *col1, float4 *guide, int *key, float *var0,
                       float *var1, bool lds16, hipEvent_t *ev, hipStream_t stream);

// rt_temporal.hip: temporal accumulation, both entries (d: validated, in this build's layout, for
// rt_scene_temporal with no motion table and no clamp; dx_tab / dy_tab: the current view's ray tables at one sample,
// needed with identical views too once an object moved; view[7] / prev_view[7]: rt_view_terms of the two views;
// same_view: they are the same bytes; ev: null, or two timing events)
int rt_temporal_launch(const rt_tmotion_desc *d, const float *dx_tab, const float *dy_tab, const float view[7],
                       const float prev_view[7], bool same_view, hipEvent_t *ev, hipStream_t stream);

// rt_upsample.hip: guided upsampling (d: validated, in this build's layout; ev: null, or two timing events)
int rt_upsample_launch(const rt_upsample_desc *d, hipEvent_t *ev, hipStream_t stream);

// rt_display.hip: the display transform (d: validated, in this build's layout; hist: the scene's
// RT_DISPLAY_BINS counters, cleared here on `stream`; table: rt_display_table() on the device; ev: null, or
// RT_DISPLAY_MAX_EVENTS timing events, of which *n_ev are recorded)
#define RT_DISPLAY_MAX_EVENTS 4
int rt_display_launch(const rt_display_desc *d, uint32_t *hist, const float *table, hipEvent_t *ev, int *n_ev, hipStream_t stream);
const float *rt_display_table();   // the 256 thresholds of the sRGB encoding (host)

// rt_bloom.hip: the bloom pass (d: validated, in this build's layout; pyramid: the scene's, room for
// rt_bloom_pyramid_texels(width, height, levels) float4; ev: null, or RT_BLOOM_MAX_EVENTS + 1 timing events, of which
// *n_ev are recorded: one ahead of the first launch, one behind each)
size_t rt_bloom_pyramid_texels(int width, int height, int levels);
int rt_bloom_launch(const rt_bloom_desc *d, float4 *pyramid, hipEvent_t *ev, int *n_ev, hipStream_t stream);

// rt_indirect.hip: the indirect pass. The product's scratch, all the scene's: per slot of a group of
// at most RT_INDIRECT_GROUP rays a colour (slab) and a queue entry, a running sum per pixel when there are several
// groups, and a counter per (group, bounce). Queue 0's entries are RT_INDIRECT_ENTRY_F4 float4; those of the later
// queues (bounces > 1) carry the throughput and the key in a fourth, and two buffers of that width ping-pong.
#define RT_INDIRECT_GROUP 4
#define RT_INDIRECT_MAX_GROUPS ((RT_INDIRECT_MAX_RAYS + RT_INDIRECT_GROUP - 1) / RT_INDIRECT_GROUP)
#define RT_INDIRECT_ENTRY_F4 3
#define RT_INDIRECT_PATH_ENTRY_F4 4
#define RT_INDIRECT_MAX_COUNTS (RT_INDIRECT_MAX_GROUPS * RT_INDIRECT_MAX_BOUNCES)
#define RT_INDIRECT_MAX_EVENTS (1 + (2 + RT_INDIRECT_MAX_BOUNCES) * RT_INDIRECT_MAX_GROUPS)
struct RtIndirectScratch {
    float4 *slab, *queue, *sum;
    int *count;
    float4 *queue2;   // bounces > 1 only
};
// Emission per primitive of a kind (rt_scene_set_emission): (r, g, b, 0) at the list position; null: the
// kind has no table
struct RtEmitDev {
    const float4 *sphere, *plane, *cube;
};
// whether `variant` runs the wavefront passes (and needs the scratch) in a call of `bounces`
bool rt_indirect_wavefront(int variant, int bounces = 1);
// d: validated, in this build's layout; fc: the view's uniforms (whole frame, one sample, the pass's own ray tables);
// bvh: null or current; ev: null, or RT_INDIRECT_MAX_EVENTS timing events, of which *n_ev are recorded; bounces: 1 is
// rt_scene_indirect itself; emit: null (no kind has a table: today's instantiations), or the tables, one of them at least
int rt_indirect_launch(const rt_indirect_desc *d, int bounces, const RtFrameConsts *fc, const RtSphereBvh *bvh,
                       const float4 *d_spheres, int n_spheres, const RtEmitDev *emit, const RtIndirectScratch *scratch,
                       hipEvent_t *ev, int *n_ev, hipStream_t stream);
