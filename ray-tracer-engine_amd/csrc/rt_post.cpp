// rt_post.cpp -- the host side of the post passes, which work on a frame's buffers and not on the scene's lists: the two
// a-trous denoisers, the two temporal passes, guided upsampling, the display transform, bloom and the two indirect
// passes. Every entry checks its description before anything is enqueued -- the `else if` chain of an entry is its
// specification -- and then runs inside one call frame, PostCall, which orders the call behind the pass's last one,
// hands the launch its timing events and records the pass's event (rt_scene.h, (d) and (f)).
#include <cmath>
#include <algorithm>

#include "rt_scene.h"

// ---------------------------------------------------------------------------
// what the entries share: the head of a call, the call frame, the timing entry points
// ---------------------------------------------------------------------------
// The caller's description in this build's layout; false: a null scene or description, refused under the entry's name
template <typename D>
static bool post_desc(const char *name, const rt_scene *s, const D *d_in, D *d)
{
    if (!s || !d_in) {
        rt_set_error("%s: null scene or description", name);
        return false;
    }
    as_built(d_in, d);
    return true;
}

static const char *const kBadSize = "width and height must be in [1, RT_DENOISE_MAX_SIZE]";
static bool size_ok(int w, int h) { return w > 0 && h > 0 && w <= RT_DENOISE_MAX_SIZE && h <= RT_DENOISE_MAX_SIZE; }
static bool positive(float v) { return v > 0.f && std::isfinite(v); }   // "finite and > 0"

// A post pass is not recorded into graphs: true (and the refusal, RT_ERR_UNSUPPORTED) if `stream` is being captured
static bool refuse_capture(const char *name, const char *what, hipStream_t stream)
{
    if (!stream_capturing(stream)) return false;
    rt_set_error("%s: the stream is being captured (the %s is not recorded into graphs)", name, what);
    return true;
}

// The frame of a call of entry e on `stream`, around its launch. Whoever grows the pass's scratch does so before
// begin(), after done.host_wait().
struct PostCall {
    PostCall(rt_scene *s, RtPostEntry e, hipStream_t stream) : timer(s->post_timer[e]), done(s->post_event[kPostOwner[e]]), stream(stream) {}
    // The stream follows the pass's last call (one scratch: one call at a time). With timing on, `events` are the
    // entry's first n for the launch to record, else null.
    int begin(int n)
    {
        RT_HIP(done.order(stream));
        timer.timed = 0;
        if (!timer.on) return RT_OK;
        for (int i = 0; i < n; ++i) {
            RT_HIP(timer.ev[i].create(hipEventDefault));
            ev[i] = timer.ev[i].get();
        }
        events = ev;
        return RT_OK;
    }
    // The launch's rc, behind the pass's event: recorded also after a launch that failed half way, since what was
    // enqueued uses the scratch. `recorded`: the events a launch that succeeded recorded.
    int end(int rc, int recorded)
    {
        RT_HIP(done.record(stream));
        if (rc == RT_OK && timer.on) timer.timed = recorded;
        return rc;
    }
    RtPostTimer &timer;
    HipPendingEvent &done;
    const hipStream_t stream;
    hipEvent_t *events = nullptr;
    hipEvent_t ev[RT_POST_MAX_EVENTS];
};

// The timing switch and the timings of every timed entry; rt_scene_set_<name>_timing and rt_scene_<name>_times
static const char *const kPostName[RT_POST_ENTRIES] = {"denoise", "vdenoise", "temporal", "upsample", "display", "bloom", "indirect"};

static int post_set_timing(rt_scene *s, RtPostEntry e, int on)
{
    if (!s) {
        rt_set_error("rt_scene_set_%s_timing: null scene", kPostName[e]);
        return RT_ERR_INVALID;
    }
    s->post_timer[e].on = on != 0;
    return RT_OK;
}

// ms[i]: between events i and i + 1 of those the entry's last timed call recorded, after the pass's event, which that
// call recorded behind its work
static int post_times(rt_scene *s, RtPostEntry e, float *ms, int cap, int *n)
{
    if (!s || !ms || !n || cap < 0) {
        rt_set_error("rt_scene_%s_times: null argument", kPostName[e]);
        return RT_ERR_INVALID;
    }
    const RtPostTimer &t = s->post_timer[e];
    *n = 0;
    if (t.timed < 2 || cap < 1) return RT_OK;
    RT_HIP(s->post_event[kPostOwner[e]].host_wait());
    for (int i = 0; i + 1 < t.timed && i < cap; ++i) {
        RT_HIP(hipEventElapsedTime(&ms[i], t.ev[i].get(), t.ev[i + 1].get()));
        *n = i + 1;
    }
    return RT_OK;
}

extern "C" int rt_scene_set_denoise_timing(rt_scene *s, int on) { return post_set_timing(s, RT_POST_DENOISE, on); }
extern "C" int rt_scene_denoise_times(rt_scene *s, float *ms, int cap, int *n) { return post_times(s, RT_POST_DENOISE, ms, cap, n); }
extern "C" int rt_scene_set_vdenoise_timing(rt_scene *s, int on) { return post_set_timing(s, RT_POST_VDENOISE, on); }
extern "C" int rt_scene_vdenoise_times(rt_scene *s, float *ms, int cap, int *n) { return post_times(s, RT_POST_VDENOISE, ms, cap, n); }
extern "C" int rt_scene_set_temporal_timing(rt_scene *s, int on) { return post_set_timing(s, RT_POST_TEMPORAL, on); }
extern "C" int rt_scene_temporal_times(rt_scene *s, float *ms, int cap, int *n) { return post_times(s, RT_POST_TEMPORAL, ms, cap, n); }
extern "C" int rt_scene_set_upsample_timing(rt_scene *s, int on) { return post_set_timing(s, RT_POST_UPSAMPLE, on); }
extern "C" int rt_scene_upsample_times(rt_scene *s, float *ms, int cap, int *n) { return post_times(s, RT_POST_UPSAMPLE, ms, cap, n); }
extern "C" int rt_scene_set_display_timing(rt_scene *s, int on) { return post_set_timing(s, RT_POST_DISPLAY, on); }
extern "C" int rt_scene_display_times(rt_scene *s, float *ms, int cap, int *n) { return post_times(s, RT_POST_DISPLAY, ms, cap, n); }
extern "C" int rt_scene_set_bloom_timing(rt_scene *s, int on) { return post_set_timing(s, RT_POST_BLOOM, on); }
extern "C" int rt_scene_bloom_times(rt_scene *s, float *ms, int cap, int *n) { return post_times(s, RT_POST_BLOOM, ms, cap, n); }
extern "C" int rt_scene_set_indirect_timing(rt_scene *s, int on) { return post_set_timing(s, RT_POST_INDIRECT, on); }
extern "C" int rt_scene_indirect_times(rt_scene *s, float *ms, int cap, int *n) { return post_times(s, RT_POST_INDIRECT, ms, cap, n); }

int RtRayTables::prepare(HipPendingEvent &done, int width, int height, float aspect_)
{
    if (tab.get() && w == width && h == height && memcmp(&aspect, &aspect_, sizeof aspect) == 0) return RT_OK;
    RT_HIP(done.host_wait());
    const size_t need = (size_t)width + (size_t)height;
    w = h = 0;                           // a reserve or an upload that fails leaves no stale match
    RT_HIP(tab.reserve(need));
    std::vector<float> host(need);
    rt_raygen_fill(width, height, aspect_, 1, host.data());
    RT_HIP(hipMemcpy(tab.get(), host.data(), sizeof(float) * need, hipMemcpyHostToDevice));
    w = width; h = height; aspect = aspect_;
    return RT_OK;
}

// A buffer that a post pass reads or writes (p: 0 if the call does not use it).
struct Range {
    uintptr_t p;
    size_t bytes;
};
// What the post passes refuse: `in_message` if an output overlaps an input, but for outs[0] being ins[alias] itself
// (alias < 0: no input may be written in place), or that two outputs overlap; null if neither.
template <size_t NOUT, size_t NIN>
static const char *overlap_message(const Range (&outs)[NOUT], const Range (&ins)[NIN], int alias, const char *in_message)
{
    auto overlap = [](const Range &a, const Range &b) { return a.p && b.p && a.p < b.p + b.bytes && b.p < a.p + a.bytes; };
    for (size_t i = 0; i < NOUT; ++i) {
        const char *bad = nullptr;
        for (size_t k = 0; k < NIN; ++k)
            if (overlap(outs[i], ins[k]) && !(i == 0 && (int)k == alias && outs[0].p == ins[k].p)) bad = in_message;
        for (size_t j = i + 1; j < NOUT; ++j)
            if (overlap(outs[i], outs[j])) bad = "two output buffers overlap";
        if (bad) return bad;
    }
    return nullptr;
}

// ---------------------------------------------------------------------------
// the two a-trous denoisers (rt_denoise.hip): the G-buffer-guided one and the variance-guided one
// (DESIGN.md 6j). One host path, denoise_call; each keeps its own timer
// ---------------------------------------------------------------------------
// Which kernel runs step 16 in the variance-guided variant 0 (variant 2 runs the other): the LDS-staged one (61 440 B),
// by the measurement of DESIGN.md 6j -- equal to the direct one at 3840 x 2160 (0.425 against 0.423 ms), 1.32 times
// faster at 960 x 540.
static const bool kVdenoiseLds16 = true;

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

extern "C" void rt_vdenoise_desc_init(rt_vdenoise_desc *d)
{
    if (!d) return;
    memset(d, 0, sizeof *d);
    d->struct_size = (uint32_t)sizeof *d;
    d->iterations = 4;
    d->normal_shift = 5;
    d->sigma_depth = 0.05f;
    d->sigma_colour = 4.f;
    d->sigma_floor = 0.015625f;
    d->min_history = 4;
    d->spatial_boost = 4.f;
    d->demodulate = 1;
}

// What the two public descriptions share, field by field (their layouts part after `pixels`); the rest is 0.
template <typename D>
static RtAtrousDesc atrous_desc(const D &d, bool plain)
{
    RtAtrousDesc a = {};
    a.struct_size = (uint32_t)sizeof(rt_vdenoise_desc);
    a.width = d.width; a.height = d.height;
    a.rgba_in = d.rgba_in;
    a.depth = d.depth; a.normal = d.normal; a.albedo = d.albedo; a.id = d.id;
    a.rgba_out = d.rgba_out;
    a.pixels = d.pixels;
    a.iterations = d.iterations;
    a.normal_shift = d.normal_shift;
    a.sigma_depth = d.sigma_depth;
    a.sigma_colour = d.sigma_colour;
    a.demodulate = d.demodulate;
    a.variant = d.variant;
    a.plain = plain;
    return a;
}

// Both denoise entries. d: in this build's layout (`name` for the messages). Only rt_scene_denoise_variance checks its
// buffers for overlaps.
static int denoise_call(rt_scene *s, const RtAtrousDesc &d, const char *name, hipStream_t stream)
{
    const char *bad = nullptr;
    if (!size_ok(d.width, d.height)) bad = kBadSize;
    else if (!d.rgba_in || !d.depth || !d.normal || !d.id || !d.rgba_out) bad = "rgba_in, depth, normal, id and rgba_out must not be NULL";
    else if (d.demodulate && !d.albedo) bad = "demodulate needs albedo";
    else if ((((uintptr_t)d.rgba_in | (uintptr_t)d.normal | (uintptr_t)d.albedo | (uintptr_t)d.rgba_out) & 15u) ||
             (((uintptr_t)d.id | (uintptr_t)d.moments) & 7u) ||
             (((uintptr_t)d.depth | (uintptr_t)d.pixels | (uintptr_t)d.variance_out) & 3u))
        bad = d.plain ? "rgba_in, normal, albedo and rgba_out must be 16-byte aligned, id 8-byte, depth and pixels 4-byte"
                      : "rgba_in, normal, albedo and rgba_out must be 16-byte aligned, id and moments 8-byte, depth, pixels and variance_out 4-byte";
    else if (d.iterations < 1 || d.iterations > RT_DENOISE_MAX_ITERATIONS) bad = "iterations is not in [1, RT_DENOISE_MAX_ITERATIONS]";
    else if (d.normal_shift < 0 || d.normal_shift > RT_DENOISE_MAX_NORMAL_SHIFT) bad = "normal_shift is not in [0, RT_DENOISE_MAX_NORMAL_SHIFT]";
    else if (!positive(d.sigma_depth)) bad = "sigma_depth is not finite and > 0";
    else if (d.plain && !std::isfinite(d.sigma_colour)) bad = "sigma_colour is not finite";
    else if (!d.plain && !(d.sigma_colour >= 0.f && d.sigma_colour <= 1048576.f)) bad = "sigma_colour is not in [0, 2^20]";
    else if (!d.plain && !positive(d.sigma_floor)) bad = "sigma_floor is not finite and > 0";
    else if (!d.plain && (d.min_history < 1 || d.min_history > RT_TEMPORAL_MAX_HISTORY)) bad = "min_history is not in [1, RT_TEMPORAL_MAX_HISTORY]";
    else if (!d.plain && (!(d.spatial_boost >= 0.f) || !std::isfinite(d.spatial_boost))) bad = "spatial_boost is not finite and >= 0";
    else if (d.variant < 0 || d.variant > 2) bad = "variant is not 0, 1 or 2";
    else if (!d.plain) {
        const size_t npx = (size_t)d.width * d.height;
        const Range outs[3] = {{(uintptr_t)d.rgba_out, npx * 16}, {(uintptr_t)d.pixels, npx * 4}, {(uintptr_t)d.variance_out, npx * 4}};
        const Range ins[6] = {{(uintptr_t)d.rgba_in, npx * 16}, {(uintptr_t)d.depth, npx * 4}, {(uintptr_t)d.normal, npx * 16},
                              {(uintptr_t)d.albedo, npx * 16}, {(uintptr_t)d.id, npx * 8}, {(uintptr_t)d.moments, npx * 8}};
        bad = overlap_message(outs, ins, 0, "an output buffer overlaps an input (only rgba_out may be rgba_in itself)");
    }
    if (bad) {
        if (d.plain)
            rt_set_error("%s: %s (%d x %d, iterations %d, normal_shift %d, variant %d)", name, bad, d.width, d.height, d.iterations,
                         d.normal_shift, d.variant);
        else
            rt_set_error("%s: %s (%d x %d, iterations %d, normal_shift %d, min_history %d, variant %d)", name, bad, d.width,
                         d.height, d.iterations, d.normal_shift, d.min_history, d.variant);
        return RT_ERR_INVALID;
    }
    if (refuse_capture(name, "denoiser", stream)) return RT_ERR_UNSUPPORTED;
    // one scratch for both entries; each has its timing state: rt_scene_denoise_times reports the last plain call,
    // whatever came after it
    PostCall call(s, d.plain ? RT_POST_DENOISE : RT_POST_VDENOISE, stream);
    const size_t npx = (size_t)d.width * d.height;
    if (npx > s->dn_col[0].capacity() || npx > s->dn_col[1].capacity() ||
        (!d.plain && (npx > s->vd_var[0].capacity() || npx > s->vd_var[1].capacity())) ||
        (d.variant != 1 && (npx > s->dn_guide.capacity() || npx > s->dn_key.capacity()))) {
        // growing releases the old buffers: after the host has seen the last call that used them end
        RT_HIP(call.done.host_wait());
        RT_HIP(s->dn_col[0].reserve(npx));
        RT_HIP(s->dn_col[1].reserve(npx));
        if (!d.plain) {
            RT_HIP(s->vd_var[0].reserve(npx));
            RT_HIP(s->vd_var[1].reserve(npx));
        }
        if (d.variant != 1) {
            RT_HIP(s->dn_guide.reserve(npx));
            RT_HIP(s->dn_key.reserve(npx));
        }
    }
    // events beside one per iteration: before the first launch, after the pack (not in variant 1), after the variance's
    // spatial estimate / v_0
    const int extra = d.plain ? 2 : 3;
    int rc = call.begin(RT_DENOISE_MAX_ITERATIONS + extra);
    if (rc != RT_OK) return rc;
    rc = d.plain ? rt_denoise_launch(&d, s->dn_col[0].get(), s->dn_col[1].get(), s->dn_guide.get(), s->dn_key.get(), call.events, stream)
                 : rt_vdenoise_launch(&d, s->dn_col[0].get(), s->dn_col[1].get(), s->dn_guide.get(), s->dn_key.get(),
                                      s->vd_var[0].get(), s->vd_var[1].get(), (d.variant == 2) != kVdenoiseLds16, call.events, stream);
    return call.end(rc, d.iterations + extra - (d.variant == 1 ? 1 : 0));
}

extern "C" int rt_scene_denoise(rt_scene *s, const rt_denoise_desc *d_in, void *stream_)
{
    rt_denoise_desc d;
    if (!post_desc("rt_scene_denoise", s, d_in, &d)) return RT_ERR_INVALID;
    return denoise_call(s, atrous_desc(d, true), "rt_scene_denoise", (hipStream_t)stream_);
}

extern "C" int rt_scene_denoise_variance(rt_scene *s, const rt_vdenoise_desc *d_in, void *stream_)
{
    rt_vdenoise_desc d;
    if (!post_desc("rt_scene_denoise_variance", s, d_in, &d)) return RT_ERR_INVALID;
    RtAtrousDesc a = atrous_desc(d, false);
    a.moments = d.moments;
    a.variance_out = d.variance_out;
    a.sigma_floor = d.sigma_floor;
    a.min_history = d.min_history;
    a.spatial_boost = d.spatial_boost;
    return denoise_call(s, a, "rt_scene_denoise_variance", (hipStream_t)stream_);
}

// ---------------------------------------------------------------------------
// temporal accumulation (rt_temporal.hip)
// ---------------------------------------------------------------------------
extern "C" void rt_temporal_desc_init(rt_temporal_desc *d)
{
    if (!d) return;
    memset(d, 0, sizeof *d);
    d->struct_size = (uint32_t)sizeof *d;
    d->max_history = 32;
    d->depth_tolerance = 0.02f;
    d->normal_cos_min = 0.9f;
}

extern "C" int rt_view_terms(int width, int height, float aspect, const rt_camera *cam, float out[7])
{
    if (!cam || !out || width <= 0 || height <= 0) {
        rt_set_error("rt_view_terms: null camera or output, or a size <= 0");
        return RT_ERR_INVALID;
    }
    rt_frame_desc fd;
    memset(&fd, 0, sizeof fd);
    fd.width = width; fd.height = height;
    fd.aspect = aspect;
    fd.cam = *cam;
    RtFrameConsts fc;
    rt_ray_origin(&fd, out);
    rt_view_rotation(&fd, &fc);
    out[3] = fc.cos_pitch; out[4] = fc.sin_pitch; out[5] = fc.cos_yaw; out[6] = fc.sin_yaw;
    return RT_OK;
}

// rt_tmotion_desc repeats rt_temporal_desc's fields: one description, one set of checks and one host path serve both
static_assert(offsetof(rt_tmotion_desc, variant) == offsetof(rt_temporal_desc, variant) &&
                  offsetof(rt_tmotion_desc, rgba_in) == offsetof(rt_temporal_desc, rgba_in) &&
                  offsetof(rt_tmotion_desc, pixels) == offsetof(rt_temporal_desc, pixels),
              "rt_tmotion_desc must begin with rt_temporal_desc's fields");
constexpr size_t kTemporalShared = offsetof(rt_temporal_desc, variant) + sizeof(int);

// Both temporal entries. d: in this build's layout; motion: rt_scene_temporal_motion (`name` for the messages).
static int temporal_call(rt_scene *s, const rt_tmotion_desc &d, bool motion, const char *name, hipStream_t stream)
{
    const bool reset = d.reset != 0;
    const char *bad = nullptr;
    if (!size_ok(d.width, d.height)) bad = kBadSize;
    else if (!d.rgba_in || !d.depth || !d.normal || !d.id || !d.rgba_out) bad = "rgba_in, depth, normal, id and rgba_out must not be NULL";
    else if (!reset && (!d.prev_rgba || !d.prev_depth || !d.prev_normal || !d.prev_id))
        bad = "prev_rgba, prev_depth, prev_normal and prev_id must not be NULL without reset";
    else if (!reset && d.moments_out && !d.prev_moments) bad = "moments_out needs prev_moments without reset";
    else if ((((uintptr_t)d.rgba_in | (uintptr_t)d.normal | (uintptr_t)d.rgba_out) & 15u) ||
             (((uintptr_t)d.id | (uintptr_t)d.moments_out) & 7u) || (((uintptr_t)d.depth | (uintptr_t)d.pixels) & 3u) ||
             (!reset && ((((uintptr_t)d.prev_rgba | (uintptr_t)d.prev_normal) & 15u) ||
                         (((uintptr_t)d.prev_id | (uintptr_t)d.prev_moments) & 7u) || ((uintptr_t)d.prev_depth & 3u))))
        bad = "rgba and normal buffers must be 16-byte aligned, id and moments 8-byte, depth and pixels 4-byte";
    else if (d.max_history < 1 || d.max_history > RT_TEMPORAL_MAX_HISTORY) bad = "max_history is not in [1, RT_TEMPORAL_MAX_HISTORY]";
    else if (!positive(d.depth_tolerance)) bad = "depth_tolerance is not finite and > 0";
    else if (!(d.normal_cos_min >= 0.f && d.normal_cos_min <= 1.f)) bad = "normal_cos_min is not in [0, 1]";
    else if (d.variant < 0 || d.variant > 1) bad = "variant is not 0 or 1";
    else if (!positive(d.aspect) || (!reset && !positive(d.prev_aspect))) bad = "aspect and prev_aspect must be finite and > 0";
    else if (motion && (d.n_sphere_motion < 0 || d.n_cube_motion < 0)) bad = "n_sphere_motion and n_cube_motion must not be negative";
    else if (motion && ((d.n_sphere_motion > 0 && !d.sphere_motion) || (d.n_cube_motion > 0 && !d.cube_motion)))
        bad = "a motion count > 0 needs its array";
    else if (motion && (((uintptr_t)d.sphere_motion | (uintptr_t)d.cube_motion) & 15u)) bad = "sphere_motion and cube_motion must be 16-byte aligned";
    else if (motion && !(d.clamp_slack >= 0.f && d.clamp_slack <= 16.f)) bad = "clamp_slack is not in [0, 16]";
    else if (motion && (d.clamp_history < 1 || d.clamp_history > RT_TEMPORAL_MAX_HISTORY)) bad = "clamp_history is not in [1, RT_TEMPORAL_MAX_HISTORY]";
    else {
        // the pass gathers: an output that overlaps an input (or another output) would be read after it was written
        const size_t npx = (size_t)d.width * d.height;
        const Range outs[3] = {{(uintptr_t)d.rgba_out, npx * 16}, {(uintptr_t)d.moments_out, npx * 8}, {(uintptr_t)d.pixels, npx * 4}};
        const Range ins[11] = {{(uintptr_t)d.rgba_in, npx * 16}, {(uintptr_t)d.depth, npx * 4}, {(uintptr_t)d.normal, npx * 16},
                               {(uintptr_t)d.id, npx * 8},
                               {reset ? 0 : (uintptr_t)d.prev_rgba, npx * 16}, {reset ? 0 : (uintptr_t)d.prev_depth, npx * 4},
                               {reset ? 0 : (uintptr_t)d.prev_normal, npx * 16}, {reset ? 0 : (uintptr_t)d.prev_id, npx * 8},
                               {reset ? 0 : (uintptr_t)d.prev_moments, npx * 8},
                               {d.n_sphere_motion > 0 ? (uintptr_t)d.sphere_motion : 0, (size_t)d.n_sphere_motion * 16},
                               {d.n_cube_motion > 0 ? (uintptr_t)d.cube_motion : 0, (size_t)d.n_cube_motion * 16}};
        bad = overlap_message(outs, ins, -1, "an output buffer overlaps an input (the pass gathers: it cannot run in place)");
    }
    if (bad) {
        rt_set_error("%s: %s (%d x %d, max_history %d, variant %d)", name, bad, d.width, d.height, d.max_history, d.variant);
        return RT_ERR_INVALID;
    }
    if (refuse_capture(name, "pass", stream)) return RT_ERR_UNSUPPORTED;
    float view[7], prev_view[7];
    rt_view_terms(d.width, d.height, d.aspect, &d.cam, view);
    const bool same_view = !reset && memcmp(&d.cam, &d.prev_cam, sizeof d.cam) == 0 && memcmp(&d.aspect, &d.prev_aspect, sizeof d.aspect) == 0;
    if (reset) memcpy(prev_view, view, sizeof view);
    else rt_view_terms(d.width, d.height, d.prev_aspect, &d.prev_cam, prev_view);
    // with identical views only a pixel of a moved object is reprojected
    const bool need_rays = !reset && (!same_view || d.n_sphere_motion > 0 || d.n_cube_motion > 0);
    PostCall call(s, RT_POST_TEMPORAL, stream);
    int rc = need_rays ? s->tp_rays.prepare(call.done, d.width, d.height, d.aspect) : RT_OK;
    if (rc == RT_OK) rc = call.begin(2);
    if (rc != RT_OK) return rc;
    rc = rt_temporal_launch(&d, need_rays ? s->tp_rays.dx() : nullptr, need_rays ? s->tp_rays.dy() : nullptr, view, prev_view,
                            same_view, call.events, stream);
    return call.end(rc, 2);
}

extern "C" int rt_scene_temporal(rt_scene *s, const rt_temporal_desc *d_in, void *stream_)
{
    rt_temporal_desc td;
    if (!post_desc("rt_scene_temporal", s, d_in, &td)) return RT_ERR_INVALID;
    rt_tmotion_desc d;
    memset(&d, 0, sizeof d);
    memcpy(&d, &td, kTemporalShared);      // no motion, no clamp
    d.struct_size = (uint32_t)sizeof d;
    return temporal_call(s, d, false, "rt_scene_temporal", (hipStream_t)stream_);
}

extern "C" void rt_tmotion_desc_init(rt_tmotion_desc *d)
{
    if (!d) return;
    memset(d, 0, sizeof *d);
    d->struct_size = (uint32_t)sizeof *d;
    d->max_history = 32;
    d->depth_tolerance = 0.02f;
    d->normal_cos_min = 0.9f;
    d->clamp = 1;
    d->clamp_slack = 0.25f;
    d->clamp_history = 4;
}

extern "C" int rt_scene_temporal_motion(rt_scene *s, const rt_tmotion_desc *d_in, void *stream_)
{
    rt_tmotion_desc d;
    if (!post_desc("rt_scene_temporal_motion", s, d_in, &d)) return RT_ERR_INVALID;
    return temporal_call(s, d, true, "rt_scene_temporal_motion", (hipStream_t)stream_);
}

// ---------------------------------------------------------------------------
// guided upsampling (rt_upsample.hip)
// ---------------------------------------------------------------------------
extern "C" void rt_upsample_desc_init(rt_upsample_desc *d)
{
    if (!d) return;
    memset(d, 0, sizeof *d);
    d->struct_size = (uint32_t)sizeof *d;
    d->normal_shift = 5;
    d->sigma_depth = 0.05f;
    d->demodulate = 1;
}

extern "C" int rt_scene_upsample(rt_scene *s, const rt_upsample_desc *d_in, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    rt_upsample_desc d;
    if (!post_desc("rt_scene_upsample", s, d_in, &d)) return RT_ERR_INVALID;
    const char *bad = nullptr;
    if (!size_ok(d.width, d.height) || d.lo_width <= 0 || d.lo_height <= 0) bad = "the sizes must be in [1, RT_DENOISE_MAX_SIZE]";
    else if (d.lo_width > d.width || d.lo_height > d.height) bad = "the lo size must not exceed the hi size";
    else if (!d.rgba_lo || !d.depth_lo || !d.normal_lo || !d.id_lo || !d.depth || !d.normal || !d.id || !d.rgba_out)
        bad = "rgba_lo, depth_lo, normal_lo, id_lo, depth, normal, id and rgba_out must not be NULL";
    else if (d.demodulate && (!d.albedo || !d.albedo_lo)) bad = "demodulate needs albedo and albedo_lo";
    else if ((((uintptr_t)d.rgba_lo | (uintptr_t)d.normal_lo | (uintptr_t)d.albedo_lo | (uintptr_t)d.normal | (uintptr_t)d.albedo |
               (uintptr_t)d.base | (uintptr_t)d.rgba_out) & 15u) ||
             (((uintptr_t)d.id_lo | (uintptr_t)d.id) & 7u) ||
             (((uintptr_t)d.depth_lo | (uintptr_t)d.depth | (uintptr_t)d.pixels) & 3u))
        bad = "rgba, normal, albedo and base buffers must be 16-byte aligned, id 8-byte, depth and pixels 4-byte";
    else if (d.normal_shift < 0 || d.normal_shift > RT_DENOISE_MAX_NORMAL_SHIFT) bad = "normal_shift is not in [0, RT_DENOISE_MAX_NORMAL_SHIFT]";
    else if (!positive(d.sigma_depth)) bad = "sigma_depth is not finite and > 0";
    else if (d.variant < 0 || d.variant > 1) bad = "variant is not 0 or 1";
    else if (d.n_sphere_select < 0 || d.n_plane_select < 0 || d.n_cube_select < 0) bad = "a table's count must not be negative";
    else if ((d.n_sphere_select > 0 && !d.sphere_select) || (d.n_plane_select > 0 && !d.plane_select) ||
             (d.n_cube_select > 0 && !d.cube_select))
        bad = "a count > 0 needs its table";
    else {
        const size_t npx = (size_t)d.width * d.height, nlo = (size_t)d.lo_width * d.lo_height;
        const Range outs[3] = {{(uintptr_t)d.rgba_out, npx * 16}, {(uintptr_t)d.pixels, npx * 4}, {(uintptr_t)d.source, npx}};
        const Range ins[13] = {{(uintptr_t)d.rgba_lo, nlo * 16}, {(uintptr_t)d.depth_lo, nlo * 4}, {(uintptr_t)d.normal_lo, nlo * 16},
                               {(uintptr_t)d.albedo_lo, nlo * 16}, {(uintptr_t)d.id_lo, nlo * 8},
                               {(uintptr_t)d.depth, npx * 4}, {(uintptr_t)d.normal, npx * 16}, {(uintptr_t)d.albedo, npx * 16},
                               {(uintptr_t)d.id, npx * 8}, {(uintptr_t)d.base, npx * 16},
                               {d.n_sphere_select > 0 ? (uintptr_t)d.sphere_select : 0, (size_t)d.n_sphere_select},
                               {d.n_plane_select > 0 ? (uintptr_t)d.plane_select : 0, (size_t)d.n_plane_select},
                               {d.n_cube_select > 0 ? (uintptr_t)d.cube_select : 0, (size_t)d.n_cube_select}};
        bad = overlap_message(outs, ins, 9, "an output buffer overlaps an input (only rgba_out may be base itself)");
    }
    if (bad) {
        rt_set_error("rt_scene_upsample: %s (%d x %d from %d x %d, normal_shift %d, variant %d)", bad, d.width, d.height,
                     d.lo_width, d.lo_height, d.normal_shift, d.variant);
        return RT_ERR_INVALID;
    }
    if (refuse_capture("rt_scene_upsample", "pass", stream)) return RT_ERR_UNSUPPORTED;
    PostCall call(s, RT_POST_UPSAMPLE, stream);
    const int rc = call.begin(2);
    if (rc != RT_OK) return rc;
    return call.end(rt_upsample_launch(&d, call.events, stream), 2);
}

// ---------------------------------------------------------------------------
// the display transform (rt_display.hip)
// ---------------------------------------------------------------------------
extern "C" void rt_display_desc_init(rt_display_desc *d)
{
    if (!d) return;
    memset(d, 0, sizeof *d);
    d->struct_size = (uint32_t)sizeof *d;
    d->meter = RT_DISPLAY_METER_AUTO;
    d->exposure = 1.f;
    d->key = 0.18f;
    d->min_exposure = 0.015625f;
    d->max_exposure = 64.f;
    d->meter_low = 512;
    d->meter_high = 973;
    d->adapt = 1.f;
    d->curve = RT_DISPLAY_ACES;
    d->white = 4.f;
    d->transfer = RT_DISPLAY_SRGB;
}

extern "C" int rt_display_transfer_table(float out[256])
{
    if (!out) {
        rt_set_error("rt_display_transfer_table: null table");
        return RT_ERR_INVALID;
    }
    memcpy(out, rt_display_table(), 256 * sizeof(float));
    return RT_OK;
}

extern "C" int rt_scene_display(rt_scene *s, const rt_display_desc *d_in, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    rt_display_desc d;
    if (!post_desc("rt_scene_display", s, d_in, &d)) return RT_ERR_INVALID;
    const bool meter = d.meter != RT_DISPLAY_METER_MANUAL;
    const char *bad = nullptr;
    if (!size_ok(d.width, d.height)) bad = kBadSize;
    else if (d.meter < RT_DISPLAY_METER_MANUAL || d.meter > RT_DISPLAY_METER_LAGGED) bad = "meter is not RT_DISPLAY_METER_MANUAL, _AUTO or _LAGGED";
    else if (d.curve < RT_DISPLAY_CLIP || d.curve > RT_DISPLAY_ACES) bad = "curve is not RT_DISPLAY_CLIP, _REINHARD or _ACES";
    else if (d.transfer < RT_DISPLAY_LINEAR || d.transfer > RT_DISPLAY_SRGB) bad = "transfer is not RT_DISPLAY_LINEAR or _SRGB";
    else if (d.variant < 0 || d.variant > 1) bad = "variant is not 0 or 1";
    else if (!d.rgba_in) bad = "rgba_in must not be NULL";
    else if (meter && !d.state) bad = "state must not be NULL unless meter is RT_DISPLAY_METER_MANUAL";
    else if (!meter && !d.rgba_out && !d.pixels) bad = "rgba_out and pixels are both NULL and meter is RT_DISPLAY_METER_MANUAL: nothing to do";
    else if ((uintptr_t)d.rgba_in & 15u) bad = "rgba_in must be 16-byte aligned";
    else if ((uintptr_t)d.rgba_out & 15u) bad = "rgba_out must be 16-byte aligned";
    else if (meter && ((uintptr_t)d.state & 15u)) bad = "state must be 16-byte aligned";
    else if (meter && ((uintptr_t)d.id & 7u)) bad = "id must be 8-byte aligned";
    else if ((uintptr_t)d.pixels & 3u) bad = "pixels must be 4-byte aligned";
    else if (meter && ((uintptr_t)d.histogram_out & 3u)) bad = "histogram_out must be 4-byte aligned";
    else if (!positive(d.exposure)) bad = "exposure is not finite and > 0";
    else if (!positive(d.key)) bad = "key is not finite and > 0";
    else if (!positive(d.min_exposure)) bad = "min_exposure is not finite and > 0";
    else if (!positive(d.max_exposure)) bad = "max_exposure is not finite and > 0";
    else if (d.min_exposure > d.max_exposure) bad = "min_exposure exceeds max_exposure";
    else if (d.meter_low < 0 || d.meter_low >= d.meter_high || d.meter_high > 1024) bad = "meter_low and meter_high are not 0 <= low < high <= 1024";
    else if (!(d.adapt > 0.f && d.adapt <= 1.f)) bad = "adapt is not in (0, 1]";
    else if (!positive(d.white)) bad = "white is not finite and > 0";
    else {
        // what MANUAL does not touch is in no one's way
        const size_t npx = (size_t)d.width * d.height;
        const Range outs[4] = {{(uintptr_t)d.rgba_out, npx * 16}, {(uintptr_t)d.pixels, npx * 4},
                               {meter ? (uintptr_t)d.state : 0, 16}, {meter ? (uintptr_t)d.histogram_out : 0, RT_DISPLAY_BINS * 4}};
        const Range ins[2] = {{(uintptr_t)d.rgba_in, npx * 16}, {meter ? (uintptr_t)d.id : 0, npx * 8}};
        bad = overlap_message(outs, ins, 0, "an output buffer (rgba_out, pixels, state, histogram_out) overlaps rgba_in or id (only rgba_out may be rgba_in itself)");
        if (bad && !strncmp(bad, "two", 3)) bad = "two of rgba_out, pixels, state and histogram_out overlap";
    }
    if (bad) {
        rt_set_error("rt_scene_display: %s (%d x %d, meter %d, curve %d, transfer %d, variant %d)", bad, d.width, d.height, d.meter,
                     d.curve, d.transfer, d.variant);
        return RT_ERR_INVALID;
    }
    if (refuse_capture("rt_scene_display", "pass", stream)) return RT_ERR_UNSUPPORTED;
    // the scratch: the histogram's counters, then the thresholds, which never change
    if (!s->dp_scratch.get()) {
        RT_HIP(s->dp_scratch.reserve(RT_DISPLAY_BINS + 256));
        const hipError_t e = hipMemcpy(s->dp_scratch.get() + RT_DISPLAY_BINS, rt_display_table(), 256 * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)s->dp_scratch.reset();
            RT_HIP(e);
        }
    }
    PostCall call(s, RT_POST_DISPLAY, stream);
    int rc = call.begin(RT_DISPLAY_MAX_EVENTS);
    if (rc != RT_OK) return rc;
    int n_ev = 0;
    rc = rt_display_launch(&d, s->dp_scratch.get(), (const float *)(s->dp_scratch.get() + RT_DISPLAY_BINS), call.events, &n_ev, stream);
    return call.end(rc, n_ev);
}

// ---------------------------------------------------------------------------
// the bloom pass (rt_bloom.hip)
// ---------------------------------------------------------------------------
extern "C" void rt_bloom_desc_init(rt_bloom_desc *d)
{
    if (!d) return;
    memset(d, 0, sizeof *d);
    d->struct_size = (uint32_t)sizeof *d;
    d->levels = 5;
    d->threshold = 1.f;
    d->limit = 64.f;
    d->spread = 0.75f;
    d->strength = 0.125f;
}

extern "C" int rt_scene_bloom(rt_scene *s, const rt_bloom_desc *d_in, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    rt_bloom_desc d;
    if (!post_desc("rt_scene_bloom", s, d_in, &d)) return RT_ERR_INVALID;
    const char *bad = nullptr;
    if (!size_ok(d.width, d.height)) bad = kBadSize;
    else if (d.levels < 1 || d.levels > RT_BLOOM_MAX_LEVELS) bad = "levels is not in [1, RT_BLOOM_MAX_LEVELS]";
    else if (d.variant < 0 || d.variant > 1) bad = "variant is not 0 or 1";
    else if (!d.rgba_in) bad = "rgba_in must not be NULL";
    else if (!d.rgba_out && !d.pixels && !d.glow_out) bad = "rgba_out, pixels and glow_out are all NULL: nothing to do";
    else if ((uintptr_t)d.rgba_in & 15u) bad = "rgba_in must be 16-byte aligned";
    else if ((uintptr_t)d.state & 15u) bad = "state must be 16-byte aligned";
    else if ((uintptr_t)d.rgba_out & 15u) bad = "rgba_out must be 16-byte aligned";
    else if ((uintptr_t)d.pixels & 3u) bad = "pixels must be 4-byte aligned";
    else if ((uintptr_t)d.glow_out & 15u) bad = "glow_out must be 16-byte aligned";
    else if (!(d.threshold >= 0.f) || !std::isfinite(d.threshold)) bad = "threshold is not finite and >= 0";
    else if (!positive(d.limit)) bad = "limit is not finite and > 0";
    else if (!(d.spread >= 0.f && d.spread <= 4.f)) bad = "spread is not in [0, 4]";
    else if (!(d.strength >= 0.f) || !std::isfinite(d.strength)) bad = "strength is not finite and >= 0";
    else {
        const size_t npx = (size_t)d.width * d.height;
        const Range outs[3] = {{(uintptr_t)d.rgba_out, npx * 16}, {(uintptr_t)d.pixels, npx * 4}, {(uintptr_t)d.glow_out, npx * 16}};
        const Range ins[2] = {{(uintptr_t)d.rgba_in, npx * 16}, {(uintptr_t)d.state, 16}};
        bad = overlap_message(outs, ins, 0, "an output buffer (rgba_out, pixels, glow_out) overlaps rgba_in or state (only rgba_out may be rgba_in itself)");
        if (bad && !strncmp(bad, "two", 3)) bad = "two of rgba_out, pixels and glow_out overlap";
    }
    if (bad) {
        rt_set_error("rt_scene_bloom: %s (%d x %d, levels %d, variant %d)", bad, d.width, d.height, d.levels, d.variant);
        return RT_ERR_INVALID;
    }
    if (refuse_capture("rt_scene_bloom", "pass", stream)) return RT_ERR_UNSUPPORTED;
    PostCall call(s, RT_POST_BLOOM, stream);
    const size_t need = rt_bloom_pyramid_texels(d.width, d.height, d.levels);
    if (need > s->bl_pyramid.capacity()) {
        // growing releases the old pyramid: after the host has seen the last call that used it end
        RT_HIP(call.done.host_wait());
        RT_HIP(s->bl_pyramid.reserve(need));
    }
    int rc = call.begin(RT_BLOOM_MAX_EVENTS + 1);
    if (rc != RT_OK) return rc;
    int n_ev = 0;
    rc = rt_bloom_launch(&d, s->bl_pyramid.get(), call.events, &n_ev, stream);
    return call.end(rc, n_ev);
}

// ---------------------------------------------------------------------------
// global illumination with a bounce budget (rt_indirect.hip)
// ---------------------------------------------------------------------------
extern "C" void rt_indirect_desc_init(rt_indirect_desc *d)
{
    if (!d) return;
    memset(d, 0, sizeof *d);
    d->struct_size = (uint32_t)sizeof *d;
    d->rays = 1;
    d->strength = 1.f;
    d->cull = -1;
}

// The host path of both entries: `name` is the entry's, bounces == 1 is rt_scene_indirect itself
static int indirect_call(rt_scene *s, const rt_indirect_desc *d_in, int bounces, const char *name, hipStream_t stream)
{
    rt_indirect_desc d;
    if (!post_desc(name, s, d_in, &d)) return RT_ERR_INVALID;
    const char *bad = nullptr;
    if (!size_ok(d.width, d.height)) bad = kBadSize;
    else if (!positive(d.aspect)) bad = "aspect is not finite and > 0";
    else if (!d.depth || !d.normal || !d.id || !d.rgba_out) bad = "depth, normal, id and rgba_out must not be NULL";
    else if ((((uintptr_t)d.normal | (uintptr_t)d.albedo | (uintptr_t)d.rgba_in | (uintptr_t)d.rgba_out) & 15u) ||
             ((uintptr_t)d.id & 7u) || (((uintptr_t)d.depth | (uintptr_t)d.pixels) & 3u))
        bad = "normal, albedo, rgba_in and rgba_out must be 16-byte aligned, id 8-byte, depth and pixels 4-byte";
    else if (d.rays < 1 || d.rays > RT_INDIRECT_MAX_RAYS) bad = "rays is not in [1, RT_INDIRECT_MAX_RAYS]";
    else if (d.ray_base < 0 || d.ray_base > (1 << 24) - d.rays) bad = "ray_base is negative, or ray_base + rays exceeds 1 << 24";
    else if (!(d.strength >= 0.f) || !std::isfinite(d.strength)) bad = "strength is not finite and >= 0";
    else if (d.cull < -1 || d.cull > 1) bad = "cull is not -1, 0 or 1";
    else if (d.variant < 0 || d.variant > 1) bad = "variant is not 0 or 1";
    else {
        const size_t npx = (size_t)d.width * d.height;
        const Range outs[2] = {{(uintptr_t)d.rgba_out, npx * 16}, {(uintptr_t)d.pixels, npx * 4}};
        const Range ins[5] = {{(uintptr_t)d.rgba_in, npx * 16}, {(uintptr_t)d.depth, npx * 4}, {(uintptr_t)d.normal, npx * 16},
                              {(uintptr_t)d.id, npx * 8}, {(uintptr_t)d.albedo, npx * 16}};
        bad = overlap_message(outs, ins, 0, "an output buffer overlaps an input (only rgba_out may be rgba_in itself)");
    }
    if (!bad) {   // SHADE's own conditions
        if (!s->have_sky) bad = "the scene has no sky";
        else if ((s->n_spheres > 0 || s->n_planes > 0 || s->n_cubes > 0 || s->n_boxes > 0) && (!s->d_tex[0].get() || s->tex_w <= 0))
            bad = "the scene has primitives but no texture";
    }
    if (bad) {
        rt_set_error("%s: %s (%d x %d)", name, bad, d.width, d.height);
        return RT_ERR_INVALID;
    }
    const bool wavefront = rt_indirect_wavefront(d.variant, bounces);
    const size_t npx = (size_t)d.width * d.height;
    const size_t slots = (size_t)std::min(d.rays, RT_INDIRECT_GROUP) * npx;   // of the largest group
    if (wavefront && slots > (size_t)0x7fffffff - (size_t)2048 * 256) {
        rt_set_error("%s: %d rays of %d x %d pixels per pass exceed the queue's index range", name,
                     std::min(d.rays, RT_INDIRECT_GROUP), d.width, d.height);
        return RT_ERR_CAPACITY;
    }
    if (refuse_capture(name, "pass", stream)) return RT_ERR_UNSUPPORTED;
    PostCall call(s, RT_POST_INDIRECT, stream);
    RT_HIP(s->stage_done.order(stream));
    int rc = rt_scene_sync_aux(s);
    if (rc != RT_OK) return rc;
    const RtSphereBvh *bvh = nullptr;
    if (d.cull != 0 && s->n_spheres > 0) {   // the shared BVH, as rt_scene_trace_rays handles it
        RtSphereBvh *b = rt_reflect_bvh(rt_scene_reflect(s));
        if (rt_sphere_bvh_stale(b, s->sphere_gen, s->n_spheres)) {
            rc = rt_scene_quiesce(s);
            if (rc != RT_OK) return rc;
            rc = rt_sphere_bvh_update(b, s->h_prev.data(), s->n_spheres, s->sphere_gen, stream);
            if (rc != RT_OK) return rc;
        }
        rc = rt_scene_wait_all_frames(s, stream);
        if (rc != RT_OK) return rc;
        bvh = b;
    }
    rc = s->ind_rays.prepare(call.done, d.width, d.height, d.aspect);   // the view's ray tables at one sample
    if (rc != RT_OK) return rc;
    const int groups = (d.rays + RT_INDIRECT_GROUP - 1) / RT_INDIRECT_GROUP;
    if (wavefront) {
        const size_t sum_px = groups > 1 ? npx : 0;
        // paths: two queues of the wider entry, which ping-pong
        const size_t q1 = slots * (bounces > 1 ? RT_INDIRECT_PATH_ENTRY_F4 : RT_INDIRECT_ENTRY_F4), q2 = bounces > 1 ? q1 : 0;
        if (slots > s->ind_slab.capacity() || q1 > s->ind_queue.capacity() || q2 > s->ind_queue2.capacity() ||
            sum_px > s->ind_sum.capacity() || (size_t)RT_INDIRECT_MAX_COUNTS > s->ind_count.capacity()) {
            // growing releases the old buffers: after the host has seen the last call that used them end
            RT_HIP(call.done.host_wait());
            RT_HIP(s->ind_slab.reserve(slots));
            RT_HIP(s->ind_queue.reserve(q1));
            RT_HIP(s->ind_queue2.reserve(q2));
            RT_HIP(s->ind_sum.reserve(sum_px));
            RT_HIP(s->ind_count.reserve(RT_INDIRECT_MAX_COUNTS));
        }
    }
    rt_frame_desc fd;
    memset(&fd, 0, sizeof fd);
    fd.struct_size = (uint32_t)sizeof fd;
    fd.opts.struct_size = (uint32_t)sizeof fd.opts;
    fd.width = d.width; fd.height = d.height;
    fd.aspect = d.aspect;
    fd.cam = d.cam;
    fd.pixels = reinterpret_cast<uint32_t *>(d.rgba_out);   // (rt_build_frame_consts wants an output; the kernels read none of fc's)
    RtFrameConsts fc;
    rc = rt_build_frame_consts(s, &fd, nullptr, &fc);
    if (rc != RT_OK) return rc;
    fc.dx_tab = s->ind_rays.dx();
    fc.dy_tab = s->ind_rays.dy();
    fc.packed = nullptr;
    rc = call.begin(RT_INDIRECT_MAX_EVENTS);
    if (rc != RT_OK) return rc;
    // the emission tables that changed: on this stream, so behind every indirect call in flight and ahead of this one
    // (a table that grows releases the old buffer: after the host has seen those calls end)
    RtEmitDev emit{};
    for (RtEmitTable &t : s->emit) {
        if (!t.dirty) continue;
        if (t.v.size() > t.d.capacity()) RT_HIP(call.done.host_wait());
        t.v_dev = t.v;
        if (!t.v_dev.empty()) {
            RT_HIP(t.d.reserve(t.v_dev.size()));
            RT_HIP(hipMemcpyAsync(t.d.get(), t.v_dev.data(), sizeof(float4) * t.v_dev.size(), hipMemcpyHostToDevice, stream));
        }
        t.dirty = false;
    }
    emit.sphere = s->emit[0].dev();
    emit.plane = s->emit[1].dev();
    emit.cube = s->emit[2].dev();
    const bool any_emit = emit.sphere || emit.plane || emit.cube;
    const RtIndirectScratch scratch{s->ind_slab.get(), s->ind_queue.get(), s->ind_sum.get(), s->ind_count.get(), s->ind_queue2.get()};
    int n_ev = 0;
    rc = rt_indirect_launch(&d, bounces, &fc, bvh, s->d_spheres.get(), s->n_spheres, any_emit ? &emit : nullptr, &scratch,
                            call.events, &n_ev, stream);
    rc = call.end(rc, n_ev);
    if (rc != RT_OK) return rc;
    s->ind_counts = wavefront ? groups * bounces : 0;
    s->ind_bounces = bounces;
    return rt_scene_note_launch(s, stream, nullptr, nullptr, nullptr);   // the pass in flight counts as a frame
}

extern "C" int rt_scene_indirect(rt_scene *s, const rt_indirect_desc *d, void *stream)
{
    return indirect_call(s, d, 1, "rt_scene_indirect", (hipStream_t)stream);
}

extern "C" void rt_indirect_paths_opts_init(rt_indirect_paths_opts *o)
{
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->struct_size = (uint32_t)sizeof *o;
    o->bounces = 2;
}

extern "C" int rt_scene_indirect_paths(rt_scene *s, const rt_indirect_desc *d, const rt_indirect_paths_opts *o_in, void *stream)
{
    rt_indirect_paths_opts o;
    rt_indirect_paths_opts_init(&o);
    if (o_in) {   // fields past the caller's size keep their defaults
        const size_t have = o_in->struct_size ? std::min((size_t)o_in->struct_size, sizeof o) : sizeof o;
        if (have >= offsetof(rt_indirect_paths_opts, bounces) + sizeof o.bounces) o.bounces = o_in->bounces;
    }
    if (o.bounces < 1 || o.bounces > RT_INDIRECT_MAX_BOUNCES) {
        rt_set_error("rt_scene_indirect_paths: bounces is not in [1, RT_INDIRECT_MAX_BOUNCES] (%d)", o.bounces);
        return RT_ERR_INVALID;
    }
    return indirect_call(s, d, o.bounces, "rt_scene_indirect_paths", (hipStream_t)stream);
}

// The last call's counters, if it was of the entry's kind (paths: bounces > 1); else none
static int indirect_counts(rt_scene *s, const char *name, bool paths, int *counts, int cap, int *n)
{
    if (!s || !counts || !n || cap < 0) {
        rt_set_error("%s: null argument", name);
        return RT_ERR_INVALID;
    }
    *n = (s->ind_bounces > 1) == paths ? std::min(cap, s->ind_counts) : 0;
    if (*n == 0) return RT_OK;
    RT_HIP(s->post_event[RT_OWNER_INDIRECT].host_wait());
    RT_HIP(hipMemcpy(counts, s->ind_count.get(), sizeof(int) * (size_t)*n, hipMemcpyDeviceToHost));
    return RT_OK;
}

extern "C" int rt_debug_indirect_counts(rt_scene *s, int *counts, int cap, int *n)
{
    return indirect_counts(s, "rt_debug_indirect_counts", false, counts, cap, n);
}

extern "C" int rt_debug_indirect_path_counts(rt_scene *s, int *counts, int cap, int *n)
{
    return indirect_counts(s, "rt_debug_indirect_path_counts", true, counts, cap, n);
}
