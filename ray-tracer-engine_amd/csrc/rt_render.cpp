// rt_render.cpp -- what a launch does: a caller's descriptions in this build's layout, the by-value frame uniforms,
// the kernel choice, and the entry points that enqueue work on the scene -- frames, ray queries, the denoiser, temporal accumulation.
//
// Reference interface replaced here:
//   rayTrace<<<...>>> launch     /root/reference/kernel.cu:1615, 1780-1783
//
// There is no CPU fallback: every render entry point needs a gfx950 device and
// fails with RT_ERR_NO_DEVICE / RT_ERR_HIP otherwise.
#include <cmath>
#include <algorithm>

#include "rt_math.h"
#include "rt_scene.h"

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

// camera::rotateDir, kernel.cu:249-250
void rt_view_rotation(const rt_frame_desc *fd, RtFrameConsts *fc)
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
    rt_view_rotation(fd, fc);

    fc->tex_r = s->d_tex[0].get(); fc->tex_g = s->d_tex[1].get(); fc->tex_b = s->d_tex[2].get();
    fc->tex_w = s->tex_w; fc->tex_h = s->tex_h;
    fc->tex_mu_x = rt_texel_margin(s->tex_w, 5.0e-7f);   // RT_UV_DELTA of rt_kernels.hip
    fc->tex_mu_y = rt_texel_margin(s->tex_h, 5.0e-7f);
    {
        const int n_pad = rt_pad64(s->n_spheres);
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

// The layout before rt_launch_opts.reflect_depth was appended: what struct_size 0 reads as.
static const size_t kOptsSizeV1 = offsetof(rt_launch_opts, reflect_depth);
static const size_t kFrameSizeV1 = offsetof(rt_frame_desc, opts) + kOptsSizeV1;

// A caller's versioned struct in this build's layout: what its struct_size (0: `size0`) does not cover reads as 0.
// Returns the bytes taken from the caller.
template <typename T>
static size_t as_built(const T *in, T *out, size_t size0 = sizeof(T))
{
    memset(out, 0, sizeof *out);
    const size_t sz = std::min<size_t>(in->struct_size ? in->struct_size : size0, sizeof *out);
    memcpy(out, in, sz);
    out->struct_size = (uint32_t)sizeof *out;
    return sz;
}

// A frame description as this build lays it out, from a caller's that may be older (shorter): the options end where
// the frame's struct_size or their own does.
void normalise_frame_desc(const rt_frame_desc *fd, rt_frame_desc *out)
{
    const size_t fsz = as_built(fd, out, kFrameSizeV1);
    const size_t have = fsz > offsetof(rt_frame_desc, opts) ? fsz - offsetof(rt_frame_desc, opts) : 0;
    size_t osz = out->opts.struct_size ? out->opts.struct_size : kOptsSizeV1;
    if (osz > have) osz = have;
    if (osz < sizeof out->opts) memset(reinterpret_cast<char *>(&out->opts) + osz, 0, sizeof out->opts - osz);
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
    const bool spheres_only = !s->refl || rt_reflect_scope(s->refl.get()) == RT_REFLECT_SPHERES;
    const bool many = s->refl && rt_reflect_samples(s->refl.get()) == RT_REFLECT_SAMPLES_MANY;
    if (spheres_only && (s->n_planes > 0 || s->n_cubes > 0 || s->n_boxes > 0))
        why = "planes, cubes or a mesh in the scene (rt_scene_set_reflect_scope(RT_REFLECT_SCENE) lifts this)";
    else if (!many && (o.spp > 1 || o.sample_base != 0 || o.sample_total > 1))
        why = "more than one sample per pixel (rt_scene_set_reflect_samples(RT_REFLECT_SAMPLES_MANY) lifts this)";
    else if (!many && o.accumulate) why = "accumulate (rt_scene_set_reflect_samples(RT_REFLECT_SAMPLES_MANY) lifts this)";
    else if (o.interleave_count > 1 || o.interleave_index != 0 || o.interleave_rows != 0) why = "interleave_*";
    else if (o.packed24) why = "packed24";
    else if (o.table_lds) why = "table_lds";
    else if (o.profile) why = "profile";
    if (why) {
        rt_set_error("rt_scene_render: reflect_depth > 0 does not support %s (%s, plain outputs)", why,
                     many ? "samples through spp / accumulate" : "one sample");
        return RT_ERR_UNSUPPORTED;
    }
    return RT_OK;
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
    if (stream_capturing(stream)) {
        rt_set_error("rt_scene_render: the stream is being captured; use rt_graph_capture, which records the frame as graph nodes");
        return RT_ERR_UNSUPPORTED;
    }
    RT_HIP(s->stage_done.order(stream));   // a sphere-table upload enqueued on some stream precedes this launch
    int rc = rt_scene_prepare_static(s, fd, stream);
    if (rc != RT_OK) return rc;
    int slot = -1;
    if (fd->opts.cull != 0) {
        float org[3];
        rt_ray_origin(fd, org);
        rc = rt_scene_prepare_eye(s, org, stream, &slot);
        if (rc != RT_OK) return rc;
    }
    if (slot >= 0) RT_HIP(rt_scene_order_reader(s->cones[slot], stream));   // the table's build (table stream) precedes its readers
    RtFrameConsts fc;
    rc = rt_build_frame_consts(s, fd, slot >= 0 ? s->cones[slot].buf.get() : nullptr, &fc);
    if (rc != RT_OK) return rc;
    RtKernelChoice kc;
    rc = rt_frame_kernel_choice(s, fd, &kc);
    if (rc != RT_OK) return rc;
    if (fc.local_rows == 0) return RT_OK;   // this rank owns no rows of the frame
    // A supersampled reflective frame (rt_scene_set_reflect_samples): anything but the request a
    // one-sample frame serves, which runs as it always has. `out` keeps the caller's outputs and sample range for the
    // resolve pass; fc becomes one sample of the frame, which the frame kernel renders into the scene's scratch.
    const rt_launch_opts &o = fd->opts;
    const bool samples = reflect_depth > 0 && s->refl && rt_reflect_samples(s->refl.get()) == RT_REFLECT_SAMPLES_MANY &&
                         !(fc.spp == 1 && fc.sample_total == 1.f && o.sample_base == 0 && !o.accumulate && o.resolve != -1);
    const RtFrameConsts out = fc;
    const int npx = fc.width * fc.local_rows;
    RtSamplesPlan plan{npx, 0, false};   // the queues hold the band's pixels, or the pixel-samples of a group
    if (samples) {
        rc = rt_reflect_samples_plan(s->refl.get(), out.spp, npx, &plan);   // (too large: refused before anything is built)
        if (rc != RT_OK) return rc;
        fc.spp = 1;
        fc.flags &= ~(RT_FLAG_ACCUMULATE | RT_FLAG_RESOLVE);
        fc.packed = nullptr;
    }
    int view = -1;
    rc = rt_scene_prepare_view(s, fd, kc, slot, &fc, stream, &view);
    if (rc != RT_OK) return rc;
    if (reflect_depth > 0) {
        // the queues, the BVH and the materials are the scene's: after every frame launched so far (a host wait only
        // when the BVH or the materials change)
        RtReflect *refl = rt_scene_reflect(s);
        // (a host wait too when the samples' scratch is re-allocated)
        if (plan.grows || rt_reflect_needs_upload(refl, s->sphere_gen, s->n_spheres)) {
            rc = rt_scene_quiesce(s);
            if (rc != RT_OK) return rc;
        }
        rc = rt_scene_wait_all_frames(s, stream);
        if (rc != RT_OK) return rc;
        float *scratch = nullptr;
        rc = rt_reflect_prepare(refl, s->h_prev.data(), s->n_spheres, s->sphere_gen, plan.entries, !samples && fc.rgba == nullptr,
                                &scratch, stream);
        if (rc != RT_OK) return rc;
        if (samples) {
            rc = rt_reflect_prepare_samples(refl, &plan);
            if (rc != RT_OK) return rc;
        } else if (!fc.rgba) {
            fc.rgba = scratch;
        }
        rc = rt_reflect_begin_frame(refl, reflect_depth, samples ? out.spp : 0, stream);
        if (rc != RT_OK) return rc;
    }
    if (s->tile_order_mode != 0) {
        rc = rt_scene_prepare_tile_order(s, kc, &fc, stream);
        if (rc != RT_OK) return rc;
    }
    // the resting-view table: the plain one-sample frame of a sphere scene (not a reflective frame, whose passes follow)
    int rest = -1;
    rc = rt_scene_prepare_rest(s, kc, &fc, reflect_depth == 0 && kc.mode == 0 && kc.feat == 0 && kc.cull && fc.spp == 1, stream, &rest);
    if (rc != RT_OK) return rc;
    if (samples) {   // the frame kernel per sample, the passes per group, the resolve pass
        rc = rt_reflect_launch_samples(s->refl.get(), &fc, &out, &kc, s->d_spheres.get(), s->n_spheres, reflect_depth, stream);
        if (rc != RT_OK) return rc;
    } else {
        if (reflect_depth > 0) {
            rc = rt_reflect_mark_frame_start(s->refl.get(), stream);
            if (rc != RT_OK) return rc;
        }
        RT_HIP(rt_dev_launch_trace(&fc, s->d_spheres.get(), kc.tile, kc.cull, kc.mode, kc.feat, stream));
        if (reflect_depth > 0) {
            rc = rt_reflect_launch(s->refl.get(), &fc, s->d_spheres.get(), s->n_spheres, reflect_depth, kc.cull == 0, stream);
            if (rc != RT_OK) return rc;
        }
    }
    s->view_last = view;
    rc = rt_scene_end_rest(s, rest, stream);
    if (rc != RT_OK) return rc;
    return rt_scene_note_launch(s, stream, slot >= 0 ? &s->cones[slot] : nullptr, view >= 0 ? &s->views[view] : nullptr,
                                rest >= 0 ? &s->rest[rest] : nullptr);
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
    rt_ray_query q;
    as_built(q_in, &q);
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
    RT_HIP(s->stage_done.order(stream));
    int rc = rt_scene_sync_aux(s);
    if (rc != RT_OK) return rc;
    const RtSphereBvh *bvh = nullptr;
    if (q.cull != 0 && s->n_spheres > 0) {
        // the BVH is shared with reflective frames: rebuilt (after a host wait for every reader) only when the list
        // changed, and read after whatever frame uploaded it last
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
    return rt_scene_note_launch(s, stream, nullptr, nullptr, nullptr);   // a query in flight counts as a frame
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
    return rt_scene_note_launch(s, stream, nullptr, nullptr, nullptr);   // it reads the raygen tables
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
// (DESIGN.md 6j). One host path, denoise_call; each keeps its own timing state
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
    if (d.width <= 0 || d.height <= 0 || d.width > RT_DENOISE_MAX_SIZE || d.height > RT_DENOISE_MAX_SIZE)
        bad = "width and height must be in [1, RT_DENOISE_MAX_SIZE]";
    else if (!d.rgba_in || !d.depth || !d.normal || !d.id || !d.rgba_out) bad = "rgba_in, depth, normal, id and rgba_out must not be NULL";
    else if (d.demodulate && !d.albedo) bad = "demodulate needs albedo";
    else if ((((uintptr_t)d.rgba_in | (uintptr_t)d.normal | (uintptr_t)d.albedo | (uintptr_t)d.rgba_out) & 15u) ||
             (((uintptr_t)d.id | (uintptr_t)d.moments) & 7u) ||
             (((uintptr_t)d.depth | (uintptr_t)d.pixels | (uintptr_t)d.variance_out) & 3u))
        bad = d.plain ? "rgba_in, normal, albedo and rgba_out must be 16-byte aligned, id 8-byte, depth and pixels 4-byte"
                      : "rgba_in, normal, albedo and rgba_out must be 16-byte aligned, id and moments 8-byte, depth, pixels and variance_out 4-byte";
    else if (d.iterations < 1 || d.iterations > RT_DENOISE_MAX_ITERATIONS) bad = "iterations is not in [1, RT_DENOISE_MAX_ITERATIONS]";
    else if (d.normal_shift < 0 || d.normal_shift > RT_DENOISE_MAX_NORMAL_SHIFT) bad = "normal_shift is not in [0, RT_DENOISE_MAX_NORMAL_SHIFT]";
    else if (!(d.sigma_depth > 0.f) || !std::isfinite(d.sigma_depth)) bad = "sigma_depth is not finite and > 0";
    else if (d.plain && !std::isfinite(d.sigma_colour)) bad = "sigma_colour is not finite";
    else if (!d.plain && !(d.sigma_colour >= 0.f && d.sigma_colour <= 1048576.f)) bad = "sigma_colour is not in [0, 2^20]";
    else if (!d.plain && (!(d.sigma_floor > 0.f) || !std::isfinite(d.sigma_floor))) bad = "sigma_floor is not finite and > 0";
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
    if (stream_capturing(stream)) {
        rt_set_error("%s: the stream is being captured (the denoiser is not recorded into graphs)", name);
        return RT_ERR_UNSUPPORTED;
    }
    const size_t npx = (size_t)d.width * d.height;
    if (npx > s->dn_col[0].capacity() || npx > s->dn_col[1].capacity() ||
        (!d.plain && (npx > s->vd_var[0].capacity() || npx > s->vd_var[1].capacity())) ||
        (d.variant != 1 && (npx > s->dn_guide.capacity() || npx > s->dn_key.capacity()))) {
        // growing releases the old buffers: after the host has seen the last call that used them end
        RT_HIP(s->dn_done.host_wait());
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
    RT_HIP(s->dn_done.order(stream));   // one scratch for both entries: one call at a time
    // each entry has its timing state: rt_scene_denoise_times reports the last plain call, whatever came after it
    HipEvent *const timer = d.plain ? s->dn_ev : s->vd_ev;
    const bool timing = d.plain ? s->dn_timing : s->vd_timing;
    int &timed = d.plain ? s->dn_timed : s->vd_timed;
    // events beside one per iteration: before the first launch, after the pack (not in variant 1), after the variance's
    // spatial estimate / v_0
    const int extra = d.plain ? 2 : 3;
    hipEvent_t ev[RT_DENOISE_MAX_ITERATIONS + 3];
    timed = 0;
    if (timing) {
        for (int i = 0; i < RT_DENOISE_MAX_ITERATIONS + extra; ++i) {
            RT_HIP(timer[i].create(hipEventDefault));
            ev[i] = timer[i].get();
        }
    }
    const int rc = d.plain ? rt_denoise_launch(&d, s->dn_col[0].get(), s->dn_col[1].get(), s->dn_guide.get(), s->dn_key.get(),
                                               timing ? ev : nullptr, stream)
                           : rt_vdenoise_launch(&d, s->dn_col[0].get(), s->dn_col[1].get(), s->dn_guide.get(), s->dn_key.get(),
                                                s->vd_var[0].get(), s->vd_var[1].get(), (d.variant == 2) != kVdenoiseLds16,
                                                timing ? ev : nullptr, stream);
    // also after a launch that failed half way: what was enqueued uses the scratch
    RT_HIP(s->dn_done.record(stream));
    if (rc == RT_OK && timing) timed = d.iterations + extra - (d.variant == 1 ? 1 : 0);
    return rc;
}

extern "C" int rt_scene_denoise(rt_scene *s, const rt_denoise_desc *d_in, void *stream_)
{
    if (!s || !d_in) {
        rt_set_error("rt_scene_denoise: null scene or description");
        return RT_ERR_INVALID;
    }
    rt_denoise_desc d;
    as_built(d_in, &d);
    return denoise_call(s, atrous_desc(d, true), "rt_scene_denoise", (hipStream_t)stream_);
}

extern "C" int rt_scene_denoise_variance(rt_scene *s, const rt_vdenoise_desc *d_in, void *stream_)
{
    if (!s || !d_in) {
        rt_set_error("rt_scene_denoise_variance: null scene or description");
        return RT_ERR_INVALID;
    }
    rt_vdenoise_desc d;
    as_built(d_in, &d);
    RtAtrousDesc a = atrous_desc(d, false);
    a.moments = d.moments;
    a.variance_out = d.variance_out;
    a.sigma_floor = d.sigma_floor;
    a.min_history = d.min_history;
    a.spatial_boost = d.spatial_boost;
    return denoise_call(s, a, "rt_scene_denoise_variance", (hipStream_t)stream_);
}

// The timing switch and the timings of every post pass (`name` for the messages).
static int pass_set_timing(rt_scene *s, const char *name, bool rt_scene::*timing, int on)
{
    if (!s) {
        rt_set_error("%s: null scene", name);
        return RT_ERR_INVALID;
    }
    s->*timing = on != 0;
    return RT_OK;
}

// ms[i]: between events i and i + 1 of the `timed` events the entry's last timed call recorded; done: what that call
// recorded behind its work
static int pass_times(rt_scene *s, const char *name, HipPendingEvent rt_scene::*done, const HipEvent *ev, int timed, float *ms,
                      int cap, int *n)
{
    if (!s || !ms || !n || cap < 0) {
        rt_set_error("%s: null argument", name);
        return RT_ERR_INVALID;
    }
    *n = 0;
    if (timed < 2 || cap < 1) return RT_OK;
    RT_HIP((s->*done).host_wait());
    for (int i = 0; i + 1 < timed && i < cap; ++i) {
        RT_HIP(hipEventElapsedTime(&ms[i], ev[i].get(), ev[i + 1].get()));
        *n = i + 1;
    }
    return RT_OK;
}

extern "C" int rt_scene_set_denoise_timing(rt_scene *s, int on)
{
    return pass_set_timing(s, "rt_scene_set_denoise_timing", &rt_scene::dn_timing, on);
}

extern "C" int rt_scene_denoise_times(rt_scene *s, float *ms, int cap, int *n)
{
    return pass_times(s, "rt_scene_denoise_times", &rt_scene::dn_done, s ? s->dn_ev : nullptr, s ? s->dn_timed : 0, ms, cap, n);
}

extern "C" int rt_scene_set_vdenoise_timing(rt_scene *s, int on)
{
    return pass_set_timing(s, "rt_scene_set_vdenoise_timing", &rt_scene::vd_timing, on);
}

extern "C" int rt_scene_vdenoise_times(rt_scene *s, float *ms, int cap, int *n)
{
    return pass_times(s, "rt_scene_vdenoise_times", &rt_scene::dn_done, s ? s->vd_ev : nullptr, s ? s->vd_timed : 0, ms, cap, n);
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
    if (d.width <= 0 || d.height <= 0 || d.width > RT_DENOISE_MAX_SIZE || d.height > RT_DENOISE_MAX_SIZE)
        bad = "width and height must be in [1, RT_DENOISE_MAX_SIZE]";
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
    else if (!(d.depth_tolerance > 0.f) || !std::isfinite(d.depth_tolerance)) bad = "depth_tolerance is not finite and > 0";
    else if (!(d.normal_cos_min >= 0.f && d.normal_cos_min <= 1.f)) bad = "normal_cos_min is not in [0, 1]";
    else if (d.variant < 0 || d.variant > 1) bad = "variant is not 0 or 1";
    else if (!(d.aspect > 0.f) || !std::isfinite(d.aspect) || (!reset && (!(d.prev_aspect > 0.f) || !std::isfinite(d.prev_aspect))))
        bad = "aspect and prev_aspect must be finite and > 0";
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
    if (stream_capturing(stream)) {
        rt_set_error("%s: the stream is being captured (the pass is not recorded into graphs)", name);
        return RT_ERR_UNSUPPORTED;
    }
    float view[7], prev_view[7];
    rt_view_terms(d.width, d.height, d.aspect, &d.cam, view);
    const bool same_view = !reset && memcmp(&d.cam, &d.prev_cam, sizeof d.cam) == 0 && memcmp(&d.aspect, &d.prev_aspect, sizeof d.aspect) == 0;
    if (reset) memcpy(prev_view, view, sizeof view);
    else rt_view_terms(d.width, d.height, d.prev_aspect, &d.prev_cam, prev_view);
    // with identical views only a pixel of a moved object is reprojected
    const bool need_rays = !reset && (!same_view || d.n_sphere_motion > 0 || d.n_cube_motion > 0);
    if (need_rays && !(s->tp_raygen.get() && s->tp_w == d.width && s->tp_h == d.height &&
                       memcmp(&s->tp_aspect, &d.aspect, sizeof d.aspect) == 0)) {
        // another size or aspect: new tables, after the host has seen the last call that read the old ones end
        RT_HIP(s->tp_done.host_wait());
        const size_t need = (size_t)d.width + (size_t)d.height;
        s->tp_w = s->tp_h = 0;
        RT_HIP(s->tp_raygen.reserve(need));
        std::vector<float> h(need);
        rt_raygen_fill(d.width, d.height, d.aspect, 1, h.data());
        RT_HIP(hipMemcpy(s->tp_raygen.get(), h.data(), sizeof(float) * need, hipMemcpyHostToDevice));
        s->tp_w = d.width; s->tp_h = d.height; s->tp_aspect = d.aspect;
    }
    RT_HIP(s->tp_done.order(stream));
    hipEvent_t ev[2];
    s->tp_timed = 0;
    if (s->tp_timing) {
        for (int i = 0; i < 2; ++i) {
            RT_HIP(s->tp_ev[i].create(hipEventDefault));
            ev[i] = s->tp_ev[i].get();
        }
    }
    const float *dx_tab = need_rays ? s->tp_raygen.get() : nullptr, *dy_tab = need_rays ? s->tp_raygen.get() + d.width : nullptr;
    const int rc = rt_temporal_launch(&d, dx_tab, dy_tab, view, prev_view, same_view, s->tp_timing ? ev : nullptr, stream);
    RT_HIP(s->tp_done.record(stream));
    if (rc == RT_OK && s->tp_timing) s->tp_timed = 2;
    return rc;
}

extern "C" int rt_scene_temporal(rt_scene *s, const rt_temporal_desc *d_in, void *stream_)
{
    if (!s || !d_in) {
        rt_set_error("rt_scene_temporal: null scene or description");
        return RT_ERR_INVALID;
    }
    rt_temporal_desc td;
    as_built(d_in, &td);
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
    if (!s || !d_in) {
        rt_set_error("rt_scene_temporal_motion: null scene or description");
        return RT_ERR_INVALID;
    }
    rt_tmotion_desc d;
    as_built(d_in, &d);
    return temporal_call(s, d, true, "rt_scene_temporal_motion", (hipStream_t)stream_);
}

extern "C" int rt_scene_set_temporal_timing(rt_scene *s, int on)
{
    return pass_set_timing(s, "rt_scene_set_temporal_timing", &rt_scene::tp_timing, on);
}

extern "C" int rt_scene_temporal_times(rt_scene *s, float *ms, int cap, int *n)
{
    return pass_times(s, "rt_scene_temporal_times", &rt_scene::tp_done, s ? s->tp_ev : nullptr, s ? s->tp_timed : 0, ms, cap, n);
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
    if (!s || !d_in) {
        rt_set_error("rt_scene_upsample: null scene or description");
        return RT_ERR_INVALID;
    }
    rt_upsample_desc d;
    as_built(d_in, &d);
    const char *bad = nullptr;
    if (d.width <= 0 || d.height <= 0 || d.width > RT_DENOISE_MAX_SIZE || d.height > RT_DENOISE_MAX_SIZE ||
        d.lo_width <= 0 || d.lo_height <= 0)
        bad = "the sizes must be in [1, RT_DENOISE_MAX_SIZE]";
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
    else if (!(d.sigma_depth > 0.f) || !std::isfinite(d.sigma_depth)) bad = "sigma_depth is not finite and > 0";
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
    if (stream_capturing(stream)) {
        rt_set_error("rt_scene_upsample: the stream is being captured (the pass is not recorded into graphs)");
        return RT_ERR_UNSUPPORTED;
    }
    RT_HIP(s->up_done.order(stream));
    hipEvent_t ev[2];
    s->up_timed = 0;
    if (s->up_timing) {
        for (int i = 0; i < 2; ++i) {
            RT_HIP(s->up_ev[i].create(hipEventDefault));
            ev[i] = s->up_ev[i].get();
        }
    }
    const int rc = rt_upsample_launch(&d, s->up_timing ? ev : nullptr, stream);
    RT_HIP(s->up_done.record(stream));
    if (rc == RT_OK && s->up_timing) s->up_timed = 2;
    return rc;
}

extern "C" int rt_scene_set_upsample_timing(rt_scene *s, int on)
{
    return pass_set_timing(s, "rt_scene_set_upsample_timing", &rt_scene::up_timing, on);
}

extern "C" int rt_scene_upsample_times(rt_scene *s, float *ms, int cap, int *n)
{
    return pass_times(s, "rt_scene_upsample_times", &rt_scene::up_done, s ? s->up_ev : nullptr, s ? s->up_timed : 0, ms, cap, n);
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
    if (!s || !d_in) {
        rt_set_error("rt_scene_display: null scene or description");
        return RT_ERR_INVALID;
    }
    rt_display_desc d;
    as_built(d_in, &d);
    auto positive = [](float v) { return v > 0.f && std::isfinite(v); };
    const bool meter = d.meter != RT_DISPLAY_METER_MANUAL;
    const char *bad = nullptr;
    if (d.width <= 0 || d.height <= 0 || d.width > RT_DENOISE_MAX_SIZE || d.height > RT_DENOISE_MAX_SIZE)
        bad = "width and height must be in [1, RT_DENOISE_MAX_SIZE]";
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
    if (stream_capturing(stream)) {
        rt_set_error("rt_scene_display: the stream is being captured (the pass is not recorded into graphs)");
        return RT_ERR_UNSUPPORTED;
    }
    // the scratch: the histogram's counters, then the thresholds, which never change
    if (!s->dp_scratch.get()) {
        RT_HIP(s->dp_scratch.reserve(RT_DISPLAY_BINS + 256));
        const hipError_t e = hipMemcpy(s->dp_scratch.get() + RT_DISPLAY_BINS, rt_display_table(), 256 * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)s->dp_scratch.reset();
            RT_HIP(e);
        }
    }
    RT_HIP(s->dp_done.order(stream));   // one histogram: one call at a time
    hipEvent_t ev[RT_DISPLAY_MAX_EVENTS];
    s->dp_timed = 0;
    if (s->dp_timing) {
        for (int i = 0; i < RT_DISPLAY_MAX_EVENTS; ++i) {
            RT_HIP(s->dp_ev[i].create(hipEventDefault));
            ev[i] = s->dp_ev[i].get();
        }
    }
    int n_ev = 0;
    const int rc = rt_display_launch(&d, s->dp_scratch.get(), (const float *)(s->dp_scratch.get() + RT_DISPLAY_BINS),
                                     s->dp_timing ? ev : nullptr, &n_ev, stream);
    // also after a launch that failed half way: what was enqueued uses the histogram
    RT_HIP(s->dp_done.record(stream));
    if (rc == RT_OK && s->dp_timing) s->dp_timed = n_ev;
    return rc;
}

extern "C" int rt_scene_set_display_timing(rt_scene *s, int on)
{
    return pass_set_timing(s, "rt_scene_set_display_timing", &rt_scene::dp_timing, on);
}

extern "C" int rt_scene_display_times(rt_scene *s, float *ms, int cap, int *n)
{
    return pass_times(s, "rt_scene_display_times", &rt_scene::dp_done, s ? s->dp_ev : nullptr, s ? s->dp_timed : 0, ms, cap, n);
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
    if (!s || !d_in) {
        rt_set_error("rt_scene_bloom: null scene or description");
        return RT_ERR_INVALID;
    }
    rt_bloom_desc d;
    as_built(d_in, &d);
    const char *bad = nullptr;
    if (d.width <= 0 || d.height <= 0 || d.width > RT_DENOISE_MAX_SIZE || d.height > RT_DENOISE_MAX_SIZE)
        bad = "width and height must be in [1, RT_DENOISE_MAX_SIZE]";
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
    else if (!(d.limit > 0.f) || !std::isfinite(d.limit)) bad = "limit is not finite and > 0";
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
    if (stream_capturing(stream)) {
        rt_set_error("rt_scene_bloom: the stream is being captured (the pass is not recorded into graphs)");
        return RT_ERR_UNSUPPORTED;
    }
    const size_t need = rt_bloom_pyramid_texels(d.width, d.height, d.levels);
    if (need > s->bl_pyramid.capacity()) {
        // growing releases the old pyramid: after the host has seen the last call that used it end
        RT_HIP(s->bl_done.host_wait());
        RT_HIP(s->bl_pyramid.reserve(need));
    }
    RT_HIP(s->bl_done.order(stream));   // one pyramid: one call at a time
    hipEvent_t ev[RT_BLOOM_MAX_EVENTS + 1];
    s->bl_timed = 0;
    if (s->bl_timing) {
        for (int i = 0; i < RT_BLOOM_MAX_EVENTS + 1; ++i) {
            RT_HIP(s->bl_ev[i].create(hipEventDefault));
            ev[i] = s->bl_ev[i].get();
        }
    }
    int n_ev = 0;
    const int rc = rt_bloom_launch(&d, s->bl_pyramid.get(), s->bl_timing ? ev : nullptr, &n_ev, stream);
    // also after a launch that failed half way: what was enqueued uses the pyramid
    RT_HIP(s->bl_done.record(stream));
    if (rc == RT_OK && s->bl_timing) s->bl_timed = n_ev;
    return rc;
}

extern "C" int rt_scene_set_bloom_timing(rt_scene *s, int on)
{
    return pass_set_timing(s, "rt_scene_set_bloom_timing", &rt_scene::bl_timing, on);
}

extern "C" int rt_scene_bloom_times(rt_scene *s, float *ms, int cap, int *n)
{
    return pass_times(s, "rt_scene_bloom_times", &rt_scene::bl_done, s ? s->bl_ev : nullptr, s ? s->bl_timed : 0, ms, cap, n);
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
    if (!s || !d_in) {
        rt_set_error("%s: null scene or description", name);
        return RT_ERR_INVALID;
    }
    rt_indirect_desc d;
    as_built(d_in, &d);
    const char *bad = nullptr;
    if (d.width <= 0 || d.height <= 0 || d.width > RT_DENOISE_MAX_SIZE || d.height > RT_DENOISE_MAX_SIZE)
        bad = "width and height must be in [1, RT_DENOISE_MAX_SIZE]";
    else if (!(d.aspect > 0.f) || !std::isfinite(d.aspect)) bad = "aspect is not finite and > 0";
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
    if (stream_capturing(stream)) {
        rt_set_error("%s: the stream is being captured (the pass is not recorded into graphs)", name);
        return RT_ERR_UNSUPPORTED;
    }
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
    // the view's ray tables at one sample: the pass's own, so that a call at another size than the frames' (half
    // resolution) does not rebuild theirs. Another size or aspect: after the host has seen the last call end
    if (!(s->ind_raygen.get() && s->ind_w == d.width && s->ind_h == d.height && memcmp(&s->ind_aspect, &d.aspect, sizeof d.aspect) == 0)) {
        RT_HIP(s->ind_done.host_wait());
        const size_t need = (size_t)d.width + (size_t)d.height;
        s->ind_w = s->ind_h = 0;
        RT_HIP(s->ind_raygen.reserve(need));
        std::vector<float> h(need);
        rt_raygen_fill(d.width, d.height, d.aspect, 1, h.data());
        RT_HIP(hipMemcpy(s->ind_raygen.get(), h.data(), sizeof(float) * need, hipMemcpyHostToDevice));
        s->ind_w = d.width; s->ind_h = d.height; s->ind_aspect = d.aspect;
    }
    const int groups = (d.rays + RT_INDIRECT_GROUP - 1) / RT_INDIRECT_GROUP;
    if (wavefront) {
        const size_t sum_px = groups > 1 ? npx : 0;
        // paths: two queues of the wider entry, which ping-pong
        const size_t q1 = slots * (bounces > 1 ? RT_INDIRECT_PATH_ENTRY_F4 : RT_INDIRECT_ENTRY_F4), q2 = bounces > 1 ? q1 : 0;
        if (slots > s->ind_slab.capacity() || q1 > s->ind_queue.capacity() || q2 > s->ind_queue2.capacity() ||
            sum_px > s->ind_sum.capacity() || (size_t)RT_INDIRECT_MAX_COUNTS > s->ind_count.capacity()) {
            // growing releases the old buffers: after the host has seen the last call that used them end
            RT_HIP(s->ind_done.host_wait());
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
    fc.dx_tab = s->ind_raygen.get();
    fc.dy_tab = s->ind_raygen.get() + d.width;
    fc.packed = nullptr;
    RT_HIP(s->ind_done.order(stream));   // one scratch: one call at a time
    // the emission tables that changed: on this stream, so behind every indirect call in flight and ahead of this one
    // (a table that grows releases the old buffer: after the host has seen those calls end)
    RtEmitDev emit{};
    for (RtEmitTable &t : s->emit) {
        if (!t.dirty) continue;
        if (t.v.size() > t.d.capacity()) RT_HIP(s->ind_done.host_wait());
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
    hipEvent_t ev[RT_INDIRECT_MAX_EVENTS];
    s->ind_timed = 0;
    if (s->ind_timing) {
        for (int i = 0; i < RT_INDIRECT_MAX_EVENTS; ++i) {
            RT_HIP(s->ind_ev[i].create(hipEventDefault));
            ev[i] = s->ind_ev[i].get();
        }
    }
    const RtIndirectScratch scratch{s->ind_slab.get(), s->ind_queue.get(), s->ind_sum.get(), s->ind_count.get(), s->ind_queue2.get()};
    int n_ev = 0;
    rc = rt_indirect_launch(&d, bounces, &fc, bvh, s->d_spheres.get(), s->n_spheres, any_emit ? &emit : nullptr, &scratch,
                            s->ind_timing ? ev : nullptr, &n_ev, stream);
    // also after a launch that failed half way: what was enqueued uses the scratch
    RT_HIP(s->ind_done.record(stream));
    if (rc != RT_OK) return rc;
    if (s->ind_timing) s->ind_timed = n_ev;
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

extern "C" int rt_scene_set_indirect_timing(rt_scene *s, int on)
{
    return pass_set_timing(s, "rt_scene_set_indirect_timing", &rt_scene::ind_timing, on);
}

extern "C" int rt_scene_indirect_times(rt_scene *s, float *ms, int cap, int *n)
{
    return pass_times(s, "rt_scene_indirect_times", &rt_scene::ind_done, s ? s->ind_ev : nullptr, s ? s->ind_timed : 0, ms, cap, n);
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
    RT_HIP(s->ind_done.host_wait());
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
