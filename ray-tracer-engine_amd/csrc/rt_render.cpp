// rt_render.cpp -- what a launch does: a caller's descriptions in this build's layout, the by-value frame uniforms,
// the kernel choice, and the entry points that enqueue a frame or a ray query on the scene (the post passes: rt_post.cpp).
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
    kc->mode = fd->opts.stats ? (fd->opts.profile ? RT_MODE_PHASES : RT_MODE_STATS) : (fd->opts.force_slow_path ? RT_MODE_FORCE_SLOW : RT_MODE_PRODUCT);
    kc->feat = s->n_boxes > 0 ? RT_FEAT_MESH : ((s->n_planes > 0 || s->n_cubes > 0) ? RT_FEAT_PRIMS : RT_FEAT_SPHERES);
    // the opt-in approximate mode exists for the product configuration only; anything else renders exactly
    // (a reflective frame is exact: `fast` is ignored there -- its L feeds the bounces; and so is
    // a launch with the table_lds field set: include/rt_engine.h)
    if (fd->opts.fast == 1 && fd->opts.reflect_depth == 0 && kc->mode == RT_MODE_PRODUCT && kc->cull && kc->tile == 8 && kc->feat != RT_FEAT_MESH &&
        fd->opts.table_lds != 1)
        kc->mode = RT_MODE_FAST;
#ifndef RT_TUNING
    if (kc->mode == RT_MODE_PHASES) {
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
    if (rt_fd_aov_field(fd)) kc->mode = RT_MODE_AOV;
    return RT_OK;
}

// The layout before rt_launch_opts.reflect_depth was appended: what struct_size 0 reads as.
static const size_t kOptsSizeV1 = offsetof(rt_launch_opts, reflect_depth);
static const size_t kFrameSizeV1 = offsetof(rt_frame_desc, opts) + kOptsSizeV1;

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
    unsigned compact_wgs = 0;   // the 1-D grid of a compact reading launch, 0: the full grid
    rc = rt_scene_prepare_rest(s, kc, &fc, reflect_depth == 0 && kc.mode == RT_MODE_PRODUCT && kc.feat == RT_FEAT_SPHERES && kc.cull && fc.spp == 1, stream, &rest,
                               samples ? nullptr : &compact_wgs);
    if (rc != RT_OK) return rc;
    if (samples) {   // the frame kernel per sample, the passes per group, the resolve pass
        rc = rt_reflect_launch_samples(s->refl.get(), &fc, &out, &kc, s->d_spheres.get(), s->n_spheres, reflect_depth, stream);
        if (rc != RT_OK) return rc;
    } else {
        if (reflect_depth > 0) {
            rc = rt_reflect_mark_frame_start(s->refl.get(), stream);
            if (rc != RT_OK) return rc;
        }
        RT_HIP(rt_dev_launch_trace_grid(&fc, s->d_spheres.get(), kc.tile, kc.cull, kc.mode, kc.feat, compact_wgs, stream));
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
