// rt_scene_tables.cpp -- the scene's cached device tables, each found or (re)built when a frame asks for it: eye cones,
// per-light columns, occluder lists, raygen tables, RtFrameAux, the tile order and the view lists. The eye cones and
// the view lists follow a moving camera and are handed over by the slot functions of rt_scene.h; the others wait on
// the host (rt_scene_quiesce) the rare times they change. (What a frame launch itself records: rt_scene_rest.cpp.)
#include <cmath>
#include <algorithm>

#include "rt_math.h"
#include "rt_scene.h"

static const int kMaxSpheresOccluders = 8192;    // the per-sphere occluder lists take n * 128 entries (2 KiB per sphere) per light

// ---------------------------------------------------------------------------
// eye cones: which table a frame with ray origin `org` reads, building it if need be
// ---------------------------------------------------------------------------
bool rt_scene_wants_eye_cones(const rt_scene *s, const float org[3])
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
int rt_scene_build_eye_cones_host(rt_scene *s, const float org[3], float4 *buf, hipStream_t stream)
{
    const int n = s->n_spheres, n_pad = rt_pad64(n), nb = n_pad / RT_BLOCK;
    if (n_pad <= RT_EYE_DEVICE_MAX) {
        RT_HIP(rt_eye_cones_launch(s->d_spheres.get(), n, org, buf, 1024, stream));
        return RT_OK;
    }
    std::vector<float4> h(rt_eye_cones_size(n));
    rt_build_eye_cones_host(s->h_prev.data(), n, org, h.data(), h.data() + n_pad, reinterpret_cast<int *>(h.data() + n_pad + 2 * nb));
    RT_HIP(hipMemcpyAsync(buf, h.data(), sizeof(float4) * h.size(), hipMemcpyHostToDevice, stream));
    RT_HIP(hipStreamSynchronize(stream));   // `h` goes out of scope
    return RT_OK;
}

// Returns the slot whose table is current for `org` (building it if none is), or -1 when the
// scene renders without eye cones. Not inside a stream capture.
int rt_scene_prepare_eye(rt_scene *s, const float org[3], hipStream_t stream, int *slot_out)
{
    *slot_out = -1;
    if (!rt_scene_wants_eye_cones(s, org)) return RT_OK;
    for (int i = 0; i < RT_CONE_SLOTS; ++i) {
        const ConeSlot &c = s->cones[i];
        if (c.valid && c.gen == s->sphere_gen && memcmp(org, c.org, sizeof c.org) == 0) {
            *slot_out = i;
            return RT_OK;
        }
    }
    ConeSlot &c = rt_slot_victim(s->cones, [s](const ConeSlot &x) { return !x.valid || x.gen != s->sphere_gen; });
    // a list beyond the one-workgroup device builder: built on the host, uploaded blocking on the caller's stream
    const bool on_host = rt_pad64(s->n_spheres) > RT_EYE_DEVICE_MAX;
    int rc = rt_scene_begin_build(s, c, rt_eye_cones_size(s->n_spheres), on_host);
    if (rc != RT_OK) return rc;
    if (on_host) rc = rt_scene_build_eye_cones_host(s, org, c.buf.get(), stream);
    else RT_HIP(rt_eye_cones_launch(s->d_spheres.get(), s->n_spheres, org, c.buf.get(), 256, s->table_stream.get()));
    if (rc != RT_OK) return rc;
    memcpy(c.org, org, sizeof c.org);
    c.gen = s->sphere_gen;
    *slot_out = (int)(&c - s->cones);
    return rt_scene_end_build(s, c, on_host);
}

// ---------------------------------------------------------------------------
// per-light column tables (host build: lights and the list rarely change)
// ---------------------------------------------------------------------------
static int rt_scene_prepare_lights(rt_scene *s, hipStream_t stream)
{
    const int n = s->n_spheres;
    const int n_pad = rt_pad64(n), nb = n_pad / RT_BLOCK;
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
    RT_HIP(s->stage_done.order(stream));   // the table the build reads may still be on its way
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

// dx / dy of the primary rays per column / row and sample (kernel.cu:1624-1625): h[total * width] then h[total * height]
void rt_raygen_fill(int width, int height, float aspect, int total, float *h)
{
    const double aspect_d = (double)aspect;
    const double width_d = (double)(float)width, height_d = (double)(float)height;
    const double hw_d = (double)((float)height / (float)width);
    for (int k = 0; k < total; ++k) {
        double ox, oy;
        rt_sample_offset(k, total, &ox, &oy);
        float *dx = h + (size_t)k * width, *dy = h + (size_t)total * width + (size_t)k * height;
        for (int x = 0; x < width; ++x) {
            const double tx_d = (2.0 * ((double)x + ox)) / width_d;
            dx[x] = (float)(aspect_d * tx_d - 1.0);
        }
        for (int y = 0; y < height; ++y) {
            const double ty_d = (2.0 * ((double)y + oy)) / height_d;
            dy[y] = (float)((aspect_d * ty_d) * hw_d - 1.0);
        }
    }
}

// dx and dy of kernel.cu:1624-1625 for every column, row and sample of a frame:
//   dx = aspect*(2*(x+0.5)/(float)width) - 1,  dy = aspect*(2*(y+0.5)/(float)height)*((float)height/width) - 1
// binary64 expressions (the literal 0.5) narrowed to float on assignment. They depend on the
// camera in no way, so a moving camera re-uses them; a new size, aspect or sample count
// rebuilds them (host, W + H divisions per sample) after waiting for the frames in flight.
int rt_scene_prepare_raygen(rt_scene *s, int width, int height, float aspect, int total)
{
    if (s->d_raygen.get() && s->rg_w == width && s->rg_h == height && s->rg_total == total &&
        memcmp(&s->rg_aspect, &aspect, sizeof aspect) == 0)
        return RT_OK;
    const int rc = rt_scene_quiesce(s);
    if (rc != RT_OK) return rc;
    const size_t need = (size_t)total * ((size_t)width + (size_t)height);
    RT_HIP(s->d_raygen.reserve(need));
    std::vector<float> h(need);
    rt_raygen_fill(width, height, aspect, total, h.data());
    RT_HIP(hipMemcpy(s->d_raygen.get(), h.data(), sizeof(float) * need, hipMemcpyHostToDevice));
    s->rg_w = width;
    s->rg_h = height;
    s->rg_total = total;
    s->rg_aspect = aspect;
    s->epoch++;
    return RT_OK;
}

// Everything of the frame that lives in RtFrameAux (device memory): pure host computation.
void rt_build_frame_aux(const rt_scene *s, RtFrameAux *ax)
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
        const int n_pad = rt_pad64(s->n_spheres);
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
    ax->sky_mu_x = rt_texel_margin(s->sky_w, 1.0e-6f);
    ax->sky_mu_y = rt_texel_margin(s->sky_h, 1.0e-6f);
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
int rt_scene_sync_aux(rt_scene *s)
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
int rt_scene_prepare_tile_order(rt_scene *s, const RtKernelChoice &kc, RtFrameConsts *fc, hipStream_t stream)
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
    RT_HIP(s->order_built.order(stream));   // an order being sorted (any layout: one event) precedes this launch
    if (!t) {                 // a new layout takes the least recently used slot
        t = lru;
        int rc = rt_scene_wait_all_frames(s, stream);   // frames that still write into the slot's old arrays
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
        t->serial = ++s->order_serial;
        RT_HIP(s->order_built.record(stream));   // launches on other streams: after the reset
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
            int rc = rt_scene_wait_all_frames(s, stream);
            if (rc != RT_OK) return rc;
            RT_HIP(rt_tile_order_launch(t->buf.cost(), t->buf.key(), t->buf.start(), t->buf.perm(), t->grid.tiles_x, t->grid.tiles_y,
                                        stream));
            RT_HIP(s->order_built.record(stream));
            t->serial = ++s->order_serial;   // a run list built from the order before is stale (rt_scene_rest.cpp)
            t->have_perm = true;
            t->since_sort = 0;
        }
    }
    t->since_sort++;
    t->same_view++;
    t->last_use = ++s->order_clock;
    fc->tile_cost = t->buf.cost();
    fc->tile_perm = t->have_perm ? t->buf.perm() : nullptr;
    s->order_cur_serial = t->serial;
    return RT_OK;
}

// The view of a frame as the view-list builders take it (block shape by rt_view_block_shape; tab, cones, out left null).
void rt_view_params_from_consts(const RtFrameConsts &fc, float aspect, RtViewParams *p)
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
int rt_scene_prepare_view(rt_scene *s, const rt_frame_desc *fd, const RtKernelChoice &kc, int cone_slot, RtFrameConsts *fc,
                          hipStream_t stream, int *view_out)
{
    *view_out = -1;
    if (!s->view_lists_mode || cone_slot < 0 || !kc.cull || kc.mode == RT_MODE_FORCE_SLOW) return RT_OK;
    RtViewParams p;
    rt_view_params_from_consts(*fc, fd->aspect, &p);
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
        // on the table stream: behind the build of the eye-cone table it reads (same stream, or finished on the host)
        ViewSlot &c = rt_slot_victim(s->views, [](const ViewSlot &x) { return !x.valid; });
        int rc = rt_scene_begin_build(s, c, rt_view_lists_size(p.nbx, p.nby), false);
        if (rc != RT_OK) return rc;
        p.tab = s->d_spheres.get();
        p.cones = s->cones[cone_slot].buf.get();
        p.out = c.buf.get();
        RT_HIP(rt_view_lists_launch(p, s->table_stream.get()));
        memcpy(c.key, key, sizeof key);
        c.nbx = p.nbx; c.nby = p.nby; c.bw = p.bw; c.bh = p.bh;
        rc = rt_scene_end_build(s, c, false);
        if (rc != RT_OK) return rc;
        v = (int)(&c - s->views);
    }
    ViewSlot &c = s->views[v];
    RT_HIP(rt_scene_order_reader(c, stream));   // the build precedes its readers
    fc->view_lists = reinterpret_cast<const float *>(c.buf.get());
    fc->view_nbx = c.nbx;
    fc->view_shift = c.bw | (c.bh << 8);
    *view_out = v;
    return RT_OK;
}

void rt_view_lists_summary(const float4 *slots, int blocks, rt_view_lists_info *out)
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
    ViewSlot &c = s->views[s->view_last];
    RT_HIP(c.built.host_wait());
    const size_t total = rt_view_lists_size(c.nbx, c.nby);
    std::vector<float4> h(total);
    RT_HIP(hipMemcpy(h.data(), c.buf.get(), sizeof(float4) * total, hipMemcpyDeviceToHost));
    out->read = 1;
    out->block_w = 1 << c.bw; out->block_h = 1 << c.bh;
    out->blocks_x = c.nbx; out->blocks_y = c.nby;
    rt_view_lists_summary(h.data(), c.nbx * c.nby, out);
    if (slots) {
        if (cap < total) {
            rt_set_error("rt_scene_view_lists_info: room for %zu float4, the lists take %zu", cap, total);
            return RT_ERR_INVALID;
        }
        memcpy(slots, h.data(), sizeof(float4) * total);
    }
    return RT_OK;
}

// for a graph's own lists (rt_graph.cpp)
int rt_view_params_for_frame(const rt_scene *s, const RtFrameConsts *fc, float aspect, int tile_w, int cull, int mode, RtViewParams *p)
{
    rt_view_params_from_consts(*fc, aspect, p);
    return s->view_lists_mode && cull && mode != RT_MODE_FORCE_SLOW && view_tiles_nest(*p, *fc, tile_w);
}
