// rt_scene.cpp -- the device-resident scene: its life, the frames in flight (ring, quiesce, the hand-over of cached
// tables: rt_scene.h), the setters that mirror host data to the device, and the accessors for rt_graph.cpp.
//
// Reference interfaces replaced here:
//   object / sprite / skybox     /root/reference/kernel.cu:1116-1244, sprite.h:11-47
#include <cmath>
#include <cstdlib>

#include "rt_scene.h"

static const int kMaxSpheres = 1 << 22;

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
    for (HipPendingEvent &done : s->post_event) RT_HIP(done.host_wait());              // a post pass still using its scratch
    return RT_OK;
}

int rt_scene_wait_all_frames(rt_scene *s, hipStream_t stream)
{
    for (int i = 0; i < RT_RING; ++i)
        if (s->ring_used[i]) RT_HIP(hipStreamWaitEvent(stream, s->ring[i].get(), 0));
    return RT_OK;
}

// A frame has just been enqueued on `stream`: give it the next ring slot, and mark the slots it read with it.
int rt_scene_note_launch(rt_scene *s, hipStream_t stream, RtTableSlot *cones, RtTableSlot *views, RtTableSlot *rest)
{
    const int k = (int)(s->ring_seq % RT_RING);
    RT_HIP(s->ring[k].create());
    // chain: whoever sees this slot's new event done has also seen the one it replaces
    if (s->ring_used[k]) RT_HIP(hipStreamWaitEvent(stream, s->ring[k].get(), 0));
    RT_HIP(hipEventRecord(s->ring[k].get(), stream));
    s->ring_used[k] = true;
    for (RtTableSlot *c : {cones, views, rest})
        if (c) {
            c->used = true;
            c->last_use = s->ring_seq;
        }
    s->ring_seq++;
    return RT_OK;
}

int rt_scene_begin_build(rt_scene *s, RtTableSlot &c, size_t total, bool on_host)
{
    if (total > c.buf.capacity() || on_host) {
        const int rc = rt_scene_quiesce(s);   // nothing may still read the buffer that is freed / overwritten from the host
        if (rc != RT_OK) return rc;
        RT_HIP(c.built.host_wait());          // the table stream has drained: returns at once, nothing stays pending
    }
    c.valid = false;
    bool grew;
    RT_HIP(c.buf.reserve(total, &grew));
    if (grew) s->epoch++;
    if (on_host) return RT_OK;
    if (!s->table_stream.get()) {
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        RT_HIP(s->table_stream.create(hipStreamNonBlocking, hi));
    }
    // ordered, on the device only, after the last frame that read this slot and after a sphere-table upload in flight
    const hipStream_t ts = s->table_stream.get();
    if (c.used) {
        if (s->ring_seq - c.last_use <= RT_RING) RT_HIP(hipStreamWaitEvent(ts, s->ring[c.last_use % RT_RING].get(), 0));
        else {
            const int rc = rt_scene_wait_all_frames(s, ts);
            if (rc != RT_OK) return rc;
        }
    }
    RT_HIP(s->stage_done.order(ts));
    return RT_OK;
}

int rt_scene_end_build(rt_scene *s, RtTableSlot &c, bool on_host)
{
    if (!on_host) RT_HIP(c.built.record(s->table_stream.get()));
    c.valid = true;
    c.used = false;
    return RT_OK;
}

extern "C" void rt_scene_destroy(rt_scene *s)
{
    if (!s) return;
    (void)rt_scene_quiesce(s);   // then nothing reads what the members release
    delete s;
}

// rt_scene_set_spheres / _planes / _cubes: a new count clears the list's emission table, the same count keeps it (as
// the roughness table, rt_reflect_spheres_changed)
static void emit_list_changed(rt_scene *s, int kind, int n_old, int n_new)
{
    RtEmitTable &t = s->emit[kind - RT_HIT_SPHERE];
    if (n_old == n_new) return;
    if (!t.v.empty()) t.dirty = true;
    t.v.clear();
}

// {cx, cy, cz, radius*radius}: the only four numbers sphere::intersect reads
// (kernel.cu:332-334); radius*radius is the same binary32 product either way.
void rt_pack_spheres(const rt_sphere *src, int n, float4 *dst)
{
    for (int i = 0; i < n; ++i)
        dst[i] = make_float4(src[i].orgin.x, src[i].orgin.y, src[i].orgin.z, src[i].radius * src[i].radius);
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
    const int n_pad = rt_pad64(n), nb = n_pad / RT_BLOCK;
    const size_t total = (size_t)n + (size_t)n_pad + (size_t)nb + ((size_t)n_pad + 3) / 4;   // in float4 units
    std::vector<float4> packed((size_t)n);
    if (n > 0) {
        rt_pack_spheres(host_spheres, n, packed.data());
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
    if (total > s->h_stage.capacity()) RT_HIP(s->stage_done.host_wait());   // before it is freed
    RT_HIP(s->h_stage.reserve(total));
    if (n > 0) {
        // the staging buffer is reused: wait for the previous upload to have left it
        RT_HIP(s->stage_done.host_wait());
        float4 *h_orig = s->h_stage.get(), *h_sorted = h_orig + n, *h_blocks = h_sorted + n_pad;
        int *h_idx = reinterpret_cast<int *>(h_blocks + nb);
        memcpy(h_orig, packed.data(), sizeof(float4) * (size_t)n);
        rt_build_sorted_blocks(packed.data(), n, h_sorted, h_blocks, h_idx);
        RT_HIP(hipMemcpyAsync(s->d_spheres.get(), s->h_stage.get(), sizeof(float4) * total, hipMemcpyHostToDevice, stream));
        RT_HIP(s->stage_done.record(stream));
        s->h_prev.swap(packed);
    } else {
        s->h_prev.clear();
    }
    s->sphere_gen++;
    s->epoch++;
    s->n_blocks = nb;
    if (s->refl) rt_reflect_spheres_changed(s->refl.get(), s->n_spheres, n);
    emit_list_changed(s, RT_HIT_SPHERE, s->n_spheres, n);
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
    if (s->refl) rt_reflect_kind_list_changed(s->refl.get(), 0, s->n_planes, n);
    emit_list_changed(s, RT_HIT_PLANE, s->n_planes, n);
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
    if (s->refl) rt_reflect_kind_list_changed(s->refl.get(), 1, s->n_cubes, n);
    emit_list_changed(s, RT_HIT_CUBE, s->n_cubes, n);
    s->n_cubes = n;
    s->epoch++;
    return RT_OK;
}

// The reference-layout mesh, flattened by rt_mesh_flatten, as device arrays.
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
    RtFlatMesh m;
    { const int rc = rt_mesh_flatten(mesh, &m); if (rc != RT_OK) return rc; }
    RT_HIP(s->d_tris.reserve(m.tris.size()));
    RT_HIP(s->d_boxes.reserve(m.boxes.size()));
    RT_HIP(s->d_tri_idx.reserve(m.idx.size() ? m.idx.size() : 1));
    RT_HIP(s->d_box_spheres.reserve(m.box_spheres.size()));
    RT_HIP(hipMemcpy(s->d_box_spheres.get(), m.box_spheres.data(), sizeof(float) * m.box_spheres.size(), hipMemcpyHostToDevice));
    RT_HIP(hipMemcpy(s->d_tris.get(), m.tris.data(), sizeof(RtTriDev) * m.tris.size(), hipMemcpyHostToDevice));
    RT_HIP(hipMemcpy(s->d_boxes.get(), m.boxes.data(), sizeof(RtBoxDev) * m.boxes.size(), hipMemcpyHostToDevice));
    if (!m.idx.empty()) RT_HIP(hipMemcpy(s->d_tri_idx.get(), m.idx.data(), sizeof(int) * m.idx.size(), hipMemcpyHostToDevice));
    RT_HIP(s->d_tri9.reserve(m.tri9.size()));
    RT_HIP(hipMemcpy(s->d_tri9.get(), m.tri9.data(), sizeof(float) * m.tri9.size(), hipMemcpyHostToDevice));
    RT_HIP(s->d_tri_bs.reserve(m.tri_bs.size()));
    RT_HIP(hipMemcpy(s->d_tri_bs.get(), m.tri_bs.data(), sizeof(float) * m.tri_bs.size(), hipMemcpyHostToDevice));
    RT_HIP(s->d_tri_nrm.reserve(m.tri_nrm.size()));
    RT_HIP(hipMemcpy(s->d_tri_nrm.get(), m.tri_nrm.data(), sizeof(float) * m.tri_nrm.size(), hipMemcpyHostToDevice));
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

RtReflect *rt_scene_reflect(rt_scene *s)   // created on first use
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
    return rt_reflect_set_materials(rt_scene_reflect(s), per_sphere, n, s->n_spheres);
}

extern "C" int rt_scene_set_materials_ex(rt_scene *s, const rt_material_ex *per_sphere, int n)
{
    if (!s) {
        rt_set_error("rt_scene_set_materials_ex: null scene");
        return RT_ERR_INVALID;
    }
    // (as rt_scene_set_materials: the next reflective frame uploads after the frames in flight)
    return rt_reflect_set_materials_ex(rt_scene_reflect(s), per_sphere, n, s->n_spheres);
}

// The scope of reflective frames: a host-side switch, read when a frame is launched
extern "C" int rt_scene_set_reflect_scope(rt_scene *s, int scope)
{
    if (!s) {
        rt_set_error("rt_scene_set_reflect_scope: null scene");
        return RT_ERR_INVALID;
    }
    return rt_reflect_set_scope(rt_scene_reflect(s), scope);
}

// How reflective frames sample a pixel: a host-side switch, read when a frame is launched
extern "C" int rt_scene_set_reflect_samples(rt_scene *s, int mode)
{
    if (!s) {
        rt_set_error("rt_scene_set_reflect_samples: null scene");
        return RT_ERR_INVALID;
    }
    return rt_reflect_set_samples(rt_scene_reflect(s), mode);
}

extern "C" int rt_scene_set_plane_materials(rt_scene *s, const rt_material *per_plane, int n)
{
    if (!s) {
        rt_set_error("rt_scene_set_plane_materials: null scene");
        return RT_ERR_INVALID;
    }
    // (as rt_scene_set_materials: the next reflective frame uploads after the frames in flight)
    return rt_reflect_set_kind_materials(rt_scene_reflect(s), 0, per_plane, n, s->n_planes);
}

extern "C" int rt_scene_set_cube_materials(rt_scene *s, const rt_material *per_cube, int n)
{
    if (!s) {
        rt_set_error("rt_scene_set_cube_materials: null scene");
        return RT_ERR_INVALID;
    }
    return rt_reflect_set_kind_materials(rt_scene_reflect(s), 1, per_cube, n, s->n_cubes);
}

// Roughness per primitive of one kind: tables of their own beside the k tables, under the same protocol
extern "C" int rt_scene_set_roughness(rt_scene *s, int kind, const float *rho, int n)
{
    if (!s) {
        rt_set_error("rt_scene_set_roughness: null scene");
        return RT_ERR_INVALID;
    }
    const int n_list = kind == RT_HIT_SPHERE ? s->n_spheres : (kind == RT_HIT_PLANE ? s->n_planes : s->n_cubes);
    // (as rt_scene_set_materials: the next reflective frame uploads after the frames in flight)
    return rt_reflect_set_roughness(rt_scene_reflect(s), kind, rho, n, n_list);
}

// Emission per primitive of one kind: host state under rt_scene_set_roughness' protocol; the next indirect
// call uploads it (rt_post.cpp, indirect_call)
extern "C" int rt_scene_set_emission(rt_scene *s, int kind, const float *rgb, int n)
{
    if (!s) {
        rt_set_error("rt_scene_set_emission: null scene");
        return RT_ERR_INVALID;
    }
    if (kind != RT_HIT_SPHERE && kind != RT_HIT_PLANE && kind != RT_HIT_CUBE) {
        rt_set_error("rt_scene_set_emission: kind %d is not RT_HIT_SPHERE, RT_HIT_PLANE or RT_HIT_CUBE", kind);
        return RT_ERR_INVALID;
    }
    const char *what = kind == RT_HIT_SPHERE ? "sphere" : (kind == RT_HIT_PLANE ? "plane" : "cube");
    const int n_list = kind == RT_HIT_SPHERE ? s->n_spheres : (kind == RT_HIT_PLANE ? s->n_planes : s->n_cubes);
    RtEmitTable &t = s->emit[kind - RT_HIT_SPHERE];
    if (!rgb || n == 0) {
        if (!t.v.empty()) t.dirty = true;
        t.v.clear();
        return RT_OK;
    }
    // every value first, then the count (rt_reflect_set_kind_materials' order: a value's refusal does not depend on the
    // scene's lists)
    for (int i = 0; i < n; ++i) {
        for (int c = 0; c < 3; ++c) {
            const float e = rgb[3 * (size_t)i + c];
            if (!(e >= 0.f) || !std::isfinite(e)) {
                rt_set_error("rt_scene_set_emission: %s %d: emission.%c %g is not finite and >= 0", what, i, "rgb"[c], (double)e);
                return RT_ERR_INVALID;
            }
        }
    }
    if (n != n_list) {
        rt_set_error("rt_scene_set_emission: %d colours for %d %ss (one per %s, or NULL / 0)", n, n_list, what, what);
        return RT_ERR_INVALID;
    }
    std::vector<float4> v((size_t)n);
    for (int i = 0; i < n; ++i) v[(size_t)i] = make_float4(rgb[3 * (size_t)i], rgb[3 * (size_t)i + 1], rgb[3 * (size_t)i + 2], 0.f);
    // (the same table again: no re-upload)
    if (v.size() == t.v.size() && memcmp(v.data(), t.v.data(), sizeof(float4) * v.size()) == 0) return RT_OK;
    t.v.swap(v);
    t.dirty = true;
    return RT_OK;
}

// The seed of the glossy draws: a host-side value, read when a frame is launched
extern "C" int rt_scene_set_gloss_seed(rt_scene *s, unsigned seed)
{
    if (!s) {
        rt_set_error("rt_scene_set_gloss_seed: null scene");
        return RT_ERR_INVALID;
    }
    return rt_reflect_set_gloss_seed(rt_scene_reflect(s), seed);
}

// How glass continues a ray: a host-side value, read when a frame is launched
extern "C" int rt_scene_set_glass_model(rt_scene *s, int model)
{
    if (!s) {
        rt_set_error("rt_scene_set_glass_model: null scene");
        return RT_ERR_INVALID;
    }
    return rt_reflect_set_glass_model(rt_scene_reflect(s), model);
}

extern "C" int rt_scene_set_reflect_timing(rt_scene *s, int on)
{
    if (!s) {
        rt_set_error("rt_scene_set_reflect_timing: null scene");
        return RT_ERR_INVALID;
    }
    return rt_reflect_set_timing(rt_scene_reflect(s), on);
}

extern "C" int rt_scene_reflect_stats(rt_scene *s, rt_reflect_stats *out)
{
    if (!s || !out) {
        rt_set_error("rt_scene_reflect_stats: null argument");
        return RT_ERR_INVALID;
    }
    return rt_reflect_get_stats(rt_scene_reflect(s), out);
}

// Tests only (not in include/rt_engine.h): which instantiations of the reflective passes the scene's most recent
// reflective frame launched. out[0 .. 4]: GLASS, KINDS, SAMPLES, GLOSS, FRESNEL of rt_reflect_primary (0 / 1); out[5]:
// 1 the passes walked the sphere BVH, 0 the whole list; out[6]: the frame's sample groups (a one-sample frame: 1).
// Before any reflective frame: the flags -1 and 0 groups. Host state only: it waits for nothing.
extern "C" int rt_debug_reflect_dispatch(rt_scene *s, int *out, int cap)
{
    if (!s || !out || cap < RT_REFLECT_DISPATCH_FIELDS) {
        rt_set_error("rt_debug_reflect_dispatch: null argument or room for fewer than %d ints", RT_REFLECT_DISPATCH_FIELDS);
        return RT_ERR_INVALID;
    }
    rt_reflect_dispatch(s->refl.get(), out);
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

extern "C" int rt_scene_set_light_verdicts(rt_scene *s, int mode)
{
    if (!s || (mode != 0 && mode != 1)) {
        rt_set_error("rt_scene_set_light_verdicts: null scene or mode %d not in {0, 1}", mode);
        return RT_ERR_INVALID;
    }
    s->light_verdicts_mode = mode;
    return RT_OK;
}

extern "C" int rt_scene_set_view_lists(rt_scene *s, int mode)
{
    if (!s || (mode != 0 && mode != 1)) {
        rt_set_error("rt_scene_set_view_lists: null scene or mode %d not in {0, 1}", mode);
        return RT_ERR_INVALID;
    }
    s->view_lists_mode = mode;
    return RT_OK;
}
