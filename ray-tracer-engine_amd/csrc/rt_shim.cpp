// rt_shim.cpp -- the rayTrace launch shim (kernel.cu:1615, 1780-1783): same argument list, the object / skybox
// graphs are read on the host and mirrored to the one scene the library keeps for it.
#include "rt_scene.h"

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

// Tests: the scene rt_launch_raytrace and update() render through (null before the first launch).
extern "C" rt_scene *rt_debug_shim_scene(void) { return g_shim.scene; }

// memManager::operator delete on something the shim has mirrored: the next launch re-uploads.
void rt_shim_forget(const void *ptr)
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
