/*
 * include/rt_engine.h -- C ABI of the MI355X-native ray-tracing hot path.
 *
 * Drop-in boundary for ONE path of leonZtiger/Ray-Tracer-engine: the per-pixel
 * ray-generation -> sphere-scene intersection -> shading -> framebuffer-write
 * kernel (`rayTrace`, /root/reference/kernel.cu:1614-1690) together with the
 * host surface around it (kernel.cuh:3-4, memManager.h:11-18, window.h:7-16,
 * sprite.h:11-47). Plain C types only: no HIP, torch or C++ types appear in any
 * signature, so the library can be bound from C, C++, ctypes, cgo, JNI, ...
 *
 * Every entry point names the reference interface it replaces (file:line).
 * Entry points return 0 on success and a non-zero rt_status on failure, unless
 * they mirror a reference function that is void (those keep the reference's
 * fatal convention: print, reset the device, exit(99) -- memManager.cpp:3-11).
 *
 * Threading: like the reference (single Win32 UI thread) the entry points are
 * not thread-safe; use one caller thread per process. A process drives one GPU
 * through rt_scene_* / rt_launch_raytrace / update(), or several GPUs of the node
 * through rt_multi_* (one process, one scene per device; update() after
 * rt_config_set_gpus(n)); hosts that run one process per GPU (bench.py under
 * torch.distributed) render their rows with rt_scene_render and run the gather
 * themselves (rt_assemble_rows24 is its root side). See INTEGRATION.md.
 */
#ifndef RT_ENGINE_H
#define RT_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 1
#define RT_MAX_LIGHTS 8      /* reference uses light_size = 3 (kernel.cu:1692) */
#define RT_MAX_SPP 16
#define RT_MAX_PLANES 64    /* planes and cubes are tested exhaustively (no culling) */
#define RT_MAX_CUBES 256
#define RT_MAX_REFLECT_DEPTH 8  /* rt_launch_opts.reflect_depth: bounces after the primary hit */

typedef enum rt_status {
    RT_OK = 0,
    RT_ERR_INVALID = 1,      /* bad argument (null pointer, size <= 0, ...)       */
    RT_ERR_UNSUPPORTED = 2,  /* scene uses a primitive outside the sphere path    */
    RT_ERR_HIP = 3,          /* a HIP runtime call failed (see rt_last_error())   */
    RT_ERR_NO_DEVICE = 4,    /* no gfx950 device / kernel image not loadable      */
    RT_ERR_CAPACITY = 5      /* sphere_count or light_size above the build limit  */
} rt_status;

/* ------------------------------------------------------------------ *
 * POD mirrors of the reference's kernel-argument types. Layouts are   *
 * byte-compatible with the MSVC x64 / nvcc layouts the reference      *
 * hard-codes (kernel.cu:1214,1219: 40 and 32 bytes).                  *
 * ------------------------------------------------------------------ */
typedef struct rt_vec3 { float x, y, z; } rt_vec3;          /* vec3d, kernel.cu:38-40   */
typedef struct rt_ray { rt_vec3 Org, Dir; } rt_ray;          /* ray,   kernel.cu:225-236 */

typedef struct rt_camera {                                   /* camera, kernel.cu:237-262 */
    rt_vec3 Org, Dir;
    float aspect;            /* set per frame (kernel.cu:1773), unused by the kernel */
    float Camyaw, Campitch;  /* degrees; defaults 180 / -20 (kernel.cu:261)          */
} rt_camera;                                                 /* 36 bytes */

typedef struct rt_light {                                    /* light, kernel.cu:1246-1261 */
    rt_vec3 pos;
    float size, r, g, b;
} rt_light;                                                  /* 28 bytes */

typedef struct rt_sphere {                                   /* sphere : shape, kernel.cu:265-358 */
    void *vptr_slot;         /* shape has a virtual method; ignored by this library   */
    rt_vec3 orgin;           /* (sic) centre                                          */
    uint8_t reflective;      /* unused by the kernel                                  */
    uint8_t pad_[3];
    float radius;            /* holds r*r (ctor, kernel.cu:287); intersect squares it AGAIN (:334) */
    uint32_t tail_pad_;
} rt_sphere;                                                 /* 32 bytes */

typedef struct rt_plane {                                    /* plane : shape, kernel.cu:360-384 */
    void *vptr_slot;
    rt_vec3 orgin;           /* a point on the plane                                  */
    uint8_t reflective;
    uint8_t pad_[3];
    rt_vec3 normal;          /* used as given (not normalised by the kernel)          */
    uint32_t tail_pad_;
} rt_plane;                                                  /* 40 bytes (kernel.cu:1214) */

typedef struct rt_cube {                                     /* cube : shape, kernel.cu:387-509 */
    void *vptr_slot;
    rt_vec3 orgin;           /* (c1 + c2) / 2 (ctor, kernel.cu:395)                   */
    rt_vec3 normals[3];      /* unused by the kernel                                  */
    rt_vec3 bounds[2];       /* the two corners of the slab test (kernel.cu:457-485)  */
} rt_cube;                                                   /* 80 bytes */

typedef struct rt_vec2 { float u, v; } rt_vec2;              /* vec2d, kernel.cu:32-34 */

typedef struct rt_triangle {                                 /* triangle, kernel.cu:206-212 */
    rt_vec3 points[3];
    rt_vec3 normal;          /* face normal                                           */
    rt_vec3 vecNormal[3];    /* vertex normals (used when mesh.has_normals)           */
    rt_vec2 vt[3];           /* texture coordinates                                   */
} rt_triangle;                                               /* 108 bytes (kernel.cu:1018-1020) */

typedef struct rt_bvhbox {                                   /* Bvhbox, kernel.cu:512-543 */
    rt_cube *bvhbox;         /* bounds of this leaf (read by the shadow path, :1479)  */
    rt_cube *d_bvhbox;       /* same cube (read by castRay, :1297)                    */
    int *indexes;
    int *d_indexes;          /* triangle indices of this leaf                         */
    int length;
} rt_bvhbox;

typedef struct rt_mesh {                                     /* mesh, kernel.cu:559-575 (field order kept) */
    rt_triangle *d_tri_arr;
    rt_triangle *h_tri_arr;
    int poly_count;
    int bvhbox_count;        /* flat list of leaves after 10 median splits            */
    int bvhLayer_count;      /* 10                                                    */
    uint8_t has_normals;
    rt_bvhbox *h_box;
    rt_bvhbox *d_box;
    int *indexes;
} rt_mesh;

typedef struct rt_buffer {                                   /* buffer, sprite.h:11-19 */
    float *data;             /* planar floats in [0,1]                                */
    int size;                /* bytes (Sprite.cpp:14)                                 */
} rt_buffer;

typedef struct rt_sprite {                                   /* sprite, sprite.h:25-47 */
    rt_buffer *rBuff, *gBuff, *bBuff;
    int width, height;
} rt_sprite;

typedef struct rt_skybox {                                   /* skybox, kernel.cu:1116-1173 */
    rt_sphere *box;          /* centre (0,0,0), ctor radius 10000 (kernel.cu:1122,1700) */
    rt_sprite *skyboxTex;
} rt_skybox;

typedef struct rt_object {                                   /* object, kernel.cu:1176-1244 (field order kept) */
    int sphere_count, plane_count, cube_count;               /* :1231 */
    int depth;                                               /* :1232 */
    rt_sphere *s1;           /* host staging copy                                     */
    rt_sphere *d_spheres;    /* what the kernel reads (:1333)                         */
    rt_cube *c1, *d_cubes;   /* cubes read by the kernel at kernel.cu:1344-1356, 1526-1536 */
    rt_plane *planes, *d_planes; /* planes, kernel.cu:1359-1372, 1513-1523            */
    rt_mesh *mesh1;          /* triangle mesh + flat BVH (kernel.cu:1293-1328, 1475-1497);
                                NULL = no mesh (the reference's bvhbox_count = 0)       */
    rt_sprite *texture;      /* :1240, read at :1643-1655                             */
    void *mat;               /* NULL, or ONE rt_material (material, kernel.cu:213-224) that
                                rt_launch_raytrace_ex applies to every sphere when
                                opts->reflect_depth > 0; ignored otherwise                  */
    void **tot_mesh;
    int meshes;
} rt_object;

/* ------------------------------------------------------------------ *
 * memManager (memManager.h:11-18, memManager.cpp:3-22)                *
 * ------------------------------------------------------------------ */
/* check_cuda(result, func, file, line): on non-zero `err` print
 * "HIP error = <n> at <file>:<line> '<expr>'", reset the device, exit(99). */
void rt_check(int err, const char *expr, const char *file, int line);
/* memManager::operator new : managed allocation + device synchronise. */
void *rt_managed_alloc(size_t len);
/* memManager::operator delete : device synchronise + free. */
void rt_managed_free(void *ptr);

/* ------------------------------------------------------------------ *
 * Kernel launch (rayTrace<<<blocks,threads>>>, kernel.cu:1615,1780-1783) *
 * ------------------------------------------------------------------ */
typedef struct rt_launch_opts {
    uint32_t struct_size;    /* = sizeof(rt_launch_opts); for ABI growth              */
    float *rgba;             /* optional device float4 buffer, width*(y1-y0) texels:
                                linear colour BEFORE the *254 pack        */
    int y0, y1;              /* row band rendered by this call; 0,0 = whole frame.
                                `pixels`/`rgba` point at row y0 (band-local buffers)  */
    int spp;                 /* samples per pixel taken by this call (1..RT_MAX_SPP);
                                0 = 1. Sample k uses the fixed stratified offset
                                table (rt_sample_offset); 1 spp = pixel centre, as
                                the reference (kernel.cu:1624-1625)                   */
    int sample_base;         /* index of the first sample of this call               */
    int sample_total;        /* total samples of the frame (divisor at resolve);
                                0 = spp                                               */
    int accumulate;          /* 1: add into rgba (progressive); 0: overwrite          */
    int resolve;             /* 0 default: write packed words when pixels != NULL;
                                -1: leave `pixels` untouched (intermediate progressive pass) */
    int cull;                /* -1 default (on); 0 = brute force over the whole list,
                                exactly the reference's loops; 1 = conservative tile
                                culling (same output, fewer tests)                    */
    int tile;                /* 0 default; else tile width in {8,16,32,64} (64 px/wave) */
    uint64_t *stats;         /* optional device array of RT_STATS_COUNT counters      */
    int force_slow_path;     /* testing: disable every exactness-preserving shortcut  */
    int profile;             /* diagnostics: with `stats`, fill the per-phase cycle
                                counters (RT_STAT_PHASE0..) instead of work counters;
                                tuning builds of the library only (-DRT_TUNING)        */
    int interleave_count;    /* multi-GPU load balance: when > 1 this call renders the
                                row blocks k = interleave_index, +count, +2*count, ... of
                                `interleave_rows` rows each, counted from the first row
                                of the band [y0, y1) (y0 a multiple of `rows`; 0/0 = the
                                whole frame). Output buffers are compact: local row L holds
                                global row y0 + ((L / rows) * count + index) * rows + L % rows */
    int interleave_index;
    int interleave_rows;     /* block height, a power of two >= 16; 0 = 16             */
    void *packed24;          /* optional device buffer, 3 bytes per pixel (B,G,R: the packed
                                word without its zero top byte), width*rows*3 bytes, band-local
                                like `pixels`; needs width % 4 == 0. What a multi-GPU rank
                                sends to the root: a quarter less than the 32-bit words      */
    int table_lds;           /* kept for the layout; selects no kernel. It once staged the whole
                                sphere table in LDS per workgroup, which measured slower in every
                                round and was removed: 1 renders with the
                                default kernel, exactly as 0. 1 still keeps the launch exact
                                (`fast` ignored), and a frame with reflect_depth > 0 refuses it  */
    int fast;                /* 1: opt-in APPROXIMATE mode. Everything that enters a pixel continuously
                                (primary hit, normal, toL) stays exact; the ten shadow-sample
                                directions of a light are built once per light in binary32 with
                                hardware rsq / sqrt and FMAs (instead of following the reference's
                                in-place re-normalisations in binary64 trigonometry), the shadow
                                tests use FMAs and approximate roots, the texel index comes from the
                                binary32 (tx, ty) without the certainty test. NOT bit-exact: a pixel
                                is either identical or one where a discrete decision flipped (a
                                shadow sample = 0.1 of a light's brightness, a neighbouring texel):
                                about 2 pixels in 10^5 at C3. Never the
                                default; culling kernels with the default tile and no mesh only --
                                otherwise ignored (the launch is exact)                            */
    int reflect_depth;       /* 0 (default; what a shorter struct_size reads as): no reflections, the
                                frame exactly as without this field (same kernels, same launches).
                                1..RT_MAX_REFLECT_DEPTH: mirror reflections off spheres with a non-zero
                                material reflectivness (rt_scene_set_materials), at most this many
                                bounces after the primary hit (DESIGN.md "Reflections"). Spheres only
                                unless rt_scene_set_reflect_scope(s, RT_REFLECT_SCENE); under the
                                default sampling mode spp 1 and no accumulate
                                (rt_scene_set_reflect_samples(s, RT_REFLECT_SAMPLES_MANY) lifts both);
                                no interleave_*, packed24, table_lds or profile
                                (RT_ERR_UNSUPPORTED); `fast` is ignored (the launch is exact)      */
} rt_launch_opts;

enum { RT_STAT_PRIMARY_TESTS = 0, /* sphere tests issued for primary rays (per lane) */
       RT_STAT_SHADOW_TESTS = 1,  /* sphere tests issued for shadow rays (per lane)  */
       RT_STAT_CULL_TESTS = 2,    /* sphere-vs-beam tests (per lane)                 */
       RT_STAT_HIT_PIXELS = 3,
       RT_STAT_UNSHADOWED = 4,
       RT_STAT_WAVE_TEST_SLOTS = 5, /* 64 x wave-level test iterations (issue slots) */
       RT_STAT_LIST_ENTRIES = 6,  /* sum of survivor-list lengths                     */
       RT_STAT_LIST_OVERFLOWS = 7,
       RT_STAT_PHASE0 = 8,        /* 8 per-phase cycle sums (profile builds only):
                                     ray setup, primary cull, primary tests, shading+sky,
                                     beam bound, shadow cull, sample construction, shadow tests */
       RT_STAT_CLUSTERS = 16,     /* sum over waves of distinct hit spheres per tile  */
       RT_STATS_COUNT = 24 };

/* Same argument order and meaning as the reference kernel; references become
 * pointers; `stream` is a hipStream_t (NULL = default stream). `pixels` is a
 * device-accessible buffer of width*height packed 0x00RRGGBB words. objs, lights
 * and sky are read on the HOST at call time (they live in managed/host memory
 * in the reference) and mirrored into device-resident tables; texture planes
 * are uploaded once per (pointer, size) and cached -- call
 * rt_invalidate_textures() after modifying texel data in place. */
int rt_launch_raytrace(uint32_t *pixels, int width, int height, float aspect,
                       const rt_object *objs, const rt_light *lights, int light_size,
                       rt_camera cam, const rt_skybox *sky, void *stream);
int rt_launch_raytrace_ex(uint32_t *pixels, int width, int height, float aspect,
                          const rt_object *objs, const rt_light *lights, int light_size,
                          rt_camera cam, const rt_skybox *sky, void *stream,
                          const rt_launch_opts *opts);
void rt_invalidate_textures(void);

/* ------------------------------------------------------------------ *
 * Frame driver (kernel.cuh:3-4; kernel.cu:1692-1714, 1762-1792)       *
 * The C++ symbols `void onStart(); void update();` are exported too.  *
 * ------------------------------------------------------------------ */
void rt_on_start(void);      /* builds the default scene (spheres from the MSVC rand()
                                replay, 3 lights, synthetic textures)                 */
void rt_update(void);        /* one frame: size query -> launch -> sync -> setPixelBuff */
/* Scene knobs the reference keeps as compile-time globals (kernel.cu:1231,1695-1702). */
int rt_config_set_sphere_count(int n);       /* before rt_on_start(); default 1024    */
int rt_config_set_seed(unsigned int seed);   /* MSVC rand() seed; default 1           */
/* Asset files of onStart() (kernel.cu:1700,1706 and loadMesh :1181 hard-code C:\ paths): binary
 * PPM (P6) textures and an OBJ mesh. NULL / "" = not set: onStart() then looks at the
 * application's environment (RT_OBJECT_TEXTURE, RT_SKY_TEXTURE, RT_MESH_OBJ), and without
 * those uses the synthetic textures and no mesh. Call before rt_on_start().                  */
int rt_config_set_assets(const char *object_texture, const char *sky_texture, const char *mesh_obj);
rt_camera *rt_config_camera(void);           /* the global `cam` (kernel.cu:1695)     */
rt_object *rt_config_object(void);           /* the global `objs` (kernel.cu:1699); NULL before onStart(). update()
                                                reads its sphere / plane / cube / mesh fields every frame */
rt_light *rt_config_lights(int *count);      /* the global `lights` (kernel.cu:1694)  */
float rt_default_aspect(void);               /* (float)tan(90*0.5*3.1415/180), :1701  */
double rt_last_frame_ms(void);               /* device time of the last rt_update()   */

/* ------------------------------------------------------------------ *
 * Offscreen stand-in for window.cpp (window.h:7-16). The C++ symbols   *
 * getScreenWidth/getScreenHeight/setPixelBuff/... are exported (weak)  *
 * so an application's own window.cpp overrides them.                   *
 * ------------------------------------------------------------------ */
int rt_offscreen_resize(int width, int height);   /* WM_SIZE equivalent (window.cpp:29-46),
                                                      takes the RENDER size directly  */
const uint32_t *rt_offscreen_pixels(void);        /* render.buffmemory                */
int rt_offscreen_width(void);
int rt_offscreen_height(void);
int rt_offscreen_write_ppm(const char *path);     /* dump the presented frame         */

/* ------------------------------------------------------------------ *
 * Scene construction helpers (host side, no GPU needed)               *
 * ------------------------------------------------------------------ */
/* plane(pos, normal) (kernel.cu:364-367) and cube(c1, c2) (kernel.cu:391-396). */
void rt_plane_init(rt_plane *p, float px, float py, float pz, float nx, float ny, float nz);
void rt_cube_init(rt_cube *c, float ax, float ay, float az, float bx, float by, float bz);
/* sphere::sphere(org, r) (kernel.cu:285-288): stores radius = r*r.     */
void rt_sphere_init(rt_sphere *s, float x, float y, float z, float r);
/* The scene of object::loadMesh (kernel.cu:1189-1192) with the MSVC rand()
 * LCG replayed from `seed`; draw order x, y, z, r.      */
int rt_generate_spheres(rt_sphere *out, int n, unsigned int seed);
int rt_msvc_rand_sequence(unsigned int seed, int *out, int n);
/* Deterministic synthetic textures standing in for wood.jpg / sky_box.jpg
 * (kernel.cu:1700,1706; the assets are not in the reference repo). Planes are
 * k/255 with integer k, like the 8-bit decode of Sprite.cpp:35-51.
 * kind 0 = object texture (512x512), kind 1 = sky (2048x1024).           */
int rt_synth_texture_size(int kind, int *width, int *height);
int rt_synth_texture(int kind, float *r, float *g, float *b);
/* mesh(filename) (kernel.cu:575-747) + createBvhMesh (:752-937): OBJ text (v / vt / vn /
 * f with a, a//c or a/b/c tokens, triangles and quads) -> triangles -> flat list of
 * leaf boxes. Host memory only (d_* alias h_*); no GPU needed. Blank lines, which
 * corrupt the reference's parser state, are skipped. NULL on failure.            */
rt_mesh *rt_mesh_from_obj_text(const char *text);
rt_mesh *rt_mesh_load_obj(const char *path);
void rt_mesh_free(rt_mesh *m);
/* sprite(file) without OpenCV: binary PPM (P6) -> planar float planes.    */
int rt_load_ppm(const char *path, float **r, float **g, float **b, int *width, int *height);
void rt_free_planes(float *r, float *g, float *b);
/* Sub-pixel position of sample k of n (n=1 -> 0.5,0.5: the reference).    */
int rt_sample_offset(int k, int n, double *ox, double *oy);

/* ------------------------------------------------------------------ *
 * Device-resident frame pipeline (what update() uses internally;      *
 * exposed so a host can render into its own device buffers, capture   *
 * the frame into a hipGraph, or render a row band for multi-GPU).     *
 * ------------------------------------------------------------------ */
typedef struct rt_scene rt_scene;    /* opaque, device-resident copy of one scene */

rt_scene *rt_scene_create(void);
void rt_scene_destroy(rt_scene *s);
int rt_scene_set_spheres(rt_scene *s, const rt_sphere *host_spheres, int n);
int rt_scene_set_planes(rt_scene *s, const rt_plane *host_planes, int n);   /* SURVEY.md 8(f) row 2 */
int rt_scene_set_cubes(rt_scene *s, const rt_cube *host_cubes, int n);
int rt_scene_set_mesh(rt_scene *s, const rt_mesh *mesh);    /* NULL removes it; SURVEY.md 8(f) row 4 */
int rt_scene_set_texture(rt_scene *s, const float *r, const float *g, const float *b, int w, int h);
int rt_scene_set_sky(rt_scene *s, const rt_sphere *box, const float *r, const float *g,
                     const float *b, int w, int h);
int rt_scene_set_lights(rt_scene *s, const rt_light *lights, int n);

/* material, kernel.cu:213-224 (field names as the reference spells them). Only reflectivness is
 * implemented here; a material with transperancy or roughness != 0 is RT_ERR_UNSUPPORTED
 * (transparency is set through rt_material_ex, which carries an index of refraction; roughness
 * through rt_scene_set_roughness, below "Glossy reflections"). */
typedef struct rt_material {
    float reflectivness;     /* k in [0, 1]: the share of a hit's colour taken from its mirror ray */
    float transperancy;      /* must be 0 */
    float roughness;         /* must be 0 (set it with rt_scene_set_roughness) */
} rt_material;               /* 12 bytes */

/* One material per sphere of the scene's list (n == the sphere count); NULL / 0 clears them (every
 * sphere then has k = 0). A reflectivness that is NaN or outside [0, 1]: RT_ERR_INVALID. The
 * materials survive rt_scene_set_spheres with the same count and are cleared by a different count.
 *
 * Semantics of a frame with opts.reflect_depth = D > 0, per pixel (DESIGN.md "Reflections"): R_0 is
 * the reference's primary ray, w = 1; for b = 0..D, castRay(R_b) over the spheres (sphere::intersect
 * with all its quirks, first index wins ties). A miss adds w * getFColor(R_b) and stops. A hit on
 * sphere i with k = material[i].reflectivness adds w * L (L = the reference's three-light sum at
 * that hit) and stops if k == 0 or b == D; otherwise it adds (w * (1 - k)) * L, then w = w * k and
 * R_{b+1} = ray(start_O, reflect(R_b.Dir, N)) (kernel.cu:1282-1285 in binary32, start_O = N*0.00001
 * + new_org as rayTrace forms it). The first term is assigned, later ones added, per channel in
 * binary32; rgba = (c, 1) and the packed word is rgbToInt(c * 254). A pixel whose primary hit has
 * k = 0, and every sky pixel, is the frame without reflections bit for bit. */
int rt_scene_set_materials(rt_scene *s, const rt_material *per_sphere, int n);

/* A material with transparency (DESIGN.md "Refraction"). The old rt_material has no index of
 * refraction, so it keeps refusing transperancy != 0; this one carries it. */
typedef struct rt_material_ex {
    float reflectivness;     /* k in [0, 1]                                                        */
    float transperancy;      /* tau in [0, 1]: the share of a hit's colour taken from the ray that
                                passes through the sphere                                          */
    float roughness;         /* must be 0 (RT_ERR_UNSUPPORTED; rt_scene_set_roughness sets it)     */
    float ior;               /* index of refraction, finite, in [1, 4], where tau > 0; ignored (may
                                be 0) where tau == 0                                               */
} rt_material_ex;            /* 16 bytes */

/* One material per sphere (n == the sphere count); NULL / 0 clears them. The same per-sphere table
 * as rt_scene_set_materials: the last call of either wins, and a call to rt_scene_set_materials
 * sets every tau to 0. It survives rt_scene_set_spheres with the same count and is cleared by a
 * different count. A NaN or out-of-range k, tau or ior (ior only where tau > 0): RT_ERR_INVALID;
 * roughness != 0, or k > 0 together with tau > 0 on one sphere: RT_ERR_UNSUPPORTED (one
 * continuation per hit). Nothing changes on an error.
 *
 * Semantics: the per-pixel loop of rt_scene_set_materials, binary32, no contraction, correctly
 * rounded division and sqrt, dot products left to right. At a hit on sphere i with tau > 0 and
 * b < D: new_org, N, start_O and L as for a mirror hit; the term is (w * (1 - tau)) * L, then
 * w = w * tau. refract(I, n, eta) for n facing against I: c = -dot(I, n),
 * q = 1 - (eta*eta) * (1 - c*c), s = sqrt(q > 0 ? q : 0) (no total internal reflection), result
 * I*eta + n*(eta*c - s), not renormalised. R_{b+1}:
 *   1. dot(D, N) >= 0 (a silhouette hit, or intersect()'s t == 0 case): R_{b+1} = ray(start_O, D).
 *   2. Else T = refract(D, N, 1/ior), P = N*(-0.00001f) + new_org, t1 = the FAR root of
 *      sphere::intersect for (P, T) against sphere i, (-B + sqrt(disc)) / a2, before its min.
 *   3. !(t1 > 0) (NaN, degenerate tiny spheres): R_{b+1} = ray(start_O, D).
 *   4. Else Q = P + T*t1, M = normalise(Q - c_i), U = refract(T, -M, ior),
 *      R_{b+1} = ray(M*0.00001f + Q, U).
 * A hit with b == D, or with tau == 0 and k == 0, ends the pixel with w * L. A pass through a glass
 * sphere is one bounce of reflect_depth. A ray that starts inside a sphere meets it at
 * intersect()'s negative near root, behind its origin, where dot(D, N) < 0: it takes rule 2 there.
 * Two consequences: the chord P..Q is not tested against other spheres (a sphere that overlaps a
 * glass sphere's interior is not seen from inside it), and glass casts full shadows (castLightRay
 * is unchanged). No Fresnel weighting, tint, attenuation or caustics. A scene where no sphere has
 * tau > 0 renders exactly as with rt_scene_set_materials. The drop-in boundary (object::mat) stays
 * mirror-only. */
int rt_scene_set_materials_ex(rt_scene *s, const rt_material_ex *per_sphere, int n);

/* What the last reflective frame of the scene did (a host wait for that frame): the sphere BVH
 * (host build, binary64, rebuilt when the spheres change), the queue length entering every
 * bounce, and -- when rt_scene_set_reflect_timing(s, 1) was called before the frame -- the
 * device time of every pass (hipEvents: [0] the frame kernel, [1] the primary pass, [1 + b]
 * bounce b). A supersampled frame (rt_scene_set_reflect_samples): queue[b] is summed over the
 * call's samples, pass_ms over its groups of samples ([0]: the frame kernel's launches), and the
 * resolve passes are counted in the last bounce's slot. */
typedef struct rt_reflect_stats {
    double bvh_build_ms;     /* host time of the last BVH build                                  */
    int bvh_nodes, bvh_depth, bvh_leaves;
    int depth;               /* reflect_depth of the frame                                       */
    int queue[RT_MAX_REFLECT_DEPTH + 1]; /* queue[b]: rays entering bounce b + 1                 */
    float pass_ms[RT_MAX_REFLECT_DEPTH + 2];
    int timed;               /* 1: pass_ms is filled                                              */
} rt_reflect_stats;
int rt_scene_set_reflect_timing(rt_scene *s, int on);
int rt_scene_reflect_stats(rt_scene *s, rt_reflect_stats *out);

typedef struct rt_frame_desc {
    uint32_t struct_size;
    int width, height;
    float aspect;
    rt_camera cam;
    uint32_t *pixels;        /* device, band-local (row y0 first); may be NULL        */
    rt_launch_opts opts;     /* rgba / band / spp / cull / stats                       */
    /* G-buffer outputs, appended after `opts` (rt_launch_opts keeps its layout): per-pixel
       guides of the frame's own primary ray, written by the frame kernel itself. Each is NULL (what a shorter struct_size reads as: the frame exactly as without
       these fields) or a device buffer in the row layout of `pixels` / `rgba` (band-local, compact rows
       under interleave_*). Any subset may be set; unset buffers are not touched; a set one is always
       overwritten (also with `accumulate`). On a hit they hold castRay's values, as rt_hit does for the
       pixel's ray from rt_scene_primary_rays; on a miss (sky) the values in brackets.                   */
    float *aov_depth;        /* float: castRay's nt -- negative for a sphere reached from inside     [+inf] */
    float *aov_normal;       /* float4, 16-byte aligned: castRay's normal (x, y, z, 0) -- a plane's as
                                stored, a triangle's interpolated when the mesh has normals       [0, 0, 0, 0] */
    int *aov_id;             /* int2, 8-byte aligned: (kind, index) as rt_hit -- RT_HIT_*, the list position,
                                for a triangle its position in the mesh's triangle array          [-1, -1] */
    float *aov_albedo;       /* float4, 16-byte aligned: the texel the frame multiplies the light sum by,
                                (r, g, b, 1) with the frame's clamp          [the sky texel (r, g, b, 1) = rgba] */
    /* The guides describe the pixel centre's primary ray; with reflect_depth > 0 they are those of the
       primary hit. A frame that sets any of them: one sample (spp <= 1, sample_total <= 1), tile 0 or 8, no
       stats, profile or force_slow_path (RT_ERR_UNSUPPORTED otherwise); `fast` is ignored (the launch is
       exact); cull 0 and 1, every kind of primitive, bands, interleave_*, packed24 and accumulate work.
       A misaligned pointer: RT_ERR_INVALID. Either refusal writes nothing. The drop-in rt_launch_raytrace_ex has
       none (its rt_launch_opts does not carry them); rt_multi_render refuses them (RT_ERR_UNSUPPORTED) and
       rt_graph_capture returns NULL with the field's name in rt_last_error().                              */
} rt_frame_desc;

/* fd->struct_size and fd->opts.struct_size are honoured: a caller built against an older, shorter
 * rt_frame_desc / rt_launch_opts gets its missing tail fields as 0. (0 in either reads as the
 * layout before reflect_depth was appended.) */
int rt_scene_render(rt_scene *s, const rt_frame_desc *fd, void *stream);

/* ------------------------------------------------------------------ *
 * Ray queries: what a caller's rays hit, whether they   *
 * are blocked, and the colour the frame would give them.               *
 * ------------------------------------------------------------------ */
enum { RT_HIT_NONE = -1, RT_HIT_TRIANGLE = 0, RT_HIT_SPHERE = 1, RT_HIT_PLANE = 2, RT_HIT_CUBE = 3 };   /* castRay's hit_type */

/* castRay's outputs (kernel.cu:1287-1431) for one ray; 64 bytes. A miss: t = +inf, kind = index = -1, the rest 0. */
typedef struct rt_hit {
    float t;                 /* nt (a sphere reached from inside: its negative near root); +inf on a miss          */
    int kind;                /* RT_HIT_*                                                                          */
    int index;               /* position in the scene's list; triangle: index into the mesh's triangle array      */
    float u, v;              /* nu, nv of a triangle hit, else 0                                                  */
    float tx, ty;            /* texture coordinates as castRay forms them (plane: 0.5, 0.5)                       */
    rt_vec3 normal;          /* as castRay forms it (plane: as stored, not normalised; triangle: interpolated when
                                the mesh has vertex normals)                                                      */
    rt_vec3 new_org;         /* as castRay forms it (triangle: the hit point displaced by the whole normal)       */
    uint32_t pad_[3];
} rt_hit;

#define RT_MAX_QUERY_RAYS (1 << 26)
enum { RT_QUERY_NEAREST = 0, RT_QUERY_OCCLUDED = 1, RT_QUERY_SHADE = 2 };
typedef struct rt_ray_query {
    uint32_t struct_size;    /* sizeof(rt_ray_query); 0 reads as this layout. Fields past a caller's size read as 0 */
    int mode;                /* RT_QUERY_*                                                                        */
    int n;                   /* rays, 0 <= n <= RT_MAX_QUERY_RAYS; 0: nothing is done                             */
    int cull;                /* -1 (default) or 1: spheres through the scene's sphere BVH; 0: the whole lists. The
                                results are the same bits either way                                              */
    const rt_ray *rays;      /* device, n rays, used as given (directions are not normalised)                     */
    rt_hit *hits;            /* device, n records: required for NEAREST, optional for SHADE (the primary hit)     */
    int *occluded;           /* device, n words: required for OCCLUDED                                            */
    float *rgba;             /* device, float4 per ray (SHADE): (c, 1)                                            */
    uint32_t *packed;        /* device, word per ray (SHADE): rgbToInt(c * 254). SHADE needs rgba or packed       */
} rt_ray_query;              /* rgba must be 16-byte aligned (one float4 store per ray), the other pointers 4-byte
                                aligned; RT_ERR_INVALID otherwise                                                 */

/* One query over n rays, one thread per ray, on `stream` (asynchronous; NULL = the null stream).
 *  NEAREST   castRay as the frame kernel evaluates it: mesh leaves (a leaf's triangles only if its own box passes
 *            cube::intersect), then spheres, cubes, planes; every comparison is the strict t < nt, so the first
 *            primitive found wins a tie, also across kinds. sphere::intersect, cube::intersect and Moller-Trumbore
 *            keep their quirks (negative near root from inside, the min/max macros' NaN behaviour, t >= 1e-7f).
 *  OCCLUDED  castLightRay's per-sample test (kernel.cu:1475-1536): 1 if any triangle (behind its leaf's box), sphere,
 *            plane or cube reports a hit, at any distance (the reference has no limit), else 0.
 *  SHADE     rayTrace's pixel body (kernel.cu:1633-1690) for the given ray: on a hit the texel (the frame's clamp)
 *            and the three-light sum with castLightRay from start_O = N*0.00001 + new_org, occluders of every kind;
 *            on a miss getFColor (the frame's clamp). Shading the frame's own primary rays
 *            (rt_scene_primary_rays) gives the frame's rgba and packed words bit for bit. Not a frame path: about
 *            thirty shadow traversals per hit.
 * Null or invalid arguments (a bad mode, n out of range, rays NULL with n > 0, a missing required output) return
 * RT_ERR_INVALID and write nothing; SHADE also needs the scene's texture (when it has primitives) and sky. A stream
 * that is being captured is refused (RT_ERR_UNSUPPORTED). A query is ordered after the scene's pending uploads and
 * counts as a frame in flight for the scene's update rules; the host waits only when the sphere BVH (shared with
 * reflective frames) must be rebuilt. */
int rt_scene_trace_rays(rt_scene *s, const rt_ray_query *q, void *stream);

/* The reference's primary rays (kernel.cu:1624-1631) of fd's band (opts.y0 / y1; band-local pixel order, row y0
 * first), formed exactly as the frame kernel forms them at one sample: rays_dev holds width * (y1 - y0) rays
 * (device). fd's outputs, samples, interleave and reflection fields are ignored; the scene needs what a frame
 * needs (texture, sky). */
int rt_scene_primary_rays(rt_scene *s, const rt_frame_desc *fd, rt_ray *rays_dev, void *stream);

/* ------------------------------------------------------------------ *
 * G-buffer-guided denoiser: an edge-avoiding a-trous    *
 * wavelet filter over a rendered frame, steered by the frame's guides. *
 * ------------------------------------------------------------------ */
#define RT_DENOISE_MAX_ITERATIONS 6
#define RT_DENOISE_MAX_NORMAL_SHIFT 8
#define RT_DENOISE_MAX_SIZE 32768   /* width and height */
typedef struct rt_denoise_desc {
    uint32_t struct_size;    /* sizeof(rt_denoise_desc); 0 reads as this layout. Fields past a caller's size read as 0 */
    int width, height;       /* of every buffer below: rows of `width` pixels, as a frame or a band wrote them         */
    const float *rgba_in;    /* device, float4 per pixel, 16-byte aligned: the colour to filter (rt_launch_opts.rgba)  */
    const float *depth;      /* device, the four guides in the rt_frame_desc.aov_* layouts: float, 4-byte aligned      */
    const float *normal;     /*   float4, 16-byte aligned                                                              */
    const float *albedo;     /*   float4, 16-byte aligned; may be NULL only with demodulate = 0                        */
    const int *id;           /*   int2 (kind, index), 8-byte aligned                                                   */
    float *rgba_out;         /* device, float4 per pixel, 16-byte aligned: (filtered colour, 1); may equal rgba_in     */
    uint32_t *pixels;        /* NULL, or device: the packed framebuffer of the result, rgbToInt(c * 254) as the frame  */
    int iterations;          /* 1 .. RT_DENOISE_MAX_ITERATIONS; iteration i has its taps 2^i pixels apart   [4]        */
    int normal_shift;        /* 0 .. RT_DENOISE_MAX_NORMAL_SHIFT: the normal weight is max(0, N.N')^(2^shift) [5]      */
    float sigma_depth;       /* finite, > 0: relative depth difference at which the depth weight is 1/2     [0.05]     */
    float sigma_colour;      /* finite; > 0: luminance difference at which the colour weight is 1/2; <= 0: off [0]     */
    int demodulate;          /* non-zero: filter colour / albedo and multiply the albedo back (direct light only) [1]  */
    int variant;             /* 0: the product kernels; 1: the plain one-thread-per-pixel yardstick (every tap from the
                                caller's arrays); 2: the product kernels without LDS staging (measurement). The results
                                are the same bits in all three                                                         */
} rt_denoise_desc;

/* The defaults in brackets above; sizes and pointers 0. */
void rt_denoise_desc_init(rt_denoise_desc *d);

/* Filters rgba_in into rgba_out (and `pixels`) on `stream` (a hipStream_t; NULL = the null stream): `iterations`
 * passes of a 5 x 5 B3-spline kernel {1, 4, 6, 4, 1} / 16 with holes, whose taps are weighted by how well their
 * guides agree with the centre's -- same object (id), similar normal, similar depth and, optionally, similar
 * luminance (DESIGN.md 6f gives every formula; binary32, + - * / only, so the result is defined to the bit and
 * variants 0, 1 and 2 return the same bits). A pixel with kind < 0 (sky) keeps its input bits in rgba_out, packs its
 * input colour into `pixels` and contributes to no other pixel; so does a pixel none of whose neighbours agree with
 * it, up to the demodulation round trip. Taps outside the buffer are skipped: a band is filtered as the buffer it is,
 * so bands filtered apart differ from the whole frame within 2 * (2^iterations - 1) rows of a cut.
 * demodulate = 1 assumes colour = light x albedo (frames with reflect_depth = 0); reflective frames pass 0. The
 * guides are those of one sample per pixel: a caller may filter an spp > 1 colour with the 1-spp guides of the same
 * camera.
 * The call enqueues its kernels and returns; there is no host wait (a call that is larger than any before it
 * allocates). rgba_out and `pixels` must not overlap the inputs, except that rgba_out may be rgba_in itself. The
 * scratch (two irradiance buffers and the packed guides, 52 bytes per pixel) belongs to the scene and grows on
 * demand: calls of one scene on different streams are ordered on the device, one after the other (an event, no host
 * wait); ordering the call after the frame that writes its inputs is the caller's (the same stream, or an event).
 * Before anything is enqueued, and with nothing written: NULL or misaligned pointers, sizes <= 0 or above
 * RT_DENOISE_MAX_SIZE, iterations, normal_shift or variant out of range, a sigma_depth that is not finite and > 0, a
 * sigma_colour that is not finite -> RT_ERR_INVALID; a stream that is being captured -> RT_ERR_UNSUPPORTED
 * (rt_last_error() says so). */
int rt_scene_denoise(rt_scene *s, const rt_denoise_desc *d, void *stream);

/* Device time of every launch of the scene's later denoise calls (hipEvents around each; off by default).
 * rt_scene_denoise_times waits for the last call and fills ms[0 .. *n - 1]: variants 0 and 2: [0] the pack pass,
 * [1 + i] iteration i; variant 1: [i] iteration i. cap: room in ms. */
int rt_scene_set_denoise_timing(rt_scene *s, int on);
int rt_scene_denoise_times(rt_scene *s, float *ms, int cap, int *n);

/* ------------------------------------------------------------------ *
 * Temporal accumulation: a frame's history, reprojected *
 * into the current view by the frame's own G-buffer.                   *
 * ------------------------------------------------------------------ */
#define RT_TEMPORAL_MAX_HISTORY 256
typedef struct rt_temporal_desc {
    uint32_t struct_size;        /* sizeof(rt_temporal_desc); 0 reads as this layout. Fields past a caller's size read as 0 */
    int width, height;           /* of every buffer below: whole frames, rows of `width` pixels                            */
    float aspect;                /* the view the current buffers were rendered with (rt_frame_desc.aspect / cam)           */
    rt_camera cam;
    float prev_aspect;           /* the view the prev_* buffers were rendered with                                         */
    rt_camera prev_cam;
    const float *rgba_in;        /* device, float4, 16-byte aligned: the current colour (may be a jittered sample's)       */
    const float *depth;          /* device, the current guides in the rt_frame_desc.aov_* layouts: float, 4-byte aligned   */
    const float *normal;         /*   float4, 16-byte aligned                                                              */
    const int *id;               /*   int2 (kind, index), 8-byte aligned                                                   */
    const float *prev_rgba;      /* device, float4: (accumulated colour, history length n) -- a former rgba_out            */
    const float *prev_depth;     /* device: the guides of the frame that former call accumulated, same layouts             */
    const float *prev_normal;
    const int *prev_id;
    const float *prev_moments;   /* NULL, or device, float2, 8-byte aligned: a former moments_out                          */
    float *rgba_out;             /* device, float4, 16-byte aligned: (new accumulated colour, new n)                       */
    float *moments_out;          /* NULL, or device, float2, 8-byte aligned: running means of (luma, luma^2); needs
                                    prev_moments unless `reset`                                                            */
    uint32_t *pixels;            /* NULL, or device: the packed framebuffer of rgba_out's colour, rgbToInt(c * 254)        */
    int reset;                   /* non-zero: no history is read (every prev_* may be NULL): rgba_out = (colour, 1)        */
    int max_history;             /* 1 .. RT_TEMPORAL_MAX_HISTORY: n stops growing there (weight 1 / n of a new frame) [32] */
    float depth_tolerance;       /* finite, > 0: relative, on squared distances to the previous eye               [0.02]   */
    float normal_cos_min;        /* in [0, 1]: smallest cosine between the two normals                            [0.9]    */
    int variant;                 /* 0: the product kernel; 1: the plain one-thread-per-pixel yardstick. The same bits      */
} rt_temporal_desc;

/* The defaults in brackets above (the interface's own choices, not measurements); sizes, views and pointers 0. */
void rt_temporal_desc_init(rt_temporal_desc *d);

/* Blends the current colour into the history on `stream` (a hipStream_t; NULL = the null stream). Per pixel: its
 * world point (its primary ray, formed as rt_scene_primary_rays forms it, times `depth`) is taken into the previous
 * view; the four previous pixels around where it lands are kept if they show the same surface -- equal id, a distance
 * to the previous eye that agrees with prev_depth within depth_tolerance, a normal within normal_cos_min -- and
 * blended bilinearly into a history (colour H, length n_prev); the result is H + (c - H) / n with
 * n = min(n_prev + 1, max_history), and the luminance moments likewise. A pixel without history -- `reset`, sky, a
 * depth that is not finite and > 0, a point behind the previous eye or outside its frame, no agreeing tap -- gets
 * (c, 1). With cam / aspect equal to prev_cam / prev_aspect byte for byte the only tap is the pixel itself with
 * weight 1: a standing camera gives the exact running mean. DESIGN.md 6i gives every formula; binary32, + - * / and
 * compares only, so the result is defined to the bit and both variants return the same bits.
 * The scene is assumed static between the two frames: there are no motion vectors, a moved object is rejected by
 * its depth or only by chance. A caller that moves objects or lights passes `reset`, or calls
 * rt_scene_temporal_motion below, which takes a displacement per sphere and cube and clamps the history.
 * The call enqueues one kernel and returns; there is no host wait (the first call of a size or aspect uploads that
 * view's ray tables). The pass gathers: no output may overlap an input. Calls of one scene on different streams are
 * ordered on the device, one after the other (an event); ordering the call after the frames that wrote its inputs is
 * the caller's. Before anything is enqueued, and with nothing written: NULL or misaligned pointers (float4 buffers
 * 16 bytes, id and moments 8, depth and pixels 4), sizes <= 0 or above RT_DENOISE_MAX_SIZE, max_history, variant,
 * depth_tolerance or normal_cos_min out of range or not finite, an aspect that is not finite and > 0, missing prev_*
 * without `reset`, moments_out without prev_moments unless `reset`, an output that overlaps an input or another
 * output -> RT_ERR_INVALID; a stream that is being captured -> RT_ERR_UNSUPPORTED. */
int rt_scene_temporal(rt_scene *s, const rt_temporal_desc *d, void *stream);

/* Temporal accumulation over moving spheres and cubes, with a history clamp. Every field of
 * rt_temporal_desc, in the same order and with the same meaning, then the motion and the clamp. */
typedef struct rt_tmotion_desc {
    uint32_t struct_size;        /* sizeof(rt_tmotion_desc); 0 reads as this layout. Fields past a caller's size read as 0 */
    int width, height;
    float aspect;
    rt_camera cam;
    float prev_aspect;
    rt_camera prev_cam;
    const float *rgba_in;
    const float *depth;
    const float *normal;
    const int *id;
    const float *prev_rgba;
    const float *prev_depth;
    const float *prev_normal;
    const int *prev_id;
    const float *prev_moments;
    float *rgba_out;
    float *moments_out;
    uint32_t *pixels;
    int reset;
    int max_history;             /*                                                                                 [32]   */
    float depth_tolerance;       /*                                                                                 [0.02] */
    float normal_cos_min;        /*                                                                                 [0.9]  */
    int variant;                 /* 0: the product kernel; 1: the plain one-thread-per-pixel yardstick. The same bits      */
    const float *sphere_motion;  /* NULL, or device, float4 per sphere, 16-byte aligned: .xyz = the sphere's centre now
                                    minus its centre in the frame the history was accumulated over; .w is ignored [NULL]   */
    int n_sphere_motion;         /* spheres the array covers; a sphere at or past it did not move (0 with NULL)     [0]    */
    const float *cube_motion;    /* the same per cube: a translation of both corners                                [NULL] */
    int n_cube_motion;           /*                                                                                 [0]    */
    int clamp;                   /* non-zero: the reprojected history is clamped to the colour box of the current
                                    frame's 3 x 3 neighbourhood                                                     [1]    */
    float clamp_slack;           /* finite, in [0, 16]: each side of the box is widened by this share of its extent [0.25] */
    int clamp_history;           /* 1 .. RT_TEMPORAL_MAX_HISTORY: where the clamp changed the history colour, the
                                    history length counts as at most this                                           [4]    */
} rt_tmotion_desc;

/* The defaults in brackets above (the interface's own choices, not measurements); sizes, views and pointers 0. */
void rt_tmotion_desc_init(rt_tmotion_desc *d);

/* rt_scene_temporal for scenes whose spheres and cubes move by translation and whose lights move. Per pixel, the
 * displacement m of the object its id names (spheres and cubes inside their tables; planes, triangles and everything
 * else: 0) is taken out of the world point before that goes into the previous view, so the depth test compares
 * prev_depth with where the surface point was; a displacement that is not finite leaves the pixel at (c, 1). With
 * identical views a pixel whose m is zero takes rt_scene_temporal's single tap (a standing camera keeps the exact
 * running mean on everything that did not move); a mover goes through the reprojection. With `clamp`, the
 * reprojected history colour H is clamped per channel to [lo - e, hi + e], lo / hi the minimum / maximum of rgba_in
 * over the 3 x 3 pixels around the pixel that lie inside the buffer and e = (hi - lo) * clamp_slack; where that
 * changed H the history length is cut to clamp_history before the blend (a shadow that travelled over a pixel is
 * forgotten within a few frames). DESIGN.md 6k gives every formula; both variants return the same bits, and with both
 * counts 0 and clamp = 0 they are rt_scene_temporal's. Rotation and scaling, moving planes and meshes and per-pixel
 * motion vectors are out of scope; lights carry no motion of their own: the clamp answers a moved light, and `reset`
 * remains. The host side is rt_scene_temporal's: one kernel, no host wait but the ray-table upload of a new size or
 * aspect, ordered with every temporal call of the scene, timed by rt_scene_set_temporal_timing. Refused with
 * RT_ERR_INVALID before anything is enqueued: everything rt_scene_temporal refuses, a negative count, a count > 0
 * with a NULL array, a motion array that is not 16-byte aligned, clamp_slack not finite or outside [0, 16],
 * clamp_history out of range, an output that overlaps a motion array; a capturing stream: RT_ERR_UNSUPPORTED. */
int rt_scene_temporal_motion(rt_scene *s, const rt_tmotion_desc *d, void *stream);

/* What the kernels get as uniforms for a view, pure host code: out[0..2] the origin of every primary ray
 * (eyePos + cam.Org), out[3..6] cos_pitch, sin_pitch, cos_yaw, sin_yaw of camera::rotateDir. */
int rt_view_terms(int width, int height, float aspect, const rt_camera *cam, float out[7]);

/* Device time of the scene's later temporal calls (hipEvents around the launch; off by default).
 * rt_scene_temporal_times waits for the last call and fills ms[0 .. *n - 1] (one launch: *n <= 1). cap: room in ms. */
int rt_scene_set_temporal_timing(rt_scene *s, int on);
int rt_scene_temporal_times(rt_scene *s, float *ms, int cap, int *n);

/* ------------------------------------------------------------------ *
 * Variance-guided denoiser: rt_scene_denoise's filter   *
 * with a luminance threshold per pixel, scaled by the variance that    *
 * rt_scene_temporal's moments (or the neighbourhood) show there.       *
 * ------------------------------------------------------------------ */
typedef struct rt_vdenoise_desc {
    uint32_t struct_size;    /* sizeof(rt_vdenoise_desc); 0 reads as this layout. Fields past a caller's size read as 0 */
    int width, height;       /* as rt_denoise_desc, field for field, down to `pixels`                                   */
    const float *rgba_in;    /* device, float4, 16-byte aligned: the colour to filter; with `moments`, w is the history
                                length n that rt_scene_temporal wrote beside them                                       */
    const float *depth;
    const float *normal;
    const float *albedo;     /*   may be NULL only with demodulate = 0                                                  */
    const int *id;
    float *rgba_out;         /* device, float4, 16-byte aligned: (filtered colour, 1); may equal rgba_in                */
    uint32_t *pixels;        /* NULL, or device: the packed framebuffer of the result                                   */
    const float *moments;    /* NULL, or device, float2, 8-byte aligned: a moments_out of rt_scene_temporal     [NULL]  */
    float *variance_out;     /* NULL, or device, float, 4-byte aligned: the variance after the last iteration, in the
                                filter's domain (of the demodulated luminance when demodulating); 0 for sky     [NULL]  */
    int iterations;          /* 1 .. RT_DENOISE_MAX_ITERATIONS                                                  [4]     */
    int normal_shift;        /* 0 .. RT_DENOISE_MAX_NORMAL_SHIFT                                                [5]     */
    float sigma_depth;       /* finite, > 0                                                                     [0.05]  */
    float sigma_colour;      /* finite, 0 .. 2^20: the luminance threshold in standard deviations               [4]     */
    float sigma_floor;       /* finite, > 0: the luminance threshold where the variance is 0                    [2^-6]  */
    int min_history;         /* 1 .. RT_TEMPORAL_MAX_HISTORY: a pixel whose n is below it (or every pixel, without
                                `moments`) takes its variance from its 7 x 7 neighbourhood                      [4]     */
    float spatial_boost;     /* finite, >= 0: factor on that spatial estimate                                   [4]     */
    int demodulate;          /* as rt_denoise_desc                                                              [1]     */
    int variant;             /* 0: the product kernels; 1: the plain one-thread-per-pixel yardstick; 2: the product
                                kernels with the direct kernel instead of the LDS-staged one at step 16 (measurement:
                                DESIGN.md 6j). The same bits in all three                                               */
} rt_vdenoise_desc;

/* The defaults in brackets above (the interface's own choices -- those of the SVGF filter this stage restates -- not
 * measurements); sizes and pointers 0. */
void rt_vdenoise_desc_init(rt_vdenoise_desc *d);

/* rt_scene_denoise with a per-pixel colour weight: e_c = S / (S + g g), S(p) = sigma_colour^2 * (the 3 x 3 mean of the
 * variance around p) + sigma_floor^2. The variance of a pixel starts as max(m2 - m1 m1, 0) of `moments` (divided by
 * the squared luminance of the albedo when demodulating) where rgba_in.w >= min_history, elsewhere as spatial_boost
 * times the variance of the luminance over the agreeing pixels of its 7 x 7 neighbourhood; every iteration carries it
 * along as sum(w w v) / (sum w)^2. Where the history has converged the threshold is sigma_floor and edges the history
 * resolved stay; where it is short the threshold opens and the noise is filtered. DESIGN.md 6j gives every formula;
 * binary32, + - * / and compares only: defined to the bit, all variants return the same bits, and with a variance of 0
 * (or sigma_colour = 0) the result is rt_scene_denoise's with sigma_colour = sigma_floor.
 * Host behaviour is rt_scene_denoise's: the call enqueues and returns; the scratch is the scene's denoise scratch and
 * two variance arrays (60 bytes per pixel), so calls of this entry point and of rt_scene_denoise on one scene, on
 * whatever streams, are ordered on the device by one event. rgba_out may be rgba_in itself; no other output may overlap
 * an input or another output. Before anything is enqueued, and with nothing written: what rt_scene_denoise refuses,
 * misaligned moments or variance_out, sigma_colour, sigma_floor, min_history or spatial_boost out of range or not
 * finite, an overlap -> RT_ERR_INVALID; a stream that is being captured -> RT_ERR_UNSUPPORTED. */
int rt_scene_denoise_variance(rt_scene *s, const rt_vdenoise_desc *d, void *stream);

/* Device time of every launch of the scene's later variance-guided calls (off by default). rt_scene_vdenoise_times
 * waits for the last call and fills ms[0 .. *n - 1]: variants 0 and 2: [0] the pack pass, [1] the spatial-estimate
 * pass, [2 + i] iteration i; variant 1: [0] the initial variance, [1 + i] iteration i. cap: room in ms. */
int rt_scene_set_vdenoise_timing(rt_scene *s, int on);
int rt_scene_vdenoise_times(rt_scene *s, float *ms, int cap, int *n);

/* ------------------------------------------------------------------ *
 * Guided upsampling: a colour rendered at a lower       *
 * resolution brought to full resolution, steered by both frames'       *
 * guides.                                                              *
 * ------------------------------------------------------------------ */
typedef struct rt_upsample_desc {
    uint32_t struct_size;         /* sizeof(rt_upsample_desc); 0 reads as this layout. Fields past a caller's size read as 0 */
    int width, height;            /* full resolution ("hi"), W x H: of depth .. source                                      */
    int lo_width, lo_height;      /* low resolution ("lo"), w x h, w <= W and h <= H: of rgba_lo .. id_lo                   */
    const float *rgba_lo;         /* device, float4, 16-byte aligned: the colour to upsample                                */
    const float *depth_lo;        /* device, the lo frame's guides in the rt_frame_desc.aov_* layouts: float, 4-byte aligned */
    const float *normal_lo;       /*   float4, 16-byte aligned                                                              */
    const float *albedo_lo;       /*   float4, 16-byte aligned; may be NULL only with demodulate = 0                        */
    const int *id_lo;             /*   int2 (kind, index), 8-byte aligned                                                   */
    const float *depth;           /* device, the hi frame's guides, same layouts                                            */
    const float *normal;
    const float *albedo;          /*   may be NULL only with demodulate = 0                                                 */
    const int *id;
    const float *base;            /* NULL, or device, float4, 16-byte aligned, W x H: what a pixel that is not upsampled
                                     takes, all four words (the plain frame); may be rgba_out itself                [NULL]  */
    float *rgba_out;              /* device, float4, 16-byte aligned, W x H                                                 */
    uint32_t *pixels;             /* NULL, or device: the packed framebuffer of rgba_out, rgbToInt(c * 254)                 */
    uint8_t *source;              /* NULL, or device, a byte per hi pixel: 1 upsampled, 0 sky or not selected, 2 selected
                                     but without a counting tap                                                             */
    const uint8_t *sphere_select; /* NULL, or device, a byte per sphere: non-zero = its pixels are upsampled         [NULL] */
    int n_sphere_select;          /* spheres the table covers; an index at or past it reads as 0                     [0]    */
    const uint8_t *plane_select;  /* the same per plane                                                                     */
    int n_plane_select;
    const uint8_t *cube_select;   /* the same per cube (a triangle always reads as 0)                                       */
    int n_cube_select;
    int use_tables;               /* 0: every hit pixel is selected, the tables are not read; else only those named  [0]    */
    int normal_shift;             /* 0 .. RT_DENOISE_MAX_NORMAL_SHIFT: as rt_denoise_desc                            [5]    */
    float sigma_depth;            /* finite, > 0: as rt_denoise_desc                                                 [0.05] */
    int demodulate;               /* non-zero: upsample colour / albedo_lo and multiply the hi albedo back           [1]    */
    int variant;                  /* 0: the product kernel, one thread per hi pixel; 1: at the exact 2 x ratio a second
                                     implementation (a lane per 2 x 2 quad, neighbouring lo columns from neighbouring
                                     lanes; slower, kept for the cross-check), else the same kernel. The same bits          */
} rt_upsample_desc;

/* The defaults in brackets above; sizes and pointers 0. */
void rt_upsample_desc_init(rt_upsample_desc *d);

/* Brings rgba_lo to W x H on `stream` (a hipStream_t; NULL = the null stream). A hi pixel is selected if it shows an
 * object (kind >= 0) and, with use_tables, its object's table entry is non-zero. A selected pixel takes the weighted
 * mean of the four lo pixels around its centre ((x + 0.5) w / W - 0.5), each weighted by its bilinear factor times
 * rt_scene_denoise's normal and depth factors with the hi pixel as the centre, and counted only if it shows the same
 * object; demodulated, the lo colours are divided by albedo_lo first and the mean is multiplied by the hi albedo.
 * Every other pixel -- sky, not selected, no counting tap -- takes base's four words, or without base the plain
 * bilinear mean of rgba_lo. DESIGN.md 6l gives every formula; binary32, + - * / and compares only, so the result is
 * defined to the bit and both variants return the same bits.
 * The call enqueues one kernel and returns; there is no host wait. Calls of one scene on different streams are ordered
 * on the device, one after the other (an event); ordering the call after the frames that wrote its inputs is the
 * caller's. Before anything is enqueued, and with nothing written: NULL or misaligned required pointers (float4
 * buffers 16 bytes, id 8, depth and pixels 4), sizes <= 0 or above RT_DENOISE_MAX_SIZE, lo_width > width or
 * lo_height > height, normal_shift or variant out of range, a sigma_depth that is not finite and > 0, demodulate
 * without both albedos, a negative count, a count > 0 with a NULL table, an output that overlaps an input or another
 * output (only rgba_out may be base itself: a pixel reads only its own base pixel) -> RT_ERR_INVALID; a stream that
 * is being captured -> RT_ERR_UNSUPPORTED. */
int rt_scene_upsample(rt_scene *s, const rt_upsample_desc *d, void *stream);

/* Device time of the scene's later upsample calls (hipEvents around the launch; off by default).
 * rt_scene_upsample_times waits for the last call and fills ms[0 .. *n - 1] (one launch: *n <= 1). cap: room in ms. */
int rt_scene_set_upsample_timing(rt_scene *s, int on);
int rt_scene_upsample_times(rt_scene *s, float *ms, int cap, int *n);

/* ------------------------------------------------------------------ *
 * The display transform: the stage that ends the       *
 * chain. A float colour of high dynamic range is metered, exposed,    *
 * tone-mapped and packed, linearly or sRGB-encoded.                    *
 * ------------------------------------------------------------------ */
#define RT_DISPLAY_BINS 512            /* luminance bins: sixteen per octave from 2^-16 to 2^16 */
#define RT_DISPLAY_METER_MANUAL 0
#define RT_DISPLAY_METER_AUTO 1
#define RT_DISPLAY_METER_LAGGED 2
#define RT_DISPLAY_CLIP 0
#define RT_DISPLAY_REINHARD 1
#define RT_DISPLAY_ACES 2
#define RT_DISPLAY_LINEAR 0
#define RT_DISPLAY_SRGB 1

typedef struct rt_display_desc {
    uint32_t struct_size;         /* sizeof(rt_display_desc); 0 reads as this layout. Fields past a caller's size read as 0  */
    int width, height;            /* whole frames, each in [1, RT_DENOISE_MAX_SIZE]                                          */
    const float *rgba_in;         /* device, float4, 16-byte aligned: the colour to show                                     */
    const int *id;                /* NULL, or device, int2 (kind, index), 8-byte aligned: read by the metering only          */
    float *rgba_out;              /* NULL, or device, float4, 16-byte aligned: the display-linear colour after the curve,
                                     alpha copied bit for bit; may be rgba_in itself                                         */
    uint32_t *pixels;             /* NULL, or device: the packed words                                                       */
    float *state;                 /* device, float[4], 16-byte aligned, kept by the caller from call to call like a temporal
                                     history: {exposure, metered luminance, metered share of the pixels, valid}; all zero =
                                     no state yet. Required unless meter is RT_DISPLAY_METER_MANUAL, which does not touch it  */
    uint32_t *histogram_out;      /* NULL, or device, uint32[RT_DISPLAY_BINS]: the metered histogram (not with MANUAL)       */
    int meter;                    /* RT_DISPLAY_METER_*                                                             [AUTO]   */
    float exposure;               /* finite, > 0: the manual exposure, and the fallback where nothing can be metered   [1]   */
    float key;                    /* finite, > 0: the metered luminance is brought to it                            [0.18]   */
    float min_exposure;           /* finite, > 0, min <= max: the limits of a metered exposure              [2^-6]           */
    float max_exposure;           /*                                                                          [2^6]          */
    int meter_low, meter_high;    /* the window of the ranked luminances in 1/1024ths, 0 <= low < high <= 1024 [512] [973]   */
    float adapt;                  /* in (0, 1]: the share of the way from the state's exposure to the metered one       [1]   */
    int meter_sky;                /* non-zero: pixels without a hit (id kind < 0) are metered too                       [0]   */
    int curve;                    /* RT_DISPLAY_CLIP, _REINHARD, _ACES                                               [ACES]   */
    float white;                  /* finite, > 0: Reinhard's white point                                               [4]   */
    int transfer;                 /* RT_DISPLAY_LINEAR (rgbToInt(c * 254), today's pack), RT_DISPLAY_SRGB            [SRGB]   */
    int variant;                  /* 0: the product (a strided kernel, the histogram and the thresholds in LDS); 1: the
                                     plain yardstick (a thread per pixel, global atomics, the table from global memory, a
                                     serial resolve). The same bits                                                          */
} rt_display_desc;

/* The defaults in brackets above; sizes and pointers 0. */
void rt_display_desc_init(rt_display_desc *d);

/* T[0 .. 255], the thresholds of the sRGB encoding: T[0] = 0, T[v] = the binary32 nearest to EOTF((v - 0.5) / 255) with
 * EOTF(c) = c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4), formed in binary64 on the host; strictly
 * increasing. A channel's code is the number of v in 1 .. 255 with o >= T[v]. The kernels read this very table. */
int rt_display_transfer_table(float out[256]);

/* Shows rgba_in on `stream` (a hipStream_t; NULL = the null stream); (r, g, b, a) = rgba_in[p]. Binary32 + - * / and
 * compares on colours, integers on the histogram, T for the encoding: defined to the bit, both variants the same bits.
 * 1. Metering (AUTO, LAGGED): l = (0.2126 r + 0.7152 g) + 0.0722 b. p is metered iff l > 0, l is finite and (meter_sky
 *    != 0, or id is NULL, or id[p].kind >= 0); its bin is k = clamp((bits(l) >> 19) - 1776, 0, 511); h[k] counts.
 * 2. Resolve: N = sum h; e0 = state[0] and valid0 = (state[3] == 1) as they were on entry. N == 0: e = valid0 ? e0 :
 *    exposure, the state becomes (e, 0, 0, 1) and histogram_out is not written. Otherwise, in 64-bit integers, lo =
 *    (N meter_low) >> 10, hi = (N meter_high + 1023) >> 10; with cum the exclusive prefix sum of h, take_k = max(0,
 *    min(cum[k + 1], hi) - max(cum[k], lo)); s = sum take_k k; m = (256 s) / (hi - lo); Lm = the float with the bits
 *    (1776 << 19) + (m << 11) + (1 << 18); et = key / Lm, raised to min_exposure, then lowered to max_exposure; e =
 *    (valid0 and adapt < 1) ? e0 + (et - e0) adapt : et; the state becomes (e, Lm, float(N) / float(width height), 1)
 *    and histogram_out receives h.
 * 3. The exposure applied, E: MANUAL: exposure; AUTO: the e this call resolved; LAGGED: valid0 ? e0 : exposure -- the
 *    frame is shown with the exposure its predecessor resolved and read once.
 * 4. The curve on c = (r E, g E, b E). CLIP: o = c. REINHARD: L = max(luma(c), 0), o = c ((1 + L / (white white)) /
 *    (1 + L)). ACES, per channel: x = min(max(c, 0), 1024), o = (x (2.51 x + 0.03)) / (x (2.43 x + 0.59) + 0.14).
 *    After REINHARD and ACES o = min(max(o, 0), 1) (a NaN gives 0). rgba_out[p] = (o, a).
 * 5. The pack. LINEAR: rgbToInt(o * 254). SRGB: (code(o.r) << 16) + (code(o.g) << 8) + code(o.b) by T; a NaN gives 0.
 * With MANUAL, exposure 1, CLIP and LINEAR the call returns rgba_in's own bits and the frame's own packed words.
 * A call with both outputs NULL and a metering mode only meters. The call enqueues (AUTO: the metering, the resolve,
 * the apply pass; LAGGED: one fused pass, the resolve; MANUAL: the apply pass) and returns; E is read from `state` on
 * the device and there is no host wait. The histogram scratch is the scene's and is cleared at the head of every call;
 * calls of one scene on different streams are ordered on the device, one after the other (an event). Ordering the call
 * after the work that wrote rgba_in, id and state, and a reader of the outputs and of state after the call, is the
 * caller's. Before anything is enqueued, and with nothing written: NULL or misaligned pointers (rgba_in, rgba_out and
 * state 16 bytes, id 8, pixels and histogram_out 4), sizes, meter, curve, transfer or variant out of range, knobs
 * that are not finite or out of range, no output with MANUAL, state missing with AUTO or LAGGED, an output that
 * overlaps an input or another output (only rgba_out may be rgba_in itself) -> RT_ERR_INVALID; a stream that is being
 * captured -> RT_ERR_UNSUPPORTED. */
int rt_scene_display(rt_scene *s, const rt_display_desc *d, void *stream);

/* Device time of every launch of the scene's later display calls (off by default). rt_scene_display_times waits for
 * the last call and fills ms[0 .. *n - 1]: AUTO: metering, resolve, apply; LAGGED: the fused pass, resolve; MANUAL: the
 * apply pass. cap: room in ms. */
int rt_scene_set_display_timing(rt_scene *s, int on);
int rt_scene_display_times(rt_scene *s, float *ms, int cap, int *n);

/* ------------------------------------------------------------------ *
 * The bloom pass: the stage ahead of the display       *
 * transform that makes a bright source look bright. The part of a     *
 * float colour above a luminance threshold is filtered down a pyramid *
 * of half-resolution levels, walked back up and added to the frame,   *
 * on the linear colour, before exposure and curve.                    *
 * ------------------------------------------------------------------ */
#define RT_BLOOM_MAX_LEVELS 8
#define RT_BLOOM_MAX_EVENTS 16         /* timed launches of a call at most: 2 levels */

typedef struct rt_bloom_desc {
    uint32_t struct_size;         /* sizeof(rt_bloom_desc); 0 reads as this layout. Fields past a caller's size read as 0    */
    int width, height;            /* whole frames, each in [1, RT_DENOISE_MAX_SIZE]                                          */
    const float *rgba_in;         /* device, float4, 16-byte aligned: the linear colour of high dynamic range                */
    const float *state;           /* NULL, or device, float[4], 16-byte aligned: the display transform's state, read only    */
    float *rgba_out;              /* NULL, or device, float4, 16-byte aligned: the colour with its glare, alpha copied bit
                                     for bit; may be rgba_in itself                                                          */
    uint32_t *pixels;             /* NULL, or device: rgbToInt(rgba_out * 254), today's pack                                 */
    float *glow_out;              /* NULL, or device, float4, 16-byte aligned: (T, 0), the glare alone before `strength`     */
    int levels;                   /* in [1, RT_BLOOM_MAX_LEVELS]: the pyramid's levels                                 [5]   */
    float threshold;              /* finite, >= 0: the luminance on the screen's scale above which light blooms        [1]   */
    float limit;                  /* finite, > 0: the ceiling of a bright channel on the screen's scale               [64]   */
    float spread;                 /* finite, in [0, 4]: the weight of every coarser level on the way up             [0.75]   */
    float strength;               /* finite, >= 0: the weight of the glare in the frame                            [0.125]   */
    int variant;                  /* 0: the product (LDS-staged tiles); 1: the plain yardstick (a thread per output pixel,
                                     16 and 4 taps from global memory). The same bits                                        */
} rt_bloom_desc;

/* The defaults in brackets above; sizes and pointers 0. They are choices of taste, not measurements: five levels reach
 * 32 pixels either way, a threshold of 1 is the screen's white, and the glare of a source far above it stays an
 * eighth of what it spreads. */
void rt_bloom_desc_init(rt_bloom_desc *d);

/* Blooms rgba_in on `stream` (a hipStream_t; NULL = the null stream). Binary32 + - *, one / and compares, in the order
 * written: defined to the bit, both variants the same bits. w_0 x h_0 is the frame, w_k = (w_{k-1} + 1) >> 1 and h_k
 * likewise for k = 1 .. L = levels (a level may be one pixel wide or high); clampx clamps a column index to the
 * source's [0, ws - 1], clampy a row index to [0, hs - 1]; luma(r, g, b) = (0.2126 r + 0.7152 g) + 0.0722 b.
 * 1. Scale: E = 1 if state is NULL or state[3] != 1, else state[0]; t = threshold / E, lim = limit / E. A frame that
 *    rt_scene_display exposes at E blooms what will end above `threshold` on the screen's scale. The state is read on
 *    the device: no call waits on the host.
 * 2. Bright pass, (r, g, b, a) = rgba_in[p]: l = luma(r, g, b). If l is finite and l > t: s = (l - t) / l and per
 *    channel v = c s, v = v > 0 ? v : 0 (a NaN gives 0), v = v > lim ? lim : v. Otherwise v = 0. Br(p) = (v, 0) is
 *    never stored: the first downsample evaluates it at each tap.
 * 3. Down, from a source S of ws x hs to (x, y) of the next level, per channel: x0 = clampx(2x - 1), x1 = 2x, x2 =
 *    clampx(2x + 1), x3 = clampx(2x + 2), rows y0 .. y3 likewise; H(j) = ((S(x0, j) + S(x3, j)) + 3 (S(x1, j) +
 *    S(x2, j))) 0.125 for j = y0 .. y3; D = ((H(y0) + H(y3)) + 3 (H(y1) + H(y2))) 0.125. B_1 = Down(Br), B_k =
 *    Down(B_{k-1}).
 * 4. Up, from a source S of wc x hc to (x, y) of the level below: cx = x >> 1, nx = clampx(cx + ((x & 1) ? 1 : -1)),
 *    cy and ny likewise; G(j) = 0.75 S(cx, j) + 0.25 S(nx, j) for j = cy, ny; U = 0.75 G(cy) + 0.25 G(ny).
 * 5. Chain: A_L = B_L; A_k = B_k + spread Up(A_{k+1}) for k = L - 1 .. 1; T = Up(A_1) at w_0 x h_0.
 * 6. Combine, per channel: o = (T == 0) ? c : c + strength T. rgba_out[p] = (o, a), pixels[p] = rgbToInt(o * 254),
 *    glow_out[p] = (T, 0).
 * A pixel that nothing bright reaches keeps its own bits, -0 and NaN included; a frame with nothing above t comes back
 * as itself, its pixels the frame's own packed words. The call enqueues 2 levels launches (the downsamples, the
 * upsamples, the combine) and returns. The pyramid is the scene's, sum of w_k h_k float4, grown on demand (only then
 * the host waits for the scene's earlier bloom calls) and never shrunk; calls of one scene on different streams are
 * ordered on the device, one after the other (an event). Ordering the call after the work that wrote rgba_in and
 * state, and a reader of the outputs after the call, is the caller's. Before anything is enqueued, and with nothing
 * written: NULL or misaligned pointers (rgba_in, state, rgba_out and glow_out 16 bytes, pixels 4), sizes, levels or
 * variant out of range, threshold not finite or < 0, limit not finite or <= 0, spread not finite or outside [0, 4],
 * strength not finite or < 0, no output at all, an output that overlaps an input or another output (only rgba_out may
 * be rgba_in itself: the combine reads rgba_in[p] alone, after the first downsample has finished) -> RT_ERR_INVALID; a
 * stream that is being captured -> RT_ERR_UNSUPPORTED. */
int rt_scene_bloom(rt_scene *s, const rt_bloom_desc *d, void *stream);

/* Device time of every launch of the scene's later bloom calls (off by default). rt_scene_bloom_times waits for the
 * last call and fills ms[0 .. *n - 1], *n = 2 levels <= RT_BLOOM_MAX_EVENTS: the downsamples from the frame on, the
 * upsamples from the coarsest level on, the combine. cap: room in ms. */
int rt_scene_set_bloom_timing(rt_scene *s, int on);
int rt_scene_bloom_times(rt_scene *s, float *ms, int cap, int *n);

/* Order in which a launch starts its tiles. 1 (default): in blocks of 16 x 16 tiles, the block with the longest
 * tile first -- the frame kernel records every tile's wave duration, and from the previous launch's durations the
 * blocks are sorted on the device (three small kernels, ~15 us): after 1, 2, 4, 8, 16, 32, 64, 96, ... launches of an
 * unchanged view (camera, sphere list) and layout (frame size, rows, tile shape), every third launch while the view
 * keeps changing. A launch then ends with its cheap tiles instead of draining the SIMDs behind a few expensive ones
 * (C3: 0.38 -> 0.35 ms per frame, an eighth of the frame 0.085 -> 0.071 ms; a moving camera 0.398 -> 0.381 ms).
 * 0: grid order. Scheduling only: the pixels are the same bits either way. A frame graph sorts its own order at the
 * head of every replay (from the durations of the previous one).                                                  */
int rt_scene_set_tile_order(rt_scene *s, int mode);

/* Per-view candidate lists of the primary rays. 1 (default): for every view (ray origin, rotation, frame size, aspect)
 * the frame is cut into blocks of pixels (64 x 64 at full-HD and above, smaller at small frames) and the spheres the
 * primary rays of each block can hit are listed front to back once, on the device, beside the previous frame; the
 * tiles of every frame of that view walk their block's list instead of each culling and ordering the sphere table for
 * itself. A resting camera builds once, a moving one once per frame. Only where the scene has eye cones (64 spheres
 * or more) and whole tiles nest in the blocks; a block with more than 64 candidates leaves its tiles on the old
 * path. 0: every tile culls for itself. The pixels are the same bits either way. A frame graph builds its own lists. */
int rt_scene_set_view_lists(rt_scene *s, int mode);
typedef struct rt_view_lists_info {
    int read;                  /* 1: the last launch on the scene read view lists (else everything below is 0) */
    int block_w, block_h;      /* pixels */
    int blocks_x, blocks_y, blocks;
    int overflowed;            /* blocks with more than 64 candidates (their tiles cull for themselves) */
    int not_built;             /* blocks without a usable cone (likewise) */
    int longest;               /* longest list */
    float mean;                /* mean list length */
} rt_view_lists_info;
/* Waits for the lists' build. slots (optional, room for `cap` 16-byte records): a copy of the lists, per block 97
 * records: {count, flags, 0, 0} (ints), 64 entries {x, y, z, radius^2}, 64 list positions (ints), 64 bounds (floats). */
int rt_scene_view_lists_info(rt_scene *s, rt_view_lists_info *out, float *slots, size_t cap);
/* The host builder's lists for a sphere list and a frame (no device involved; tests). beams (optional): per block the
 * cone's unit axis and slope (-1: no usable cone). */
int rt_debug_view_lists_host(const rt_sphere *spheres, int n, const rt_frame_desc *fd, rt_view_lists_info *out,
                             float *slots, size_t cap, float *beams);

/* Light verdicts of a resting view. 1 (default): the second launch with bit-identical inputs (camera, frame
 * size, rows, tile shape, interleave, sphere list, lights, textures; the output buffers and the stream may differ)
 * among the scene's recent launches -- the one before it, or one of a repeating cycle of up to four layouts such as
 * the row bands of a frame -- also writes, per tile, which lights it found to add nothing to any pixel of the tile (all pixels facing away, a full
 * occluder, every shadow sample of every pixel shadowed) and which it found clear of every occluder; the launches
 * after it skip the former and take the latter's brightness without looking for occluders. A launch with other inputs
 * does neither, so a moving camera renders as it did. One-sample frames of sphere scenes (no cubes, planes or mesh;
 * not stats, force_slow_path, fast, G-buffer or reflective frames; not frame graphs or rt_multi). 0: every launch
 * evaluates every light. The pixels are the same bits either way: what is skipped is what the same code skipped, or
 * ran to no effect, on the same inputs.                                                                             */
int rt_scene_set_light_verdicts(rt_scene *s, int mode);
typedef struct rt_light_verdicts_info {
    int state;                 /* what the last frame launch on the scene did: 0 nothing, 1 wrote a table, 2 read one */
    int slot;                  /* which of the scene's tables (-1: none) */
    int tiles_x, tiles_y;      /* the table: one 64-bit word per tile of the launch, row by row */
    int unwritten;             /* tiles the writing launch left untouched: words still all ones, which a reader evaluates
                                  (0 as long as the launch's grid is cut to its rows, so that every tile has a pixel) */
    long long nothing, clear;  /* (group, light) entries with code 1 resp. 2 over the whole table */
} rt_light_verdicts_info;
/* Tests and profiles; waits for the launch that wrote the table. words (optional, room for `cap` words): a copy of the
 * table, two bits per (group, light) at 16 * group + 2 * light for the tile's first 4 groups and the first 8 lights:
 * 0 evaluate, 1 adds nothing, 2 all clear.                                                                          */
int rt_debug_light_verdicts(rt_scene *s, rt_light_verdicts_info *out, unsigned long long *words, size_t cap);
/* Shadow counts: the same table also remembers, for up to `records` lights per tile that the writing launch walked to the
 * end (code 0: neither dark nor clear), every pixel's number of unshadowed samples; the reading launches take it in place
 * of the occluder search and the ten samples. Same switch (rt_scene_set_light_verdicts), same key, same launches.    */
typedef struct rt_shadow_counts_info {
    int state, slot;           /* as in rt_light_verdicts_info */
    int tiles_x, tiles_y;
    int records;               /* records per tile (R) */
    long long tagged;          /* records in use over the whole table */
    long long tiles_tagged;    /* tiles with at least one */
    long long tagged_all;      /* records in use over all of the scene's tables (a frame rendered in row bands has one per band) */
} rt_shadow_counts_info;
/* Tests and profiles; waits for the launch that wrote the table. tags (optional, `cap` tiles): a dword per tile, byte r =
 * 0x80 | group << 3 | light of record r, 0 = free. counts (optional, `cap` tiles): records * 64 bytes per tile, record
 * by record, a byte per lane of the tile's wave.                                                                       */
int rt_debug_shadow_counts(rt_scene *s, rt_shadow_counts_info *out, unsigned *tags, unsigned char *counts, size_t cap);
/* Tests: overwrites the tags and / or the records (null: left as they are) of the table that the last launch wrote or
 * read; n = tiles_x * tiles_y. Waits for every launch in flight.                                                        */
int rt_debug_set_shadow_counts(rt_scene *s, const unsigned *tags, const unsigned char *counts, size_t n);
/* Primary records: the third part of the same table. For every pixel of the writing launch's grid a dword -- bits 0-7 the
 * entry of the tile's view list that is the pixel's closest hit (0xff: a miss, 0xfe: the tile has no record and reading
 * launches walk its list as before), bits 8-31 the clamped texel index, of the object texture for a hit, of the sky for a
 * miss. Reading launches evaluate that one entry and fetch that texel. Same switch, same key, same launches.          */
typedef struct rt_primary_records_info {
    int state, slot;           /* as in rt_light_verdicts_info */
    int tiles_x, tiles_y;
    int tile_w;                /* a tile is tile_w x 64 / tile_w pixels; lane = row in tile * tile_w + column in tile */
    long long tiles_recorded;  /* tiles with a record (no valid pixel says 0xfe) */
    long long hit_pixels, miss_pixels;   /* valid pixels of those tiles */
} rt_primary_records_info;
/* Tests and profiles; waits for the launch that wrote the table. dwords (optional, `cap` = 64 * tiles): the raw records at
 * tile * 64 + lane. positions (optional, same size): the position in the sphere table that a pixel's entry resolves to
 * through the view list the launch read, -1 for a miss, -2 where the tile has no record or the lane is outside the frame. */
int rt_debug_primary_records(rt_scene *s, rt_primary_records_info *out, unsigned *dwords, int *positions, size_t cap);
/* Tests: overwrites the records of the table that the last launch wrote or read; n = 64 * tiles_x * tiles_y. Waits for
 * every launch in flight.                                                                                            */
int rt_debug_set_primary_records(rt_scene *s, const unsigned *dwords, size_t n);
/* Tile summaries: the fourth part of the same table, a dword per tile of the writing launch's grid. Bit 0, settled: the
 * tile has a primary record, at most 4 groups under at most 8 lights, and every (group, light) entry of its word is 1 --
 * no light adds to any of its pixels (a tile without a hit pixel: trivially). Reading launches store 0 for its hit pixels
 * and the sky texel of the record for the others, and evaluate nothing else of it. Bit 1: no valid pixel of the tile is a
 * miss. Bits 8-15: the tile's group count, saturating at 255. Same switch, same key, same launches.                  */
typedef struct rt_tile_summaries_info {
    int state, slot;           /* as in rt_light_verdicts_info */
    int tiles_x, tiles_y;
    long long settled;         /* tiles with bit 0 */
    long long settled_no_miss; /* of those, tiles with bit 1 as well */
} rt_tile_summaries_info;
/* Tests and profiles; waits for the launch that wrote the table. dwords (optional, `cap` = tiles): the raw summaries,
 * row by row.                                                                                                        */
int rt_debug_tile_summaries(rt_scene *s, rt_tile_summaries_info *out, unsigned *dwords, size_t cap);
/* Tests: overwrites the summaries of the table that the last launch wrote or read; n = tiles_x * tiles_y. Waits for
 * every launch in flight.                                                                                            */
int rt_debug_set_tile_summaries(rt_scene *s, const unsigned *dwords, size_t n);
/* The compact reading launch of a resting view. 1 (default): once a view's table has a run list -- built on the device
 * from the tile summaries and primary records after the recording launch, and again after every re-sort of the tile
 * order and every rt_debug_set_tile_summaries / rt_debug_set_primary_records -- and the builder's two counts have
 * reached the host (the launches never wait for them: until then they keep the full grid) and say that at least a
 * quarter of the tiles can be streamed, a reading launch starts
 * one workgroup per run of R settled tiles, which it streams, and behind those one per tile that still computes,
 * instead of one per tile. 0: the full grid. Both give the same frame, bit for bit. Frames recorded by rt_graph_capture, and callers of the
 * launch configuration that have no list, keep the full grid. */
int rt_scene_set_compact_launch(rt_scene *s, int on);
typedef struct rt_compact_launch_info {
    int compact;                      /* 1: the last frame launch was a compact one */
    unsigned n_unsettled, n_streamed; /* ... its tiles with a wave of their own, and streamed in runs */
    unsigned run, workgroups;         /* ... R, and its grid: n_unsettled + ceil(n_streamed / R) */
    int ahead;                        /* ... 1: the runs' workgroups ahead of the others (rt_debug_set_compact_run) */
    unsigned long long rebuilds;      /* run lists built on this scene so far */
    int list_built;                   /* 1: the table the last launch wrote or read has a run list; then: */
    int tiles_x, tiles_y;
    unsigned list_n_unsettled, list_n_streamed;   /* its header */
} rt_compact_launch_info;
/* Tests and profiles; waits for the list's build. list (optional, `cap` = tiles): the list's entries (tile_y << 16) | tile_x,
 * the n_unsettled tiles that keep their wave first, in the launch's order, then the streamed ones in theirs. */
int rt_debug_compact_launch(rt_scene *s, rt_compact_launch_info *out, unsigned *list, size_t cap);
/* Profiles and tests: R of the run lists built from now on (1 ... 64; default 64), where their runs lie in the grid
 * (0 behind the tiles that keep their wave, 1 (default) ahead of them; a list built otherwise is rebuilt) and the share
 * of streamed tiles, in percent of the launch's tiles, below which a launch keeps the full grid (default 25). Same frames. */
int rt_debug_set_compact_run(rt_scene *s, int run, int ahead, int min_percent);
/* Tests: the order that run list was built from -- the tile order at that build, or grid order -- `cap` = tiles entries
 * (tile_y << 16) | tile_x. Waits for every launch in flight. */
int rt_debug_compact_order(rt_scene *s, unsigned *order, size_t cap);
/* Tests: the long-lived scene rt_launch_raytrace(_ex) and update() render through, for rt_debug_light_verdicts and
 * rt_scene_view_lists_info; owned by the library, NULL before the first launch.                                     */
rt_scene *rt_debug_shim_scene(void);

/* hipGraph-captured frame loop (config C4): `passes` samples per pixel + resolve + optional async copy of the packed
 * frame to pinned host memory, recorded once and replayed per frame. passes > 0: the samples are taken by ONE kernel
 * node (the sample loop runs inside the kernel); passes < 0: |passes| progressive one-sample nodes, each adding into
 * opts.rgba (needs opts.rgba) -- the same bits in the end, 9 % slower at C4, for callers that present between passes. */
typedef struct rt_frame_graph rt_frame_graph;
rt_frame_graph *rt_graph_capture(rt_scene *s, const rt_frame_desc *fd, int passes,
                                 uint32_t *host_pixels /* pinned, may be NULL */, void *stream);
/* Replays the frame. If the scene's tables were rewritten since the graph was built (another
 * sphere list, other lights -- also when nothing rendered since rt_scene_set_lights; the same
 * lights set again do not count --, textures, or a direct render at another resolution) the
 * graph is rebuilt first -- it never replays against tables it was not built for.             */
int rt_graph_launch(rt_frame_graph *g, void *stream);
/* A camera move (kernel.cu:1716-1759 moves `cam` every frame): the kernel nodes' by-value
 * uniforms are replaced with hipGraphExecKernelNodeSetParams and the eye-cone table is rebuilt
 * by a kernel node of the graph itself -- no re-capture, no synchronisation.                  */
int rt_graph_set_camera(rt_frame_graph *g, const rt_camera *cam);
void rt_graph_destroy(rt_frame_graph *g);

/* ------------------------------------------------------------------ *
 * Several GPUs of one node, one process (BASELINE C5): *
 * the frame's rows are dealt to the devices in 16-row blocks           *
 * round-robin, every device renders its rows as 3 bytes per pixel,     *
 * ONE RCCL gather over xGMI brings them to the first device, and one   *
 * small kernel there scatters the rows home and widens them to the     *
 * 0x00RRGGBB words setPixelBuff() consumes (kernel.cu:1788). update()  *
 * takes this path when rt_config_set_gpus(n > 1) was called (or the    *
 * application's environment said RT_GPUS=n when onStart() ran).        *
 * ------------------------------------------------------------------ */
typedef struct rt_multi rt_multi;
enum { RT_MULTI_AUTO = 0,       /* RCCL for distinct devices IF its gather passes a self-test at creation
                                   (every rank's 256 known bytes arrive in its slot of the root's buffer),
                                   else peer copies; rt_multi_note() says which and why              */
       RT_MULTI_RCCL = 1,       /* ncclCommInitAll + one ncclGather per frame (librccl loaded with dlopen);
                                   creation fails if the self-test does. With ONE device the whole exchange
                                   still runs (24-bit rows, one-rank in-place gather, scatter kernel)  */
       RT_MULTI_PEER_COPY = 2   /* the first device pulls the rows with hipMemcpyPeerAsync (SDMA over xGMI);
                                   accepts the same device several times (one-GPU rehearsal of the path) */ };
rt_multi *rt_multi_create(int n_gpus);                       /* devices 0 .. n_gpus-1, RT_MULTI_AUTO; NULL on failure */
int rt_multi_create_ex(const int *devices, int n, int transport, rt_multi **out);
void rt_multi_destroy(rt_multi *m);
int rt_multi_device_count(const rt_multi *m);
int rt_multi_transport(const rt_multi *m);
rt_scene *rt_multi_scene(rt_multi *m, int i, int *device);   /* the i-th device's scene (hipSetDevice(*device) before using it) */
/* the same scene on every device (rt_scene_set_* per device) */
int rt_multi_set_spheres(rt_multi *m, const rt_sphere *host_spheres, int n);
int rt_multi_set_planes(rt_multi *m, const rt_plane *host_planes, int n);
int rt_multi_set_cubes(rt_multi *m, const rt_cube *host_cubes, int n);
int rt_multi_set_mesh(rt_multi *m, const rt_mesh *mesh);
int rt_multi_set_texture(rt_multi *m, const float *r, const float *g, const float *b, int w, int h);
int rt_multi_set_sky(rt_multi *m, const rt_sphere *box, const float *r, const float *g, const float *b, int w, int h);
int rt_multi_set_lights(rt_multi *m, const rt_light *lights, int n);
/* One frame, or one row band of it (width, height, aspect, cam and opts.spp / cull / tile of `fd`;
 * opts.y0 / y1 select a band of whole 16-row blocks, dealt to the devices from the band's first row;
 * its output pointers and interleave fields are ignored). The assembled rows land at their place in
 * `pixels_dev0` (the WHOLE frame's buffer in memory of the first device) or, if that is NULL, in an
 * internal buffer (rt_multi_frame). There are two internal buffers: a call that begins a frame -- a whole
 * frame, or a band with y0 == 0 -- takes the other one, and every later band of that frame lands in the same
 * one, so after a frame's last band rt_multi_frame / rt_multi_download give the whole frame, and the frame
 * before it stays readable meanwhile. Asynchronous; two frames (or bands) may be in flight. After a change of
 * the frame's size there is no last frame until a render has succeeded (rt_multi_frame NULL, rt_multi_download
 * and rt_multi_stream_wait fail). */
int rt_multi_render(rt_multi *m, const rt_frame_desc *fd, uint32_t *pixels_dev0);
int rt_multi_sync(rt_multi *m);                              /* wait for every frame enqueued so far */
int rt_multi_stream_wait(rt_multi *m, void *stream);         /* `stream` (first device) waits ON THE DEVICE for the frame /
                                                                band enqueued last: copies of it need no host wait */
const char *rt_multi_note(const rt_multi *m);                /* transport chosen at creation, and why */
unsigned long long rt_multi_gathers(const rt_multi *m);      /* ncclGather groups issued so far (RCCL transport) */
const uint32_t *rt_multi_frame(const rt_multi *m);           /* device pointer of the last assembled frame */
int rt_multi_download(rt_multi *m, uint32_t *host);          /* sync + copy the last frame to host memory */
/* The root side of the exchange alone, for hosts that run the gather themselves (one process per GPU:
 * bench.py under torch.distributed): `recv` = n slots of slot_rows rows of width*3 bytes, slot r being
 * what rank r rendered with interleave (n, r, 16) into opts.packed24; `frame` = width*height words. */
int rt_assemble_rows24(const void *recv, uint32_t *frame, int width, int height, int n, int slot_rows, void *stream);
int rt_config_set_gpus(int n);                               /* update(): devices used per frame; default 1. n < 0:
                                                                rehearsal of the path on one GPU -- |n| shares of the
                                                                frame, all on device 0, RT_MULTI_PEER_COPY */

/* ------------------------------------------------------------------ *
 * Introspection / diagnostics                                         *
 * ------------------------------------------------------------------ */
int rt_abi_version(void);
const char *rt_last_error(void);
int rt_device_count(void);
int rt_set_soft_errors(int on);  /* 1: rt_check() records + returns instead of exit(99) */
/* Device evaluation of the library's scalar building blocks, for bit-for-bit
 * comparison with the CPU oracle (tests only; all pointers are HOST arrays).
 * op: 0 cosf, 1 sinf, 2 acosf, 3 atan2f(a,b)                                    */
int rt_debug_math(int op, const float *a, const float *b, float *out, int n);
/* A float4 copy kernel over n16 float4s (16-byte aligned, disjoint device buffers): the copy the denoiser's traffic
 * floor is measured with (tools/bench_denoise.py). */
int rt_debug_copy16(const void *src, void *dst, size_t n16, void *stream);
/* What a launch of the resting-view reader's geometry costs before it computes anything (tools/launch_floor_probe.py):
 * one-wave workgroups with the reader's LDS bytes and 72 registers. cfgs: n_cfgs triples {what, workgroups, run} --
 * what 0: empty workgroups; 1: one scalar load each, waited for; 2: each stores the float4 and the packed word of `run`
 * consecutive 8x8 tiles of a width x height frame (grid order; tiles beyond the frame are not written); 3: a linear
 * float4 fill of the frame's bytes (width * height * 20; workgroups and run ignored). `rounds` interleaved rounds after
 * `preroll` fills, `reps` launches per timing; ms[c * rounds + r] = milliseconds per launch. */
int rt_debug_launch_floor(int width, int height, const int *cfgs, int n_cfgs, int rounds, int reps, int preroll, float *ms);
/* sphere::intersect on the device: hit[i], t[i] for rays[i] vs spheres[i].      */
int rt_debug_intersect(const rt_sphere *spheres, const rt_ray *rays, int n, int *hit, float *t);
/* The 10 shadow-sample directions of castLightRay (kernel.cu:1442-1468) and its
 * brightness result for (start, normal, light) against `spheres`.               */
int rt_debug_light(const rt_sphere *spheres, int n_spheres, const rt_vec3 *start,
                   const rt_vec3 *normal, const rt_light *light, int n,
                   float *dirs /* n*30 */, float *brightness /* n */);
/* The exact sample directions (n*30) next to the approximate ones of the frame kernel's sample pre-pass (n*30) and the
 * pre-pass's guard flags (n*10: 1 = the approximate direction may be used), for its error bound (tests only).   */
int rt_debug_light_prepass(const rt_vec3 *start, const rt_light *light, int n, float *dirs, float *approx_dirs, int *approx_ok);
/* The culling kernels' shortcuts against the long forms they stand for, evaluated on the
 * device for n pseudo-random inputs derived from `seed` (tests only):
 *  what 0: lean normalise vs the IEEE one on vectors of every scale -> out[0] = differing results
 *  what 1: lean sqrt vs IEEE sqrtf on EVERY float in [2^-96, 2^40] (n, seed ignored) -> out[0] = differing results
 *  what 2: approximate (tx, ty) of a unit normal vs the exact binary64 expressions of
 *          kernel.cu:1402-1403 -> out[0], out[1] = max |error| of tx, ty (as float bits in the
 *          low word), out[2] = lanes the 512x512 certainty test accepted, out[3] = accepted
 *          lanes whose texel index differs from the exact one (must be 0)                   */
int rt_debug_shortcuts(int what, unsigned seed, long long n, unsigned long long out[4]);
/* The per-sphere occluder lists the culling kernels use for one light (host computation, no GPU): for every sphere i
 * of the list the number of spheres a shadow ray leaving i's surface towards `light` can hit at all (counts[i]; -1: no
 * list), the beam slope the list holds for (kcaps[i]) and the list positions of its first `cap` members
 * (members[i*cap ..]; likeliest occluder first). Tests only.                                                      */
int rt_debug_occluder_lists(const rt_sphere *spheres, int n, const rt_light *light, int *counts, float *kcaps, int *members, int cap);
/* ... plus every list's offset into the light's entry array (offsets[i], or NULL) and the number of entries that array is
 * allocated with (the kernel reads whole steps of 64 entries from a list's offset on)                                     */
/* The beam slope of every group of pixels on a sphere (what the frame kernel takes instead of bounding the sample spread
 * per tile; -1: none), host builder and device builder (either pointer may be NULL; the device one needs a GPU), the
 * same for one ball, and the spread s = sigma / (|l.pos| - frob) at ONE start with the 3x3 matrix it comes from */
int rt_debug_sphere_beam_slopes(const rt_sphere *spheres, int n, const rt_light *light, float *host_kbeam, float *device_kbeam);
double rt_debug_sphere_beam_slope(const double lpos[3], const double centre[3], double r0);
double rt_debug_beam_sine(const double lpos[3], const double start[3], double *sigma, double *frob, double m9[9]);
/* ... and as the DEVICE builds them (what a scene uses: one wave per sphere, members in list order); needs a GPU */
int rt_debug_occluder_lists_device(const rt_sphere *spheres, int n, const rt_light *light, int *counts, float *kcaps, int *members, int cap);
/* The tile order of rt_scene_set_tile_order as the DEVICE sorts it, for a grid of tiles_x x tiles_y tiles and their
 * durations cost[tiles_x * tiles_y] (row-major; needs a GPU; tests only). Blocks of 16 x 16 tiles, nbx = ceil(tiles_x / 16)
 * per row of blocks: key[nb] = the longest tile of every block, start[nb] = where each block's tiles start in the order,
 * perm[tiles_x * tiles_y] = the order, (tile_y << 16) | tile_x. One launch of the three kernels on a stream of the
 * call's own, which it waits for. via_configs != 0: the kernels are launched from the functions and geometries a frame
 * graph makes its kernel nodes from. A grid the library keeps in grid order (a coordinate above 0xffff, more than 4096
 * blocks): RT_ERR_UNSUPPORTED, nothing is launched or written.                                                      */
int rt_debug_tile_order(const unsigned *cost, int tiles_x, int tiles_y, int via_configs, unsigned *key, unsigned *start,
                        unsigned *perm);
/* The sphere BVH of the reflective frames, built on the host (no GPU needed; tests only). Node j:
 * lohi[6j..6j+5] = its box (lo xyz, hi xyz: binary32, rounded outward from the binary64 extents of
 * its spheres), meta[2j] = first child (the second is meta[2j] + 1) or, for a leaf, the first
 * position in `order`, meta[2j+1] = 0 for an inner node or the leaf's sphere count (1..4). Node 0
 * is the root; order[] lists the sphere indices leaf by leaf. Returns RT_ERR_CAPACITY if cap is too
 * small for the tree (2n nodes always suffice). */
int rt_debug_sphere_bvh(const rt_sphere *spheres, int n, float *lohi, int *meta, int *order, int cap,
                        int *n_nodes, int *depth);
/* Host evaluation of the reflective passes' ray casts (the same code the kernels run): for each ray,
 * nearest hit (hit_index[i], -1 = none, and t[i]) and any-hit (any[i]); use_bvh = 0 walks the whole
 * list (the brute-force variant). Either output pointer group may be NULL.                       */
int rt_debug_bvh_cast(const rt_sphere *spheres, int n, const rt_ray *rays, int n_rays, int use_bvh,
                      int *hit_index, float *t, int *any);
/* reflect(I, N), kernel.cu:1282-1285, in binary32 as the kernels evaluate it (n vectors).        */
int rt_debug_reflect(const rt_vec3 *I, const rt_vec3 *N, int n, rt_vec3 *out);
/* refract(I, N, eta) of rt_scene_set_materials_ex, in binary32 as the kernels evaluate it.       */
int rt_debug_refract(const rt_vec3 *I, const rt_vec3 *N, const float *eta, int n, rt_vec3 *out);
/* The glass step of rt_scene_set_materials_ex for rays[i] hitting `sphere` with ior[i] (the same
 * code the kernels run, from sphere::intersect's hit to R_{b+1}): out[i] = R_{b+1}; entered[i] = 1
 * when the ray passed through the sphere (rule 4), 0 when it leaves undeviated (rules 1 and 3),
 * -1 when intersect() reports no hit (out[i] = rays[i]).                                          */
int rt_debug_transmit(const rt_sphere *sphere, const float *ior, const rt_ray *rays, int n,
                      rt_ray *out, int *entered);
/* rf_gloss of rt_scene_set_roughness (the same code the kernels run) for n tuples (R, N, rho, key, b):
 * out[i] = the continuation; what[i] (may be NULL) = 0 nothing drawn (rho == 0), else 1, | 2 when the
 * halved fourth draw was taken, | 4 when R' was rejected and out[i] = R.                            */
int rt_debug_gloss(const rt_vec3 *R, const rt_vec3 *N, const float *rho, const unsigned *key, const int *b, int n,
                   rt_vec3 *out, int *what);
/* key(px, py, s, seed) of rt_scene_set_roughness for n tuples.                                      */
int rt_debug_gloss_key(const unsigned *px, const unsigned *py, const unsigned *s, const unsigned *seed, int n,
                       unsigned *key);
/* sizeof of the reflective passes' queue entry (48; its last word carries the glossy key).          */
int rt_debug_reflect_entry_size(void);
/* F(c, ior) of rt_scene_set_glass_model(RT_GLASS_FRESNEL), in binary32 as the kernels evaluate it.  */
int rt_debug_fresnel(const float *c, const float *ior, int n, float *F);
/* The glass hit of the Fresnel model for rays[i] hitting `sphere` with ior[i], rho[i], key[i], b[i]
 * (the same code the kernels run, from sphere::intersect's hit to R_{b+1}): out[i] = R_{b+1};
 * choice[i] = 1 rule 1 (nothing drawn), 2 reflected, 3 through the sphere (rule 4), 4 rule 3, -1 when
 * intersect() reports no hit (out[i] = rays[i]). F, u, what may be NULL: the reflectance, the draw
 * (both 0 where nothing was drawn) and rt_debug_gloss's `what` of the perturbation.               */
int rt_debug_glass_choice(const rt_sphere *sphere, const float *ior, const float *rho, const unsigned *key,
                          const int *b, const rt_ray *rays, int n, rt_ray *out, int *choice, float *F, float *u,
                          int *what);
int rt_debug_occluder_lists_ex(const rt_sphere *spheres, int n, const rt_light *light, int *counts, float *kcaps, int *members, int cap,
                               int *offsets, int *entries_allocated);

/* ------------------------------------------------------------------ *
 * Reflective frames over the whole scene.              *
 * ------------------------------------------------------------------ */
/* The scope of a frame with opts.reflect_depth > 0. RT_REFLECT_SPHERES (the default): spheres only,
 * exactly as before this switch existed -- a scene that holds a plane, a cube or a mesh is
 * RT_ERR_UNSUPPORTED and nothing is written. RT_REFLECT_SCENE lifts that one refusal. Any other value:
 * RT_ERR_INVALID. A host-side switch, read when a frame is launched: no wait, no device needed.
 *
 * Semantics under RT_REFLECT_SCENE: the per-pixel loop of rt_scene_set_materials / _ex with three
 * substitutions.
 *   Nearest hit. castRay(R_b) is castRay over the whole scene, as RT_QUERY_NEAREST defines it: mesh
 *     leaves behind their boxes, then spheres, then cubes, then planes, the strict `t < nt` across
 *     kinds, every primitive test with its quirks (a cube's negative tmin from inside, a plane hit only
 *     for denom < 0, Moller-Trumbore's t >= 1e-7f).
 *   Hit frame. N, new_org, the texel and start_O = N*0.00001 + new_org are as rt_hit / castRay form
 *     them for that kind: a plane's normal as stored (not normalised), a cube's the normalised
 *     hit - centre, a triangle's new_org displaced by the whole normal, texture coordinates as castRay's
 *     ((0.5, 0.5) for a plane). reflect(R_b.Dir, N) takes that N as it is. Two consequences: a plane
 *     whose stored normal is not a unit vector is not a mirror (the reflected direction is neither the
 *     mirror direction nor a unit vector), and a ray reflected off a cube near an edge -- where
 *     hit - centre points away from the face's own normal -- may re-enter the same cube.
 *   Light. L is the three-light sum with castLightRay's any-hit over every kind (RT_QUERY_OCCLUDED).
 * Everything else is unchanged: k comes from the hit primitive's table (below; a triangle always has
 * k = 0), weights and the order of additions are as before, glass rules 1..4 apply at glass spheres
 * (glass stays a sphere property; the chord stays untested, now also against planes, cubes and
 * triangles). A sky pixel, and a pixel whose primary hit has k = 0 and tau = 0, is the plain frame
 * bit for bit. A scene with no spheres at all is legal. rt_reflect_stats.queue[b] counts rays of every
 * kind of hit.
 * Still RT_ERR_UNSUPPORTED under either scope, with nothing written: under the default sampling mode
 * (rt_scene_set_reflect_samples below) spp > 1 and accumulate; under either mode interleave_*,
 * packed24, table_lds, profile, rt_graph_capture and rt_multi_render. The drop-in boundary
 * (rt_launch_raytrace_ex, object::mat) keeps the spheres-only scope. */
enum { RT_REFLECT_SPHERES = 0, RT_REFLECT_SCENE = 1 };
int rt_scene_set_reflect_scope(rt_scene *s, int scope);
/* One material per plane / per cube of the scene's list, under rt_scene_set_materials' rules per list:
 * n must equal the list's count (RT_ERR_INVALID); NULL / 0 clears the table (every k = 0) and always
 * succeeds; the table survives rt_scene_set_planes / rt_scene_set_cubes with the same count and is
 * cleared by a different count; a NaN k or a k outside [0, 1] is RT_ERR_INVALID; transperancy or
 * roughness != 0 is RT_ERR_UNSUPPORTED (the values are checked before the count). Nothing changes on
 * an error. The tables may be set under either scope; only frames under RT_REFLECT_SCENE read them. */
int rt_scene_set_plane_materials(rt_scene *s, const rt_material *per_plane, int n);
int rt_scene_set_cube_materials(rt_scene *s, const rt_material *per_cube, int n);

/* ------------------------------------------------------------------ *
 * Glossy reflections.                                  *
 * ------------------------------------------------------------------ */
/* Roughness per primitive of one kind: kind = RT_HIT_SPHERE, RT_HIT_PLANE or RT_HIT_CUBE (anything
 * else: RT_ERR_INVALID; a triangle has roughness 0), one value in [0, 1] per primitive of that
 * kind's list. NULL or n == 0 clears the kind's table (every rho = 0) and always succeeds. A count
 * other than the list's, a NaN or a value outside [0, 1]: RT_ERR_INVALID, and nothing changes on an
 * error. A table follows its kind's k table: it survives rt_scene_set_spheres / _planes / _cubes with
 * the same count and is cleared by a different count; the plane and cube tables may be set under
 * either scope and are read only under RT_REFLECT_SCENE.
 *
 * Roughness has an entry of its own, and rt_material / rt_material_ex keep refusing a non-zero
 * roughness field: those structs describe a surface that one ray continues deterministically, and
 * callers (the drop-in boundary among them) rely on a frame that is a function of the scene alone.
 * A rough surface makes the frame a function of the sample index and of a seed as well, which only
 * a caller that asked for it by name should get.
 *
 * Semantics: the per-pixel loop of rt_scene_set_materials under either scope, with one change. At a
 * hit b (0: the primary hit) that continues as a mirror (k > 0, b < D, not glass) on a primitive
 * with rho > 0, R_{b+1}'s direction is not R = reflect(R_b.Dir, N) but gloss(R, N, rho, key, b).
 * All integer arithmetic is uint32 and wraps:
 *   mix(x):  x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 *   key = mix(mix(mix(mix(seed) ^ s) ^ py) ^ px)    px, py: the pixel in the full frame (py counts
 *         from row 0 of the frame, not from opts.y0); s: the absolute sample index, sample_base + j
 *         under RT_REFLECT_SAMPLES_MANY and 0 under the default mode; seed: rt_scene_set_gloss_seed
 *   draw(key, b, t), axis a = 0, 1, 2:  h = mix(key + 0x9e3779b9 * ((b*4 + t)*3 + a + 1)),
 *         u_a = float(h >> 8) * 2^-23 - 1            (exact, in [-1, 1))
 *   u = the first of the draws t = 0, 1, 2, 3 with (ux*ux + uy*uy) + uz*uz <= 1; if none, draw 3
 *       with every component multiplied by 0.5f
 *   G = (R.x + rho*ux, R.y + rho*uy, R.z + rho*uz), R' = normalise(G) (G as it is where its length
 *       is 0); the continuation is R' if dot(R', N) * dot(R, N) > 0 (both dots left to right; a NaN
 *       fails), else R unchanged.
 * binary32, no contraction, correctly rounded division and sqrt. rho == 0 draws nothing: a scene
 * whose tables hold no value > 0 renders exactly as without them. Roughness on a glass sphere
 * (tau > 0) or on a surface with k == 0 is accepted and has no effect (a glass sphere: under
 * RT_GLASS_PLAIN; under RT_GLASS_FRESNEL, below, it frosts the glass). The multiplicity of a glossy
 * lobe comes from spp and accumulate under RT_REFLECT_SAMPLES_MANY, or from one sample per frame
 * with a new seed (or sample_base) accumulated by rt_scene_temporal. What a reflective frame
 * refuses, and rt_reflect_stats, are unchanged. */
int rt_scene_set_roughness(rt_scene *s, int kind, const float *rho, int n);
/* The seed of the glossy draws (default 0, any value): a host-side value, read when a frame is
 * launched: no wait, no device needed. */
int rt_scene_set_gloss_seed(rt_scene *s, unsigned seed);

/* ------------------------------------------------------------------ *
 * Fresnel glass.                                       *
 * ------------------------------------------------------------------ */
/* How a glass sphere (rt_scene_set_materials_ex, transperancy > 0) continues a ray. RT_GLASS_PLAIN
 * (the default): always through the sphere, as described there. RT_GLASS_FRESNEL: a hit reflects
 * with the dielectric reflectance F of its angle and index, and goes through otherwise -- one ray
 * per hit, chosen by a hashed draw, its weight unchanged. Any other value: RT_ERR_INVALID, and
 * nothing changes. A host-side value like the gloss seed, read when a frame is launched: no wait, no
 * device needed; it survives rt_scene_set_spheres and rt_scene_set_materials*, and has no effect on
 * a frame without glass or with reflect_depth 0.
 *
 * Semantics under RT_GLASS_FRESNEL: the per-pixel loop of rt_scene_set_materials_ex with one change.
 * The colour term of a glass hit and its weight are as there ((w * (1 - tau)) * L, then w = w * tau);
 * at a continuing glass hit b on sphere i, with D, N, start_O, new_org as there and mix, key, gloss
 * of rt_scene_set_roughness:
 *   1. dot(D, N) >= 0 (rule 1): the ray leaves undeviated from start_O; nothing is drawn.
 *   2. c = -dot(D, N); eta = 1 / ior; q = 1 - (eta*eta) * (1 - c*c); ct = sqrt(q > 0 ? q : 0);
 *      rs = (c - ior*ct) / (c + ior*ct); rp = (ct - ior*c) / (ct + ior*c);
 *      F = (rs*rs + rp*rp) * 0.5f        (the unpolarised reflectance, not Schlick's approximation)
 *   3. h = mix(mix(key ^ 0x46726573) + 0x9e3779b9 * (b + 1)); u = float(h >> 8) * 2^-24, in [0, 1)
 *   4. u < F (a NaN F fails): R_{b+1} = ray(start_O, reflect(D, N)), its direction replaced by
 *      gloss(R, N, rho_i, key, b) where sphere i's roughness is > 0 -- what a mirror hit would do.
 *   5. otherwise the glass step as it is (rules 3 and 4); where the ray went through (rule 4) and
 *      rho_i > 0, its direction U is replaced by gloss(U, M, rho_i, key, b), M the exit normal.
 * binary32, no contraction, correctly rounded division and sqrt, dot products left to right. Under
 * this model roughness on a glass sphere is frosted glass; under RT_GLASS_PLAIN it has no effect.
 * Internal reflection along the chord is not modelled: a pass through the sphere is one bounce.
 * The multiplicity of the two branches comes from spp, accumulate and rt_scene_temporal, as for
 * glossy reflections. What a reflective frame refuses (k > 0 with tau > 0 on one sphere included)
 * and rt_reflect_stats are unchanged. */
enum { RT_GLASS_PLAIN = 0, RT_GLASS_FRESNEL = 1 };
int rt_scene_set_glass_model(rt_scene *s, int model);

/* ------------------------------------------------------------------ *
 * Supersampled reflective frames.                      *
 * ------------------------------------------------------------------ */
/* How a frame with opts.reflect_depth > 0 samples a pixel. RT_REFLECT_SAMPLES_ONE (the default): one
 * sample, exactly as before this switch existed -- spp > 1, sample_base != 0, sample_total > 1 and
 * accumulate are RT_ERR_UNSUPPORTED and nothing is written. RT_REFLECT_SAMPLES_MANY lifts those
 * refusals: the frame takes spp 1..RT_MAX_SPP, sample_base, sample_total, accumulate and resolve = -1
 * with the plain frame's range checks and errors. Any other value: RT_ERR_INVALID, the mode unchanged.
 * A host-side switch, read when a frame is launched: no wait, no device needed.
 *
 * The result, to the bit. n = spp (0 reads as 1), total = sample_total > 0 ? sample_total : n,
 * base = sample_base.
 *   Per sample k = base .. base + n - 1, ascending: R_0^k is the primary ray the plain frame forms
 *     for sample k of total (rt_sample_offset(k, total)), and c_k the colour the per-pixel loop of
 *     rt_scene_set_materials / _ex / rt_scene_set_reflect_scope gives that ray: w = 1, depth D, the
 *     scene's scope and tables, the first term assigned and later ones added.
 *   Sum. S = +0, then S = S + c_k per channel in binary32, in ascending k (as the plain frame sums
 *     its samples).
 *   Without accumulate rgba = (S, (float)n); with it rgba = (old.xyz + S, old.w + (float)n).
 *   With pixels set and resolve != -1: m = total == 1 ? v : v / (float)total for each channel v of
 *     the rgba just formed, and the word is rgbToInt(f2i(m.r*254), f2i(m.g*254), f2i(m.b*254));
 *     resolve = -1 leaves pixels untouched.
 * Consequences: a pixel none of whose samples has a primary hit with k > 0 or tau > 0 is the plain
 * frame with the same sample fields bit for bit (rgba with .w, and the packed word). One call with
 * spp = 4 equals four one-sample accumulate calls in ascending k (resolve = -1 until the last) bit
 * for bit. A 2 + 2 split is old + (c_2 + c_3), which is NOT the four-in-one sum ((c_0 + c_1) + c_2)
 * + c_3 -- as for plain frames. A request a one-sample frame serves (one sample, total 1, base 0, no
 * accumulate, resolve != -1) runs exactly as under RT_REFLECT_SAMPLES_ONE: same launches, same bits.
 * Still RT_ERR_UNSUPPORTED under either mode, with nothing written: interleave_*, packed24, table_lds,
 * profile, rt_graph_capture, rt_multi_render, and G-buffer outputs (aov_*) with more than one sample.
 * `fast` stays ignored, cull = 0 stays the whole-list variant, row bands work. The samples of a call
 * are processed in groups of four on scene-owned scratch (about 112 bytes per pixel-sample of a group,
 * plus 16 per pixel when there are several groups); a group whose pixel-samples exceed the queues'
 * index range is RT_ERR_CAPACITY. The drop-in boundary (rt_launch_raytrace_ex) keeps
 * RT_REFLECT_SAMPLES_ONE. */
enum { RT_REFLECT_SAMPLES_ONE = 0, RT_REFLECT_SAMPLES_MANY = 1 };
int rt_scene_set_reflect_samples(rt_scene *s, int mode);

/* ------------------------------------------------------------------ *
 * One-bounce global illumination: a hashed diffuse     *
 * gather pass over a frame's G-buffer.                                *
 * ------------------------------------------------------------------ */
#define RT_INDIRECT_MAX_RAYS 16
typedef struct rt_indirect_desc {
    uint32_t struct_size;     /* sizeof(rt_indirect_desc); 0 reads as this layout; fields past a caller's size read as 0 */
    int width, height;        /* whole frames, rows of `width` pixels (as rt_temporal_desc)                             */
    float aspect;             /* the view the guides were rendered with (rt_frame_desc.aspect / cam)                    */
    rt_camera cam;
    const float *depth;       /* device, the four guides in the rt_frame_desc.aov_* layouts and alignments              */
    const float *normal;
    const int   *id;
    const float *albedo;      /* NULL: the factor is 1 (the output is the irradiance term itself)                       */
    const float *rgba_in;     /* NULL, or device, float4, 16-byte aligned: the colour the indirect term is added to     */
    float *rgba_out;          /* device, float4, 16-byte aligned; may equal rgba_in, overlaps nothing else              */
    uint32_t *pixels;         /* NULL, or device: the packed word of rgba_out's colour, rgbToInt(c * 254)               */
    int rays;                 /* 1 .. RT_INDIRECT_MAX_RAYS: gather rays per pixel                               [1]     */
    int ray_base;             /* >= 0, ray_base + rays <= 1 << 24: index of the call's first ray                [0]     */
    uint32_t seed;            /*                                                                                [0]     */
    float strength;           /* finite, >= 0: factor on the indirect term                                      [1]     */
    int cull;                 /* -1 or 1: the sphere BVH; 0: the whole lists; the same bits                     [-1]    */
    int variant;              /* 0: the product kernels; 1: the plain one-thread-per-pixel yardstick; the same bits [0] */
} rt_indirect_desc;

/* The defaults in brackets above; sizes, view and pointers 0. */
void rt_indirect_desc_init(rt_indirect_desc *d);

/* Adds every surface pixel's one-bounce indirect diffuse light to a colour, on `stream` (a hipStream_t; NULL = the
 * null stream). p = y * width + x; all arithmetic binary32, no contraction, correctly rounded division and sqrt, dot
 * products left to right; mix, key as rt_scene_set_roughness defines them:
 *   1. A pixel is dead if id[p].kind < 0, depth[p] is not finite, or nn = (n.x*n.x + n.y*n.y) + n.z*n.z of the normal
 *      guide is 0 or not finite. A dead pixel casts nothing; its rgba_out is rgba_in[p]'s bits ((0, 0, 0, 1) without
 *      rgba_in) and its packed word the pack of that colour.
 *   2. O = the origin of the view's primary rays, D = the pixel's primary direction as rt_scene_primary_rays forms it,
 *      P = O + D * depth per component (a negative depth -- a sphere seen from inside -- as it is), n = normalise(normal
 *      guide), negated if dot(n, D) > 0, start = n * 0.00001f + P.
 *   3. For j = 0 .. rays - 1: key = key(x, y, ray_base + j, seed); kg = mix(key ^ 0x47497261);
 *      draw(t, a) = float(mix(kg + 0x9e3779b9 * (t*2 + a + 1)) >> 8) * 2^-23 - 1. For t = 0 .. 5: x1 = draw(t, 0),
 *      x2 = draw(t, 1), s = x1*x1 + x2*x2; the first t with s < 1 gives r = sqrt(1 - s) and the point of the unit sphere
 *      u = ((2*x1)*r, (2*x2)*r, 1 - 2*s) (Marsaglia); no such t: u = 0. G = normalise(n + u), or n unless
 *      dot(G, n) > 0. c_j = the colour RT_QUERY_SHADE gives ray(start, G): direct light at what it hits, getFColor on
 *      a miss.
 *   4. S = 0.f; S = S + c_j in ascending j; E = S / (float)rays.
 *   5. I = strength * E, then I = I * albedo.rgb where albedo is given.
 *   6. rgba_out = (rgba_in.rgb + I, rgba_in.a), or (I, 1) without rgba_in; pixels = rgbToInt(f2i(c * 254) ...) of it.
 * normalise(n + point of the unit sphere) is cosine-distributed about n, and the light model carries no 1 / pi: the
 * Lambert estimator under that density is albedo x radiance, unweighted. Distinct (ray_base + j) are distinct samples:
 * a caller accumulates over frames with ray_base = the frame number (rt_scene_temporal), or filters the term
 * (rt_scene_denoise); at 4K the intended use is the pass at half resolution and rt_scene_upsample (README).
 * One bounce; the guides are the primary hit's, so what a mirror or glass shows gets the light of the mirror's own
 * surface point (a caller scales by 1 - k through the id guide); no importance sampling; whole frames only.
 * Host behaviour is rt_scene_trace_rays': ordered after pending uploads, counted as a frame in flight, a host wait
 * only when the shared sphere BVH must be rebuilt, the scratch grows (variant 0: 256 bytes per pixel, plus 16 with
 * more than 4 rays; it belongs to the scene) or a view of another size or aspect needs its ray tables. Calls of one
 * scene on different streams are ordered on the device by an event; ordering the call after the frame that wrote its
 * inputs is the caller's. Before anything is enqueued, and with nothing written: NULL or misaligned required pointers,
 * sizes <= 0 or above RT_DENOISE_MAX_SIZE, an aspect that is not finite and > 0, rays, ray_base, cull or variant out
 * of range, a strength that is not finite and >= 0, an output that overlaps an input other than rgba_out == rgba_in,
 * a scene without sky, or with primitives and no texture -> RT_ERR_INVALID; a frame whose pixels times 4 rays exceed
 * the queue's index range -> RT_ERR_CAPACITY; a stream that is being captured -> RT_ERR_UNSUPPORTED. */
int rt_scene_indirect(rt_scene *s, const rt_indirect_desc *d, void *stream);

/* Device time of every launch of the scene's later indirect calls (hipEvents around each; off by default).
 * rt_scene_indirect_times waits for the last call and fills ms[0 .. *n - 1]: variant 1: [0] the kernel; variant 0: per
 * group of at most 4 rays [3g] the cast pass, [3g + 1] the shade pass, [3g + 2] the resolve pass. cap: room in ms. */
int rt_scene_set_indirect_timing(rt_scene *s, int on);
int rt_scene_indirect_times(rt_scene *s, float *ms, int cap, int *n);

/* The gather direction of step 3 (the same code the kernels run, no GPU needed; tests only) for `count` pairs
 * (n[i], key[i]), n as step 2 leaves it: G[i]; tries[i] (may be NULL) = the pairs drawn until one qualified, 1 .. 6,
 * or 0 when none did (u = 0). */
int rt_debug_indirect_dir(const rt_vec3 *n, const unsigned *key, int count, rt_vec3 *G, int *tries);
/* The queue lengths of the scene's last variant-0 indirect call, one per group of rays (waits for the call; tests and
 * tools): counts[0 .. *n - 1], the gather rays that hit something. cap: room in counts. */
int rt_debug_indirect_counts(rt_scene *s, int *counts, int cap, int *n);

/* ------------------------------------------------------------------ *
 * Multi-bounce global illumination: diffuse paths in   *
 * the gather pass.                                                    *
 * ------------------------------------------------------------------ */
#define RT_INDIRECT_MAX_BOUNCES 4
typedef struct rt_indirect_paths_opts {
    uint32_t struct_size;   /* sizeof; 0 reads as this layout; fields past a caller's size read as their defaults */
    int bounces;            /* 1 .. RT_INDIRECT_MAX_BOUNCES: surface hits a gather path may shade            [2] */
} rt_indirect_paths_opts;

/* The defaults in brackets above. */
void rt_indirect_paths_opts_init(rt_indirect_paths_opts *o);

/* rt_scene_indirect whose gather rays are diffuse paths of at most `bounces` shaded surface hits. `d` is
 * rt_scene_indirect's description, every field with its meaning, checks and error texts; o == NULL: the defaults.
 * Steps 1, 2, 4, 5 and 6 of rt_scene_indirect hold unchanged and so does the arithmetic; only c_j of step 3 changes.
 * For gather ray j of a live pixel (x, y), with B = bounces:
 *   O_0 = start, D_0 = G as step 3 forms them, key_0 = key(x, y, ray_base + j, seed). For b = 0 .. B - 1:
 *   (a) the nearest hit of ray(O_b, D_b) as RT_QUERY_NEAREST finds it;
 *   (b) a miss: term = getFColor(O_b, D_b); the path ends after (d);
 *   (c) a hit: h_b = castRay's record, term = what RT_QUERY_SHADE gives the hit: direct light times the hit's texel;
 *   (d) b == 0: L = 0.f + term per channel (what rt_scene_indirect stores); b >= 1: L = L + T_b * term;
 *   (e) b == B - 1: the path ends;
 *   (f) a_b = the texel (c) read for h_b (the same index expression and clamp); T_1 = a_0, T_{b+1} = T_b * a_b per
 *       channel;
 *   (g) n = h_b.normal, nn = (n.x*n.x + n.y*n.y) + n.z*n.z; nn 0 or not finite: the path ends (the dead rule of
 *       step 1). n = normalise(n), negated if dot(n, D_b) > 0; P = O_b + D_b * t_b per component (the record's own hit
 *       point, not new_org; a negative t as it is); O_{b+1} = n * 0.00001f + P; key_{b+1} = mix(key_b ^ 0x426f756e);
 *       D_{b+1} = step 3's direction for n under key_{b+1}.
 *   c_j = L.
 * Every continuation draw has the cosine density about n and the model carries no 1 / pi, so a bounce weighs the texel
 * alone, as step 5 does. Mirrors and glass met by a gather ray count as diffuse surfaces with their texel, as SHADE
 * treats them. No Russian roulette: a path ends by a miss, a dead normal or the budget only.
 * bounces == 1 issues exactly the launches of rt_scene_indirect and gives its bits. Both entries share one host path:
 * the same ordering, the same refusals (under this entry's name), one scratch. Variant 0 with bounces > 1 takes 576
 * bytes of scratch per pixel (per slot of a group of 4 rays a 16-byte colour and two queue entries of 64 bytes: origin,
 * direction, hit, slot, throughput and key), 16 more per pixel with more than 4 rays, and 64 bytes of counters.
 * bounces out of range -> RT_ERR_INVALID, naming the field, with nothing written. */
int rt_scene_indirect_paths(rt_scene *s, const rt_indirect_desc *d, const rt_indirect_paths_opts *o, void *stream);

/* rt_scene_set_indirect_timing / rt_scene_indirect_times serve this entry too. With bounces > 1: variant 1: [0] the
 * kernel; variant 0: per group of at most 4 rays the cast pass, `bounces` shade-and-continue passes and the resolve
 * pass, (2 + bounces) intervals a group. */

/* The queue lengths of the scene's last variant-0 rt_scene_indirect_paths call with bounces > 1 (waits for the call;
 * tests and tools): counts[group * bounces + b] = the entries that entered bounce b's shade pass. *n = groups *
 * bounces, at most cap; 0 after any other indirect call (and rt_debug_indirect_counts gives 0 after such a call). */
int rt_debug_indirect_path_counts(rt_scene *s, int *counts, int cap, int *n);
/* key_b of (g) for `count` keys key_0 (the same code the kernels run, no GPU needed; tests only): out[i]. b >= 0. */
int rt_debug_indirect_path_key(const unsigned *key, int count, int b, unsigned *out);

/* ------------------------------------------------------------------ *
 * Emissive surfaces: spheres, planes and cubes that     *
 * light the gather paths of the two indirect entries.                  *
 * ------------------------------------------------------------------ */
/* Emission per primitive of one kind, under rt_scene_set_roughness' protocol: kind = RT_HIT_SPHERE, RT_HIT_PLANE or
 * RT_HIT_CUBE (anything else, RT_HIT_TRIANGLE included: RT_ERR_INVALID, naming the kind; a triangle emits nothing);
 * rgb holds 3 * n floats, one colour per primitive of that kind's list, n the list's count. NULL or n == 0 clears the
 * kind's table and always succeeds. A value that is not finite and >= 0 (the message names the kind, the primitive,
 * the channel and the value; the values are checked before the count), or another count than the list's:
 * RT_ERR_INVALID, and nothing changes on an error. A table behaves as the
 * roughness table when its list is set again: it survives rt_scene_set_spheres / _planes / _cubes with the same count
 * and is cleared by a different count.
 *
 * Host-side state, read when an indirect call is launched: no wait, no device needed here. The scene's next
 * rt_scene_indirect / rt_scene_indirect_paths call uploads a table that changed (16 bytes per primitive) on its own
 * stream, ordered on the device after the scene's indirect calls in flight; only a table that grows waits on the host
 * for them. rt_indirect_desc and rt_indirect_paths_opts are unchanged.
 *
 * Semantics: steps 1 to 6 of rt_scene_indirect and (a) to (g) of rt_scene_indirect_paths with one change. The colour
 * RT_QUERY_SHADE gives a gather hit (c_j of step 3; `term` of (c)) becomes term + e per channel in binary32, e the
 * table entry of the hit record's (kind, index); e = 0 for a triangle and for a kind without a table. Everything after
 * uses that sum as it used the term: 0.f + term at bounce 0, L + T_b * term later, the order of the sums, steps 4 to 6.
 * The texel throughput of an emitter is its texel, as for any surface; a miss is getFColor; dead pixels, keys and
 * directions are unchanged, so emission changes no path and no queue length. Without a table (never set, or every
 * kind cleared) a call launches the kernels it launched before emission existed and gives their bits; an all-zero
 * table gives the same bits through the other instantiations.
 * Emission is found by the cosine-distributed gather rays alone: no emitter is sampled directly, so a small bright one
 * is noisy (rt_scene_temporal and the denoisers are the remedy). The frame kernel, RT_QUERY_SHADE, the ray queries and
 * the reflective passes do not read the tables: an emitter seen by the primary ray is the caller's to add from the id
 * guide (Scene.emission_term in the Python wrapper), one seen in a mirror or through glass is not shown. */
int rt_scene_set_emission(rt_scene *s, int kind, const float *rgb, int n);

#ifdef __cplusplus
}
#endif
#endif /* RT_ENGINE_H */
