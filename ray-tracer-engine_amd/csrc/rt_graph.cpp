// rt_graph.cpp -- the frame as a hipGraph (BASELINE config C4: 4-spp progressive
// accumulation, one graph replay per frame). Replaces the reference's per-frame
// malloc -> H2D -> launch -> sync -> free sequence (/root/reference/kernel.cu:1762-1792)
// with a graph built once:
//
//   [eye-cone build]  ->  [view-list build]  ->  [tile order: keys, sort, expand]  ->  [sample pass 0] -> ... -> [sample pass p-1]  ->  [copy to the present buffer]
//
// (the tile order -- blocks of 16 x 16 tiles, longest tile first, DESIGN.md section 4d -- is sorted at the head of every
// replay from the wave durations the passes of the previous replay recorded into the graph's own arrays)
//
// The nodes are added explicitly (no stream capture), so each kernel node's by-value frame
// uniforms can be replaced in the instantiated graph: a camera move -- the reference moves
// `cam` every frame (kernel.cu:1716-1764) -- is hipGraphExecKernelNodeSetParams on the pass
// nodes and on the build node, whose kernel then rebuilds the graph's OWN eye-cone table on
// the device at the next replay. No re-capture, no synchronisation, and the graph never reads
// a table that a direct render on the same scene has rebuilt for another camera.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/rt_engine.h"
#include "rt_internal.h"
#include "rt_tables.h"

struct rt_frame_graph {
    rt_scene *scene = nullptr;
    rt_frame_desc fd;
    int passes = 1;         // kernel nodes that render samples: 1 (all samples in one launch) or one per sample
    int samples = 1;        // samples per pixel of the frame
    uint32_t *host_pixels = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    // nodes whose parameters follow the camera
    hipGraphNode_t build_node = nullptr;
    hipGraphNode_t view_node = nullptr;      // the graph's own view lists (RtFrameConsts::view_lists), built after the cones
    hipKernelNodeParams view_kparams;
    RtViewParams view_params;
    DevArray<float4> views;
    bool views_on = false;
    hipGraphNode_t pass_node[RT_MAX_SPP] = {};
    bool pass_live[RT_MAX_SPP] = {};
    hipKernelNodeParams pass_params[RT_MAX_SPP];
    hipKernelNodeParams build_params;
    // argument storage the node parameters point at
    RtFrameConsts fc[RT_MAX_SPP];
    const float4 *spheres = nullptr;
    const float4 *build_tab = nullptr;
    int build_n = 0;
    float build_org[3] = {0, 0, 0};
    DevArray<float4> cones;          // the graph's own eye-cone table
    bool cones_on_device = false;    // built by the graph's build node (else by the host at (re)build time)
    unsigned long long epoch = 0;    // rt_scene_epoch() the nodes were built against
    RtTileOrderBuf order;            // launch order of the passes' tiles (rt_scene_set_tile_order)
    bool order_on = false;
};

static void release_graph(rt_frame_graph *g)
{
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
    if (g->graph) (void)hipGraphDestroy(g->graph);
    g->exec = nullptr;
    g->graph = nullptr;
    g->build_node = nullptr;
    g->view_node = nullptr;
    for (int p = 0; p < RT_MAX_SPP; ++p) g->pass_live[p] = false;
}

static rt_frame_desc pass_desc(const rt_frame_graph *g, int p)
{
    rt_frame_desc fd = g->fd;
    if (g->passes == 1) {   // every sample in one launch (the sums are formed in registers, in the same order)
        fd.opts.spp = g->samples;
        fd.opts.sample_base = 0;
        fd.opts.sample_total = g->samples;
        fd.opts.accumulate = 0;
        fd.opts.resolve = 0;
        return fd;
    }
    fd.opts.spp = 1;
    fd.opts.sample_base = p;
    fd.opts.sample_total = g->passes;
    fd.opts.accumulate = p > 0 ? 1 : 0;
    fd.opts.resolve = (p == g->passes - 1) ? 0 : -1;
    return fd;
}

// Fill the argument storage (frame uniforms of every pass, build origin) for the current camera.
static int fill_arguments(rt_frame_graph *g, bool with_cones)
{
    rt_ray_origin(&g->fd, g->build_org);
    for (int p = 0; p < g->passes; ++p) {
        const rt_frame_desc fd = pass_desc(g, p);
        const int rc = rt_build_frame_consts(g->scene, &fd, with_cones ? g->cones.get() : nullptr, &g->fc[p]);
        if (rc != RT_OK) return rc;
        if (g->order_on) {
            g->fc[p].tile_perm = g->order.perm();
            g->fc[p].tile_cost = g->order.cost();
        }
    }
    if (g->views_on) {   // one view for all passes: the same camera, frame and block shape
        const int nbx = g->view_params.nbx, nby = g->view_params.nby;
        RtViewParams vp;
        (void)rt_view_params_for_frame(g->scene, &g->fc[0], g->fd.aspect, 8, 1, 0, &vp);
        if (vp.nbx != nbx || vp.nby != nby) {
            rt_set_error("rt_graph: the view lists' geometry changed under a recorded graph");
            return RT_ERR_INVALID;
        }
        vp.tab = rt_scene_sphere_table(g->scene);
        vp.cones = g->cones.get();
        vp.out = g->views.get();
        g->view_params = vp;
        for (int p = 0; p < g->passes; ++p) {
            g->fc[p].view_lists = reinterpret_cast<const float *>(g->views.get());
            g->fc[p].view_nbx = vp.nbx;
            g->fc[p].view_shift = vp.bw | (vp.bh << 8);
        }
    }
    return RT_OK;
}

// (Re)build graph and executable against the scene as it is now.
static int build_graph(rt_frame_graph *g, hipStream_t stream)
{
    rt_scene *s = g->scene;
    {   // an earlier replay may still be running: it reads the nodes and the cone table rebuilt here
        const int rc = rt_scene_quiesce(s);
        if (rc != RT_OK) return rc;
    }
    release_graph(g);
    {   // sample passes are one-sample launches of one frame: same tables for all of them
        rt_frame_desc fd0 = pass_desc(g, 0);
        const int rc = rt_scene_prepare_static(s, &fd0, stream);
        if (rc != RT_OK) return rc;
    }
    float org[3];
    rt_ray_origin(&g->fd, org);
    const int n = rt_scene_sphere_count(s);
    const bool want_cones = g->fd.opts.cull != 0 && rt_scene_wants_eye_cones(s, org);
    g->cones_on_device = want_cones && ((n + 63) & ~63) <= RT_EYE_DEVICE_MAX;
    if (want_cones) {
        RT_HIP(g->cones.reserve(rt_eye_cones_size(n)));
        if (!g->cones_on_device) {   // list too long for the device builder: host build, blocking upload
            const int rc = rt_scene_build_eye_cones_host(s, org, g->cones.get(), stream);
            if (rc != RT_OK) return rc;
        }
    }
    // the passes' launch order: all passes render the same rows with the same tile shape
    RtTileGrid tg;
    g->order_on = false;
    {
        const rt_frame_desc fd0 = pass_desc(g, 0);
        RtKernelChoice kc0;
        RtFrameConsts fc0;
        int rc0 = rt_frame_kernel_choice(s, &fd0, &kc0);
        if (rc0 == RT_OK) rc0 = rt_build_frame_consts(s, &fd0, nullptr, &fc0);
        if (rc0 != RT_OK) return rc0;
        // the graph's own view lists: where it has its own eye cones and the passes' tiles nest in the blocks
        g->views_on = want_cones && rt_view_params_for_frame(s, &fc0, g->fd.aspect, kc0.tile, kc0.cull, kc0.mode, &g->view_params) != 0;
        if (g->views_on) RT_HIP(g->views.reserve(rt_view_lists_size(g->view_params.nbx, g->view_params.nby)));
        tg = rt_tile_grid(kc0.tile, fc0.width, fc0.local_rows);
        if (rt_scene_tile_order_mode(s) != 0 && tg.ok) {
            RT_HIP(g->order.reserve(tg));
            RT_HIP(hipMemset(g->order.cost(), 0, sizeof(unsigned) * tg.n));   // no durations yet: the first replay sorts zeros (any order)
            g->order_on = true;
        }
    }
    int rc = fill_arguments(g, want_cones);
    if (rc != RT_OK) return rc;
    g->spheres = rt_scene_sphere_table(s);

    RT_HIP(hipGraphCreate(&g->graph, 0));
    hipGraphNode_t prev = nullptr;
    if (g->cones_on_device) {
        g->build_tab = g->spheres;
        g->build_n = n;
        memset(&g->build_params, 0, sizeof g->build_params);
        const void *func;
        unsigned lds;
        rt_eye_cones_kernel_config(n, 1024, &func, &g->build_params.gridDim, &g->build_params.blockDim, &lds);
        g->build_params.func = const_cast<void *>(func);
        g->build_params.sharedMemBytes = lds;
        float4 *cones = g->cones.get();
        void *args[] = {&g->build_tab, &g->build_n, &g->build_org[0], &g->build_org[1], &g->build_org[2], &cones};
        g->build_params.kernelParams = args;
        RT_HIP(hipGraphAddKernelNode(&g->build_node, g->graph, nullptr, 0, &g->build_params));
        g->build_params.kernelParams = nullptr;   // `args` is a local: re-pointed on every update
        prev = g->build_node;
    }
    if (g->views_on) {   // after the cone table it reads (a host-built one is already there)
        memset(&g->view_kparams, 0, sizeof g->view_kparams);
        const void *func;
        rt_view_lists_kernel_config(g->view_params, &func, &g->view_kparams.gridDim, &g->view_kparams.blockDim);
        g->view_kparams.func = const_cast<void *>(func);
        void *args[] = {&g->view_params};
        g->view_kparams.kernelParams = args;
        RT_HIP(hipGraphAddKernelNode(&g->view_node, g->graph, prev ? &prev : nullptr, prev ? 1 : 0, &g->view_kparams));
        g->view_kparams.kernelParams = nullptr;
        prev = g->view_node;
    }
    if (g->order_on) {   // keys -> sort -> expand, from the durations of the previous replay
        const void *func[3];
        dim3 grid[3], block[3];
        rt_tile_order_kernel_configs(tg.tiles_x, tg.tiles_y, func, grid, block);
        const unsigned *c_cost = g->order.cost(), *c_key = g->order.key(), *c_start = g->order.start();
        unsigned *key = g->order.key(), *start = g->order.start(), *perm = g->order.perm();
        void *a0[] = {&c_cost, &key, &tg.nbx, &tg.tiles_x, &tg.tiles_y};
        void *a1[] = {&c_key, &start, &tg.nbx, &tg.nby, &tg.tiles_x, &tg.tiles_y};
        void *a2[] = {&c_start, &perm, &tg.n, &tg.tiles_x, &tg.nbx};
        void **args[3] = {a0, a1, a2};
        for (int k = 0; k < 3; ++k) {
            hipKernelNodeParams kp;
            memset(&kp, 0, sizeof kp);
            kp.func = const_cast<void *>(func[k]);
            kp.gridDim = grid[k];
            kp.blockDim = block[k];
            kp.kernelParams = args[k];
            hipGraphNode_t node;
            RT_HIP(hipGraphAddKernelNode(&node, g->graph, prev ? &prev : nullptr, prev ? 1 : 0, &kp));
            prev = node;
        }
    }
    for (int p = 0; p < g->passes; ++p) {
        const rt_frame_desc fd = pass_desc(g, p);
        RtKernelChoice kc;
        rc = rt_frame_kernel_choice(s, &fd, &kc);
        if (rc != RT_OK) return rc;
        if (g->fc[p].local_rows == 0) continue;
        hipKernelNodeParams &kp = g->pass_params[p];
        memset(&kp, 0, sizeof kp);
        const void *func;
        unsigned lds;
        RT_HIP(rt_dev_trace_config(&g->fc[p], kc.tile, kc.cull, kc.mode, kc.feat, &func, &kp.gridDim, &kp.blockDim, &lds));
        kp.func = const_cast<void *>(func);
        kp.sharedMemBytes = lds;
        void *args[] = {&g->fc[p], &g->spheres};
        kp.kernelParams = args;
        RT_HIP(hipGraphAddKernelNode(&g->pass_node[p], g->graph, prev ? &prev : nullptr, prev ? 1 : 0, &kp));
        kp.kernelParams = nullptr;
        g->pass_live[p] = true;
        prev = g->pass_node[p];
    }
    if (g->host_pixels && g->fd.pixels) {
        int y0 = g->fd.opts.y0, y1 = g->fd.opts.y1;
        if (y0 == 0 && y1 == 0) y1 = g->fd.height;
        hipGraphNode_t copy;
        RT_HIP(hipGraphAddMemcpyNode1D(&copy, g->graph, prev ? &prev : nullptr, prev ? 1 : 0, g->host_pixels, g->fd.pixels,
                                       sizeof(uint32_t) * (size_t)g->fd.width * (size_t)(y1 - y0), hipMemcpyDeviceToHost));
    }
    RT_HIP(hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0));
    g->epoch = rt_scene_epoch(s);
    return RT_OK;
}

extern "C" rt_frame_graph *rt_graph_capture(rt_scene *s, const rt_frame_desc *fd, int passes,
                                            uint32_t *host_pixels, void *stream)
{
    // passes > 0: that many samples per pixel, taken by ONE kernel node (the sample loop runs in the kernel: one pass
    // over the tile setup, no read-modify-write of the float4 frame between samples, no launch gaps -- C4 0.91 ms against
    // 1.00 as four nodes); passes < 0: |passes| progressive one-sample nodes, each adding into opts.rgba (a caller that
    // shows the frame between passes). The frames are the same bits either way.
    const bool progressive = passes < 0;
    if (progressive) passes = -passes;
    if (!s || !fd || passes < 1 || passes > RT_MAX_SPP) {
        rt_set_error("rt_graph_capture: invalid argument");
        return nullptr;
    }
    if (progressive && passes > 1 && !fd->opts.rgba) {
        rt_set_error("rt_graph_capture: progressive passes need opts.rgba (float4 accumulation buffer)");
        return nullptr;
    }
    if (fd->opts.stats) {
        rt_set_error("rt_graph_capture: the instrumented kernels are not recorded into graphs");
        return nullptr;
    }
    if (rt_frame_reflect_depth(fd) != 0) {
        rt_set_error("rt_graph_capture: reflect_depth > 0 is not recorded into graphs (RT_ERR_UNSUPPORTED)");
        return nullptr;
    }
    if (const char *aov = rt_frame_aov_field(fd)) {
        rt_set_error("rt_graph_capture: %s (G-buffer outputs) is not recorded into graphs (RT_ERR_UNSUPPORTED)", aov);
        return nullptr;
    }
    rt_frame_graph *g = new rt_frame_graph();
    g->scene = s;
    normalise_frame_desc(fd, &g->fd);   // (a caller's shorter struct ends before the newer fields)
    g->samples = passes;
    g->passes = progressive ? passes : 1;
    g->host_pixels = host_pixels;
    if (build_graph(g, (hipStream_t)stream) != RT_OK) {
        rt_graph_destroy(g);
        return nullptr;
    }
    return g;
}

// Push the argument storage into the instantiated graph.
static int update_nodes(rt_frame_graph *g)
{
    if (g->build_node) {
        float4 *cones = g->cones.get();
        void *args[] = {&g->build_tab, &g->build_n, &g->build_org[0], &g->build_org[1], &g->build_org[2], &cones};
        g->build_params.kernelParams = args;
        const hipError_t e = hipGraphExecKernelNodeSetParams(g->exec, g->build_node, &g->build_params);
        g->build_params.kernelParams = nullptr;
        RT_HIP(e);
    }
    if (g->view_node) {
        void *args[] = {&g->view_params};
        g->view_kparams.kernelParams = args;
        const hipError_t e = hipGraphExecKernelNodeSetParams(g->exec, g->view_node, &g->view_kparams);
        g->view_kparams.kernelParams = nullptr;
        RT_HIP(e);
    }
    for (int p = 0; p < g->passes; ++p) {
        if (!g->pass_live[p]) continue;
        void *args[] = {&g->fc[p], &g->spheres};
        g->pass_params[p].kernelParams = args;
        const hipError_t e = hipGraphExecKernelNodeSetParams(g->exec, g->pass_node[p], &g->pass_params[p]);
        g->pass_params[p].kernelParams = nullptr;
        RT_HIP(e);
    }
    return RT_OK;
}

extern "C" int rt_graph_launch(rt_frame_graph *g, void *stream)
{
    if (!g || !g->scene) return RT_ERR_INVALID;
    if (!g->exec || g->epoch != rt_scene_epoch(g->scene)) {
        // the scene's tables were rewritten since the nodes were built: never replay against them
        const int rc = build_graph(g, (hipStream_t)stream);
        if (rc != RT_OK) return rc;
    }
    RT_HIP(hipGraphLaunch(g->exec, (hipStream_t)stream));
    return rt_scene_note_launch(g->scene, (hipStream_t)stream, nullptr, nullptr, nullptr);   // a graph has tables of its own, and no light verdicts
}

extern "C" int rt_graph_set_camera(rt_frame_graph *g, const rt_camera *cam)
{
    if (!g || !cam || !g->scene) return RT_ERR_INVALID;
    g->fd.cam = *cam;
    float org[3];
    rt_ray_origin(&g->fd, org);
    const bool want_cones = g->fd.opts.cull != 0 && rt_scene_wants_eye_cones(g->scene, org);
    const bool structure_same = g->exec && g->epoch == rt_scene_epoch(g->scene) && want_cones == (g->build_node != nullptr) &&
                                (want_cones ? g->cones_on_device : true);
    if (!structure_same) {   // host-built cones, a camera at a non-finite position, a changed scene: rebuild
        const int rc = rt_scene_quiesce(g->scene);
        if (rc != RT_OK) return rc;
        release_graph(g);
        return RT_OK;        // rebuilt by the next rt_graph_launch, on its stream
    }
    const int rc = fill_arguments(g, want_cones);
    if (rc != RT_OK) return rc;
    return update_nodes(g);
}

extern "C" void rt_graph_destroy(rt_frame_graph *g)
{
    if (!g) return;
    if (g->scene) (void)rt_scene_quiesce(g->scene);
    release_graph(g);
    delete g;
}
