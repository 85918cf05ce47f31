// rt_debug.cpp -- diagnostics for the tests (rt_debug_*): device evaluation of scalar building blocks and the host
// restatements of the table builders, host arrays in and out.
#include <limits.h>

#include "rt_scene.h"

// launchers defined in rt_kernels.hip
extern "C" hipError_t rt_dev_launch_dbg_shortcuts(int what, unsigned seed, long long n, unsigned long long *out, hipStream_t stream);
extern "C" hipError_t rt_dev_launch_dbg_math(int op, const float *a, const float *b, float *out, int n,
                                             hipStream_t stream);
extern "C" hipError_t rt_dev_launch_dbg_floor(int what, int workgroups, int run, const unsigned *table, float4 *rgba, unsigned *packed,
                                              int width, int height, hipStream_t stream);
extern "C" hipError_t rt_dev_launch_dbg_intersect(const float4 *tab, const float *rays, int n, int *hit,
                                                  float *t, hipStream_t stream);
extern "C" hipError_t rt_dev_launch_dbg_light(const RtFrameConsts *fc, const float4 *tab, const float *starts,
                                              const float *normals, int light_index, int n, float *dirs,
                                              float *bright, float *adirs, int *aok, hipStream_t stream);

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
    rt_pack_spheres(spheres, n, tab.data());
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
    rt_pack_spheres(spheres, n, tab.data());
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
    rt_pack_spheres(spheres, n, tab.data());
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
    rt_pack_spheres(spheres, n, tab.data());
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
    if (n_spheres) rt_pack_spheres(spheres, n_spheres, tab.data());
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

// The tile order of a grid of tiles_x x tiles_y tiles as the DEVICE sorts it from cost[] (rt_tile_order_launch: what a
// scene's launches use), downloaded: key[nb], start[nb], perm[n]. via_configs != 0: the same three kernels launched from
// the functions and geometries of rt_tile_order_kernel_configs, as a frame graph's kernel nodes are. A grid that
// rt_tile_grid does not accept: RT_ERR_UNSUPPORTED, nothing launched.
extern "C" int rt_debug_tile_order(const unsigned *cost, int tiles_x, int tiles_y, int via_configs, unsigned *key, unsigned *start,
                                   unsigned *perm)
{
    // The argument and grid checks come before the first HIP call: a refusal needs no device, and
    // tests/test_tile_order_cpu.py relies on that on machines without one.
    if (!cost || !key || !start || !perm || tiles_x <= 0 || tiles_y <= 0) {
        rt_set_error("rt_debug_tile_order: bad argument");
        return RT_ERR_INVALID;
    }
    const int tile_w = 8, tile_h = 64 / tile_w;
    if (tiles_x > INT_MAX / tile_w || tiles_y > INT_MAX / tile_h) {
        rt_set_error("rt_debug_tile_order: %d x %d tiles cannot be ordered", tiles_x, tiles_y);
        return RT_ERR_UNSUPPORTED;
    }
    const RtTileGrid g = rt_tile_grid(tile_w, tile_w * tiles_x, tile_h * tiles_y);
    if (!g.ok || g.tiles_x != tiles_x || g.tiles_y != tiles_y) {
        rt_set_error("rt_debug_tile_order: %d x %d tiles cannot be ordered", tiles_x, tiles_y);
        return RT_ERR_UNSUPPORTED;
    }
    RtTileOrderBuf buf;
    HipStream stream;
    RT_HIP(buf.reserve(g));
    RT_HIP(stream.create(hipStreamNonBlocking));
    // everything on `stream`, a non-blocking one: the null stream's work is not ordered against it
    RT_HIP(hipMemcpyAsync(buf.cost(), cost, sizeof(unsigned) * (size_t)g.n, hipMemcpyHostToDevice, stream.get()));
    // known contents where the kernels must write: an entry of perm[] they leave out is no tile
    RT_HIP(hipMemsetAsync(buf.perm(), 0xff, sizeof(unsigned) * (size_t)g.n, stream.get()));
    RT_HIP(hipMemsetAsync(buf.key(), 0xa5, sizeof(unsigned) * (size_t)g.nb, stream.get()));
    RT_HIP(hipMemsetAsync(buf.start(), 0, sizeof(unsigned) * (size_t)g.nb, stream.get()));     // in range: the third kernel indexes perm[] by it
    if (!via_configs) {
        RT_HIP(rt_tile_order_launch(buf.cost(), buf.key(), buf.start(), buf.perm(), g.tiles_x, g.tiles_y, stream.get()));
    } else {
        // What this path tests is the functions, grids and blocks of rt_tile_order_kernel_configs. The argument lists
        // below are this function's own, written from the comment at rt_tile_order_kernel_configs; the lists
        // rt_graph.cpp builds for its kernel nodes are not exercised here (graph replays are: test_gpu_parity.py).
        const void *func[3];
        dim3 grid[3], block[3];
        rt_tile_order_kernel_configs(g.tiles_x, g.tiles_y, func, grid, block);
        const unsigned *d_cost = buf.cost();
        unsigned *d_key = buf.key(), *d_start = buf.start(), *d_perm = buf.perm();
        const unsigned *d_key_in = d_key, *d_start_in = d_start;
        int tx = g.tiles_x, ty = g.tiles_y, nbx = g.nbx, nby = g.nby, n = g.n;
        void *keys_args[] = {&d_cost, &d_key, &nbx, &tx, &ty};
        void *sort_args[] = {&d_key_in, &d_start, &nbx, &nby, &tx, &ty};
        void *expand_args[] = {&d_start_in, &d_perm, &n, &tx, &nbx};
        RT_HIP(hipLaunchKernel(func[0], grid[0], block[0], keys_args, 0, stream.get()));
        RT_HIP(hipLaunchKernel(func[1], grid[1], block[1], sort_args, 0, stream.get()));
        RT_HIP(hipLaunchKernel(func[2], grid[2], block[2], expand_args, 0, stream.get()));
    }
    RT_HIP(hipStreamSynchronize(stream.get()));
    RT_HIP(hipMemcpy(key, buf.key(), sizeof(unsigned) * (size_t)g.nb, hipMemcpyDeviceToHost));
    RT_HIP(hipMemcpy(start, buf.start(), sizeof(unsigned) * (size_t)g.nb, hipMemcpyDeviceToHost));
    RT_HIP(hipMemcpy(perm, buf.perm(), sizeof(unsigned) * (size_t)g.n, hipMemcpyDeviceToHost));
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
    rt_view_rotation(&fd, &fc);
    RtViewParams p;
    rt_view_params_from_consts(fc, fd.aspect, &p);
    std::vector<float4> tab((size_t)n);
    rt_pack_spheres(spheres, n, tab.data());
    const size_t total = rt_view_lists_size(p.nbx, p.nby);
    std::vector<float4> h(total);
    p.out = h.data();
    rt_build_view_lists_host(tab.data(), p, h.data());
    memset(out, 0, sizeof *out);
    out->block_w = 1 << p.bw; out->block_h = 1 << p.bh;
    out->blocks_x = p.nbx; out->blocks_y = p.nby;
    rt_view_lists_summary(h.data(), p.nbx * p.nby, out);
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

// What a launch of the reading kernel's geometry costs before it computes anything (tools/launch_floor_probe.py,
// DESIGN.md 6a). cfgs: n_cfgs triples {what, workgroups, run} (rt_dev_launch_dbg_floor in rt_kernels.hip says what each
// is). After `preroll` launches of the linear fill, `rounds` rounds; a round times every configuration once, in the
// order given -- the rounds are interleaved, so a drift of the clock meets all of them alike --, `reps` launches
// back to back between two events. ms[c * rounds + r]: milliseconds per launch.
extern "C" int rt_debug_launch_floor(int width, int height, const int *cfgs, int n_cfgs, int rounds, int reps, int preroll, float *ms)
{
    if (width < 1 || height < 1 || width > 16384 || height > 16384 || ((size_t)width * (size_t)height) % 4 != 0 || !cfgs || n_cfgs < 1 ||
        rounds < 1 || reps < 1 || preroll < 0 || !ms) {
        rt_set_error("rt_debug_launch_floor: bad argument");
        return RT_ERR_INVALID;
    }
    const size_t pixels = (size_t)width * (size_t)height;
    int max_wg = 1;
    for (int c = 0; c < n_cfgs; ++c) {
        const int what = cfgs[3 * c], wg = cfgs[3 * c + 1], run = cfgs[3 * c + 2];
        if (what < 0 || what > 3 || wg < 1 || wg > (1 << 22) || run < 1 || run > 4096) {
            rt_set_error("rt_debug_launch_floor: configuration %d is {%d, %d, %d}", c, what, wg, run);
            return RT_ERR_INVALID;
        }
        if (wg > max_wg) max_wg = wg;
    }
    DevArray<unsigned> table, packed;
    DevArray<float4> rgba;
    RT_HIP(table.reserve((size_t)max_wg));
    RT_HIP(packed.reserve(pixels));
    RT_HIP(rgba.reserve(pixels * 5 / 4));   // the linear fill writes the packed words' bytes behind the float4
    RT_HIP(hipMemset(table.get(), 0, sizeof(unsigned) * (size_t)max_wg));
    HipEvent e0, e1;
    RT_HIP(e0.create(hipEventDefault));
    RT_HIP(e1.create(hipEventDefault));
    for (int i = 0; i < preroll; ++i)
        RT_HIP(rt_dev_launch_dbg_floor(3, 1, 1, table.get(), rgba.get(), packed.get(), width, height, nullptr));
    RT_HIP(hipDeviceSynchronize());
    for (int r = 0; r < rounds; ++r)
        for (int c = 0; c < n_cfgs; ++c) {
            RT_HIP(rt_dev_launch_dbg_floor(cfgs[3 * c], cfgs[3 * c + 1], cfgs[3 * c + 2], table.get(), rgba.get(), packed.get(), width, height, nullptr));
            RT_HIP(hipEventRecord(e0.get(), nullptr));
            for (int i = 0; i < reps; ++i)
                RT_HIP(rt_dev_launch_dbg_floor(cfgs[3 * c], cfgs[3 * c + 1], cfgs[3 * c + 2], table.get(), rgba.get(), packed.get(), width, height, nullptr));
            RT_HIP(hipEventRecord(e1.get(), nullptr));
            RT_HIP(hipEventSynchronize(e1.get()));
            float t = 0.f;
            RT_HIP(hipEventElapsedTime(&t, e0.get(), e1.get()));
            ms[(size_t)c * rounds + r] = t / (float)reps;
        }
    return RT_OK;
}
