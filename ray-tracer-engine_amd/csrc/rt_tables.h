// rt_tables.h -- builders of the culling tables (rt_tables.hip); internal to the library.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "rt_internal.h"

// Largest beam slope the eye cones are valid for (RtFrameConsts::cone_kcap): tiles whose own
// beam is wider (tiny resolutions) fall back to the 3-D blocks.
#define RT_CONE_KCAP 0.1
// Longest list (padded to 64) the one-workgroup device builder sorts in LDS (8 B per key).
#define RT_EYE_DEVICE_MAX 8192

// A sphere count padded to whole waves of 64: the length of every Morton-, column- and cone-ordered table.
inline int rt_pad64(int n) { return (n + 63) & ~63; }

void rt_build_sorted_blocks(const float4 *tab, int n, float4 *sorted, float4 *blocks, int *orig);
void rt_build_light_columns(const float4 *tab, int n, const float u[3], float4 *sorted, float4 *blocks);
// Per sphere S of the table and one light: the entries a shadow ray from S's surface towards the light can hit
// (see RtFrameAux::cand_hdr). hdr: n records; ent: the concatenated lists.
#include <vector>
struct RtCandHdr;
void rt_build_occluder_lists(const float4 *tab, int n, const float lpos[3], std::vector<RtCandHdr> &hdr, std::vector<float4> &ent);
// Slope of the beam the frame kernel gives a group of shadow rays that start at `start` (binary64 restatement of the
// kernel's bound; NaN when it has none).
double rt_light_beam_slope(const double lpos[3], const double start[3]);
// ... and its supremum over every start in the ball B(c, r0) (the slope a group of pixels on that sphere uses); -1: none
double rt_sphere_beam_slope(const double lpos[3], const double c[3], double r0);
double rt_beam_sine_at_start(const double lpos[3], const double start[3], double *sigma, double *frob, double m9[9]);
// The lists built on the device (one wave per sphere): hdr: n records, ent: n * RT_CAND_CAP entries (a slot per sphere).
hipError_t rt_occluder_lists_launch(const float4 *tab, int n, const float lpos[3], RtCandHdr *hdr, float4 *ent, hipStream_t stream);
void rt_build_eye_cones_host(const float4 *tab, int n, const float org[3], float4 *sorted, float4 *blocks, int *orig);

size_t rt_eye_cones_size(int n);   // float4 units: [n_pad entries][2 per block][n_pad ints]
// Build the table on the device, on `stream`, with one workgroup of `threads` (a multiple of 64, <= 1024)
// (tab: the list-order table in device memory).
hipError_t rt_eye_cones_launch(const float4 *tab, int n, const float org[3], float4 *out, int threads, hipStream_t stream);
// The same launch as a graph kernel node: function, geometry and dynamic LDS; the arguments are
// (const float4 *tab, int n, float ox, float oy, float oz, float4 *out).
void rt_eye_cones_kernel_config(int n, int threads, const void **func, dim3 *grid, dim3 *block, unsigned *lds_bytes);

// View lists (RtFrameConsts::view_lists): one view -- ray origin, rotation, eye_nz, frame size and aspect -- cut into
// blocks of 2^bw x 2^bh pixels; per block the front-to-back list of the spheres a primary ray of the block can hit.
// `cones`: the eye-cone table of the same origin (rt_eye_cones_launch) or null; `tab`: the scene's sphere allocation
// ([n] list order | Morton order | blocks | positions, rt_scene::d_spheres).
struct RtViewParams {
    const float4 *tab;
    const float4 *cones;
    int n, n_blocks;
    float org[3];
    float cos_pitch, sin_pitch, cos_yaw, sin_yaw;
    float eye_nz, aspect;
    int width, height;
    int bw, bh;                // log2 of the block's width and height in pixels
    int nbx, nby;
    float4 *out;               // nbx * nby slots of RT_VIEW_SLOT float4
};
// The block's cone as the builders hand it to the member test: unit axis and slope (ok = false: no usable cone).
struct RtViewBeam {
    float ux, uy, uz, k;
    bool ok;
};
RtViewBeam rt_view_block_beam(const RtViewParams &p, int bx, int by);
// Block size for a frame: 64 x 64 pixels, halved (down to a tile, 8 x 8) while the frame has fewer than 256 blocks.
void rt_view_block_shape(int width, int height, int *bw, int *bh);
inline size_t rt_view_lists_size(int nbx, int nby) { return (size_t)nbx * (size_t)nby * RT_VIEW_SLOT; }   // float4 units
hipError_t rt_view_lists_launch(const RtViewParams &p, hipStream_t stream);
// The same launch as a graph kernel node; the argument is (RtViewParams p).
void rt_view_lists_kernel_config(const RtViewParams &p, const void **func, dim3 *grid, dim3 *block);
// Host restatement: the member test over the whole list-order table `tab` (n entries), no block level.
void rt_build_view_lists_host(const float4 *tab, const RtViewParams &p, float4 *out);

// Order of the tiles of a launch (RtFrameConsts::tile_perm): blocks of RT_TILE_ORDER_BLOCK x RT_TILE_ORDER_BLOCK tiles,
// the block with the longest tile first (cost[tile]: wave durations of the previous launch, shader clocks; 0 = never
// rendered), tiles row-major inside a block; perm[] = (tile_y << 16) | tile_x. Three small kernels on `stream` (the
// blocks' longest tiles into key[]; the blocks sorted, where each starts into start[]; a thread per tile writes perm[]).
// Always a permutation of the tiles, whatever cost[] holds. At most RT_TILE_ORDER_MAX_BLOCKS blocks; key[], start[]:
// one unsigned per block.
#define RT_TILE_ORDER_BLOCK 16
#define RT_TILE_ORDER_MAX_BLOCKS 4096
hipError_t rt_tile_order_launch(const unsigned *cost, unsigned *key, unsigned *start, unsigned *perm, int tiles_x, int tiles_y,
                                hipStream_t stream);

// The tiles of a launch (tile_w x 64 / tile_w pixels over width x rows) and their blocks; ok: the launch has tiles and
// the kernels above can order them (else it keeps grid order).
struct RtTileGrid {
    int tiles_x, tiles_y, nbx, nby, n, nb;
    bool ok;
};
inline RtTileGrid rt_tile_grid(int tile_w, int width, int rows)
{
    RtTileGrid g;
    const int th = 64 / tile_w;
    g.tiles_x = (width + tile_w - 1) / tile_w;
    g.tiles_y = (rows + th - 1) / th;
    g.nbx = (g.tiles_x + RT_TILE_ORDER_BLOCK - 1) / RT_TILE_ORDER_BLOCK;
    g.nby = (g.tiles_y + RT_TILE_ORDER_BLOCK - 1) / RT_TILE_ORDER_BLOCK;
    g.ok = g.tiles_x > 0 && g.tiles_y > 0 && g.tiles_x <= 0xffff && g.tiles_y <= 0xffff &&
           (long long)g.nbx * g.nby <= RT_TILE_ORDER_MAX_BLOCKS;
    g.n = g.ok ? g.tiles_x * g.tiles_y : 0;
    g.nb = g.ok ? g.nbx * g.nby : 0;
    return g;
}
// The arrays of rt_tile_order_launch in one allocation: [cap] durations | [cap] order | [nb_cap] block keys |
// [nb_cap] block starts.
struct RtTileOrderBuf {
    DevArray<unsigned> mem;
    size_t cap = 0, nb_cap = 0;
    unsigned *cost() const { return mem.get(); }
    unsigned *perm() const { return mem.get() + cap; }
    unsigned *key() const { return mem.get() + 2 * cap; }
    unsigned *start() const { return mem.get() + 2 * cap + nb_cap; }
    bool fits(const RtTileGrid &g) const { return (size_t)g.n <= cap && (size_t)g.nb <= nb_cap; }
    // Room for grid g: re-allocates only when it does not fit, and then keeps none of the old contents.
    hipError_t reserve(const RtTileGrid &g)
    {
        if (fits(g)) return hipSuccess;
        cap = nb_cap = 0;
        hipError_t e = mem.reset();
        if (e == hipSuccess) e = mem.reserve(2 * (size_t)g.n + 2 * (size_t)g.nb);
        if (e != hipSuccess) return e;
        cap = (size_t)g.n;
        nb_cap = (size_t)g.nb;
        return hipSuccess;
    }
};
void rt_tile_order_kernel_configs(int tiles_x, int tiles_y, const void *func[3], dim3 grid[3], dim3 block[3]);

// The run list of a compact reading launch (the list section of the RT_REST_* layout block, rt_device.h): a stable
// partition of the launch's order -- perm[], or grid order when it is null -- into the tiles that keep a wave of their
// own and, behind them, the streamable ones, with the header {n_unsettled, n_streamed, run, n_ahead} in front. Three small
// launches on `stream`; they read the table's summaries and, for settled tiles with miss lanes, their primary records.
#define RT_REST_LIST_BLOCK 256
#define RT_REST_LIST_MAX_BLOCKS 4096          // what the one-workgroup sum of the blocks' counts holds: 2^20 tiles
struct RtRestListParams {
    unsigned char *table;      // the resting-view table of the launch's T tiles
    const unsigned *perm;      // T entries (tile_y << 16) | tile_x, or null
    unsigned *scratch;         // rt_rest_list_scratch(T) dwords: a flag per place of the order, a count per block
    int tile_w, width, local_rows, y0, y1, il_count, il_index, il_rows;   // the launch's geometry, as in RtFrameConsts
    unsigned run;              // R, 1 ... RT_REST_LIST_RUN_MAX
    unsigned ahead;            // 1: the runs' workgroups in front of the one-wave tiles' (header: n_ahead), 0: behind them
};
inline size_t rt_rest_list_scratch(size_t tiles) { return tiles + (tiles + RT_REST_LIST_BLOCK - 1) / RT_REST_LIST_BLOCK; }
inline bool rt_rest_list_fits(size_t tiles) { return tiles > 0 && (tiles + RT_REST_LIST_BLOCK - 1) / RT_REST_LIST_BLOCK <= RT_REST_LIST_MAX_BLOCKS; }
hipError_t rt_rest_list_launch(const RtRestListParams &p, hipStream_t stream);
