// rt_scene_rest.cpp -- the resting-view tables (RtFrameConsts::rest_rd / rest_wr; the
// layout is the RT_REST_* block of rt_device.h): the key a table is kept under, which launch records, reads or does
// neither, and the rt_debug_* read-backs and setters of a table's sections. The hand-over is note (h) of rt_scene.h.
#include "rt_scene.h"

// The key is, bit for bit, everything the frame kernel's decisions depend on: its uniforms (outputs, tile order and the
// table pointers themselves excluded), which instantiation runs, and the generation of what lies behind the uniforms'
// pointers -- `sphere_gen` for the sphere list and everything built from it, `epoch` for every buffer that is rewritten
// or re-allocated after a quiesce (textures, sky, RtFrameAux with its lights, light tables, occluder lists, raygen
// tables, a slot that grew); the cone table and the view lists are rebuilt in place only for another origin, view or
// sphere list, all of which the key holds.
// Policy: a launch whose key has a table reads it (RT_MODE_REST_READ). One whose key has none but is among the scene's last
// RT_REST_SLOTS table-less keys (rest_seen) writes one (RT_MODE_REST_WRITE) and leaves that history. A launch with any other
// key does neither and enters the history in place of its oldest entry: a moving camera records nothing, a view at rest
// records on its second launch, and so does every layout of a frame rendered as a repeating cycle of up to
// RT_REST_SLOTS launches (update()'s three row bands) on the cycle's second pass. A launch out of scope leaves the
// history as it is (it changes nothing a key holds); switching light verdicts off clears it.
static void rest_key(const rt_scene *s, const RtKernelChoice &kc, const RtFrameConsts &fc, RtRestKey *k)
{
    memset(k, 0, sizeof *k);   // (padding too: the key is compared with memcmp)
    k->fc = fc;
    k->fc.rgba = nullptr; k->fc.packed = nullptr; k->fc.packed24 = nullptr; k->fc.stats = nullptr;
    k->fc.tile_perm = nullptr; k->fc.tile_cost = nullptr;
    k->fc.aov_depth = nullptr; k->fc.aov_normal = nullptr; k->fc.aov_id = nullptr; k->fc.aov_albedo = nullptr;
    k->fc.rest_rd = nullptr; k->fc.rest_wr = nullptr;
    k->epoch = s->epoch;
    k->sphere_gen = s->sphere_gen;
    k->tile = kc.tile; k->cull = kc.cull; k->mode = kc.mode; k->feat = kc.feat;
}

// The compact reading launch of a launch that reads table c: rebuilds the table's run list when
// it is stale, adopts the builder's counts once they have arrived, and then points the launch at the list. The rules
// are beside RestSlot (rt_scene.h). *workgroups: the 1-D grid, 0 = the full grid, which gives the same frame.
static int rest_run_list(rt_scene *s, RestSlot &c, const RtKernelChoice &kc, RtFrameConsts *fc, hipStream_t stream, unsigned *workgroups)
{
    const size_t tiles = (size_t)c.tiles_x * (size_t)c.tiles_y;
    if (!s->compact_mode || c.tiles_x > 0xffff || c.tiles_y > 0xffff || !rt_rest_list_fits(tiles)) return RT_OK;
    unsigned char *table = reinterpret_cast<unsigned char *>(c.buf.get());
    const unsigned long long serial = fc->tile_perm ? s->order_cur_serial : 0;
    // A build costs three small launches and a copy on the frame's stream, and a view that rests for a dozen frames
    // while the host runs ahead of the device would pay for it and never see a compact frame (bench.py's held positions:
    // 9 % slower with a build at every first read and re-sort). So: no first build before the device has finished the
    // recording launch -- a host that is further ahead than that is not looking at a view known to rest --, and no
    // rebuild for another order before the counts of the build before have arrived, i.e. before compact launches can
    // follow it at all.
    bool stale = c.list_perm != fc->tile_perm || c.list_order_serial != serial || c.list_run != s->compact_run || c.list_ahead != s->compact_ahead;
    bool arrived = false;
    if (!c.list_built) RT_HIP(c.built.complete(&arrived));
    else if (!c.list_adopted) RT_HIP(c.list_done.complete(&arrived));
    if (!c.list_built ? !arrived : (stale && !c.list_adopted && !arrived)) return RT_OK;   // this launch keeps the full grid
    if (c.list_built && !c.list_adopted && arrived) {
        c.list_n[0] = c.list_counts.get()[0];
        c.list_n[1] = c.list_counts.get()[1];
        c.list_adopted = true;
    }
    // The reader with the compact head (MODE 8) renders a one-wave tile some 4 % slower than MODE 6 does: with few tiles
    // to stream the full grid is the faster launch, and nothing is rebuilt for it.
    if (c.list_adopted && (unsigned long long)c.list_n[1] * 100ull < (unsigned long long)s->compact_min_percent * tiles) return RT_OK;
    if (!c.list_built || stale) {
        const int rc = rt_scene_wait_all_frames(s, stream);   // frames in flight read the list that is rewritten
        if (rc != RT_OK) return rc;
        RT_HIP(c.list_counts.reserve(RT_REST_LIST_HEADER));
        RT_HIP(c.list_scratch.reserve(rt_rest_list_scratch(tiles)));
        RtRestListParams p;
        p.table = table;
        p.perm = fc->tile_perm;
        p.scratch = c.list_scratch.get();
        p.tile_w = kc.tile; p.width = fc->width; p.local_rows = fc->local_rows; p.y0 = fc->y0; p.y1 = fc->y1;
        p.il_count = fc->il_count; p.il_index = fc->il_index; p.il_rows = fc->il_rows;
        p.run = s->compact_run;
        p.ahead = s->compact_ahead;
        RT_HIP(rt_rest_list_launch(p, stream));
        RT_HIP(hipMemcpyAsync(c.list_counts.get(), table + RT_REST_LIST_OFFSET(tiles), sizeof(unsigned) * RT_REST_LIST_HEADER, hipMemcpyDeviceToHost, stream));
        RT_HIP(c.list_done.record(stream));
        c.list_built = true;
        c.list_perm = fc->tile_perm;
        c.list_order_serial = serial;
        c.list_run = s->compact_run;
        c.list_ahead = s->compact_ahead;
        s->list_rebuilds++;
    }
    if (!c.list_adopted) {
        bool done = false;
        RT_HIP(c.list_done.complete(&done));
        if (!done) return RT_OK;   // this launch keeps the full grid
        c.list_n[0] = c.list_counts.get()[0];
        c.list_n[1] = c.list_counts.get()[1];
        c.list_adopted = true;
    }
    RT_HIP(c.list_done.order(stream));   // a build for another order that is still under way (another stream's: a device-side wait)
    if ((size_t)c.list_n[0] + (size_t)c.list_n[1] != tiles) {
        rt_set_error("rt_scene_render: a run list of %u + %u tiles for a table of %zu", c.list_n[0], c.list_n[1], tiles);
        return RT_ERR_INVALID;
    }
    // The one-wave tiles' workgroups find their entry at tile_perm[blockIdx.x]: with the runs ahead of them (the measured
    // variant) the pointer is set back by the runs' workgroups, and no workgroup reads in front of the list.
    const unsigned n_runs = (c.list_n[1] + c.list_run - 1) / c.list_run;
    const uintptr_t list = reinterpret_cast<uintptr_t>(table + RT_REST_LIST_OFFSET(tiles)) + sizeof(unsigned) * RT_REST_LIST_HEADER;
    fc->tile_perm = reinterpret_cast<const unsigned *>(list - (c.list_ahead ? sizeof(unsigned) * (size_t)n_runs : 0));
    fc->flags |= RT_FLAG_COMPACT;
    *workgroups = c.list_n[0] + n_runs;
    s->compact_last.compact = 1;
    s->compact_last.n_unsettled = c.list_n[0];
    s->compact_last.n_streamed = c.list_n[1];
    s->compact_last.run = c.list_run;
    s->compact_last.ahead = (int)c.list_ahead;
    s->compact_last.workgroups = *workgroups;
    return RT_OK;
}

int rt_scene_prepare_rest(rt_scene *s, const RtKernelChoice &kc, RtFrameConsts *fc, bool eligible, hipStream_t stream, int *slot_out, unsigned *workgroups_out)
{
    *slot_out = -1;
    if (workgroups_out) *workgroups_out = 0;
    s->compact_last = RtCompactLast();
    s->rest_last = -1;
    s->rest_last_wrote = 0;
    if (!s->light_verdicts_mode)
        for (bool &b : s->rest_seen_valid) b = false;
    if (!eligible || !s->light_verdicts_mode) return RT_OK;
    RtRestKey key;
    rest_key(s, kc, *fc, &key);
    const int tiles_x = (int)rt_rest_tiles_x(fc->width, kc.tile), tiles_y = (int)rt_rest_tiles_y(fc->local_rows, kc.tile);   // the launch's grid
    const size_t tiles = (size_t)tiles_x * (size_t)tiles_y;
    int v = -1, seen = -1;
    for (int i = 0; i < RT_REST_SLOTS; ++i) {
        if (s->rest[i].valid && memcmp(&s->rest[i].key, &key, sizeof key) == 0) v = i;
        if (s->rest_seen_valid[i] && memcmp(&s->rest_seen[i], &key, sizeof key) == 0) seen = i;
    }
    if (v >= 0) {
        RestSlot &c = s->rest[v];
        if (c.tiles_x != tiles_x || c.tiles_y != tiles_y || c.buf.capacity() * sizeof(float4) < RT_REST_TABLE_BYTES(tiles)) {
            rt_set_error("rt_scene_render: light verdicts of %d x %d tiles for a launch of %d x %d", c.tiles_x, c.tiles_y, tiles_x, tiles_y);
            return RT_ERR_INVALID;
        }
        RT_HIP(rt_scene_order_reader(c, stream));   // the writing launch precedes its readers
        fc->rest_rd = reinterpret_cast<const unsigned char *>(c.buf.get());
        *slot_out = v;
        if (workgroups_out) {
            const int rc = rest_run_list(s, c, kc, fc, stream, workgroups_out);
            if (rc != RT_OK) return rc;
        }
    } else if (seen >= 0) {
        s->rest_seen_valid[seen] = false;
        RestSlot &c = rt_slot_victim(s->rest, [](const RestSlot &x) { return !x.valid; });
        const size_t total = (RT_REST_TABLE_BYTES(tiles) + sizeof(float4) - 1) / sizeof(float4);
        if (total > c.buf.capacity()) {
            const int rc = rt_scene_quiesce(s);   // nothing may still read or write the buffer that is freed
            if (rc != RT_OK) return rc;
            RT_HIP(c.built.host_wait());
        }
        c.valid = false;
        c.list_built = false;   // the run list of what the slot held
        c.list_adopted = false;
        RT_HIP(c.buf.reserve(total));
        // on the frame's stream: behind the slot's last writer and, through the frame ring, its last reader
        RT_HIP(c.built.order(stream));
        if (c.used) {
            if (s->ring_seq - c.last_use <= RT_RING) RT_HIP(hipStreamWaitEvent(stream, s->ring[c.last_use % RT_RING].get(), 0));
            else {
                const int rc = rt_scene_wait_all_frames(s, stream);
                if (rc != RT_OK) return rc;
            }
        }
        // all ones: a word no launch writes (code 3 is "evaluate" to a reader), so a read-back can count unwritten tiles
        // The record tags behind the words take the same fill in the same call (a second one costs a recording launch
        // another launch on its stream): every tile the launch renders stores its tag dword, 0 where it took no record,
        // and an all-ones tag of a tile it did not render names group 15, which no iteration has -- RT_SHADOW_TAG_UNWRITTEN
        // to the read-back. The records themselves are read only where a tag points and stay as they are. The primary
        // records behind them need no fill either: the launch stores every lane of every tile it renders, and a reader
        // of the same key renders exactly those tiles. The same holds for the tile summaries behind those.
        RT_HIP(hipMemsetAsync(c.buf.get(), 0xff, RT_REST_FILL_BYTES(tiles), stream));
        c.key = key;
        c.tiles_x = tiles_x;
        c.tiles_y = tiles_y;
        fc->rest_wr = reinterpret_cast<unsigned char *>(c.buf.get());
        v = (int)(&c - s->rest);
        *slot_out = v;
        s->rest_last_wrote = 1;
    } else {
        s->rest_seen[s->rest_seen_next] = key;
        s->rest_seen_valid[s->rest_seen_next] = true;
        s->rest_seen_next = (s->rest_seen_next + 1) % RT_REST_SLOTS;
    }
    s->rest_last = v;
    return RT_OK;
}

// After the launch: a table it wrote becomes readable behind the launch's event.
int rt_scene_end_rest(rt_scene *s, int slot, hipStream_t stream)
{
    if (slot < 0 || !s->rest_last_wrote) return RT_OK;
    RestSlot &c = s->rest[slot];
    RT_HIP(c.built.record(stream));
    c.valid = true;
    c.used = false;
    return RT_OK;
}

// ---------------------------------------------------------------------------
// read-backs and setters of the table the last launch wrote or read (tests and profiles)
// ---------------------------------------------------------------------------
static size_t tiles_of(const RestSlot &c) { return (size_t)c.tiles_x * (size_t)c.tiles_y; }

// `bytes` at `offset` of a table, to the host or from it
static hipError_t copy_section(RestSlot &c, size_t offset, size_t bytes, void *host, hipMemcpyKind dir)
{
    char *dev = reinterpret_cast<char *>(c.buf.get()) + offset;
    return dir == hipMemcpyDeviceToHost ? hipMemcpy(host, dev, bytes, dir) : hipMemcpy(dev, host, bytes, dir);
}

// What every read-back starts with: *c = the last launch's table, its writer waited for, and `out`'s common fields; or
// null and a zeroed `out` with slot -1 when that launch had none (or was a writing launch that failed).
template <typename Info>
static int last_table(rt_scene *s, Info *out, const char *who, RestSlot **c)
{
    *c = nullptr;
    if (!s || !out) {
        rt_set_error("%s: null argument", who);
        return RT_ERR_INVALID;
    }
    memset(out, 0, sizeof *out);
    out->slot = -1;
    if (s->rest_last < 0 || !s->rest[s->rest_last].valid) return RT_OK;
    RestSlot &t = s->rest[s->rest_last];
    RT_HIP(t.built.host_wait());
    out->state = s->rest_last_wrote ? 1 : 2;
    out->slot = s->rest_last;
    out->tiles_x = t.tiles_x;
    out->tiles_y = t.tiles_y;
    *c = &t;
    return RT_OK;
}

// What both setters start with: the last launch's table, which must hold `n` = `per_tile` x tiles `unit`; no launch
// still reads it and its writer has finished.
static int last_table_to_set(rt_scene *s, bool args, const char *who, size_t n, size_t per_tile, const char *unit, const char *of, RestSlot **c)
{
    if (!s || !args || s->rest_last < 0 || !s->rest[s->rest_last].valid) {
        rt_set_error("%s: the last launch neither wrote nor read a table", who);
        return RT_ERR_INVALID;
    }
    RestSlot &t = s->rest[s->rest_last];
    if (n != per_tile * tiles_of(t)) {
        rt_set_error("%s: %zu %s given, the table has %d x %d%s", who, n, unit, t.tiles_x, t.tiles_y, of);
        return RT_ERR_INVALID;
    }
    const int rc = rt_scene_quiesce(s);   // no launch still reads the table
    if (rc != RT_OK) return rc;
    RT_HIP(t.built.host_wait());
    *c = &t;
    return RT_OK;
}

// What the last frame launch on this scene did with light verdicts (waits for the launch that wrote the table).
extern "C" int rt_debug_light_verdicts(rt_scene *s, rt_light_verdicts_info *out, unsigned long long *words, size_t cap)
{
    RestSlot *c;
    const int rc = last_table(s, out, "rt_debug_light_verdicts", &c);
    if (rc != RT_OK || !c) return rc;
    const size_t n = tiles_of(*c);
    std::vector<unsigned long long> h(n);
    RT_HIP(copy_section(*c, 0, RT_REST_WORD_BYTES * n, h.data(), hipMemcpyDeviceToHost));
    for (unsigned long long w : h) {
        if (w == ~0ull) {
            out->unwritten++;
            continue;
        }
        for (int b = 0; b < 64; b += 2) {
            const unsigned code = (unsigned)(w >> b) & 3u;
            if (code == RT_VERDICT_NOTHING) out->nothing++;
            if (code == RT_VERDICT_CLEAR) out->clear++;
        }
    }
    if (words) {
        if (cap < n) {
            rt_set_error("rt_debug_light_verdicts: room for %zu words, the table has %zu", cap, n);
            return RT_ERR_INVALID;
        }
        memcpy(words, h.data(), sizeof(unsigned long long) * n);
    }
    return RT_OK;
}

// The shadow counts of the last launch's table (waits for the launch that wrote it).
extern "C" int rt_debug_shadow_counts(rt_scene *s, rt_shadow_counts_info *out, unsigned *tags, unsigned char *counts, size_t cap)
{
    RestSlot *c;
    const int rc = last_table(s, out, "rt_debug_shadow_counts", &c);
    if (rc != RT_OK) return rc;
    out->records = RT_SHADOW_RECORDS;
    if (!c) return RT_OK;
    const size_t n = tiles_of(*c);
    std::vector<unsigned> h;   // the last table's tags
    for (RestSlot &o : s->rest) {   // every table the scene holds: a frame rendered in row bands has one per band
        if (!o.valid) continue;
        RT_HIP(o.built.host_wait());
        const size_t m = tiles_of(o);
        std::vector<unsigned> ht(m);
        RT_HIP(copy_section(o, RT_REST_TAGS_OFFSET(m), RT_REST_TAG_BYTES * m, ht.data(), hipMemcpyDeviceToHost));
        for (unsigned &t : ht) {
            if (t == RT_SHADOW_TAG_UNWRITTEN) t = 0;   // (a tile the writing launch did not render: no record)
            int k = 0;
            for (int r = 0; r < 4; ++r) k += ((t >> (8 * r)) & 0x80u) ? 1 : 0;
            out->tagged_all += k;
            if (&o == c) {
                out->tagged += k;
                out->tiles_tagged += k ? 1 : 0;
            }
        }
        if (&o == c) h.swap(ht);
    }
    if (tags || counts) {
        if (cap < n) {
            rt_set_error("rt_debug_shadow_counts: room for %zu tiles, the table has %zu", cap, n);
            return RT_ERR_INVALID;
        }
        if (tags) memcpy(tags, h.data(), sizeof(unsigned) * n);
        if (counts) RT_HIP(copy_section(*c, RT_REST_COUNTS_OFFSET(n), RT_REST_COUNT_BYTES * n, counts, hipMemcpyDeviceToHost));
    }
    return RT_OK;
}

// Tests: overwrite the tags and / or the records of the table the last launch wrote or read (either may be null).
extern "C" int rt_debug_set_shadow_counts(rt_scene *s, const unsigned *tags, const unsigned char *counts, size_t n)
{
    RestSlot *c;
    const int rc = last_table_to_set(s, true, "rt_debug_set_shadow_counts", n, 1, "tiles", "", &c);
    if (rc != RT_OK) return rc;
    if (tags) RT_HIP(copy_section(*c, RT_REST_TAGS_OFFSET(n), RT_REST_TAG_BYTES * n, const_cast<unsigned *>(tags), hipMemcpyHostToDevice));
    if (counts) RT_HIP(copy_section(*c, RT_REST_COUNTS_OFFSET(n), RT_REST_COUNT_BYTES * n, const_cast<unsigned char *>(counts), hipMemcpyHostToDevice));
    return RT_OK;
}

// The primary records of the last launch's table (waits for the launch that wrote it). The tile's place in the frame,
// and with it its block of the view lists, is formed as the kernel forms it, from the uniforms in the slot's key.
extern "C" int rt_debug_primary_records(rt_scene *s, rt_primary_records_info *out, unsigned *dwords, int *positions, size_t cap)
{
    RestSlot *cp;
    const int rc = last_table(s, out, "rt_debug_primary_records", &cp);
    if (rc != RT_OK || !cp) return rc;
    RestSlot &c = *cp;
    const size_t n = tiles_of(c);
    std::vector<unsigned> h(64 * n);
    RT_HIP(copy_section(c, RT_REST_PRIMARY_OFFSET(n), RT_REST_PRIMARY_BYTES * n, h.data(), hipMemcpyDeviceToHost));
    const RtFrameConsts &fc = c.key.fc;
    const int tw = c.key.tile, th = 64 / tw;
    out->tile_w = tw;
    if ((dwords || positions) && cap < 64 * n) {
        rt_set_error("rt_debug_primary_records: room for %zu records, the table has %zu", cap, 64 * n);
        return RT_ERR_INVALID;
    }
    std::vector<float4> lists;   // the view lists the launch read (a tile with a record read one)
    int nbx = 0;
    if (positions && fc.view_lists && s->view_last >= 0 && reinterpret_cast<const float *>(s->views[s->view_last].buf.get()) == fc.view_lists) {
        ViewSlot &v = s->views[s->view_last];
        RT_HIP(v.built.host_wait());
        lists.resize(rt_view_lists_size(v.nbx, v.nby));
        RT_HIP(hipMemcpy(lists.data(), v.buf.get(), sizeof(float4) * lists.size(), hipMemcpyDeviceToHost));
        nbx = v.nbx;
    }
    int il_sh = 0;
    while ((1 << il_sh) < fc.il_rows) ++il_sh;
    auto row_of = [&](int ly) { return fc.y0 + ((((ly >> il_sh) * fc.il_count + fc.il_index) << il_sh) | (ly & (fc.il_rows - 1))); };
    for (int ty = 0; ty < c.tiles_y; ++ty)
        for (int tx = 0; tx < c.tiles_x; ++tx) {
            const size_t tile = (size_t)ty * c.tiles_x + tx;
            bool valid[64], has = true, any = false;
            for (int l = 0; l < 64; ++l) {
                const int px = tx * tw + l % tw, ly = ty * th + l / tw;
                valid[l] = px < fc.width && ly < fc.local_rows && row_of(ly) < fc.y1;
                any = any || valid[l];
                if (valid[l] && (h[tile * 64 + l] & 0xffu) == RT_PRIMARY_NONE) has = false;
            }
            has = has && any;
            const int *keys = nullptr;
            if (has && !lists.empty()) {
                const int vblk = (row_of(ty * th) >> (fc.view_shift >> 8)) * nbx + ((tx * tw) >> (fc.view_shift & 255));
                keys = reinterpret_cast<const int *>(lists.data() + (size_t)vblk * RT_VIEW_SLOT + 1 + RT_VIEW_CAP);
            }
            if (has) out->tiles_recorded++;
            for (int l = 0; l < 64; ++l) {
                const unsigned e = h[tile * 64 + l] & 0xffu;
                if (has && valid[l]) (e == RT_PRIMARY_MISS ? out->miss_pixels : out->hit_pixels)++;
                if (positions) positions[tile * 64 + l] = !(has && valid[l]) ? -2 : e == RT_PRIMARY_MISS ? -1 : (keys && e < RT_VIEW_CAP) ? keys[e] : -2;
            }
        }
    if (dwords) memcpy(dwords, h.data(), sizeof(unsigned) * 64 * n);
    return RT_OK;
}

// Tests: overwrite the primary records of the table the last launch wrote or read.
extern "C" int rt_debug_set_primary_records(rt_scene *s, const unsigned *dwords, size_t n)
{
    RestSlot *c;
    const int rc = last_table_to_set(s, dwords != nullptr, "rt_debug_set_primary_records", n, 64, "records", " tiles of 64", &c);
    if (rc != RT_OK) return rc;
    RT_HIP(copy_section(*c, RT_REST_PRIMARY_OFFSET(tiles_of(*c)), sizeof(unsigned) * n, const_cast<unsigned *>(dwords), hipMemcpyHostToDevice));
    c->list_built = c->list_adopted = false;   // the run list was built from the records
    return RT_OK;
}

// The tile summaries of the last launch's table (waits for the launch that wrote it).
extern "C" int rt_debug_tile_summaries(rt_scene *s, rt_tile_summaries_info *out, unsigned *dwords, size_t cap)
{
    RestSlot *c;
    const int rc = last_table(s, out, "rt_debug_tile_summaries", &c);
    if (rc != RT_OK || !c) return rc;
    const size_t n = tiles_of(*c);
    std::vector<unsigned> h(n);
    RT_HIP(copy_section(*c, RT_REST_SUMMARY_OFFSET(n), RT_REST_SUMMARY_BYTES * n, h.data(), hipMemcpyDeviceToHost));
    for (unsigned d : h) {
        if (!(d & RT_TILE_SETTLED)) continue;
        out->settled++;
        if (d & RT_TILE_NO_MISS) out->settled_no_miss++;
    }
    if (dwords) {
        if (cap < n) {
            rt_set_error("rt_debug_tile_summaries: room for %zu tiles, the table has %zu", cap, n);
            return RT_ERR_INVALID;
        }
        memcpy(dwords, h.data(), sizeof(unsigned) * n);
    }
    return RT_OK;
}

// Tests: overwrite the tile summaries of the table the last launch wrote or read.
extern "C" int rt_debug_set_tile_summaries(rt_scene *s, const unsigned *dwords, size_t n)
{
    RestSlot *c;
    const int rc = last_table_to_set(s, dwords != nullptr, "rt_debug_set_tile_summaries", n, 1, "tiles", "", &c);
    if (rc != RT_OK) return rc;
    RT_HIP(copy_section(*c, RT_REST_SUMMARY_OFFSET(n), RT_REST_SUMMARY_BYTES * n, const_cast<unsigned *>(dwords), hipMemcpyHostToDevice));
    c->list_built = c->list_adopted = false;   // the run list was built from the summaries
    return RT_OK;
}

// The compact reading launch: the switch, R, and what the last frame launch did.
extern "C" int rt_scene_set_compact_launch(rt_scene *s, int on)
{
    if (!s || (on != 0 && on != 1)) {
        rt_set_error("rt_scene_set_compact_launch: null scene or %d not in {0, 1}", on);
        return RT_ERR_INVALID;
    }
    s->compact_mode = on;
    return RT_OK;
}

extern "C" int rt_debug_set_compact_run(rt_scene *s, int run, int ahead, int min_percent)
{
    if (!s || run < 1 || run > (int)RT_REST_LIST_RUN_MAX || (ahead != 0 && ahead != 1) || min_percent < 0 || min_percent > 100) {
        rt_set_error("rt_debug_set_compact_run: null scene, %d not in 1 ... %u, %d not in {0, 1} or %d not in 0 ... 100", run, RT_REST_LIST_RUN_MAX, ahead, min_percent);
        return RT_ERR_INVALID;
    }
    s->compact_run = (unsigned)run;
    s->compact_ahead = (unsigned)ahead;
    s->compact_min_percent = (unsigned)min_percent;
    return RT_OK;
}

extern "C" int rt_debug_compact_launch(rt_scene *s, rt_compact_launch_info *out, unsigned *list, size_t cap)
{
    if (!s || !out) {
        rt_set_error("rt_debug_compact_launch: null argument");
        return RT_ERR_INVALID;
    }
    memset(out, 0, sizeof *out);
    out->compact = s->compact_last.compact;
    out->n_unsettled = s->compact_last.n_unsettled;
    out->n_streamed = s->compact_last.n_streamed;
    out->run = s->compact_last.run;
    out->ahead = s->compact_last.ahead;
    out->workgroups = s->compact_last.workgroups;
    out->rebuilds = s->list_rebuilds;
    if (s->rest_last < 0 || !s->rest[s->rest_last].valid || !s->rest[s->rest_last].list_built) return RT_OK;
    RestSlot &c = s->rest[s->rest_last];
    RT_HIP(c.list_done.host_wait());
    out->list_built = 1;
    out->tiles_x = c.tiles_x;
    out->tiles_y = c.tiles_y;
    out->list_n_unsettled = c.list_counts.get()[0];
    out->list_n_streamed = c.list_counts.get()[1];
    if (list) {
        const size_t n = tiles_of(c);
        if (cap < n) {
            rt_set_error("rt_debug_compact_launch: room for %zu tiles, the list has %zu", cap, n);
            return RT_ERR_INVALID;
        }
        RT_HIP(copy_section(c, RT_REST_LIST_OFFSET(n) + 4u * RT_REST_LIST_HEADER, sizeof(unsigned) * n, list, hipMemcpyDeviceToHost));
    }
    return RT_OK;
}

// The order the last launch's run list was built from, (tile_y << 16) | tile_x per place: the tile order's perm[] at that
// build, or grid order where the launch had none. Waits for the list's build. (Tests: the list must be a stable
// partition of exactly this.)
extern "C" int rt_debug_compact_order(rt_scene *s, unsigned *order, size_t cap)
{
    if (!s || !order || s->rest_last < 0 || !s->rest[s->rest_last].valid || !s->rest[s->rest_last].list_built) {
        rt_set_error("rt_debug_compact_order: null argument, or the last launch's table has no run list");
        return RT_ERR_INVALID;
    }
    RestSlot &c = s->rest[s->rest_last];
    const size_t n = tiles_of(c);
    if (cap < n) {
        rt_set_error("rt_debug_compact_order: room for %zu tiles, the order has %zu", cap, n);
        return RT_ERR_INVALID;
    }
    const int rc = rt_scene_quiesce(s);   // (no sort under way)
    if (rc != RT_OK) return rc;
    RT_HIP(c.list_done.host_wait());
    if (c.list_perm) RT_HIP(hipMemcpy(order, c.list_perm, sizeof(unsigned) * n, hipMemcpyDeviceToHost));
    else
        for (size_t i = 0; i < n; ++i) order[i] = (unsigned)((i / (size_t)c.tiles_x) << 16) | (unsigned)(i % (size_t)c.tiles_x);
    return RT_OK;
}
