// gs_api.hip -- the part of libgsrast.so's C ABI (include/gs_rasterizer.h) that knows a Frame: context, device arena, frame
// pool, the counter hand-over and the forward / backward orchestration that replaces _module_function.forward / .backward
// of the reference (RAST:830-1163), and the calls bound to a frame (gs_channels_*, gs_touched_rows, gs_frame_*).  The entry
// points that hold no frame are gs_api_calls.hip's; what both share is gs_host.h.
#include "../../include/gs_channels.h"
#include "../../include/gs_sparse.h"
#include "../../include/gs_view_hints.h"
#include "gs_host.h"
#include "gs_sort_key.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <cstdlib>

thread_local std::string g_last_error;

// What RAST:998-1019 saves for backward, in this library's layouts (DESIGN.md "HBM layout").
struct FrameBufs {
    DevBuf mask, ids, cam_index, rec, box, ntiles, depth_codes, offsets, keys_a, keys_b, vals_a, vals_b, tile_start, pose, tile_order, cuts, cut_mag;
    void release(int64_t* total)
    {
        DevBuf* all[] = { &mask, &ids, &cam_index, &rec, &box, &ntiles, &depth_codes, &offsets, &keys_a, &keys_b, &vals_a, &vals_b,
                          &tile_start, &pose, &tile_order, &cuts, &cut_mag };
        for (DevBuf* b : all) b->release(total);
    }
};

// A frame as the library sees it.  Callers hold an opaque ticket (index + generation, encoded in the gs_frame* value)
// that is resolved under the ctx mutex on every use, so a released, recycled or foreign handle is an error, never a
// dereference of freed memory.
struct Frame {
    FrameBufs bufs;                     // kept (grow-only) when the slot is recycled
    gs_frame_info info{};
    int depth_bits = 0;
    void* keys_sorted = nullptr;
    int key_bytes = 4;                  // element of the key arrays: 2, 4 or 8 (gs_sort_key.h)
    int32_t* vals_sorted = nullptr;
    bool live = false;
    int cut_cap = 0;                    // list-cut records the forward of this frame could claim (0: it wrote none)
    int bwd_reference_order = 0;        // gs_config.bwd_reference_order of the forward that made the frame (gs_backward_projected has no config)
    int n_objects = 0;                  // pose rows of the forward that made the frame (the backward's pose gradient has as many)
    bool rgb_only = false;              // gs_forward ran with gs_config.rgb_only: no `last` exists for the frame (gs_channels_* refuse it)
    bool max_tiles_known = false;       // k_project of this frame left the largest tile count of one point in the tile arrays (frames from records: no)
    // the view table (gs_common.h) as this frame's forward found it: the layout it belongs to (0: none), and whether k_filter left the
    // frame's read and write slot behind the tile order (frames from records, or of an empty scene: no)
    uint32_t view_epoch = 0;
    bool view_keyed = false;
    uint32_t generation = 0;
    uint64_t bwd_serial = 0;            // gs_ctx::bwd_serial of the last backward blend on this frame (0: none has run)
    // gs_project_shard_begin: the hand-over of M (and the object-id check) has not been read yet; slot of the pinned counters
    // the frame's publish kernel writes, its ticket and the stream to fall back on
    int pending_slot = -1;
    int32_t pending_ticket = 0;
    hipStream_t pending_stream = nullptr;
};

int gs_prof_begin(GsProf* p, int kid, hipStream_t s)
{
    if (!p || !((p->mask >> kid) & 1ull)) return -1;
    GsProf::Rec r; r.kid = kid;
    hipEvent_t* ev[2] = { &r.a, &r.b };
    for (hipEvent_t* e : ev) {
        if (!p->spare.empty()) { *e = p->spare.back(); p->spare.pop_back(); }
        else if (hipEventCreate(e) != hipSuccess) return -1;
    }
    (void)hipEventRecord(r.a, s);
    p->recs.push_back(r);
    return (int)p->recs.size() - 1;
}

void gs_prof_end(GsProf* p, int rec, hipStream_t s)
{
    if (!p || rec < 0) return;
    (void)hipEventRecord(p->recs[rec].b, s);
}

extern "C" int gs_abi_version(void) { return GS_ABI_VERSION; }
extern "C" const char* gs_last_error(void) { return g_last_error.c_str(); }

extern "C" const char* gs_kernel_names(void)
{
    return "k_filter,k_scan_tiles_publish,k_project,k_keygen,k_sort_hist,"
           "k_sort_rowscan,k_sort_scatter,k_blend_fwd,k_blend_bwd_tile,k_bwd_points,k_sum_rows,k_tile_order,k_blend_bwd_repair";
}

extern "C" int gs_create(int32_t device, gs_ctx** out)
{
    if (!out) return fail(GS_ERR_INVALID_ARGUMENT, "gs_create: out is NULL");
    int count = 0;
    HIP_TRY(hipGetDeviceCount(&count));
    if (device < 0 || device >= count) return fail(GS_ERR_INVALID_ARGUMENT, "gs_create: no such HIP device");
    HIP_TRY(hipSetDevice(device));
    gs_ctx* c = new gs_ctx();
    c->device = device;
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&c->host_counters), sizeof(GsCounters) * GS_COUNTER_SLOTS, hipHostMallocMapped | hipHostMallocCoherent);
    if (e != hipSuccess) { delete c; return fail(GS_ERR_HIP, std::string("hipHostMalloc: ") + hipGetErrorString(e)); }
    std::memset(c->host_counters, 0, sizeof(GsCounters) * GS_COUNTER_SLOTS);
    e = hipHostGetDevicePointer(reinterpret_cast<void**>(&c->host_counters_dev), c->host_counters, 0);
    if (e != hipSuccess) { (void)hipHostFree(c->host_counters); delete c; return fail(GS_ERR_HIP, std::string("hipHostGetDevicePointer: ") + hipGetErrorString(e)); }
    e = c->counters.ensure(sizeof(GsCounters), &c->device_bytes);
    if (e == hipSuccess) e = hipMemset(c->counters.p, 0, sizeof(GsCounters));      // every later frame leaves them reset (gs_publish_counters)
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->switch_event, hipEventDisableTiming);
    if (e != hipSuccess) { c->counters.release(&c->device_bytes); (void)hipHostFree(c->host_counters); delete c; return fail(GS_ERR_OUT_OF_MEMORY, "gs_create: counters"); }
    *out = c;
    return GS_OK;
}

extern "C" int gs_destroy(gs_ctx* c)
{
    if (!c) return GS_OK;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    for (Frame* f : c->frames) { f->bufs.release(&c->device_bytes); delete f; }
    DevBuf* all[] = { &c->block_counts, &c->block_offsets, &c->tile_block_sums, &c->hist, &c->scan_tmp, &c->first_hist,
                      &c->counters, &c->partial, &c->visited, &c->zero_row, &c->sums, &c->loss_ws, &c->view_table, &c->pose_scratch,
                      &c->ch_partial, &c->ch_flags, &c->row_block_totals, &c->merge_tags, &c->merge_ids,
                      &c->knn_sort, &c->knn_hist, &c->knn_points, &c->knn_tree, &c->mix_records, &c->mix_sums, &c->mix_partial,
                      &c->mixg_queries, &c->mixg_partial, &c->mixg_sums, &c->mixg_x_partial, &c->mcmc_ws, &c->appearance_ws, &c->bilateral_ws, &c->depth_ws,
                      &c->geometry_ws, &c->background_ws, &c->filter3d_ws };
    for (DevBuf* b : all) b->release(&c->device_bytes);
    for (ResampleTable* rt : c->resample_tables) { rt->buf.release(&c->device_bytes); delete rt; }
    for (GsProf::Rec& r : c->prof.recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (hipEvent_t e : c->prof.spare) (void)hipEventDestroy(e);
    if (c->switch_event) (void)hipEventDestroy(c->switch_event);
    if (c->host_counters) (void)hipHostFree(c->host_counters);
    delete c;
    return GS_OK;
}

extern "C" int gs_profile_enable(gs_ctx* c, uint64_t kernel_mask)
{
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, "gs_profile_enable: ctx is NULL");
    std::lock_guard<std::mutex> lock(c->mu);
    c->prof.mask = kernel_mask;
    return GS_OK;
}

extern "C" int gs_profile_read(gs_ctx* c, double* total_ms, int64_t* launches, int32_t n, int32_t reset)
{
    if (!c || !total_ms || !launches) return fail(GS_ERR_INVALID_ARGUMENT, "gs_profile_read: NULL argument");
    std::lock_guard<std::mutex> lock(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    GsProf& p = c->prof;
    for (GsProf::Rec& r : p.recs) {
        HIP_TRY(hipEventSynchronize(r.b));
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, r.a, r.b));
        p.total_ms[r.kid] += ms; p.launches[r.kid] += 1;
        p.spare.push_back(r.a); p.spare.push_back(r.b);
    }
    p.recs.clear();
    for (int i = 0; i < n && i < KID_COUNT_; ++i) { total_ms[i] = p.total_ms[i]; launches[i] = p.launches[i]; }
    if (reset) for (int i = 0; i < KID_COUNT_; ++i) { p.total_ms[i] = 0.0; p.launches[i] = 0; }
    return GS_OK;
}

extern "C" int64_t gs_ctx_device_bytes(const gs_ctx* c) { return c ? c->device_bytes : 0; }
extern "C" int64_t gs_ctx_counter_wait_ns(const gs_ctx* c) { return c ? c->counter_wait_ns : 0; }
// ---- frame tickets ------------------------------------------------------------------------------------------------
static gs_frame* ticket_of(int slot, uint32_t generation)
{
    return reinterpret_cast<gs_frame*>((uintptr_t)(((uint64_t)generation << 32) | (uint64_t)(uint32_t)(slot + 1)));
}

// resolves a ticket (mutex held); nullptr for anything that is not a live frame of THIS ctx
static Frame* resolve(gs_ctx* c, const gs_frame* h)
{
    const uint64_t v = (uint64_t)(uintptr_t)h;
    const uint32_t lo = (uint32_t)v, gen = (uint32_t)(v >> 32);
    if (lo == 0 || lo > c->frames.size()) return nullptr;
    Frame* f = c->frames[lo - 1];
    if (!f->live || f->generation != gen) return nullptr;
    return f;
}

static Frame* acquire_frame(gs_ctx* c, int* slot)
{
    for (size_t i = 0; i < c->frames.size(); ++i)
        if (!c->frames[i]->live) { Frame* f = c->frames[i]; f->live = true; f->generation += 1; if (f->generation == 0) f->generation = 1; *slot = (int)i; return f; }
    Frame* f = new Frame();
    f->live = true; f->generation = 1;
    c->frames.push_back(f);
    *slot = (int)c->frames.size() - 1;
    return f;
}

static void drop_frame(gs_ctx* c, Frame* f)
{
    if (!f || !f->live) return;
    if (f->pending_slot > 0) c->slots_busy &= ~(1ull << f->pending_slot);      // a late write into a freed slot is harmless: tickets are unique
    f->pending_slot = -1;
    f->live = false;
    for (size_t i = 0; i < c->frames.size(); ++i) if (c->frames[i] == f && c->transient == (int)i) c->transient = -1;
}

// The frame of a forward-type call (mutex held, stream entered); the transient frame of the last keep == 0 call goes first.
// Whoever begins a frame drops it again if one of its stages fails.
static Frame* begin_frame(gs_ctx* c, const gs_camera* cam, int T, int keep, int* slot)
{
    if (c->transient >= 0) drop_frame(c, c->frames[c->transient]);
    Frame* f = acquire_frame(c, slot);
    f->info = gs_frame_info{};
    f->bwd_serial = 0;
    f->view_epoch = 0; f->view_keyed = false;
    // (known before the stages run: a kept frame gets list cuts for its backward, and the tile count lays out the tile arrays)
    f->info.kept_for_backward = keep ? 1 : 0;
    f->info.n_tiles = T; f->info.camera_height = cam->camera_height; f->info.camera_width = cam->camera_width;
    return f;
}

static void finish_frame(gs_ctx* c, Frame* f, int slot, int64_t N, int M, uint32_t K, int stages, gs_frame** frame_out)
{
    f->info.n_points = N; f->info.n_points_in_camera = M; f->info.n_keys = K;
    f->info.stages = stages;
    if (!f->info.kept_for_backward) c->transient = slot;
    *frame_out = ticket_of(slot, f->generation);
}

// The one description of a frame's device buffers.  Records: one 64-byte row per point.  Tile arrays (GS_TILE_INTS):
// tile_start | tile_end | tile_work | tile_cut (T each) | spare, max tiles, two spare.  Tile order (GS_ORDER_INTS):
// order (T) | n_heavy | n_items | pad pad | item_base.
static GsFrameView frame_view(const Frame& f)
{
    const FrameBufs& B = f.bufs;
    const int T = f.info.n_tiles;
    GsFrameView v{};
    float4* rec = B.rec.as<float4>();
    v.PA = rec; v.PB = rec + 1; v.PC = rec + 2; v.PD = rec + 3;
    v.box = B.box.as<ushort4>(); v.ntiles = B.ntiles.as<int32_t>(); v.depth_codes = B.depth_codes.as<int32_t>(); v.offsets = B.offsets.as<uint32_t>();
    v.ids = B.ids.as<int32_t>(); v.cam_index = B.cam_index.as<int32_t>(); v.mask = B.mask.as<int8_t>(); v.pose = B.pose.as<GsPose>();
    v.T = T;
    int32_t* tiles = B.tile_start.as<int32_t>();
    v.tile_start = tiles; v.tile_end = tiles + T; v.tile_work = tiles + 2 * (size_t)T; v.tile_cut = tiles + 3 * (size_t)T;
    v.max_tiles = tiles + GS_TILE_INTS(T) - GS_TILE_SPARE_MAX_TILES;
    v.tile_ints = (int)GS_TILE_INTS(T);
    v.tile_order = B.tile_order.as<int32_t>(); v.n_heavy = v.tile_order + T;
    v.keys_sorted = f.keys_sorted; v.vals_sorted = f.vals_sorted;
    v.cuts = f.cut_cap > 0 ? B.cuts.as<float4>() : nullptr; v.cut_mag = B.cut_mag.as<float2>();
    return v;
}

static int waves_per_tile(int n_tiles);
static int bits_for(uint32_t v) { int b = 0; while (v) { ++b; v >>= 1; } return b < 1 ? 1 : b; }

// ---- the counter hand-over ------------------------------------------------------------------------------------------
// The one device->host hand-over of a frame: M, K, the depth-code range (and the bad-object-id count).  The last
// prologue kernel writes them into pinned host memory and then the ticket; spinning on it costs a few microseconds
// where a copy + stream synchronisation left the GPU idle for ~30.  Waits for `ticket` in counter slot `slot`.
static int read_counters(gs_ctx* c, hipStream_t s, int32_t ticket, int slot, GsCounters* out)
{
    volatile GsCounters* hc = c->host_counters + slot;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spin = 0; hc->reserved != ticket; ++spin) {
        if ((spin & 0xfffu) == 0xfffu) {
            const hipError_t q = hipStreamQuery(s);
            if (q == hipSuccess) {                         // stream drained: the ticket must be there now
                if (hc->reserved != ticket) return fail(GS_ERR_HIP, "frame counters were not published");
                break;
            }
            if (q != hipErrorNotReady) return fail(GS_ERR_HIP, std::string("waiting for the frame counters: ") + hipGetErrorString(q));
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(30))
                return fail(GS_ERR_HIP, "timed out waiting for the frame counters");
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    c->counter_wait_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    *out = c->host_counters[slot];
    if (out->bad_object_ids != 0)
        return fail(GS_ERR_INVALID_ARGUMENT, "point_object_id holds " + std::to_string(out->bad_object_ids) +
                                             " value(s) outside [0, n_objects) on valid rows");
    return GS_OK;
}

// Reads the hand-over of a frame begun with gs_project_shard_begin (mutex held): M, K and the object-id verdict.  A frame
// whose read fails is dropped.
static int resolve_pending(gs_ctx* c, Frame* f)
{
    if (f->pending_slot <= 0) return GS_OK;
    HIP_TRY(hipSetDevice(c->device));
    GsCounters hc;
    const int rc = read_counters(c, f->pending_stream, f->pending_ticket, f->pending_slot, &hc);
    if (rc != GS_OK) { drop_frame(c, f); return rc; }          // (which frees the frame's counter slot)
    c->slots_busy &= ~(1ull << f->pending_slot);
    f->pending_slot = -1;
    f->info.n_points_in_camera = hc.M;
    f->info.n_keys = hc.K;
    return GS_OK;
}

// The live frame of this ctx that handle h names (mutex held); with `pending`, its deferred hand-over is read first.
static int lookup(gs_ctx* c, const gs_frame* h, const char* who, bool pending, Frame** out)
{
    Frame* f = resolve(c, h);
    if (!f) return fail(GS_ERR_STATE, who, "not a live frame of this context");
    if (pending)
        if (const int rc = resolve_pending(c, f)) return rc;
    *out = f;
    return GS_OK;
}

static int check_geometry(const gs_camera* cam, const gs_config* cfg, const char* who, int* tiles_x, int* tiles_y)
{
    const int H = cam->camera_height, W = cam->camera_width;
    if (W <= 0 || H <= 0 || (!cfg->allow_partial_tiles && (W % GS_TILE != 0 || H % GS_TILE != 0)))        // RAST:1193-1194
        return fail(GS_ERR_INVALID_ARGUMENT, who, "camera_width and camera_height must be positive multiples of 16 "
                                             "(or set gs_config.allow_partial_tiles)");
    *tiles_x = (W + GS_TILE - 1) / GS_TILE; *tiles_y = (H + GS_TILE - 1) / GS_TILE;
    if (*tiles_x > 65535 || *tiles_y > 65535) return fail(GS_ERR_INVALID_ARGUMENT, who, "image too large");
    return GS_OK;
}

static int check_scene(const gs_scene* sc, const gs_camera* cam, const char* who)
{
    const int64_t N = sc->n_points;
    if (N < 0 || N >= (int64_t)1 << 31) return fail(GS_ERR_INVALID_ARGUMENT, who, "n_points out of range");
    if (cam->n_objects <= 0) return fail(GS_ERR_INVALID_ARGUMENT, who, "n_objects must be >= 1");
    if (N > 0 && (!sc->point_cloud || !sc->point_cloud_features || !sc->point_invalid_mask || !sc->point_object_id))
        return fail(GS_ERR_INVALID_ARGUMENT, who, "NULL scene array");
    if (!cam->q_pointcloud_camera || !cam->t_pointcloud_camera || !cam->camera_intrinsics)
        return fail(GS_ERR_INVALID_ARGUMENT, who, "NULL camera array");
    if (((uintptr_t)sc->point_cloud_features & 15u) != 0)
        return fail(GS_ERR_INVALID_ARGUMENT, who, "point_cloud_features must be 16-byte aligned");
    return GS_OK;
}

static int check_forward_out(const gs_forward_out* out, const gs_config* cfg, int keep, const char* who)
{
    if (!out->rasterized_image) return fail(GS_ERR_INVALID_ARGUMENT, who, "rasterized_image is NULL");
    if (!cfg->rgb_only && (!out->rasterized_depth || !out->pixel_accumulated_alpha ||
                           !out->pixel_offset_of_last_effective_point || !out->pixel_valid_point_count))
        return fail(GS_ERR_INVALID_ARGUMENT, who, "an output is NULL although rgb_only is false");
    if (keep && cfg->rgb_only) return fail(GS_ERR_INVALID_ARGUMENT, who, "rgb_only frames cannot be kept for backward (RAST:478-484)");
    return GS_OK;
}

// The sort's first radix pass inside k_keygen (k_binning.hip), for a per-point stage over `rows` rows: the default up to
// GS_FIRST_PASS_MAX_BLOCKS blocks of 256 rows.  Measured on both sides of the cap (profiles/sort_first_pass_ab.json):
// at 1954 blocks (cfg3_headline, 12.9 pairs per point) the pass saves 30 us of a 640 us step; at 7813 blocks (cfg5_infer2e6, two
// million small splats, 3 to 4 pairs per point, a 16 MB table) k_keygen's short runs, k_project's strided stores and the longer row
// scan cost what the pass saves, and the frame lost 4.7 fps at a parent spread of 3.4: above the cap the three-kernel pass runs.
// Nothing was measured between the two sizes; the cap is the power of two between them.  GS_SORT_FIRST_PASS=0 keeps the three-kernel
// pass everywhere; read on every call, so that one process can compare both.  The table (2 KB per 256 rows) is written whether or
// not the frame's keys turn out to have the 8 depth bits the pass needs (the width is known only afterwards).
#define GS_FIRST_PASS_MAX_BLOCKS 4096
static bool sort_first_pass_enabled(int64_t rows)
{
    if ((rows + 255) / 256 > GS_FIRST_PASS_MAX_BLOCKS) return false;
    const char* e = getenv("GS_SORT_FIRST_PASS");
    return !(e && e[0] == '0');
}

// The narrow key class (gs_sort_key.h: 16-bit keys without the byte k_keygen's first pass has placed), GS_SORT_NARROW_KEYS, read on
// every call like GS_SORT_FIRST_PASS: 0 keeps the 32-bit layout everywhere, 1 takes the narrow one where a frame can, "require"
// does the same and makes a forward whose frame ended up in another class fail with GS_ERR_STATE (tests prove with it which path ran).
#define GS_NARROW_KEYS_DEFAULT 1
enum NarrowKeys { NARROW_OFF, NARROW_ON, NARROW_REQUIRED };
static NarrowKeys sort_narrow_keys()
{
    const char* e = getenv("GS_SORT_NARROW_KEYS");
    if (!e || !e[0]) return GS_NARROW_KEYS_DEFAULT ? NARROW_ON : NARROW_OFF;
    if (e[0] == '0') return NARROW_OFF;
    return strcmp(e, "require") == 0 ? NARROW_REQUIRED : NARROW_ON;
}
static int check_required_key_class(const Frame* f)
{
    if (sort_narrow_keys() == NARROW_REQUIRED && f->key_bytes != 2)
        return fail(GS_ERR_STATE, "GS_SORT_NARROW_KEYS=require: the frame's sort keys are " + std::to_string(f->key_bytes) + " bytes wide");
    return GS_OK;
}

// ---- the view table (gs_common.h): per-view dispatch orders of the forward blend ---------------------------------------------
// GS_VIEW_HINTS, read on every call like GS_SORT_NARROW_KEYS: the number of slots at every image size, at most GS_VIEW_MAX_SLOTS; 1 = one
// slot that every pose matches (the last backward's order, whatever its view; no frame looks its pose up); 0 = no hint.  Unset:
// GS_VIEW_SLOTS_DEFAULT (64 views: 2 MB of orders at 8160 tiles) from GS_VIEW_MIN_TILES tiles on, one slot below.  An order can only
// help a launch of more workgroups than the chip holds at once (k_blend_fwd: 8 workgroups on each of 256 CUs = 2048), and below that the
// lookup is pure cost: measured at 8160 tiles (cfg3_headline: k_blend_fwd 0.144 -> 0.135 ms) and at 2074 (cfg2_clustered: k_blend_fwd
// unchanged, k_filter, whose 899 blocks are all resident so that block 0's chain is the kernel's, 0.0074 -> 0.0085 ms, the step 0.2 to
// 0.7 % slower).  Nothing was measured between the two sizes; the threshold is the power of two between them, twice the resident slots.
#define GS_VIEW_SLOTS_DEFAULT 64
#define GS_VIEW_MIN_TILES 4096
static int view_slots_wanted(int T)
{
    const char* e = getenv("GS_VIEW_HINTS");
    if (!e || !e[0]) return T >= GS_VIEW_MIN_TILES ? GS_VIEW_SLOTS_DEFAULT : 1;
    const long n = strtol(e, nullptr, 10);
    return n < 0 ? 0 : (n > GS_VIEW_MAX_SLOTS ? GS_VIEW_MAX_SLOTS : (int)n);
}
// The table as a forward over T tiles uses it (mutex held, stream entered): laid out again, and emptied, when the tile count or the slot
// count is not the table's -- frames of the old layout still in flight then leave it alone (backward_views).  base NULL: none.
static int view_table(gs_ctx* c, int T, hipStream_t s, GsViewTable* out)
{
    *out = GsViewTable{ nullptr, 0, 0 };
    const int S = view_slots_wanted(T);
    if (S == 0 || T <= 0) return GS_OK;
    if (c->view_T != T || c->view_S != S) {
        c->view_T = 0; c->view_S = 0;
        if (const int rc = grow(c, "forward", { NEED(c->view_table, 4 * GS_VIEW_INTS(S, T)) })) return rc;
        HIP_TRY(hipMemsetAsync(c->view_table.p, 0, 4 * (size_t)(GS_VIEW_HDR_INTS + GS_VIEW_KEY_INTS * S), s));     // cursor, last slot, every key's tag
        c->view_T = T; c->view_S = S; c->view_epoch += 1;
    }
    *out = GsViewTable{ c->view_table.as<int32_t>(), S, T };
    return GS_OK;
}
// The table as the backward of frame f writes it: the layout the frame's forward saw, or none.
static GsViewTable backward_views(const gs_ctx* c, const Frame* f)
{
    if (f->view_epoch == 0 || f->view_epoch != c->view_epoch || c->view_T != f->info.n_tiles) return GsViewTable{ nullptr, 0, 0 };
    return GsViewTable{ c->view_table.as<int32_t>(), c->view_S, c->view_T };
}

// ---- per-point half: filter, compaction, projection (+ tile counts, scan, publication) ----------------------------
// On success the frame's buffers hold mask / ids / cam_index / records / box / ntiles.  The counters (M, K, depth-code range,
// bad object ids) are handed over through pinned memory; `wait` says when the host reads them:
//   WAIT_NOW    before this function returns (M and K are filled in);
//   WAIT_LATER  the caller reads slot 0 itself (read_counters) after it has queued more work -- nothing else may publish before;
//   WAIT_FRAME  the frame keeps a slot of its own and whoever needs M first reads it (resolve_pending, gs_project_shard_begin).
enum CounterWait { WAIT_NOW, WAIT_LATER, WAIT_FRAME };

static int run_project_stage(gs_ctx* c, Frame* f, const gs_scene* sc, const gs_camera* cam, const gs_config* cfg, hipStream_t s,
                             CounterWait wait, GsProjectArgs* pa_out, int* M_out, uint32_t* K_out)
{
    FrameBufs& B = f->bufs;
    const int64_t N = sc->n_points;
    const int T = f->info.n_tiles;
    const size_t nb = (size_t)((N + 255) / 256);
    const size_t Np = (size_t)(N > 0 ? N : 1);
    int rc = grow(c, "forward", { NEED(B.mask, Np), NEED(B.ids, 4 * Np), NEED(B.cam_index, 4 * Np),
                       NEED(B.rec, 64 * Np),
                       NEED(B.box, 8 * Np), NEED(B.ntiles, 4 * Np), NEED(B.depth_codes, 4 * Np), NEED(B.offsets, 4 * Np),
                       NEED(B.tile_start, 4 * GS_TILE_INTS(T)),    // tile_start | tile_end | tile_work | tile_cut | four ints, cleared together
                       NEED(B.tile_order, 4 * GS_ORDER_INTS(T)),   // + heavy-tile count, item count and item bases behind the order
                       NEED(B.pose, sizeof(GsPose) * (size_t)cam->n_objects),
                       NEED(c->block_counts, 4 * (nb + 1)), NEED(c->block_offsets, 4 * (nb + 1)),
                       NEED(c->tile_block_sums, 4 * (nb + 1)) });
    if (rc != GS_OK) return rc;
    // the digit table only for a call that goes on to bin these points (gs_forward, the one caller that waits later): the shard entry
    // points hand records out, and whoever renders them has k_boxes_from_records build the table over ITS blocks
    const bool first_pass = wait == WAIT_LATER && sort_first_pass_enabled(N);
    if (first_pass && (rc = grow(c, "forward", { NEED(c->first_hist, 4 * gs_first_hist_elems(N)) })) != GS_OK) return rc;
    f->n_objects = cam->n_objects;

    GsProjectArgs pa{};
    pa.prof = &c->prof;
    pa.point_cloud = sc->point_cloud; pa.features = sc->point_cloud_features; pa.invalid = sc->point_invalid_mask;
    pa.object_id = sc->point_object_id; pa.N = N; pa.q_pc = cam->q_pointcloud_camera; pa.t_pc = cam->t_pointcloud_camera;
    pa.n_objects = cam->n_objects; pa.Kmat = cam->camera_intrinsics; pa.H = cam->camera_height; pa.W = cam->camera_width;
    pa.near_plane = cfg->near_plane; pa.far_plane = cfg->far_plane; pa.depth_scale = cfg->depth_to_sort_key_scale;
    pa.v = frame_view(*f);
    pa.block_counts = c->block_counts.as<int32_t>(); pa.block_offsets = c->block_offsets.as<int32_t>();
    pa.tile_block_sums = c->tile_block_sums.as<uint32_t>();
    pa.first_hist = first_pass ? c->first_hist.as<uint32_t>() : nullptr;
    pa.counters = c->counters.as<GsCounters>();
    int slot = 0;
    if (wait == WAIT_FRAME && N > 0) {
        const uint64_t free_slots = ~c->slots_busy;
        if (free_slots != 0ull) { slot = __builtin_ctzll(free_slots); c->slots_busy |= 1ull << slot; }     // none left: wait at once
    }
    pa.host_mirror = c->host_counters_dev + slot; pa.ticket = ++c->ticket;
    if (c->ticket == 0x7fffffff) c->ticket = 0;
    // only a frame that goes on to its own blend looks its pose up (the shard entry points hand records out: no blend, no tile order)
    if (wait == WAIT_LATER && N > 0) {
        if ((rc = view_table(c, T, s, &pa.views)) != GS_OK) return rc;
        if (pa.views.S < 2) pa.views = GsViewTable{ nullptr, 0, 0 };      // one slot: nothing to look up
        f->view_keyed = pa.views.base != nullptr;
    }
    gs_launch_project(pa, s, wait != WAIT_LATER);      // WAIT_LATER: the caller decides who publishes the counters (run_forward_tail)
    f->max_tiles_known = true;
    HIP_TRY(hipGetLastError());
    *pa_out = pa;
    *M_out = 0; *K_out = 0u;
    if (slot > 0) {
        f->pending_slot = slot; f->pending_ticket = pa.ticket; f->pending_stream = s;
        return GS_OK;
    }
    if (N > 0 && wait != WAIT_LATER) {
        GsCounters hc;
        if ((rc = read_counters(c, s, pa.ticket, 0, &hc)) != GS_OK) return rc;
        *M_out = hc.M; *K_out = hc.K;
    }
    return GS_OK;
}

// The per-point half of gs_forward_projected: the records arrive from elsewhere; the frame keeps its own copy for backward,
// and tile boxes, counts and depth codes are recomputed from them.  The counters are published from run_forward_tail.
static int run_records_stage(gs_ctx* c, Frame* f, const float* records, int64_t m, const gs_config* cfg, hipStream_t s,
                             GsProjectArgs* pa_out)
{
    FrameBufs& B = f->bufs;
    const int T = f->info.n_tiles;
    const size_t Mp = (size_t)(m > 0 ? m : 1);
    const size_t nb = (size_t)((m + 255) / 256);
    const int rc = grow(c, "forward", { NEED(B.rec, 64 * Mp), NEED(B.box, 8 * Mp), NEED(B.ntiles, 4 * Mp), NEED(B.depth_codes, 4 * Mp), NEED(B.offsets, 4 * Mp),
                             NEED(B.tile_start, 4 * GS_TILE_INTS(T)), NEED(B.tile_order, 4 * GS_ORDER_INTS(T)),
                             NEED(c->tile_block_sums, 4 * (nb + 1)) });
    if (rc != GS_OK) return rc;
    const bool first_pass = sort_first_pass_enabled(m);
    if (first_pass) if (const int rc2 = grow(c, "forward", { NEED(c->first_hist, 4 * gs_first_hist_elems(m)) })) return rc2;
    if (m > 0) HIP_TRY(hipMemcpyAsync(B.rec.p, records, (size_t)m * 64, hipMemcpyDeviceToDevice, s));
    GsProjectArgs pa{};
    pa.prof = &c->prof; pa.N = m; pa.H = f->info.camera_height; pa.W = f->info.camera_width; pa.depth_scale = cfg->depth_to_sort_key_scale;
    pa.v = frame_view(*f);
    pa.tile_block_sums = c->tile_block_sums.as<uint32_t>();
    pa.first_hist = first_pass ? c->first_hist.as<uint32_t>() : nullptr;
    pa.counters = c->counters.as<GsCounters>();
    pa.host_mirror = c->host_counters_dev; pa.ticket = ++c->ticket;
    if (c->ticket == 0x7fffffff) c->ticket = 0;
    gs_launch_boxes_from_records(pa, (int)m, s, false);
    f->max_tiles_known = false;
    HIP_TRY(hipGetLastError());
    *pa_out = pa;
    return GS_OK;
}

// ---- per-pixel half: key build, sort, tile ranges, blend ----------------------------------------------------------
// K_bound: pair capacity the buffers and the launch geometry are sized for; depth_bits: width of the depth field of the keys.
// Both may be PREDICTIONS (run_forward_tail): the kernels take the frame's real pair count from the device counters and stay
// inside K_bound whatever it is, and any depth_bits >= the real width sorts into the same order.
static int run_raster_stage(gs_ctx* c, Frame* f, const GsProjectArgs& pa, int64_t n_rows, int M_bound, uint32_t K_bound, int depth_bits,
                            const gs_config* cfg, const gs_forward_out* out, hipStream_t s, bool publish)
{
    FrameBufs& B = f->bufs;
    const int T = f->info.n_tiles, H = f->info.camera_height, W = f->info.camera_width, tiles_x = (W + GS_TILE - 1) / GS_TILE;
    // list cuts for the backward's heavy tiles (k_blend_fwd): only a frame that will be back-propagated wants them.
    // Policy (measured): segments pay where the ordinary waves do not fill the chip anyway (T * G waves for 5120
    // slots: cfg2_clustered 0.38 -> 0.22 ms) and cost where they do (cfg3_clustered 0.31 -> 0.34 ms: more, shorter work items in a
    // launch that was already full).  GS_BWD_SEGMENTS=0 / 1 forces never / always.
    static const int seg_env = []{ const char* e = getenv("GS_BWD_SEGMENTS"); return e ? (e[0] == '0' ? 0 : 1) : -1; }();
    const bool want_cuts = seg_env >= 0 ? seg_env == 1 : (int64_t)T * waves_per_tile(T) < 6144;
    int cut_cap = 0;
    if (want_cuts && f->info.kept_for_backward && !cfg->rgb_only && K_bound > 0) {
        // every long list has its records at start / GS_SEG + tile (k_blend_fwd.hip): K / GS_SEG + T + 1 of them hold all lists'.  (Nothing
        // is claimed at run time: a capacity that could run out would make WHICH lists get cuts, and with it the last bits of the
        // gradients, depend on the order of the claims.)
        cut_cap = (int)std::min<uint64_t>((uint64_t)K_bound / GS_SEG + (uint64_t)T + 2, 0x7fffffffu);
        if (const int rc = grow(c, "forward", { NEED(B.cuts, (size_t)cut_cap * 256 * sizeof(float4)), NEED(B.cut_mag, (size_t)cut_cap * 256 * sizeof(float2)) }))
            return rc;
    }
    f->cut_cap = cut_cap;
    const int tile_bits = bits_for((uint32_t)(T > 1 ? T - 1 : 1));
    // the key class: compact 32-bit keys whenever they fit, 16-bit ones behind k_keygen's first pass when the other digits fit
    uint32_t* const first_hist = depth_bits >= 8 ? pa.first_hist : nullptr;    // below 8 depth bits digit 0 holds tile bits: the full-pass loop
    const int key_bytes = gs_key_bytes(depth_bits + tile_bits, depth_bits, first_hist != nullptr, sort_narrow_keys() != NARROW_OFF);
    if (depth_bits + tile_bits > 63) return fail(GS_ERR_INVALID_ARGUMENT, "sort key needs more than 63 bits");
    const size_t Kp = K_bound > 0 ? K_bound : 1;
    const size_t hist_elems = gs_sort_hist_elems(K_bound);
    if (const int rc = grow(c, "forward", { NEED(B.keys_a, (size_t)key_bytes * Kp), NEED(B.keys_b, (size_t)key_bytes * Kp), NEED(B.vals_a, 4 * Kp), NEED(B.vals_b, 4 * Kp),
                                 NEED(c->hist, 4 * hist_elems), NEED(c->scan_tmp, 4 * GS_SORT_DIGITS) }))
        return rc;

    GsBinArgs ba{};
    ba.prof = &c->prof;
    ba.N = n_rows; ba.M = M_bound; ba.K = K_bound; ba.counters = c->counters.as<GsCounters>();
    ba.tiles_x = tiles_x;
    ba.depth_bits = depth_bits; ba.key_bits = depth_bits + tile_bits;
    ba.v = frame_view(*f);
    ba.tile_block_sums = pa.tile_block_sums;
    ba.counters_rw = pa.counters; ba.host_mirror = publish ? pa.host_mirror : nullptr; ba.ticket = pa.ticket;   // publish: k_keygen's last block hands the counters over
    ba.block_offsets = pa.block_offsets; ba.block_counts = pa.block_counts;     // NULL for records that did not come from k_project
    ba.keys_a = B.keys_a.p; ba.keys_b = B.keys_b.p; ba.key_bytes = key_bytes;
    ba.vals_a = B.vals_a.as<int32_t>(); ba.vals_b = B.vals_b.as<int32_t>();
    ba.hist = c->hist.as<uint32_t>(); ba.scan_tmp = c->scan_tmp.as<uint32_t>();
    ba.first_hist = first_hist;
    ba.keys_sorted = &f->keys_sorted; ba.vals_sorted = &f->vals_sorted;
    gs_launch_binning(ba, s);
    HIP_TRY(hipGetLastError());

    GsBlendFwdArgs fa{};
    fa.prof = &c->prof;
    fa.H = H; fa.W = W; fa.tiles_x = tiles_x; fa.rgb_only = cfg->rgb_only;
    fa.v = frame_view(*f);                  // (taken after the binning, which said where the sorted pairs are)
    fa.key_bytes = key_bytes; fa.depth_bits = depth_bits; fa.K = K_bound; fa.counters = ba.counters;
    fa.image = out->rasterized_image; fa.depth = out->rasterized_depth; fa.acc_alpha = out->pixel_accumulated_alpha;
    fa.last = out->pixel_offset_of_last_effective_point; fa.count = out->pixel_valid_point_count;
    fa.cut_cap = cut_cap;
    // the dispatch order: the frame's read slot of the view table where k_filter left one, otherwise whichever slot was written last
    static const bool use_hint = []{ const char* e = getenv("GS_FWD_ORDER_HINT"); return !(e && e[0] == '0'); }();
    GsViewTable views;
    if (const int rc = view_table(c, T, s, &views)) return rc;
    f->view_epoch = views.base ? c->view_epoch : 0;
    if (views.base && use_hint) {
        fa.views = views;
        fa.view_slot = f->view_keyed ? fa.v.n_heavy + GS_ORDER_READ_SLOT : views.base + 1;
        fa.view_slot_bias = f->view_keyed ? 0 : 1;
    }
    // tile ranges are all zero when K == 0, so the kernel writes the "no contributor" values itself
    gs_launch_blend_fwd(fa, s);
    HIP_TRY(hipGetLastError());
    f->depth_bits = depth_bits;
    f->key_bytes = key_bytes;
    f->info.sort_key_bits = depth_bits + tile_bits;
    return GS_OK;
}

// Everything of a forward after the per-point kernels have been QUEUED (their counters not yet read): the per-pixel half and
// the one device->host hand-over of the frame.
//
// The reference stops twice per forward to learn M and K on the host (RAST:870, 916-931).  Here the host needs them only to
// size buffers and grids, so in steady state it does not stop in the middle at all: binning, sort and blend are queued at
// once on PREDICTED sizes -- pair capacity = what the last frame of this ctx needed + 25 %, key width from the depth-code range
// + 25 % of the last frame that had a point in camera -- and the hand-over is read AFTER the last launch,
// when the GPU has the whole forward in its queue instead of nothing.  The kernels read the real pair count on the device and
// never leave the predicted capacity, so a wrong prediction is harmless: the host sees it in the counters (K beyond the
// capacity, or depth codes wider than the key field), grows the buffers and queues the per-pixel half again with the exact
// sizes before the call returns (GS_SIZING_REDONE; the caller's outputs are simply written a second time, in stream order).
// The first frame of a ctx, a new image size and GS_PREDICT_SIZES=0 take the exact path: wait, then queue (GS_SIZING_EXACT).
static int run_forward_tail(gs_ctx* c, Frame* f, const GsProjectArgs& pa, int64_t n_rows, int M_known, const gs_config* cfg,
                            const gs_forward_out* out, hipStream_t s, int* M_out, uint32_t* K_out)
{
    static const bool predict = []{ const char* e = getenv("GS_PREDICT_SIZES"); return !(e && e[0] == '0'); }();
    const int T = f->info.n_tiles, H = f->info.camera_height, W = f->info.camera_width;
    int rc;
    f->info.sizing = GS_SIZING_EXACT;
    *M_out = 0; *K_out = 0u;
    if (n_rows == 0) {                                     // nothing was published: an empty frame
        rc = run_raster_stage(c, f, pa, 0, 0, 0u, 1, cfg, out, s, false);
        return rc != GS_OK ? rc : check_required_key_class(f);
    }
    const int tile_bits = bits_for((uint32_t)(T > 1 ? T - 1 : 1));
    bool predicted = false;
    int bits_p = 0; uint32_t K_p = 0;
    if (predict && c->seen.valid && c->seen.H == H && c->seen.W == W) {
        bits_p = bits_for((uint32_t)(c->seen.max_code + c->seen.max_code / 4));
        const uint64_t want = (uint64_t)c->seen.K + c->seen.K / 4 + 4096;      // buffers grow to this if they have to (once)
        K_p = (uint32_t)std::min<uint64_t>(want, 0x7fffffffu);
        predicted = K_p > 0 && bits_p + tile_bits <= 63;
    }
    if (predicted) {
        if ((rc = run_raster_stage(c, f, pa, n_rows, M_known >= 0 ? M_known : (int)n_rows, K_p, bits_p, cfg, out, s, true)) != GS_OK) return rc;
    } else {
        gs_launch_publish(pa, (int)((n_rows + 255) / 256), s);            // exact sizing: the hand-over is a launch of its own, and the host waits for it here
        HIP_TRY(hipGetLastError());
    }
    GsCounters hc;
    if ((rc = read_counters(c, s, pa.ticket, 0, &hc)) != GS_OK) return rc;
    if (hc.K >= (1u << 31)) return fail(GS_ERR_INVALID_ARGUMENT, "more than 2^31 sort pairs (tile ranges are int32, RAST:954-957)");
    const int bits = bits_for((uint32_t)(hc.max_depth_code > 0 ? hc.max_depth_code : 0));
    if (predicted && hc.K <= K_p && bits <= bits_p) {
        f->info.sizing = GS_SIZING_PREDICTED;
    } else {
        if (predicted) {
            // the per-pixel half ran on sizes that did not hold: its results are void (not out of bounds).  Again, exactly.
            HIP_TRY(hipMemsetAsync(pa.v.tile_start, 0, sizeof(int32_t) * (size_t)pa.v.tile_ints, s));
            f->max_tiles_known = false;                 // (k_project's word went with them: the backward's row sum then looks for giant points itself)
            f->info.sizing = GS_SIZING_REDONE;
        }
        if ((rc = run_raster_stage(c, f, pa, n_rows, hc.M, hc.K, bits, cfg, out, s, false)) != GS_OK) return rc;
    }
    // (a frame with no point in camera says nothing about the depth range: the key width of the last frame that had one stays
    // the prediction, or the frame after an empty view would always be rendered twice)
    if (!(c->seen.valid && c->seen.H == H && c->seen.W == W && hc.M == 0)) c->seen.max_code = hc.max_depth_code;
    c->seen.valid = true; c->seen.H = H; c->seen.W = W; c->seen.K = hc.K;
    *M_out = hc.M; *K_out = hc.K;
    return check_required_key_class(f);
}

extern "C" int gs_forward(gs_ctx* c, const gs_scene* sc, const gs_camera* cam, const gs_config* cfg,
                          const gs_forward_out* out, int32_t keep, gs_frame** frame_out, gs_stream stream_)
{
    if (!c || !sc || !cam || !cfg || !out || !frame_out) return fail(GS_ERR_INVALID_ARGUMENT, "gs_forward: NULL argument");
    int tiles_x = 0, tiles_y = 0, rc;
    if ((rc = check_geometry(cam, cfg, "gs_forward", &tiles_x, &tiles_y)) != GS_OK) return rc;
    if ((rc = check_scene(sc, cam, "gs_forward")) != GS_OK) return rc;
    if ((rc = check_forward_out(out, cfg, keep, "gs_forward")) != GS_OK) return rc;
    std::lock_guard<std::mutex> lock(c->mu);
    hipStream_t s;
    if ((rc = enter_call(c, stream_, &s)) != GS_OK) return rc;
    int slot = -1;
    Frame* f = begin_frame(c, cam, tiles_x * tiles_y, keep, &slot);
    GsProjectArgs pa{};
    int M = 0; uint32_t K = 0;
    rc = run_project_stage(c, f, sc, cam, cfg, s, WAIT_LATER, &pa, &M, &K);
    if (rc == GS_OK) rc = run_forward_tail(c, f, pa, sc->n_points, -1, cfg, out, s, &M, &K);
    if (rc != GS_OK) { drop_frame(c, f); return rc; }
    f->bwd_reference_order = cfg->bwd_reference_order;
    f->rgb_only = cfg->rgb_only != 0;
    finish_frame(c, f, slot, sc->n_points, M, K, GS_STAGE_PROJECT | GS_STAGE_RASTER, frame_out);
    return GS_OK;
}

// gs_project_shard: the frame's (M,16) record rows and ids, copied out
static int copy_projection(const Frame* f, int M, float* records_out, int32_t* ids_out, hipStream_t s)
{
    HIP_TRY(hipMemcpyAsync(records_out, f->bufs.rec.p, (size_t)M * 64, hipMemcpyDeviceToDevice, s));
    if (ids_out) HIP_TRY(hipMemcpyAsync(ids_out, f->bufs.ids.p, (size_t)M * 4, hipMemcpyDeviceToDevice, s));
    return GS_OK;
}

extern "C" int gs_project_shard(gs_ctx* c, const gs_scene* sc, const gs_camera* cam, const gs_config* cfg,
                                float* records_out, int32_t* ids_out, int32_t keep, gs_frame** frame_out, gs_stream stream_)
{
    if (!c || !sc || !cam || !cfg || !frame_out) return fail(GS_ERR_INVALID_ARGUMENT, "gs_project_shard: NULL argument");
    if (sc->n_points > 0 && !records_out) return fail(GS_ERR_INVALID_ARGUMENT, "gs_project_shard: records_out is NULL");
    if (((uintptr_t)records_out & 15u) != 0) return fail(GS_ERR_INVALID_ARGUMENT, "gs_project_shard: records_out must be 16-byte aligned");
    int tiles_x = 0, tiles_y = 0, rc;
    if ((rc = check_geometry(cam, cfg, "gs_project_shard", &tiles_x, &tiles_y)) != GS_OK) return rc;
    if ((rc = check_scene(sc, cam, "gs_project_shard")) != GS_OK) return rc;
    std::lock_guard<std::mutex> lock(c->mu);
    hipStream_t s;
    if ((rc = enter_call(c, stream_, &s)) != GS_OK) return rc;
    int slot = -1;
    Frame* f = begin_frame(c, cam, tiles_x * tiles_y, keep, &slot);
    GsProjectArgs pa{};
    int M = 0; uint32_t K = 0;
    rc = run_project_stage(c, f, sc, cam, cfg, s, WAIT_NOW, &pa, &M, &K);
    if (rc == GS_OK && M > 0) rc = copy_projection(f, M, records_out, ids_out, s);
    if (rc != GS_OK) { drop_frame(c, f); return rc; }
    finish_frame(c, f, slot, sc->n_points, M, K, GS_STAGE_PROJECT, frame_out);
    return GS_OK;
}

extern "C" int gs_project_shard_begin(gs_ctx* c, const gs_scene* sc, const gs_camera* cam, const gs_config* cfg,
                                      int32_t keep, gs_frame** frame_out, gs_stream stream_)
{
    if (!c || !sc || !cam || !cfg || !frame_out) return fail(GS_ERR_INVALID_ARGUMENT, "gs_project_shard_begin: NULL argument");
    int tiles_x = 0, tiles_y = 0, rc;
    if ((rc = check_geometry(cam, cfg, "gs_project_shard_begin", &tiles_x, &tiles_y)) != GS_OK) return rc;
    if ((rc = check_scene(sc, cam, "gs_project_shard_begin")) != GS_OK) return rc;
    std::lock_guard<std::mutex> lock(c->mu);
    hipStream_t s;
    if ((rc = enter_call(c, stream_, &s)) != GS_OK) return rc;
    int slot = -1;
    Frame* f = begin_frame(c, cam, tiles_x * tiles_y, keep, &slot);
    GsProjectArgs pa{};
    int M = 0; uint32_t K = 0;
    rc = run_project_stage(c, f, sc, cam, cfg, s, WAIT_FRAME, &pa, &M, &K);
    if (rc != GS_OK) { drop_frame(c, f); return rc; }
    finish_frame(c, f, slot, sc->n_points, M, K, GS_STAGE_PROJECT, frame_out);
    return GS_OK;
}

extern "C" int gs_forward_projected(gs_ctx* c, const float* records, int64_t m, const gs_camera* cam, const gs_config* cfg,
                                    const gs_forward_out* out, int32_t keep, gs_frame** frame_out, gs_stream stream_)
{
    if (!c || !cam || !cfg || !out || !frame_out) return fail(GS_ERR_INVALID_ARGUMENT, "gs_forward_projected: NULL argument");
    if (m < 0 || m >= (int64_t)1 << 31) return fail(GS_ERR_INVALID_ARGUMENT, "gs_forward_projected: m out of range");
    if (m > 0 && !records) return fail(GS_ERR_INVALID_ARGUMENT, "gs_forward_projected: records is NULL");
    int tiles_x = 0, tiles_y = 0, rc;
    if ((rc = check_geometry(cam, cfg, "gs_forward_projected", &tiles_x, &tiles_y)) != GS_OK) return rc;
    if ((rc = check_forward_out(out, cfg, keep, "gs_forward_projected")) != GS_OK) return rc;
    std::lock_guard<std::mutex> lock(c->mu);
    hipStream_t s;
    if ((rc = enter_call(c, stream_, &s)) != GS_OK) return rc;
    int slot = -1;
    Frame* f = begin_frame(c, cam, tiles_x * tiles_y, keep, &slot);
    GsProjectArgs pa{};
    int M_seen = 0; uint32_t K = 0;
    rc = run_records_stage(c, f, records, m, cfg, s, &pa);
    if (rc == GS_OK) rc = run_forward_tail(c, f, pa, m, (int)m, cfg, out, s, &M_seen, &K);
    if (rc != GS_OK) { drop_frame(c, f); return rc; }
    f->bwd_reference_order = cfg->bwd_reference_order;
    finish_frame(c, f, slot, m, (int)m, K, GS_STAGE_RASTER, frame_out);
    return GS_OK;
}

extern "C" int gs_frame_get_info(gs_ctx* c, const gs_frame* h, gs_frame_info* info)
{
    if (!c || !info) return fail(GS_ERR_INVALID_ARGUMENT, "gs_frame_get_info: NULL argument");
    std::lock_guard<std::mutex> lock(c->mu);
    Frame* f;
    if (const int rc = lookup(c, h, "gs_frame_get_info", true, &f)) return rc;
    *info = f->info;
    return GS_OK;
}

static int64_t export_count(const Frame* f, gs_export what)
{
    const int64_t M = f->info.n_points_in_camera, K = f->info.n_keys, T = f->info.n_tiles, N = f->info.n_points;
    const bool proj = (f->info.stages & GS_STAGE_PROJECT) != 0, rast = (f->info.stages & GS_STAGE_RASTER) != 0;
    switch (what) {
    case GS_X_POINT_ID_IN_CAMERA_LIST: return proj ? M : -1;
    case GS_X_POINT_IN_CAMERA_MASK: return proj ? N : -1;
    case GS_X_POINT_ALPHA_AFTER_ACTIVATION: case GS_X_POINT_RADII: case GS_X_NUM_OVERLAP_TILES: case GS_X_POINT_DEPTH: return M;
    case GS_X_ACCUMULATED_NUM_OVERLAP_TILES: return rast ? M : -1;
    case GS_X_POINT_UV: return 2 * M;
    case GS_X_POINT_IN_CAMERA: case GS_X_POINT_COLOR: return 3 * M;
    case GS_X_POINT_UV_CONIC_AND_RESCALE: return 4 * M;
    case GS_X_RECORDS: return proj ? 16 * M : -1;
    case GS_X_SORT_KEY: case GS_X_POINT_OFFSET_WITH_SORT_KEY: return rast ? K : -1;
    case GS_X_TILE_POINTS_START: case GS_X_TILE_POINTS_END: return rast ? T : -1;
    default: return -1;
    }
}

extern "C" int64_t gs_frame_export_count(gs_ctx* c, const gs_frame* h, gs_export what)
{
    if (!c) return -1;
    std::lock_guard<std::mutex> lock(c->mu);
    Frame* f = resolve(c, h);
    if (f && resolve_pending(c, f) != GS_OK) return -1;
    return f ? export_count(f, what) : -1;
}

extern "C" int gs_frame_export(gs_ctx* c, const gs_frame* h, gs_export what, void* dst, gs_stream stream_)
{
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, "gs_frame_export: ctx is NULL");
    if (!dst) return fail(GS_ERR_INVALID_ARGUMENT, "gs_frame_export: dst is NULL");
    if (what < 0 || what >= GS_X_COUNT_) return fail(GS_ERR_INVALID_ARGUMENT, "gs_frame_export: unknown export id");
    std::lock_guard<std::mutex> lock(c->mu);
    Frame* f;
    int rc;
    if ((rc = lookup(c, h, "gs_frame_export", true, &f)) != GS_OK) return rc;
    if (export_count(f, what) < 0) return fail(GS_ERR_STATE, "gs_frame_export: this frame does not hold that stage");
    hipStream_t s;
    if ((rc = enter_call(c, stream_, &s)) != GS_OK) return rc;
    const GsFrameView v = frame_view(*f);
    if (what == GS_X_RECORDS) {                  // the (M,16) rows as they are: what the owner of a shard sends to the renderers
        if (f->info.n_points_in_camera > 0)
            HIP_TRY(hipMemcpyAsync(dst, v.PA, (size_t)f->info.n_points_in_camera * 64, hipMemcpyDeviceToDevice, s));
        return GS_OK;
    }
    GsExportArgs a{};
    a.what = (int)what; a.N = f->info.n_points; a.M = (int)f->info.n_points_in_camera; a.K = (uint32_t)f->info.n_keys;
    a.T = v.T; a.depth_bits = f->depth_bits; a.key_bytes = f->key_bytes; a.depth_codes = v.depth_codes;
    a.ids = v.ids; a.PA = v.PA; a.PB = v.PB; a.PC = v.PC; a.PD = v.PD;
    a.ntiles = v.ntiles; a.offsets = v.offsets;
    a.keys_sorted = v.keys_sorted; a.vals_sorted = v.vals_sorted;
    a.tile_start = v.tile_start; a.tile_end = v.tile_end; a.mask = v.mask;
    a.dst = dst;
    gs_launch_export(a, s);
    HIP_TRY(hipGetLastError());
    return GS_OK;
}

// ---- backward -----------------------------------------------------------------------------------------------------
// waves per tile of the backward blend: one wave per tile is the cheapest in instructions, but a small image
// has too few tiles to fill 1024 SIMDs, so tiles are split into 2 or 4 quadrant groups (more rows of `partial`)
static int waves_per_tile(int n_tiles)
{
    int G = 1;
    if (const char* e = getenv("GS_BWD_WAVES_PER_TILE")) G = atoi(e);
    else if (n_tiles < 2000) G = 4;      // measured at 976x544 (2074 tiles): G = 2 0.167 ms, G = 4 0.203, G = 1 0.235
    else if (n_tiles < 6144) G = 2;      // at 1920x1088 (8160 tiles): G = 1 0.259 ms, G = 2 0.285
    if (G != 1 && G != 2 && G != 4) G = 1;
    return G;
}

static bool bwd_prefill_enabled()
{
    const char* e = getenv("GS_BWD_PREFILL");
    return !(e && e[0] == '0');
}

// fills the blend half of the arguments; sums_out = where the per-splat sums go
static int prepare_backward_blend(gs_ctx* c, Frame* f, const float* grad_image, const float* acc_alpha, const int32_t* last,
                                  float* mag_image, float4* sums_out, int strict, hipStream_t stream, GsBackwardArgs* a_out)
{
    const uint32_t K = (uint32_t)f->info.n_keys;
    const int G = waves_per_tile(f->info.n_tiles);
    const size_t rows = (size_t)(K > 0 ? K : 1) * (size_t)G;
    const size_t flag_bytes = (rows + 15) / 16 * 16;
    hipError_t e = c->partial.ensure(rows * 12 * sizeof(float), &c->device_bytes);
    if (e != hipSuccess) return fail(GS_ERR_OUT_OF_MEMORY, "backward: partial-sum buffer");
    const size_t Mp = (size_t)(f->info.n_points_in_camera > 0 ? f->info.n_points_in_camera : 1);
    // Row flags (K*G bytes) and per-point `touched` bytes behind them.  They are TAGGED, not cleared: a backward writes its own tag
    // (1..255) and reads a flag as set only if it holds that tag, so the 6 MB clear per backward is gone; the buffer is zeroed when it
    // is (re)allocated and when the tags wrap round.  A reallocation is told by the capacity, never by the address: the allocator
    // may hand back the block just freed, and a grown tail left uncleared holds stray bytes equal to the current tag.
    const size_t cap_before = c->visited.cap;
    e = c->visited.ensure(flag_bytes + Mp + 16, &c->device_bytes);
    if (e != hipSuccess) return fail(GS_ERR_OUT_OF_MEMORY, "backward: visited buffer");
    if (c->visited.cap != cap_before || c->visit_gen == 255) {
        HIP_TRY(hipMemsetAsync(c->visited.p, 0, c->visited.cap, stream));
        c->visit_gen = 0;
    }
    c->visit_gen += 1;
    c->bwd_serial += 1;                               // this backward owns the tags from here on
    c->touched_offset = flag_bytes;
    f->bwd_serial = c->bwd_serial;
    if (!c->zero_row.p) {
        if (c->zero_row.ensure(64, &c->device_bytes) != hipSuccess) return fail(GS_ERR_OUT_OF_MEMORY, "backward: zero row");
        HIP_TRY(hipMemsetAsync(c->zero_row.p, 0, c->zero_row.cap, stream));
    }
    GsBackwardArgs a{};
    a.prof = &c->prof;
    a.views = backward_views(c, f);
    a.view_slot = f->view_keyed ? frame_view(*f).n_heavy + GS_ORDER_WRITE_SLOT : nullptr;
    a.N = f->info.n_points; a.M = (int)f->info.n_points_in_camera; a.K = K;
    a.H = f->info.camera_height; a.W = f->info.camera_width;
    a.tiles_x = (a.W + GS_TILE - 1) / GS_TILE;
    a.v = frame_view(*f);
    a.grad_image = grad_image; a.acc_alpha = acc_alpha; a.last = last;
    a.partial = c->partial.as<float>();
    a.visited = c->visited.as<uint8_t>();
    a.G = G;
    a.item_cap = f->cut_cap;                          // >= the segments of all heavy tiles together (never binds: deterministic)
    // heavy-tile threshold in half-means of work: sharing a tile among four waves costs more work in total and shortens the launch
    // only where long walks are what the launch waits for; twice the mean measured best on both clustered workloads and changes
    // nothing on the uniform ones (max / mean = 2).  GS_BWD_HEAVY_X2 overrides; GS_BWD_SPLIT_HEAVY=0 = no heavy tiles.
    static const int heavy_env = []{ const char* e = getenv("GS_BWD_SPLIT_HEAVY"); if (e && e[0] == '0') return 0;
                                     const char* x = getenv("GS_BWD_HEAVY_X2"); return x ? atoi(x) : -1; }();
    a.heavy_factor_x2 = heavy_env >= 0 ? heavy_env : 4;
    a.strict = strict ? 1 : 0;
    a.gen = c->visit_gen;
    a.touched = c->visited.as<uint8_t>() + flag_bytes;
    a.zero_row = c->zero_row.as<float4>();
    a.max_tiles_hint = f->max_tiles_known ? a.v.max_tiles : nullptr;
    a.sums = sums_out;
    a.mag_image = mag_image;
    a.live_sums = bwd_prefill_enabled() ? 1 : 0;
    *a_out = a;
    return GS_OK;
}

static int prepare_backward_points(const Frame* f, const gs_scene* sc, const gs_camera* cam, const gs_config* cfg,
                                   int32_t sh_band, const gs_backward_out* out, const float4* sums, GsBackwardArgs* a)
{
    a->N = f->info.n_points; a->M = (int)f->info.n_points_in_camera;
    a->v = frame_view(*f);
    a->sums = const_cast<float4*>(sums);
    a->point_cloud = sc->point_cloud; a->features = sc->point_cloud_features; a->object_id = sc->point_object_id;
    a->Kmat = cam->camera_intrinsics;
    a->sh_band = sh_band; a->f_color = cfg->grad_color_factor; a->f_high = cfg->grad_high_order_color_factor;
    a->f_s = cfg->grad_s_factor; a->f_q = cfg->grad_q_factor; a->f_alpha = cfg->grad_alpha_factor;
    a->grad_pc = out->grad_pointcloud; a->grad_feat = out->grad_pointcloud_features; a->grad_uv = out->grad_viewspace;
    a->mag = out->magnitude_grad_viewspace;
    a->n_affected = out->num_affected_pixels;
    a->hook_gpc = out->hook_grad_point_in_camera; a->hook_gfeat = out->hook_grad_pointfeatures_in_camera;
    a->hook_guv = out->hook_grad_viewspace; a->hook_mag = out->hook_magnitude_grad_viewspace;
    a->hook_ids = out->hook_point_id_in_camera_list; a->hook_ntiles = out->hook_num_overlap_tiles;
    a->hook_depth = out->hook_point_depth; a->hook_uv = out->hook_point_uv_in_camera;
    if (const gs_controller_accumulators* ca = out->controller) {
        if (!ca->accumulated_num_in_camera || !ca->accumulated_num_pixels || !ca->accumulated_view_space_position_gradients ||
            !ca->accumulated_view_space_position_gradients_avg || !ca->accumulated_position_gradients || !ca->accumulated_position_gradients_norm)
            return fail(GS_ERR_INVALID_ARGUMENT, "backward: controller accumulators must all be given");
        a->c_num_in_camera = ca->accumulated_num_in_camera; a->c_num_pixels = ca->accumulated_num_pixels;
        a->c_vs_grad = ca->accumulated_view_space_position_gradients; a->c_vs_grad_avg = ca->accumulated_view_space_position_gradients_avg;
        a->c_pos_grad = ca->accumulated_position_gradients; a->c_pos_grad_norm = ca->accumulated_position_gradients_norm;
    }
    return GS_OK;
}

static int check_backward_points_args(const Frame* f, const gs_scene* sc, const gs_camera* cam, const gs_backward_out* out, const char* who,
                                      bool pose_only = false)
{
    if (sc->n_points > 0 && !pose_only && (!out->grad_pointcloud || !out->grad_pointcloud_features))
        return fail(GS_ERR_INVALID_ARGUMENT, who, "grad_pointcloud / grad_pointcloud_features are mandatory");
    if (sc->n_points != f->info.n_points || cam->camera_height != f->info.camera_height || cam->camera_width != f->info.camera_width)
        return fail(GS_ERR_INVALID_ARGUMENT, who, "scene/camera do not match the frame");
    if (((uintptr_t)out->grad_pointcloud_features & 15u) != 0 || ((uintptr_t)sc->point_cloud_features & 15u) != 0)
        return fail(GS_ERR_INVALID_ARGUMENT, who, "feature arrays must be 16-byte aligned");
    if (out->hook_grad_pointfeatures_in_camera && ((uintptr_t)out->hook_grad_pointfeatures_in_camera & 15u) != 0)
        return fail(GS_ERR_INVALID_ARGUMENT, who, "hook feature array must be 16-byte aligned");
    return GS_OK;
}

// gs_backward, and gs_backward_ex with a depth and/or an alpha gradient (extra != NULL: checked by the caller)
static int backward_impl(gs_ctx* c, gs_frame* h, const gs_scene* sc, const gs_camera* cam, const gs_config* cfg,
                         const float* grad_image, const gs_backward_extra* extra, const float* acc_alpha, const int32_t* last,
                         int32_t sh_band, const gs_backward_out* out, gs_stream stream_)
{
    if (!c || !sc || !cam || !cfg || !out) return fail(GS_ERR_INVALID_ARGUMENT, "gs_backward: NULL argument");
    if (!grad_image || !acc_alpha || !last) return fail(GS_ERR_INVALID_ARGUMENT, "gs_backward: NULL image-sized input");
    std::lock_guard<std::mutex> lock(c->mu);
    Frame* f;
    int rc;
    if ((rc = lookup(c, h, "gs_backward", false, &f)) != GS_OK) return rc;
    if (!f->info.kept_for_backward) return fail(GS_ERR_STATE, "gs_backward: frame was not kept for backward");
    if (f->info.stages != (GS_STAGE_PROJECT | GS_STAGE_RASTER)) return fail(GS_ERR_STATE, "gs_backward: frame does not come from gs_forward");
    // pose gradient: both pointers or neither; with them, the two point gradients may be left out (pose-only backward)
    const bool pose = out->grad_q_pointcloud_camera || out->grad_t_pointcloud_camera;
    if (pose && (!out->grad_q_pointcloud_camera || !out->grad_t_pointcloud_camera))
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_backward: grad_q_pointcloud_camera and grad_t_pointcloud_camera must be given together");
    const bool points = !pose || out->grad_pointcloud || out->grad_pointcloud_features;
    if (pose && cam->n_objects != f->n_objects)
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_backward: camera n_objects does not match the frame's forward");
    if ((rc = check_backward_points_args(f, sc, cam, out, "gs_backward", !points)) != GS_OK) return rc;
    hipStream_t s;
    if ((rc = enter_call(c, stream_, &s)) != GS_OK) return rc;
    if (c->sums.ensure((size_t)(f->info.n_points_in_camera > 0 ? f->info.n_points_in_camera : 1) * 48, &c->device_bytes) != hipSuccess)
        return fail(GS_ERR_OUT_OF_MEMORY, "gs_backward: per-point sums buffer");
    if (pose && c->pose_scratch.ensure(gs_pose_scratch_size((int)f->info.n_points_in_camera, f->n_objects), &c->device_bytes) != hipSuccess)
        return fail(GS_ERR_OUT_OF_MEMORY, "gs_backward: pose-gradient scratch");
    GsBackwardArgs a{};
    if ((rc = prepare_backward_blend(c, f, grad_image, acc_alpha, last, out->magnitude_grad_viewspace_on_image, c->sums.as<float4>(), cfg->bwd_reference_order, s, &a)) != GS_OK) return rc;
    if ((rc = prepare_backward_points(f, sc, cam, cfg, sh_band, out, c->sums.as<float4>(), &a)) != GS_OK) return rc;
    if (extra) {                    // the AUX kernels, walking every heavy tile whole (no cut records: k_backward.hip)
        a.grad_depth = extra->grad_rasterized_depth; a.depth = extra->rasterized_depth;
        a.grad_alpha = extra->grad_pixel_accumulated_alpha;
        a.aux = 1;
        a.v.cuts = nullptr;
    }
    // What an untouched point receives (zeros in every per-point output, the hook's copies of forward data, the controller's in-camera
    // count) is written by fill blocks of the blend's launch and the points stage visits the touched points only -- when both run in
    // this call and the blend is launched at all.  GS_BWD_PREFILL=0: the points stage writes everything itself (and k_sum_rows runs
    // in its previous mapping: prepare_backward_blend).  Read per call (not cached), so that one process can compare the two forms.
    a.prefill = points && a.grad_feat && a.v.T > 0 && a.K > 0 && bwd_prefill_enabled();
    gs_launch_backward_blend(a, s);        // (the tile order it writes goes into the view table too)
    if (points) gs_launch_backward_points(a, s);            // pose-only: no point gradients, hook arrays or controller statistics
    if (pose) gs_launch_pose_grad(a, f->n_objects, c->pose_scratch.p, out->grad_q_pointcloud_camera, out->grad_t_pointcloud_camera, s);
    HIP_TRY(hipGetLastError());
    return GS_OK;
}

extern "C" int gs_backward(gs_ctx* c, gs_frame* h, const gs_scene* sc, const gs_camera* cam, const gs_config* cfg,
                           const float* grad_image, const float* acc_alpha, const int32_t* last,
                           int32_t sh_band, const gs_backward_out* out, gs_stream stream_)
{
    return backward_impl(c, h, sc, cam, cfg, grad_image, nullptr, acc_alpha, last, sh_band, out, stream_);
}

extern "C" int gs_backward_ex(gs_ctx* c, gs_frame* h, const gs_scene* sc, const gs_camera* cam, const gs_config* cfg,
                              const float* grad_image, const gs_backward_extra* extra, const float* acc_alpha, const int32_t* last,
                              int32_t sh_band, const gs_backward_out* out, gs_stream stream_)
{
    if (extra && extra->grad_rasterized_depth && !extra->rasterized_depth)
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_backward_ex: grad_rasterized_depth needs rasterized_depth (the forward's output)");
    if (extra && !extra->grad_rasterized_depth && !extra->grad_pixel_accumulated_alpha) extra = nullptr;   // exactly gs_backward
    return backward_impl(c, h, sc, cam, cfg, grad_image, extra, acc_alpha, last, sh_band, out, stream_);
}

extern "C" int gs_backward_projected(gs_ctx* c, gs_frame* h, const float* grad_image, const float* acc_alpha, const int32_t* last,
                                     float* splat_sums_out, float* mag_image, gs_stream stream_)
{
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, "gs_backward_projected: ctx is NULL");
    if (!grad_image || !acc_alpha || !last) return fail(GS_ERR_INVALID_ARGUMENT, "gs_backward_projected: NULL image-sized input");
    if (((uintptr_t)splat_sums_out & 15u) != 0) return fail(GS_ERR_INVALID_ARGUMENT, "gs_backward_projected: splat_sums_out must be 16-byte aligned");
    std::lock_guard<std::mutex> lock(c->mu);
    Frame* f;
    int rc;
    if ((rc = lookup(c, h, "gs_backward_projected", false, &f)) != GS_OK) return rc;
    if (!f->info.kept_for_backward) return fail(GS_ERR_STATE, "gs_backward_projected: frame was not kept for backward");
    if (!(f->info.stages & GS_STAGE_RASTER)) return fail(GS_ERR_STATE, "gs_backward_projected: frame holds no raster stage");
    if (f->info.n_points_in_camera > 0 && !splat_sums_out) return fail(GS_ERR_INVALID_ARGUMENT, "gs_backward_projected: splat_sums_out is NULL");
    hipStream_t s;
    if ((rc = enter_call(c, stream_, &s)) != GS_OK) return rc;
    GsBackwardArgs a{};
    if ((rc = prepare_backward_blend(c, f, grad_image, acc_alpha, last, mag_image, reinterpret_cast<float4*>(splat_sums_out), f->bwd_reference_order, s, &a)) != GS_OK) return rc;
    gs_launch_backward_blend(a, s);        // (the tile order it writes goes into the view table too)
    HIP_TRY(hipGetLastError());
    return GS_OK;
}

extern "C" int gs_backward_shard(gs_ctx* c, gs_frame* h, const gs_scene* sc, const gs_camera* cam, const gs_config* cfg,
                                 const float* splat_sums, int32_t sh_band, const gs_backward_out* out, gs_stream stream_)
{
    if (!c || !sc || !cam || !cfg || !out) return fail(GS_ERR_INVALID_ARGUMENT, "gs_backward_shard: NULL argument");
    if (((uintptr_t)splat_sums & 15u) != 0) return fail(GS_ERR_INVALID_ARGUMENT, "gs_backward_shard: splat_sums must be 16-byte aligned");
    std::lock_guard<std::mutex> lock(c->mu);
    Frame* f;
    int rc;
    if ((rc = lookup(c, h, "gs_backward_shard", true, &f)) != GS_OK) return rc;
    if (!f->info.kept_for_backward) return fail(GS_ERR_STATE, "gs_backward_shard: frame was not kept for backward");
    if (!(f->info.stages & GS_STAGE_PROJECT)) return fail(GS_ERR_STATE, "gs_backward_shard: frame holds no projection stage");
    if (f->info.n_points_in_camera > 0 && !splat_sums) return fail(GS_ERR_INVALID_ARGUMENT, "gs_backward_shard: splat_sums is NULL");
    if (out->grad_q_pointcloud_camera || out->grad_t_pointcloud_camera)
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_backward_shard: pose gradients are not available on the staged (Gaussian-parallel) path; "
                                             "use gs_backward");
    if ((rc = check_backward_points_args(f, sc, cam, out, "gs_backward_shard")) != GS_OK) return rc;
    hipStream_t s;
    if ((rc = enter_call(c, stream_, &s)) != GS_OK) return rc;
    GsBackwardArgs a{};
    a.prof = &c->prof;
    if ((rc = prepare_backward_points(f, sc, cam, cfg, sh_band, out, reinterpret_cast<const float4*>(splat_sums), &a)) != GS_OK) return rc;
    gs_launch_backward_points(a, s);
    HIP_TRY(hipGetLastError());
    return GS_OK;
}

// ---- feature channels (include/gs_channels.h, k_channels.hip) --------------------------------------------------------------
// The checks both directions share (mutex held); on success the stream is entered and *f_out is the frame.
static int channels_enter(gs_ctx* c, const gs_frame* h, int32_t n_channels, const char* who, gs_stream stream_, Frame** f_out, hipStream_t* s_out)
{
    if (n_channels < 1 || n_channels > GS_CHANNELS_MAX)
        return fail(GS_ERR_INVALID_ARGUMENT, who, "n_channels must be in 1.." + std::to_string(GS_CHANNELS_MAX));
    Frame* f;
    if (const int rc = lookup(c, h, who, true, &f)) return rc;
    if (f->info.stages != (GS_STAGE_PROJECT | GS_STAGE_RASTER))
        return fail(GS_ERR_INVALID_ARGUMENT, who, "the frame must come from gs_forward (frames made from records or shards are not supported)");
    if (f->rgb_only) return fail(GS_ERR_INVALID_ARGUMENT, who, "an rgb_only frame has no pixel_offset_of_last_effective_point");
    if (const int rc = enter_call(c, stream_, s_out)) return rc;
    *f_out = f;
    return GS_OK;
}

static GsChannelsArgs channels_args(const Frame* f, int32_t n_channels, const int32_t* last)
{
    GsChannelsArgs a{};
    a.v = frame_view(*f);
    a.M = (int)f->info.n_points_in_camera; a.K = (uint32_t)f->info.n_keys;
    a.H = f->info.camera_height; a.W = f->info.camera_width; a.tiles_x = (a.W + GS_TILE - 1) / GS_TILE;
    a.C = n_channels; a.last = last;
    return a;
}

extern "C" int gs_channels_forward(gs_ctx* c, const gs_frame* h, const float* values, int32_t n_channels,
                                   const int32_t* last, float* out, gs_stream stream_)
{
    if (!c || !h || !values || !last || !out) return fail(GS_ERR_INVALID_ARGUMENT, "gs_channels_forward: NULL argument");
    std::lock_guard<std::mutex> lock(c->mu);
    Frame* f;
    hipStream_t s;
    if (const int rc = channels_enter(c, h, n_channels, "gs_channels_forward", stream_, &f, &s)) return rc;
    GsChannelsArgs a = channels_args(f, n_channels, last);
    a.values = values; a.out = out;
    if (a.K == 0u || a.M <= 0) {                // nothing was blended: the tile ranges are all empty
        HIP_TRY(hipMemsetAsync(out, 0, (size_t)a.H * (size_t)a.W * (size_t)n_channels * sizeof(float), s));
        return GS_OK;
    }
    gs_launch_channels_fwd(a, s);
    HIP_TRY(hipGetLastError());
    return GS_OK;
}

extern "C" int gs_channels_backward(gs_ctx* c, const gs_frame* h, const float* grad_out, int32_t n_channels,
                                    const int32_t* last, float* grad_values, gs_stream stream_)
{
    if (!c || !h || !grad_out || !last || !grad_values) return fail(GS_ERR_INVALID_ARGUMENT, "gs_channels_backward: NULL argument");
    std::lock_guard<std::mutex> lock(c->mu);
    Frame* f;
    hipStream_t s;
    if (const int rc = channels_enter(c, h, n_channels, "gs_channels_backward", stream_, &f, &s)) return rc;
    GsChannelsArgs a = channels_args(f, n_channels, last);
    a.grad_out = grad_out; a.grad_values = grad_values;
    // rows outside the camera are zero; k_channels_sum writes every in-camera row
    if (f->info.n_points > 0) HIP_TRY(hipMemsetAsync(grad_values, 0, (size_t)f->info.n_points * (size_t)n_channels * sizeof(float), s));
    if (a.K == 0u || a.M <= 0) return GS_OK;
    // scratch of one channel chunk: four partial rows (one per quadrant) per (point, tile) pair, their flags, one byte per point
    const size_t rows = (size_t)a.K * 4, row_flags = (rows + 15) / 16 * 16;
    if (const int rc = grow(c, "gs_channels_backward", { NEED(c->ch_partial, rows * (size_t)gs_channels_chunk(n_channels) * sizeof(float)),
                                 NEED(c->ch_flags, row_flags + (size_t)a.M) }))
        return rc;
    a.partial = c->ch_partial.as<float>(); a.flags = c->ch_flags.as<uint8_t>(); a.touched = a.flags + row_flags;
    a.flag_bytes = row_flags + (size_t)a.M;
    HIP_TRY(gs_launch_channels_bwd(a, s));
    HIP_TRY(hipGetLastError());
    return GS_OK;
}

// ---- touched rows (include/gs_sparse.h, k_sparse.hip; the row-selective Adam step that reads the list: gs_api_calls.hip) ----
// No host synchronisation and no device-to-host copy: the count stays on the device.
extern "C" int gs_touched_rows(gs_ctx* c, const gs_frame* h, int32_t* ids_out, int64_t capacity, int32_t* count_out, gs_stream stream_)
{
    if (!c || !h || !ids_out || !count_out) return fail(GS_ERR_INVALID_ARGUMENT, "gs_touched_rows: NULL argument");
    std::lock_guard<std::mutex> lock(c->mu);
    Frame* f;
    int rc;
    if ((rc = lookup(c, h, "gs_touched_rows", false, &f)) != GS_OK) return rc;      // (a frame only begun has had no backward: nothing to wait for)
    if (!(f->info.stages & GS_STAGE_PROJECT))
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_touched_rows: the frame holds no projection stage (frames made from records are not supported)");
    if (capacity < f->info.n_points_in_camera) return fail(GS_ERR_INVALID_ARGUMENT, "gs_touched_rows: capacity is below the frame's n_points_in_camera");
    if (f->bwd_serial == 0) return fail(GS_ERR_STATE, "gs_touched_rows: no backward has run on this frame");
    if (f->bwd_serial != c->bwd_serial)
        return fail(GS_ERR_STATE, "gs_touched_rows: another backward has run on this context since the frame's (the list describes the latest one only)");
    const int M = (int)f->info.n_points_in_camera;
    // no pair: the blend did not run and wrote no tag (stale bytes never equal this backward's tag, but nothing needs reading)
    const int M_eff = (f->info.n_keys > 0 && f->info.n_tiles > 0) ? M : 0;
    HIP_TRY(hipSetDevice(c->device));           // the scratch grows before the stream enters: a call that fails here leaves it alone
    if ((rc = grow(c, "gs_touched_rows", { NEED(c->row_block_totals, (size_t)(gs_rows_blocks(M_eff) + 1) * sizeof(uint32_t)) })) != GS_OK) return rc;
    hipStream_t s;
    if ((rc = enter_call(c, stream_, &s)) != GS_OK) return rc;
    gs_launch_touched_rows(c->visited.as<uint8_t>() + c->touched_offset, c->visit_gen, frame_view(*f).ids, M_eff,
                           c->row_block_totals.as<uint32_t>(), ids_out, capacity, count_out, s);
    HIP_TRY(hipGetLastError());
    return GS_OK;
}

extern "C" int gs_frame_heavy_tiles(gs_ctx* c, const gs_frame* h, int32_t* n_out, gs_stream stream_)
{
    if (!c || !n_out) return fail(GS_ERR_INVALID_ARGUMENT, "gs_frame_heavy_tiles: NULL argument");
    std::lock_guard<std::mutex> lock(c->mu);
    Frame* f;
    int rc;
    if ((rc = lookup(c, h, "gs_frame_heavy_tiles", false, &f)) != GS_OK) return rc;
    // the counts are the frame's own (k_tile_order writes them into its tile-order buffer), but only a backward writes them
    if (f->bwd_serial == 0) return fail(GS_ERR_STATE, "gs_frame_heavy_tiles: no backward has run on this frame");
    if (!(f->info.stages & GS_STAGE_RASTER) || f->info.n_tiles <= 0 || f->info.n_keys <= 0 || !f->bufs.tile_order.p) { n_out[0] = n_out[1] = 0; return GS_OK; }
    hipStream_t s;
    if ((rc = enter_call(c, stream_, &s)) != GS_OK) return rc;
    HIP_TRY(hipMemcpyAsync(n_out, frame_view(*f).n_heavy, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return GS_OK;
}

extern "C" int gs_frame_release(gs_ctx* c, gs_frame* h)
{
    if (!c || !h) return GS_OK;
    std::lock_guard<std::mutex> lock(c->mu);
    Frame* f = resolve(c, h);
    if (!f) return fail(GS_ERR_STATE, "gs_frame_release: not a live frame of this context (already released?)");
    drop_frame(c, f);
    return GS_OK;
}

// ---- diagnostic build only (make stats): counters of the blend kernels, tools/blend_stats.py ----
#ifdef GS_STATS
__device__ unsigned long long gs_stats_counters[32];
__device__ unsigned long long gs_stats_wave_times[2 * 65536];
extern "C" int gs_debug_wave_times_read(unsigned long long* out, int n_waves)
{
    if (hipDeviceSynchronize() != hipSuccess) return -2;
    if (n_waves > 65536) n_waves = 65536;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(gs_stats_wave_times), sizeof(unsigned long long) * 2 * (size_t)n_waves) != hipSuccess) return -2;
    return 0;
}
extern "C" int gs_debug_stats_read(unsigned long long* out32, int reset)
{
    if (hipDeviceSynchronize() != hipSuccess) return -2;
    if (hipMemcpyFromSymbol(out32, HIP_SYMBOL(gs_stats_counters), sizeof(unsigned long long) * 32) != hipSuccess) return -2;
    if (reset) {
        unsigned long long z[32] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(gs_stats_counters), z, sizeof(z)) != hipSuccess) return -2;
    }
    return 0;
}
#endif

// ---- include/gs_view_hints.h: the view table, copied out for tests and diagnostics -------------------------------------------
extern "C" int gs_view_hints_read(gs_ctx* c, const gs_frame* frame, int32_t slot, int32_t* n_slots, int32_t* n_tiles,
                                  float* keys, int32_t* filled, int32_t slot_cap, int32_t* order, int32_t order_cap, int32_t* frame_slots)
{
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, "gs_view_hints_read: ctx is NULL");
    if (slot_cap < 0 || order_cap < 0) return fail(GS_ERR_INVALID_ARGUMENT, "gs_view_hints_read: negative capacity");
    std::lock_guard<std::mutex> lock(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    const int S = c->view_S, T = c->view_T;
    if (slot > S) return fail(GS_ERR_INVALID_ARGUMENT, "gs_view_hints_read: no such slot");
    if (n_slots) *n_slots = S;
    if (n_tiles) *n_tiles = T;
    const GsViewTable tab{ c->view_table.as<int32_t>(), S, T };
    if (S > 0 && (keys || filled)) {
        std::vector<int32_t> words((size_t)GS_VIEW_KEY_INTS * S);
        HIP_TRY(hipMemcpy(words.data(), tab.key(0), 4 * words.size(), hipMemcpyDeviceToHost));
        for (int i = 0; i < S && i < slot_cap; ++i) {
            if (keys) std::memcpy(keys + (size_t)GS_VIEW_KEY_FLOATS * i, &words[(size_t)GS_VIEW_KEY_INTS * i], 4 * GS_VIEW_KEY_FLOATS);
            if (filled) filled[i] = words[(size_t)GS_VIEW_KEY_INTS * i + 7] == T ? 1 : 0;
        }
    }
    if (order && slot >= 0 && S > 0 && T > 0 && order_cap > 0)
        HIP_TRY(hipMemcpy(order, tab.order(slot), 4 * (size_t)std::min(T, order_cap), hipMemcpyDeviceToHost));
    if (frame_slots) {
        frame_slots[0] = frame_slots[1] = -2;
        if (frame) {
            Frame* f;
            if (const int rc = lookup(c, frame, "gs_view_hints_read", false, &f)) return rc;
            if (f->view_keyed && f->view_epoch != 0 && f->view_epoch == c->view_epoch)
                HIP_TRY(hipMemcpy(frame_slots, frame_view(*f).n_heavy + GS_ORDER_READ_SLOT, 8, hipMemcpyDeviceToHost));
        }
    }
    return GS_OK;
}
