// gs_host.h -- what the two host files of libgsrast.so share (gs_api.hip: everything that knows a Frame; gs_api_calls.hip: the
// entry points that hold none): the error text, the grow-only device buffers, the context, and the prologue and body of a call.
// Included by those two files only.
#pragma once
#include "../../include/gs_rasterizer.h"
#include "gs_common.h"

#include <initializer_list>
#include <mutex>
#include <string>
#include <vector>

// what gs_last_error() returns, per thread (defined in gs_api.hip)
extern thread_local std::string g_last_error __attribute__((visibility("hidden")));

static int fail(int code, const std::string& msg)
{
    g_last_error = msg;
    return code;
}

// "who: msg", who being the entry point that refuses the call
static int fail(int code, const char* who, const std::string& msg)
{
    g_last_error.assign(who).append(": ").append(msg);
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e__ = (expr);                                                                   \
        if (e__ != hipSuccess)                                                                     \
            return fail(e__ == hipErrorOutOfMemory ? GS_ERR_OUT_OF_MEMORY : GS_ERR_HIP,            \
                        std::string(#expr) + ": " + hipGetErrorString(e__));                       \
    } while (0)

// Grow-only device buffer.  Growth (hipFree + hipMalloc) happens only when a frame is larger
// than anything seen before; steady-state frames allocate nothing.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes, int64_t* total)
    {
        if (bytes <= cap) return hipSuccess;
        size_t want = bytes + bytes / 4 + 256;     // 25 % slack: K drifts from frame to frame
        if (p) { (void)hipFree(p); *total -= (int64_t)cap; p = nullptr; cap = 0; }
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = want; *total += (int64_t)want;
        return hipSuccess;
    }
    void release(int64_t* total) { if (p) { (void)hipFree(p); *total -= (int64_t)cap; } p = nullptr; cap = 0; }
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

struct GsProf {
    uint64_t mask = 0;
    struct Rec { int kid; hipEvent_t a, b; };
    std::vector<Rec> recs;          // records in flight since the last read
    std::vector<hipEvent_t> spare;  // recycled events
    double total_ms[KID_COUNT_] = {};
    int64_t launches[KID_COUNT_] = {};
};

// gs_image_resample: both axes of one geometry on the device (start, count, weight of x, then of y, in one buffer)
struct ResampleTable {
    int H_in = 0, W_in = 0, h_full = 0, w_full = 0;
    DevBuf buf;
    GsResampleAxis ax{}, ay{};
    std::vector<unsigned char> host;    // what the upload reads: lives as long as the table
};

struct Frame;                           // gs_api.hip: only that file looks inside one

#define GS_COUNTER_SLOTS 64
struct gs_ctx {
    int device = 0;
    GsProf prof;
    std::mutex mu;
    int64_t device_bytes = 0;
    std::vector<Frame*> frames;         // slot i of the ticket space (recycled, generation-tagged)
    int transient = -1;                 // slot of the frame of the last keep_for_backward == 0 call
    // scratch shared by all frames (stream ordered)
    DevBuf block_counts, block_offsets, tile_block_sums, hist, scan_tmp, counters, partial, visited, zero_row, sums, loss_ws;
    // the per-point stage's [digit][block] pair counts + their row scans (k_project.hip: gs_bin_digits_*; k_binning.hip: k_keygen's first
    // pass).  Written by the frame's per-point kernel, read by every binning of the SAME call (the second one of a re-sized frame too):
    // nothing else touches it, and the K-sized hist of the later passes is a buffer of its own
    DevBuf first_hist;
    DevBuf pose_scratch;                // per-block pose-gradient records (k_pose.hip), grown on demand
    DevBuf mcmc_ws;                     // gs_mcmc_regulariser: its per-block sums and totals, read by nothing else
    DevBuf appearance_ws;               // gs_appearance_backward / _moments: their per-block sums, read by nothing else
    DevBuf background_ws;               // gs_background_backward: its per-block sums, read by nothing else
    DevBuf filter3d_ws;                 // gs_filter3d_rate: the bits of the smallest seen rate, read by nothing else
    DevBuf bilateral_ws;                // gs_bilateral_slice_backward: the block sums of split footprints, read by nothing else
    DevBuf depth_ws;                    // gs_depth_loss_forward: its finished moments and per-block sums, read by nothing else
    DevBuf geometry_ws;                 // gs_normal_loss_forward / gs_depth_smooth_forward: their per-tile sums, read by nothing else
    DevBuf ch_partial, ch_flags;        // gs_channels_backward: partial rows and row flags of one channel chunk; never shared with partial / visited
    uint8_t visit_gen = 0;                 // tag of the last backward's flags in `visited` (0: the buffer is all zero)
    // The last backward blend of the context: its number (visit_gen wraps, this does not) and where its per-point `touched` bytes
    // begin in `visited`.  A frame whose bwd_serial is not this one no longer owns the tags (gs_touched_rows).
    uint64_t bwd_serial = 0;
    size_t touched_offset = 0;
    DevBuf row_block_totals;               // gs_touched_rows: one count per compaction block
    DevBuf merge_tags, merge_ids;          // gs_merge_rows: one tag byte per point-cloud row, the id words of all lists (block totals: row_block_totals)
    DevBuf knn_sort, knn_hist, knn_points, knn_tree;   // gs_knn: its own work memory, read by nothing else (a kept frame never sees it)
    DevBuf mix_records, mix_sums, mix_partial;         // gs_mixture_*: their own work memory, read by nothing else
    DevBuf mixg_queries, mixg_partial, mixg_sums, mixg_x_partial;   // gs_mixture_*_backward: theirs (and mix_records, mix_sums)
    std::vector<struct ResampleTable*> resample_tables;   // gs_image_resample: the tables of the geometries seen, oldest first
    GsCounters* host_counters = nullptr;   // pinned, device-visible, GS_COUNTER_SLOTS of them; written by gs_publish_counters (k_keygen's last block or k_scan_tiles_publish)
    GsCounters* host_counters_dev = nullptr;   // the device's address of it
    uint64_t slots_busy = 1ull;            // slot 0 serves the calls that wait at once; the others belong to frames begun and not yet read
    int32_t ticket = 0;                    // sequence number of the last forward
    int64_t counter_wait_ns = 0;           // host time spent waiting for frame counters so far (gs_ctx_counter_wait_ns)
    // Predicted sizing of the per-pixel half (run_forward_tail): what the last frame of this ctx needed, for an image of this
    // size.  The next frame's binning, sort and blend are queued on it without waiting for the frame's own counters.
    struct { bool valid = false; int H = 0, W = 0; uint32_t K = 0; int max_code = 0; } seen;
    // dispatch orders for the forward blend: the view table (gs_common.h), view_S slots of view_T tiles each, every filled one a complete
    // permutation of [0, view_T) written by k_tile_order.  Laid out (and emptied) by the first forward with another tile count or slot
    // count (gs_api.hip: view_table); view_epoch counts the layouts, and a frame of an earlier one writes nothing.  A hint only moves work in time.
    DevBuf view_table;
    int view_T = 0, view_S = 0;
    uint32_t view_epoch = 0;
    // stream hand-over: the scratch above is recycled in stream order, so work arriving on another stream waits for
    // everything issued on the previous one
    bool has_stream = false;
    hipStream_t last_stream = nullptr;
    hipEvent_t switch_event = nullptr;
};

// Entering a call that launches on stream s (mutex held).
static hipError_t enter_stream(gs_ctx* c, hipStream_t s)
{
    if (c->has_stream && c->last_stream != s) {
        hipError_t e = hipEventRecord(c->switch_event, c->last_stream);
        if (e != hipSuccess) return e;
        e = hipStreamWaitEvent(s, c->switch_event, 0);
        if (e != hipSuccess) return e;
    }
    c->has_stream = true; c->last_stream = s;
    return hipSuccess;
}

// The prologue of every call that launches work (mutex held), after the checks that can refuse the call: the ctx's device,
// then the stream hand-over.  *s_out = the call's stream.
static int enter_call(gs_ctx* c, gs_stream stream_, hipStream_t* s_out)
{
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream_);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(enter_stream(c, s));
    *s_out = s;
    return GS_OK;
}

// A buffer a stage grows before it queues anything; the out-of-memory error names the first one that cannot grow.
struct Need { DevBuf* buf; size_t bytes; const char* name; };
#define NEED(buf, bytes) Need{ &(buf), (bytes), #buf }

static int grow(gs_ctx* c, const char* who, std::initializer_list<Need> needs)
{
    for (const Need& n : needs)
        if (n.buf->ensure(n.bytes, &c->device_bytes) != hipSuccess)
            return fail(GS_ERR_OUT_OF_MEMORY, who, std::string("device allocation failed: ") + n.name);
    return GS_OK;
}

// A call that holds no frame, after its argument checks: the ctx's lock, its device, the scratch it grows (before the stream
// enters: a call that fails here leaves the stream alone), the stream hand-over, the launch, the launch's error.  `launch` takes
// the call's hipStream_t; a call with nothing to grow passes {}, and a buffer it needs only sometimes with 0 bytes.
template <typename Launch>
static int queued_call(gs_ctx* c, gs_stream stream_, const char* who, std::initializer_list<Need> needs, Launch&& launch)
{
    std::lock_guard<std::mutex> lock(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (const int rc = grow(c, who, needs)) return rc;
    hipStream_t s;
    if (const int rc = enter_call(c, stream_, &s)) return rc;
    launch(s);
    HIP_TRY(hipGetLastError());
    return GS_OK;
}

