// exec.h -- private, host only, on top of ctx.h: what crosses the units that run a finalized plan (api.hip, forward.hip, pages.hip, whole.hip,
// comm.hip).  Everything else of those units stays in their anonymous namespaces.
#pragma once

#include "ctx.h"

namespace sbbseg {

// forward.hip
int run_plan(sbbseg_ctx* c, int n, uint8_t* d_labels, float* d_probs);                // the plan over n patches whose input forms are filled
int fill_ingest(sbbseg_ctx* c, IngestParams& ip);                                     // the input-form pointers of the lane in use
int resolve_pending(sbbseg_ctx* c);                                                   // profiling events still in flight -> the ops' totals
// api.hip
int labels_to_host(sbbseg_ctx* c, const void* d_plane, void* host, size_t pixels, int channels);
// pages.hip
void nearest_map(int src_len, int dst_len, std::vector<int>& m);                      // cv2.resize(..., INTER_NEAREST)'s index rule
int views_staging(sbbseg_ctx* c, size_t bytes);                                       // c->h_views / c->views hold `bytes`, the staging is free
// comm.hip
void comm_release(sbbseg_ctx* c);

// activation buffers and stream of lane L become the ones run_plan / fill_ingest see
struct LaneScope {
    sbbseg_ctx* c; hipStream_t saved;
    LaneScope(sbbseg_ctx* c_, int lane) : c(c_), saved(c_->stream)
    {
        if (lane == 1) {
            for (auto& t : c->tensors) t.buf = t.lane_buf[1];
            c->stream = c->lane_stream;
        }
    }
    ~LaneScope()
    {
        for (auto& t : c->tensors) t.buf = t.lane_buf[0];
        c->stream = saved;
    }
};

// the owned-region tables a chunk has set in c->rr (region_level_table) end with the chunk
struct RegionOff { sbbseg_ctx* c; ~RegionOff() { c->rr.on = false; } };

// the one-patch launches of run_plan may split their K range (launch_op) while this lives: the whole-image branch of one page.  Reset on every
// way out (a throwing run_plan included): later n == 1 launches must not split
struct KsplitScope {
    sbbseg_ctx* c;
    explicit KsplitScope(sbbseg_ctx* c_) : c(c_) { c->ksplit_now = c->ksplit; }
    ~KsplitScope() { c->ksplit_now = false; }
};

// A pooled list of n_tiles tiles, cut into launches: run_chunk(lane, first, nb) queues tiles [first, first + nb) on lane `lane`.
template <typename F>
int run_chunked(sbbseg_ctx* c, int n_tiles, F&& run_chunk)
{
    // chunks of equal size (108 tiles at max_batch 70 -> 54 + 54, not 70 + 38): launches shrink evenly.
    // (Profiling runs every launch alone on one lane: its chunks are capped at the size a LANE's launch has in normal operation -- half a
    // chunk -- so that the per-op times describe the launches the product runs, partial last rounds of the persistent grids included.)
    const int chunk_cap = (c->profiling && c->lanes == 2 && c->lane1_batch > 0 && c->max_batch >= 4 * kMinLaneTiles) ? (c->max_batch + 1) / 2 : c->max_batch;
    const int n_chunks = (n_tiles + chunk_cap - 1) / chunk_cap;
    const int chunk = n_chunks ? (n_tiles + n_chunks - 1) / n_chunks : 0;
    bool forked = false;
    for (int done = 0; done < n_tiles; done += chunk) {
        const int nb = n_tiles - done < chunk ? n_tiles - done : chunk;
        const bool two = c->lane1_batch > 0 && c->lanes == 2 && !c->profiling && nb >= 2 * kMinLaneTiles;
        if (!two) {
            if (forked) {                                       // (a one-lane chunk behind two-lane ones: lane 1 first)
                HIPCHK(hipEventRecord(c->ev_join, c->lane_stream));
                HIPCHK(hipStreamWaitEvent(c->stream, c->ev_join, 0));
                forked = false;
            }
            if (run_chunk(0, done, nb)) return 1;               // (not forked here: a fork in front was joined above)
            continue;
        }
        const int na = (nb + 1) / 2, nb2 = nb - na;            // nb2 <= lane1_batch
        // The lanes fork ONCE per tile range and join once behind its last chunk (round 5): a lane's halves of consecutive chunks follow each
        // other on the lane's own stream and buffers, nothing of one lane depends on the other.  (Up to round 4 every chunk forked and joined:
        // the lane that finished its half first waited for the other one -- 7-10 % of the timed region had ONE kernel in flight,
        // profiles/r05_timeline_gaps.txt.)
        if (!forked) {
            HIPCHK(hipEventRecord(c->ev_fork, c->stream));     // page / threshold / earlier ranges are ordered before
            HIPCHK(hipStreamWaitEvent(c->lane_stream, c->ev_fork, 0));
            forked = true;
        }
        // (a failure from here on must still join the lanes: earlier chunks of this range are in flight on lane_stream, unordered against
        //  whatever the caller does next on the handle's stream -- stitch, reuse of c->tile_labels, destroy)
        auto join_on_error = [&]() -> int {
            if (hipEventRecord(c->ev_join, c->lane_stream) != hipSuccess || hipStreamWaitEvent(c->stream, c->ev_join, 0) != hipSuccess)
                (void)hipStreamSynchronize(c->lane_stream);
            (void)hipGetLastError();
            return 1;
        };
        if (run_chunk(0, done, na)) return join_on_error();
        if (run_chunk(1, done + na, nb2)) return join_on_error();           // (starting lane 1 later -- after lane 0's op k -- measured 3-14 % slower)
    }
    if (forked) {
        HIPCHK(hipEventRecord(c->ev_join, c->lane_stream));
        HIPCHK(hipStreamWaitEvent(c->stream, c->ev_join, 0));
    }
    return 0;
}

}  // namespace sbbseg
