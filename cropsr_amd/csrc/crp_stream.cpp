// crp_stream.cpp -- seam 1 as a PIPELINE: crp_scan_stream of the C ABI (include/cropsr_hip.h).
//
// The reference's loop is per contig (CROPSR.py:409-474: scan, score, write, next): it produces and consumes as it goes.
// The arena calls of the ABI take all contigs, scan once and then hand the tables over -- upload, scan and fetch strictly one
// after the other, the full-duplex host link used in one direction at a time.  Here the genome goes through in SLICES
// (crp_plan.cpp plan_slices: whole contigs while they fit, a contig longer than a slice cut with CRP_HALO characters of
// context either side, a hit owned by the piece its match index falls in -- crp_node.cpp packs a device's share by it too), every
// slice in an arena of its own (LANES: a few reusable arenas, slice k in lane k mod L), and three host threads keep three
// HIP streams busy -- one stream per DIRECTION of the link, because that is what lets the two directions run at the same
// time (profiles/microbench/duplex_copy.hip: 48 + 48 GB/s on two one-way streams, 56 GB/s in all when every stream carries
// both directions in turn):
//
//     uploader (the calling thread)   UP stream:   slice k + 2: host pages -> pinned staging -> H2D -> pack kernel -> the
//                                                  scan, queued behind it; an event marks the scan
//     drainer  (a helper thread)      CUT stream:  slice k + 1: wait for the scan's event, cut the owned rows (lower_bound
//                                                  kernel), rebase to contig-local positions;
//                                     DOWN stream: the D2H of the owned rows, behind an event of the CUT stream -- straight
//                                                  into the caller's tables when those are pinned, else into pinned landing
//                                                  buffers
//     copier   (a helper thread)                   slice k: when its D2H has landed, copy it out of the landing buffers into
//                                                  its place in the caller's (pageable) tables with a few threads, and hand
//                                                  the lane back
//
// What comes back is ONE table per strand, contig after contig, ascending inside a contig, positions local to the contig
// string: the reference's own order (CROPSR.py:417-434), bit for bit what crp_scan_score + a host-side split by contig give.
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "crp_internal.h"
#include "crp_plan.h"
#include "crp_roctx.h"

namespace {

constexpr int N_LAND = 4;  // pinned landing buffers of STAGE_CHUNK bytes each (pageable tables only)

struct Lane {
    crp_arena *arena = nullptr;
    uint64_t arena_words = 0;
    uint32_t *d_needles = nullptr, *d_bounds = nullptr, *d_map = nullptr;
    uint64_t needles_cap = 0, bounds_cap = 0, map_cap = 0;
    uint32_t *h_small = nullptr;  // pinned: needles (2 np) | map (2 np) | bounds (4 np)
    uint64_t h_small_cap = 0;     // in pieces
    uint32_t *d_lpos[2] = {nullptr, nullptr};
    uint64_t lpos_cap[2] = {0, 0};
    hipEvent_t scanned = nullptr;  // UP stream: this lane's scan is behind here
    hipEvent_t cut = nullptr;      // CUT stream: the rebased positions are in place
    hipEvent_t down = nullptr;     // DOWN stream: the slice's last copy is behind here
};

// a batch of D2H copies queued on the DOWN stream: at most one landing buffer's worth
struct CopyJob {
    size_t slice = 0, lane = 0;
    int buf = -1;  // the landing buffer the segments arrive in; -1: the copies go straight into pinned tables
    struct Seg {
        size_t land_off;
        void *dst;
        size_t bytes;
    } seg[8];
    int n_seg = 0;
    bool last_of_slice = false;
};

using crp::Piece;

struct Slice {
    size_t first_piece = 0, n_pieces = 0;
};

// one column of a slice's owned rows on its way down
struct Col {
    const uint8_t *d_src;
    uint8_t *dst;
    size_t bytes;
};

double seconds_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

struct crp_stream_state {
    std::vector<Lane> lanes;
    hipStream_t s_cut = nullptr, s_down = nullptr;  // (the UP stream is the context's own)
    uint8_t *land[N_LAND] = {};
    hipEvent_t landed[N_LAND] = {};
    bool land_free[N_LAND] = {};  // guarded by Shared::m during a call
};

namespace crp {

void stream_release(crp_ctx *ctx)
{
    crp_stream_state *st = ctx->stream_state;
    if (!st) return;
    ctx->stream_state = nullptr;
    (void)hipSetDevice(ctx->device);
    if (st->s_cut) (void)hipStreamSynchronize(st->s_cut);
    if (st->s_down) (void)hipStreamSynchronize(st->s_down);
    for (Lane &l : st->lanes) {
        if (l.arena) (void)crp_arena_destroy(l.arena);
        (void)hipFree(l.d_needles);
        (void)hipFree(l.d_bounds);
        (void)hipFree(l.d_map);
        (void)hipFree(l.d_lpos[0]);
        (void)hipFree(l.d_lpos[1]);
        if (l.h_small) (void)hipHostFree(l.h_small);
        if (l.scanned) (void)hipEventDestroy(l.scanned);
        if (l.cut) (void)hipEventDestroy(l.cut);
        if (l.down) (void)hipEventDestroy(l.down);
    }
    for (int b = 0; b < N_LAND; ++b) {
        if (st->land[b]) (void)hipHostFree(st->land[b]);
        if (st->landed[b]) (void)hipEventDestroy(st->landed[b]);
    }
    if (st->s_cut) (void)hipStreamDestroy(st->s_cut);
    if (st->s_down) (void)hipStreamDestroy(st->s_down);
    delete st;
}

}  // namespace crp

namespace {

size_t lanes_wanted()
{
    if (const char *e = std::getenv("CRP_STREAM_LANES")) return (size_t)std::max(2, std::min(8, std::atoi(e)));
    return 4;
}

uint64_t slice_words_for(uint64_t slice_chars)
{
    if (!slice_chars) slice_chars = 64ull << 20;
    return std::min<uint64_t>(crp_arena_max_words(), std::max<uint64_t>(crp::slice_words_min(CRP_HALO), slice_chars / 64 + 2));
}

int small_host_buffer(crp_ctx *ctx, Lane &l, uint64_t np)
{
    if (l.h_small_cap >= np && l.h_small) return CRP_OK;
    if (l.h_small) (void)hipHostFree(l.h_small);
    l.h_small = nullptr;
    l.h_small_cap = 0;
    const uint64_t cap = np + np / 2 + 1024;
    CRP_HIP(ctx, hipHostMalloc(reinterpret_cast<void **>(&l.h_small), 8 * cap * sizeof(uint32_t), hipHostMallocDefault));
    l.h_small_cap = cap;
    return CRP_OK;
}

// a lane's buffers for the ownership cuts of a slice of np pieces: the pinned scratch, the needles, their bounds, the piece map
int cut_buffers(crp_ctx *ctx, Lane &l, uint64_t np)
{
    int rc = small_host_buffer(ctx, l, np);
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&l.d_needles), &l.needles_cap, 2 * np, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&l.d_bounds), &l.bounds_cap, 4 * np, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&l.d_map), &l.map_cap, 2 * np, sizeof(uint32_t));
    return rc;
}

// the two further streams, `want` lanes with an arena of exactly slice_words each (tables and per-lane buffers sized for a
// full slice now: a lane's first slice must not stall the pipeline on an allocation), and -- for pageable tables -- the
// landing buffers
int ensure_lanes(crp_ctx *ctx, size_t want, uint64_t slice_words, bool landing)
{
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->stream_state) {
        ctx->stream_state = new (std::nothrow) crp_stream_state();
        if (!ctx->stream_state) return CRP_ERR_NOMEM;
    }
    crp_stream_state *st = ctx->stream_state;
    if (!st->s_cut) CRP_HIP(ctx, hipStreamCreateWithFlags(&st->s_cut, hipStreamNonBlocking));
    if (!st->s_down) CRP_HIP(ctx, hipStreamCreateWithFlags(&st->s_down, hipStreamNonBlocking));
    if (st->lanes.size() < want) st->lanes.resize(want);
    for (size_t k = 0; k < want; ++k) {
        Lane &l = st->lanes[k];
        if (l.arena && l.arena_words < slice_words) {  // (a roomier arena than asked for serves as well)
            (void)crp_arena_destroy(l.arena);
            l.arena = nullptr;
        }
        if (!l.arena) {
            int rc = crp_arena_create(ctx, slice_words, &l.arena);
            if (rc != CRP_OK) return rc;
            l.arena_words = slice_words;
            const uint64_t chars = slice_words * 64;
            rc = crp::arena_reserve_tables(l.arena, chars, false);
            for (int s = 0; s < 2 && rc == CRP_OK; ++s)
                rc = crp::grow(ctx, reinterpret_cast<void **>(&l.d_lpos[s]), &l.lpos_cap[s], chars / 8 + 1024, sizeof(uint32_t));
            if (rc == CRP_OK) rc = cut_buffers(ctx, l, 4096);
            if (rc != CRP_OK) return rc;
        }
        if (!l.scanned) CRP_HIP(ctx, hipEventCreateWithFlags(&l.scanned, hipEventDisableTiming));
        if (!l.cut) CRP_HIP(ctx, hipEventCreateWithFlags(&l.cut, hipEventDisableTiming));
        if (!l.down) CRP_HIP(ctx, hipEventCreateWithFlags(&l.down, hipEventDisableTiming));
    }
    for (int b = 0; b < N_LAND; ++b)
        if (!st->landed[b]) CRP_HIP(ctx, hipEventCreateWithFlags(&st->landed[b], hipEventDisableTiming));
    for (int b = 0; b < N_LAND && landing; ++b)  // (crp_scan_stream_prepare; a scan allocates them as it first needs them)
        if (!st->land[b]) CRP_HIP(ctx, hipHostMalloc(reinterpret_cast<void **>(&st->land[b]), crp::STAGE_CHUNK, hipHostMallocDefault));
    return CRP_OK;
}

struct Shared {
    std::mutex m;
    std::condition_variable cv;
    size_t launched = 0, drained = 0;
    std::vector<CopyJob> jobs;  // drainer -> copier, in order
    size_t jobs_taken = 0;
    bool drainer_done = false;
    int failed = CRP_OK;
    std::string error;
};

void fail(Shared &sh, int rc, const std::string &what)
{
    std::lock_guard<std::mutex> lk(sh.m);
    if (sh.failed == CRP_OK) {
        sh.failed = rc;
        sh.error = what;
    }
    sh.cv.notify_all();
}

// One crp_scan_stream call: the state its three threads share -- the uploader (the calling thread), the drainer and the copier
// (the head of this file) -- grouped by the thread that writes it.  LANE k mod n_lanes goes round with slice k: the uploader's
// until sh.launched > k, then the drainer's and (its `down` event, its number in a CopyJob) the copier's, until sh.drained > k
// hands it back to the uploader.
struct StreamRun {
    // ---- written by the calling thread before the helpers start (the constructor, plan, open_lanes); read-only to all three after
    crp_ctx *const ctx;
    const uint8_t *const *const texts;
    const int guide_len;
    const bool want_pre;
    uint32_t *const host_pos[2];
    double *const host_score[2];
    const uint64_t host_cap[2];
    const std::chrono::steady_clock::time_point t_call = std::chrono::steady_clock::now();
    std::vector<Piece> pieces;  // in contig order, slice by slice
    std::vector<Slice> slices;
    bool tables_pinned = false;  // pinned tables (crp_host_alloc) take the rows by DMA directly; anything else goes through the landing buffers
    size_t n_lanes = 0;
    crp_stream_state *st = nullptr;  // (its land[] slots are filled by the drainer as it first needs them)

    // ---- guarded by sh.m, any thread: the pipeline's counters, the job queue, the first failure -- and with them
    // st->land_free[] and t_first_drained (the copier writes it; read after the join)
    Shared sh;
    double t_first_drained = 0;

    // ---- the uploader's alone; the timers are read after the join
    double up_busy = 0, up_wait = 0;
    std::vector<const uint8_t *> ptrs;
    std::vector<uint64_t> plen, offs;

    // ---- the drainer's alone (per_contig: what it points to); read by the calling thread after the join
    uint64_t *const per_contig;
    uint64_t prefix[2] = {0, 0};  // rows so far, per strand: where the next slice's rows go
    bool overflow = false;
    double drain_busy = 0, drain_wait = 0;
    int next_land = 0;  // the landing ring's next buffer
    std::vector<uint32_t> counts;

    // ---- the copier's alone; read after the join
    double copy_busy = 0, copy_wait = 0;
    uint64_t copied = 0;

    StreamRun(crp_ctx *c, const uint8_t *const *t, int gl, bool pre, uint32_t *pos_plus, double *score_plus, uint64_t cap_plus, uint32_t *pos_minus,
              double *score_minus, uint64_t cap_minus, uint64_t *pc)
        : ctx(c), texts(t), guide_len(gl), want_pre(pre), host_pos{pos_plus, pos_minus}, host_score{score_plus, score_minus},
          host_cap{cap_plus, cap_minus}, per_contig(pc)
    {
    }

    Lane &lane(size_t k) { return st->lanes[k % n_lanes]; }

    void hip_fail(hipError_t e, const char *what)
    {
        fail(sh, e == hipErrorOutOfMemory ? CRP_ERR_NOMEM : CRP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    }

    // a thread's loop; nothing may leave it but through `fail`
    template <class F>
    void guarded(const char *what, F loop)
    {
        try {
            loop();
        } catch (...) {
            fail(sh, CRP_ERR_NOMEM, what);
        }
    }

    // ---- the plan: pieces in contig order, slice by slice
    void plan(const uint64_t *lens, uint64_t n, uint64_t slice_words)
    {
        crp::plan_slices(lens, n, slice_words, CRP_HALO, pieces);
        for (size_t q = 0; q < pieces.size(); ++q) {
            const size_t k = (size_t)pieces[q].group;
            if (k >= slices.size()) {
                slices.resize(k + 1);
                slices[k].first_piece = q;
            }
            slices[k].n_pieces += 1;
        }
    }

    // where the rows go (pinned tables or the landing ring), and the lanes
    int open_lanes(uint64_t slice_words)
    {
        bool any_table = false;
        tables_pinned = true;
        for (int s = 0; s < 2; ++s) {
            if (host_pos[s] && host_cap[s]) any_table = true, tables_pinned = tables_pinned && crp::is_pinned_host(host_pos[s]);
            if (host_score[s] && host_cap[s]) any_table = true, tables_pinned = tables_pinned && crp::is_pinned_host(host_score[s]);
        }
        tables_pinned = tables_pinned && any_table;
        n_lanes = std::min<size_t>(lanes_wanted(), slices.size());
        // (a genome smaller than a slice: the one lane it needs is sized for it, not for 64 Mi characters)
        uint64_t lane_words = slice_words;
        if (slices.size() == 1) {
            uint64_t need = 1;
            for (const Piece &p : pieces) need += crp_arena_words_for(p.text_len);
            lane_words = std::max<uint64_t>(crp::slice_words_min(CRP_HALO), std::min(slice_words, need + 1));
        }
        const int rc = ensure_lanes(ctx, n_lanes, lane_words, false);
        if (rc != CRP_OK) return rc;
        st = ctx->stream_state;
        for (int b = 0; b < N_LAND; ++b) st->land_free[b] = true;
        return CRP_OK;
    }

    // ---- the uploader: slice k into its lane, the scan queued behind it
    bool upload_slice(size_t k)
    {
        {
            const auto t0 = std::chrono::steady_clock::now();
            std::unique_lock<std::mutex> lk(sh.m);
            sh.cv.wait(lk, [&] { return sh.drained + n_lanes > k || sh.failed != CRP_OK; });  // lane k mod n_lanes is free again
            up_wait += seconds_since(t0);
            if (sh.failed != CRP_OK) return false;
        }
        const auto t0 = std::chrono::steady_clock::now();
        Lane &l = lane(k);
        const Slice &sl = slices[k];
        const size_t np = sl.n_pieces;
        ptrs.resize(np);
        plen.resize(np);
        offs.resize(np);
        for (size_t j = 0; j < np; ++j) {
            const Piece &p = pieces[sl.first_piece + j];
            ptrs[j] = texts[p.contig] + p.text_lo;
            plen[j] = p.text_len;
        }
        int r = crp::arena_reset(l.arena);
        if (r == CRP_OK) r = crp_arena_add_contigs_ascii(l.arena, ptrs.data(), plen.data(), np, offs.data());
        if (r == CRP_OK) r = crp::arena_seal_async(l.arena);
        if (r == CRP_OK) r = crp::scan_begin(l.arena, guide_len, want_pre ? CRP_SCAN_PRE : 0);
        if (r == CRP_OK) r = cut_buffers(ctx, l, np);
        if (r != CRP_OK) {
            fail(sh, r, std::string("upload of slice ") + std::to_string(k) + ": " + crp_last_error(ctx));
            return false;
        }
        // the ownership needles and the piece map of this slice: written into the lane's pinned scratch, uploaded behind the scan
        uint32_t *needles = l.h_small, *map = l.h_small + 2 * l.h_small_cap;
        crp::piece_cuts(&pieces[sl.first_piece], np, offs.data(), needles, map);
        hipError_t e = hipMemcpyAsync(l.d_needles, needles, 2 * np * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(l.d_map, map, 2 * np * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipEventRecord(l.scanned, ctx->stream);
        if (e != hipSuccess) {
            hip_fail(e, "slice set-up");
            return false;
        }
        up_busy += seconds_since(t0);
        {
            std::lock_guard<std::mutex> lk(sh.m);
            sh.launched = k + 1;
        }
        sh.cv.notify_all();
        return true;
    }

    // ---- the drainer: slice k's owned rows cut, rebased and queued for the way down
    bool drain_slice(size_t k)
    {
        {
            std::unique_lock<std::mutex> lk(sh.m);
            sh.cv.wait(lk, [&] { return sh.launched > k || sh.failed != CRP_OK; });
            if (sh.failed != CRP_OK) return false;
        }
        Lane &l = lane(k);
        const Slice &sl = slices[k];
        crp_arena *a = l.arena;
        hipError_t e = hipSetDevice(ctx->device);
        if (e == hipSuccess) e = hipEventSynchronize(l.scanned);  // the upload and the scan of THIS slice, nothing behind them
        if (e != hipSuccess) return hip_fail(e, "waiting for a slice's scan"), false;
        const auto t0 = std::chrono::steady_clock::now();
        uint64_t x = 0, y = 0;
        int r = crp::scan_finish(a, &x, &y, true);
        if (r != CRP_OK) {
            fail(sh, r, std::string("scan of slice ") + std::to_string(k) + ": " + crp_last_error(ctx));
            return false;
        }
        const size_t np = sl.n_pieces;
        const uint32_t nn = (uint32_t)(2 * np);
        uint32_t *h_bounds = l.h_small + 4 * l.h_small_cap;
        for (int s = 0; s < 2 && e == hipSuccess; ++s)
            e = crp::launch_lower_bound(st->s_cut, a->d_pos[s], a->n_hits[s], l.d_needles, nn, l.d_bounds + (size_t)s * nn);
        if (e == hipSuccess) e = hipMemcpyAsync(h_bounds, l.d_bounds, 2 * (size_t)nn * sizeof(uint32_t), hipMemcpyDeviceToHost, st->s_cut);
        if (e == hipSuccess) e = hipStreamSynchronize(st->s_cut);
        if (e != hipSuccess) return hip_fail(e, "ownership cuts"), false;
        // what goes down: per strand the rebased positions and the f64 column of the owned run
        Col cols[4];
        int n_cols = 0;
        counts.resize(np);
        for (int s = 0; s < 2; ++s) {
            uint64_t first = 0, last = 0;
            if (!crp::owned_run(h_bounds + (size_t)s * 2 * np, np, &first, &last, counts.data())) {
                fail(sh, CRP_ERR_STATE, "crp_scan_stream: the owned rows of slice " + std::to_string(k) + " are not one run");
                return false;
            }
            for (size_t j = 0; j < np && per_contig; ++j) per_contig[2 * pieces[sl.first_piece + j].contig + (size_t)s] += counts[j];
            const uint64_t cnt = last - first, off = prefix[s];
            prefix[s] += cnt;
            if (!cnt) continue;
            if (!host_pos[s] && !host_score[s]) continue;  // (this strand's columns are not wanted)
            if (off + cnt > host_cap[s]) {  // the caller's tables are too small: the totals are still counted to the end
                overflow = true;
                continue;
            }
            if (host_pos[s]) {
                if (l.lpos_cap[s] < cnt) {  // (denser than the lane was sized for; the hipFree inside grow waits for the device)
                    r = crp::grow(ctx, reinterpret_cast<void **>(&l.d_lpos[s]), &l.lpos_cap[s], cnt, sizeof(uint32_t));
                    if (r != CRP_OK) {
                        fail(sh, r, std::string("rebased positions: ") + crp_last_error(ctx));
                        return false;
                    }
                }
                e = crp::launch_pos_rebase(st->s_cut, a->d_pos[s] + first, cnt, crp::PieceMap{l.d_map, l.d_map + np, (uint32_t)np}, l.d_lpos[s]);
                if (e != hipSuccess) return hip_fail(e, "rebase kernel"), false;
                cols[n_cols++] = Col{reinterpret_cast<const uint8_t *>(l.d_lpos[s]), reinterpret_cast<uint8_t *>(host_pos[s] + off), cnt * sizeof(uint32_t)};
            }
            if (host_score[s])
                cols[n_cols++] = Col{reinterpret_cast<const uint8_t *>((want_pre ? a->d_pre[s] : a->d_score[s]) + first),
                                     reinterpret_cast<uint8_t *>(host_score[s] + off), cnt * sizeof(double)};
        }
        if (!queue_columns(k, cols, n_cols)) return false;
        drain_busy += seconds_since(t0);
        return true;
    }

    // The copies of slice k's columns, queued on the DOWN stream behind the CUT stream's kernels -- nothing here waits for them:
    // the copier does, and hands the lane back.  Pageable tables: through the landing ring, a CopyJob per buffer's worth.
    bool queue_columns(size_t k, const Col *cols, int n_cols)
    {
        Lane &l = lane(k);
        hipError_t e = hipEventRecord(l.cut, st->s_cut);
        if (e == hipSuccess) e = hipStreamWaitEvent(st->s_down, l.cut, 0);
        if (e != hipSuccess) return hip_fail(e, "ordering the copies behind the cuts"), false;
        CopyJob job;
        job.slice = k;
        job.lane = k % n_lanes;
        size_t land_used = 0;
        for (int ci = 0; ci < n_cols; ++ci) {
            size_t done = 0;
            while (done < cols[ci].bytes) {
                if (tables_pinned) {
                    e = hipMemcpyAsync(cols[ci].dst, cols[ci].d_src, cols[ci].bytes, hipMemcpyDeviceToHost, st->s_down);
                    if (e != hipSuccess) return hip_fail(e, "D2H into pinned tables"), false;
                    done = cols[ci].bytes;
                    continue;
                }
                if (job.buf < 0) {  // the next landing buffer of the ring, once the copier has emptied it
                    const auto tw = std::chrono::steady_clock::now();
                    std::unique_lock<std::mutex> lk(sh.m);
                    sh.cv.wait(lk, [&] { return st->land_free[next_land] || sh.failed != CRP_OK; });
                    if (sh.failed != CRP_OK) return false;
                    st->land_free[next_land] = false;
                    lk.unlock();
                    drain_wait += seconds_since(tw);
                    job.buf = next_land;
                    next_land = (next_land + 1) % N_LAND;
                    land_used = 0;
                    if (!st->land[job.buf]) {  // (a small genome never needs more than the first)
                        e = hipHostMalloc(reinterpret_cast<void **>(&st->land[job.buf]), crp::STAGE_CHUNK, hipHostMallocDefault);
                        if (e != hipSuccess) return hip_fail(e, "landing buffer"), false;
                    }
                }
                const size_t take = std::min(cols[ci].bytes - done, crp::STAGE_CHUNK - land_used);
                e = hipMemcpyAsync(st->land[job.buf] + land_used, cols[ci].d_src + done, take, hipMemcpyDeviceToHost, st->s_down);
                if (e != hipSuccess) return hip_fail(e, "D2H into a landing buffer"), false;
                job.seg[job.n_seg++] = CopyJob::Seg{land_used, cols[ci].dst + done, take};
                done += take;
                land_used = (land_used + take + 63) & ~(size_t)63;
                if (land_used >= crp::STAGE_CHUNK || job.n_seg == 8)
                    if (!submit(job, false)) return false;
            }
        }
        return submit(job, true);
    }

    // the events behind what `job` has queued, the job to the copier, and a fresh job of the same slice in its place
    bool submit(CopyJob &job, bool last)
    {
        job.last_of_slice = last;
        hipError_t e = hipSuccess;
        if (job.buf >= 0) e = hipEventRecord(st->landed[job.buf], st->s_down);
        if (e == hipSuccess && last) e = hipEventRecord(st->lanes[job.lane].down, st->s_down);
        if (e != hipSuccess) return hip_fail(e, "landing event"), false;
        {
            std::lock_guard<std::mutex> lk(sh.m);
            sh.jobs.push_back(job);
        }
        sh.cv.notify_all();
        job.buf = -1;
        job.n_seg = 0;
        return true;
    }

    // ---- the copier: one job's segments out of its landing buffer into the caller's tables, then the buffer and the lane back
    bool copy_job(const CopyJob &job)
    {
        const auto t_wait = std::chrono::steady_clock::now();
        hipError_t e = hipSetDevice(ctx->device);
        if (e == hipSuccess && job.buf >= 0) e = hipEventSynchronize(st->landed[job.buf]);
        if (e == hipSuccess && job.last_of_slice) e = hipEventSynchronize(st->lanes[job.lane].down);
        if (e != hipSuccess) {
            fail(sh, CRP_ERR_HIP, std::string("waiting for a slice's tables: ") + hipGetErrorString(e));
            return false;
        }
        copy_wait += seconds_since(t_wait);
        const auto t0 = std::chrono::steady_clock::now();
        crp::CopySeg segs[8];
        for (int i = 0; i < job.n_seg; ++i) {
            copied += job.seg[i].bytes;
            segs[i] = crp::CopySeg{job.seg[i].dst, st->land[job.buf] + job.seg[i].land_off, job.seg[i].bytes};
        }
        crp::parallel_copy_multi(segs, job.n_seg, ctx->copy_threads);
        copy_busy += seconds_since(t0);
        {
            std::lock_guard<std::mutex> lk(sh.m);
            if (job.buf >= 0) st->land_free[job.buf] = true;
            if (job.last_of_slice) {
                sh.drained = job.slice + 1;
                if (job.slice == 0) t_first_drained = seconds_since(t_call);
            }
        }
        sh.cv.notify_all();
        return true;
    }

    // the drainer's thread: slice after slice, in order
    void drain_all()
    {
        guarded("crp_scan_stream: out of host memory while draining", [this] {
            for (size_t k = 0; k < slices.size(); ++k)
                if (!drain_slice(k)) return;
        });
        {
            std::lock_guard<std::mutex> lk(sh.m);
            sh.drainer_done = true;
        }
        sh.cv.notify_all();
    }

    // the copier's thread: job after job, in order
    void copy_all()
    {
        guarded("crp_scan_stream: out of host memory while copying", [this] {
            for (;;) {
                CopyJob job;
                {
                    std::unique_lock<std::mutex> lk(sh.m);
                    sh.cv.wait(lk, [&] { return sh.jobs_taken < sh.jobs.size() || sh.drainer_done || sh.failed != CRP_OK; });
                    if (sh.failed != CRP_OK) return;
                    if (sh.jobs_taken == sh.jobs.size()) return;  // (the drainer is done and so is its queue)
                    job = sh.jobs[sh.jobs_taken++];
                }
                if (!copy_job(job)) return;
            }
        });
    }

    // The three threads, until every slice is through or one of them has failed.  The status and, on a failure, ctx->last_error.
    int run()
    {
        std::thread drainer, copier;
        try {
            sh.jobs.reserve(4 * slices.size() + 8);
            drainer = std::thread([this] { drain_all(); });
            copier = std::thread([this] { copy_all(); });
        } catch (...) {
            fail(sh, CRP_ERR_NOMEM, "crp_scan_stream: no helper thread to be had");
            if (drainer.joinable()) drainer.join();
            ctx->last_error = "crp_scan_stream: no helper thread to be had";
            return CRP_ERR_NOMEM;
        }
        guarded("crp_scan_stream: out of host memory while uploading", [this] {
            for (size_t k = 0; k < slices.size(); ++k)
                if (!upload_slice(k)) return;
        });
        drainer.join();
        copier.join();
        if (sh.failed == CRP_OK) return CRP_OK;
        // whatever is still queued must not outlive this call (the caller's texts and tables are its to free)
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipStreamSynchronize(st->s_cut);
        (void)hipStreamSynchronize(st->s_down);
        for (size_t k = 0; k < n_lanes; ++k) st->lanes[k].arena->scan_pending = 0;
        ctx->last_error = sh.error;
        return sh.failed;
    }

    void write_stats(double *stats) const  // stats[0..11], in the order include/cropsr_hip.h gives them
    {
        const double v[12] = {seconds_since(t_call), up_busy,   drain_busy, (double)slices.size(), (double)n_lanes, t_first_drained,
                              up_wait,               drain_wait, copy_busy,  copy_wait,             (double)copied,  tables_pinned ? 1.0 : 0.0};
        std::memcpy(stats, v, sizeof v);
    }
};

}  // namespace

extern "C" {

int crp_host_alloc(uint64_t bytes, void **out)
{
    if (!out) return CRP_ERR_INVALID;
    *out = nullptr;
    if (!bytes) return CRP_OK;
    const hipError_t e = hipHostMalloc(out, bytes, hipHostMallocPortable);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *out = nullptr;
        return e == hipErrorOutOfMemory ? CRP_ERR_NOMEM : CRP_ERR_HIP;
    }
    return CRP_OK;
}

int crp_host_free(void *p)
{
    if (p && hipHostFree(p) != hipSuccess) {
        (void)hipGetLastError();
        return CRP_ERR_INVALID;
    }
    return CRP_OK;
}

static int scan_stream_impl(crp_ctx *ctx, const uint8_t *const *texts, const uint64_t *lens, uint64_t n, int guide_len, int flags,
                            uint64_t slice_chars, uint32_t *pos_plus, double *score_plus, uint64_t cap_plus, uint32_t *pos_minus,
                            double *score_minus, uint64_t cap_minus, uint64_t *per_contig, uint64_t *n_plus, uint64_t *n_minus, double *stats)
{
    crp::Range roctx_range("crp: scan stream (H2D | scan | D2H pipelined)");
    if (!ctx || (n && (!texts || !lens)) || (flags & ~CRP_SCAN_PRE)) return CRP_ERR_INVALID;
    if (guide_len < 0 || guide_len > 50) return CRP_ERR_UNSUPPORTED;
    for (uint64_t k = 0; k < n; ++k) {
        if (lens[k] && !texts[k]) return CRP_ERR_INVALID;
        if (lens[k] > 0xFFFFFFFFull) {
            ctx->last_error = "crp_scan_stream: contig " + std::to_string(k) + " has more than 2^32 - 1 characters; positions are 32-bit";
            return CRP_ERR_CAPACITY;
        }
    }
    StreamRun run(ctx, texts, guide_len, (flags & CRP_SCAN_PRE) != 0, pos_plus, score_plus, cap_plus, pos_minus, score_minus, cap_minus, per_contig);
    const uint64_t slice_words = slice_words_for(slice_chars);
    run.plan(lens, n, slice_words);
    if (per_contig && n) std::memset(per_contig, 0, 2 * n * sizeof(uint64_t));
    if (n_plus) *n_plus = 0;
    if (n_minus) *n_minus = 0;
    if (stats) std::memset(stats, 0, 12 * sizeof(double));
    if (run.slices.empty()) return CRP_OK;
    int rc = run.open_lanes(slice_words);
    if (rc == CRP_OK) rc = run.run();
    if (rc != CRP_OK) return rc;
    if (n_plus) *n_plus = run.prefix[0];
    if (n_minus) *n_minus = run.prefix[1];
    if (stats) run.write_stats(stats);
    if (run.overflow) {
        ctx->last_error = "crp_scan_stream: the caller's tables are too small: " + std::to_string(run.prefix[0]) + " '+' and " + std::to_string(run.prefix[1]) + " '-' rows are needed";
        return CRP_ERR_CAPACITY;
    }
    return CRP_OK;
}

int crp_scan_stream(crp_ctx *ctx, const uint8_t *const *texts, const uint64_t *lens, uint64_t n, int guide_len, int flags, uint64_t slice_chars,
                    uint32_t *pos_plus, double *score_plus, uint64_t cap_plus, uint32_t *pos_minus, double *score_minus, uint64_t cap_minus,
                    uint64_t *per_contig, uint64_t *n_plus, uint64_t *n_minus, double *stats)
{
    try {  // (vectors, strings and threads: nothing may throw across the C ABI)
        return scan_stream_impl(ctx, texts, lens, n, guide_len, flags, slice_chars, pos_plus, score_plus, cap_plus, pos_minus, score_minus,
                                cap_minus, per_contig, n_plus, n_minus, stats);
    } catch (...) {
        return CRP_ERR_NOMEM;
    }
}

int crp_scan_stream_prepare(crp_ctx *ctx, uint64_t slice_chars)
{
    if (!ctx) return CRP_ERR_INVALID;
    try {
        return ensure_lanes(ctx, lanes_wanted(), slice_words_for(slice_chars), true);
    } catch (...) {
        return CRP_ERR_NOMEM;
    }
}

}  // extern "C"
