// crp_node.cpp -- ONE process over N GPUs: the node handle of the C ABI (include/cropsr_hip.h, crp_node_*).
//
// The reference is one process with one contig loop (CROPSR.py:333 main, :409 the loop).  SURVEY.md section 8(b) asks
// for a handle that lets that one process reach the whole node: "multi-GPU fan-out happens inside the library (one
// stream per device), not via Python threads".  This file is that handle:
//
//   crp_plan_shares      the cut: contigs, in order, dealt to the devices as contiguous equal shares (host code, crp_plan.cpp)
//   crp_node_load        one host thread per device uploads its share (pieces with CRP_HALO characters of context) into as
//                        many arenas as the share needs (an arena addresses fewer than 2^31 characters; the reference reads a
//                        genome of any size, CROPSR.py:59) -- a SLOT is one arena of a device and what the exchange keeps
//                        beside it
//   crp_node_scan_score  one host thread per device (alive as long as the node) launches and collects ITS device's scans:
//                        the N kernels leave the host side by side and run side by side
//   crp_node_gather      the path's one exchange.  Per slot a tiny kernel finds the OWNED rows of its tables (a hit belongs
//                        to the piece that contains its match index; with contiguous shares the owned rows of a slot are
//                        one run per strand), the peers pack their positions to 16 bits (CRP_GATHER_POS16), the rows cross
//                        xGMI -- RCCL in one process: ncclCommInitAll, then per peer ncclSend and at the root ncclRecv
//                        inside ONE group, every peer->root transfer on its own point-to-point link; or device-to-device
//                        copies the root pulls on one stream per peer -- and the root expands and rebases them into ONE
//                        table per strand, contig order, positions local to the contig string: the reference's own order
//                        (CROPSR.py:417-434), bit for bit what a single GPU produces.
//
// RCCL has no time-outs.  Every wait on it here has one: the communicators are created on a helper thread that is given
// CRP_NODE_COMM_INIT_TIMEOUT_S, the grouped exchange and the histogram all-reduce are awaited by polling an event against
// CRP_NODE_COLLECTIVE_TIMEOUT_S; a wait that runs out aborts the communicators, names its stage in crp_node_last_error, and --
// unless RCCL was asked for by name (CRP_NODE_TRANSPORT=rccl) -- the same call starts over on the device-to-device
// transport, from fresh state.
//
// The one-process-per-GPU path (crp_comm.cpp) is unchanged and shares the kernels (crp_gather.hip).
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "crp_gather_cols.h"
#include "crp_internal.h"
#include "crp_plan.h"
#include "crp_rccl.h"
#include "crp_roctx.h"

namespace {

// One arena of a device and what the gatherv keeps beside it.  The buffers only grow and outlive the genome (a node serves
// genome after genome); `arena` is what a load creates and the next one destroys.
struct NodeSlot {
    crp_arena *arena = nullptr;
    size_t piece0 = 0, n_pieces = 0;  // its pieces: [piece0, piece0 + n_pieces) of crp_node::pieces, arena order (= contig order)
    // ownership cuts: two needles per piece (begin and end of its owned arena positions), searched in both tables
    uint32_t *d_needles = nullptr, *d_bounds = nullptr;
    uint64_t needles_cap = 0, bounds_cap = 0;
    uint32_t *h_bounds = nullptr;  // pinned, 2 strands x needles
    uint64_t h_bounds_cap = 0;
    // sender side of CRP_GATHER_POS16
    uint16_t *d_lo16[2] = {nullptr, nullptr};
    uint32_t *d_bstart[2] = {nullptr, nullptr};
    uint64_t lo16_cap[2] = {0, 0}, bstart_cap[2] = {0, 0};
    uint32_t n_buckets = 0;
    // CRP_NODE_HOST_GATHER: this arena's own piece map {begin[], sub[]} and the rebased positions of its owned rows
    uint32_t *d_map_self = nullptr;
    uint64_t map_self_cap = 0;
    uint32_t *d_lpos[2] = {nullptr, nullptr};
    uint64_t lpos_cap[2] = {0, 0};
    // the current gather: owned rows [first, last) of each table, and where they go in the root's tables
    uint64_t first[2] = {0, 0}, last[2] = {0, 0}, foff[2] = {0, 0};
};

struct NodeDev {
    int device = -1;
    crp_ctx *ctx = nullptr;
    std::vector<std::unique_ptr<NodeSlot>> slots;  // [0, n_slots): the arenas of the current genome
    size_t n_slots = 0;
    hipEvent_t ready = nullptr;   // everything this device contributes to the current gather is in place
    hipEvent_t waitev = nullptr;  // what a bounded wait polls
};

// One host thread per device beyond the first, alive as long as the node: crp_node_scan_score hands every one of them the
// scans of ITS device (launch + wait) and runs the first device's itself, so the N launches leave the host side by side --
// queued one after the other from a single thread, the last device's kernel would start N - 1 launch latencies late, which
// is a sixth of a 60 us scan at N = 8.  (Threads started per call would cost more than they save.)
struct NodeWorker {
    std::thread th;
    std::mutex m;
    std::condition_variable wake, finished;
    int job = 0;  // 0 idle, 1 scan, 2 leave
    bool done = true;
    NodeDev *dev = nullptr;
    int guide_len = 0, flags = 0, rc = CRP_OK;
    uint64_t n[2] = {0, 0};

    static int scan_device(NodeDev &d, int gl, int fl, uint64_t out[2])
    {
        out[0] = out[1] = 0;
        for (size_t j = 0; j < d.n_slots; ++j) {  // (a device has more than one arena only beyond 2^31 characters)
            uint64_t x = 0, y = 0;
            int r = crp::scan_begin(d.slots[j]->arena, gl, fl);
            if (r == CRP_OK) r = crp::scan_finish(d.slots[j]->arena, &x, &y);
            if (r != CRP_OK) return r;
            out[0] += x;
            out[1] += y;
        }
        return CRP_OK;
    }
    void loop()
    {
        for (;;) {
            std::unique_lock<std::mutex> lk(m);
            wake.wait(lk, [&] { return job != 0; });
            if (job == 2) return;
            NodeDev *d = dev;
            const int gl = guide_len, fl = flags;
            lk.unlock();
            uint64_t x[2] = {0, 0};
            const int r = scan_device(*d, gl, fl, x);
            lk.lock();
            rc = r;
            n[0] = x[0];
            n[1] = x[1];
            job = 0;
            done = true;
            lk.unlock();
            finished.notify_one();
        }
    }
    void post(NodeDev *d, int gl, int fl)
    {
        {
            std::lock_guard<std::mutex> lk(m);
            dev = d;
            guide_len = gl;
            flags = fl;
            done = false;
            job = 1;
        }
        wake.notify_one();
    }
    int wait(uint64_t out[2])
    {
        std::unique_lock<std::mutex> lk(m);
        finished.wait(lk, [&] { return done; });
        out[0] = n[0];
        out[1] = n[1];
        return rc;
    }
    void leave()
    {
        if (!th.joinable()) return;
        {
            std::lock_guard<std::mutex> lk(m);
            job = 2;
        }
        wake.notify_one();
        th.join();
    }
};

inline uint64_t round_up8(uint64_t x) { return (x + 7) & ~(uint64_t)7; }

double ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

double env_seconds(const char *name, double dflt)
{
    const char *e = std::getenv(name);
    return e && *e ? std::atof(e) : dflt;
}

// communicator bootstraps of this process that never returned: their helper threads still sit inside RCCL
std::atomic<int> g_boot_stuck{0};

}  // namespace

struct crp_node {
    std::vector<NodeDev> dev;
    std::vector<std::unique_ptr<NodeWorker>> workers;  // [k]: device k's scan thread (none for device 0), started by the first scan
    // the pieces of the current genome, device after device and arena after arena (crp::Piece::group: which of its device's
    // arenas), and for each the arena offset of its text's first character (load_device)
    std::vector<crp::Piece> pieces;
    std::vector<uint64_t> arena_off;
    uint64_t n_contigs = 0;
    bool loaded = false;
    bool duplicates = false;  // a device listed twice: RCCL cannot be used
    int transport_env = 0;    // CRP_NODE_TRANSPORT: 0 unset, CRP_TRANSPORT_* ("rccl": RCCL or fail; "peer": never RCCL)
    bool try_rccl = false;    // CRP_NODE_TRANSPORT=try: RCCL is attempted even when a device is listed twice, and given up as usual
    int scan_threads_env = -1;  // CRP_NODE_SCAN_THREADS: -1 unset (threads unless a device is listed twice), 0 never, 1 always
    uint64_t arena_words = 0;   // most words one arena may hold (CRP_NODE_OPT_ARENA_WORDS; default crp_arena_max_words())
    double comm_init_timeout_s = 180.0, collective_timeout_s = 300.0;  // <= 0: wait without a bound
    int test_miscount = 0;      // test hook, environment CRP_TEST_NODE_MISCOUNT: the root posts one receive 8 bytes short
    // RCCL, one communicator per logical device, created by the first gather that uses it
    std::vector<ncclComm_t> comms;
    bool comms_tried = false;
    std::string comms_error;  // why RCCL is not (or no longer) in use; crp_node_transport_note
    // root side of the last gather
    int root = -1;        // the device the buffers below live on
    crp::GatherTables tables;  // ONE table per strand and column, contig order; the peers' packed positions slot by slot
    int gflags = 0;  // flags of the last gather (CRP_NODE_HOST_GATHER: the rows wait on their own devices)
    uint32_t *d_map = nullptr;  // every slot's piece map {begin[], sub[]}, slot after slot
    uint64_t map_cap = 0;
    std::vector<uint32_t> h_map;
    std::vector<hipStream_t> pull;  // root's streams for the device-to-device transport, one per peer
    std::vector<hipEvent_t> pulled;
    std::vector<uint64_t> contig_counts;  // 2 per contig
    uint64_t total[2] = {0, 0};
    bool have_gather = false;
    double ms_total = 0, ms_exchange = 0;
    uint64_t bytes_to_root = 0;
    int transport = 0;
    std::string last_error;
};

#define NODE_HIP(node, call)                                                                 \
    do {                                                                                     \
        hipError_t e__ = (call);                                                             \
        if (e__ != hipSuccess) {                                                             \
            (node)->last_error = std::string(#call) + ": " + hipGetErrorString(e__);         \
            return e__ == hipErrorOutOfMemory ? CRP_ERR_NOMEM : CRP_ERR_HIP;                 \
        }                                                                                    \
    } while (0)

namespace {

// a status from a per-device call: its context's text becomes the node's
int dev_fail(crp_node *node, int k, int rc, const char *what)
{
    if (rc != CRP_OK)
        node->last_error = std::string(what) + " on logical device " + std::to_string(k) + ": " + crp_strerror(rc) + " [" +
                           crp_last_error(node->dev[(size_t)k].ctx) + "]";
    return rc;
}

struct SlotRef {
    int k;          // logical device
    NodeSlot *sl;
    size_t flat;    // index among the node's active slots, device after device
};

std::vector<SlotRef> active_slots(crp_node *node)
{
    std::vector<SlotRef> out;
    for (size_t k = 0; k < node->dev.size(); ++k)
        for (size_t j = 0; j < node->dev[k].n_slots; ++j) out.push_back(SlotRef{(int)k, node->dev[k].slots[j].get(), out.size()});
    return out;
}

void free_pull_streams(crp_node *node)
{
    for (hipStream_t st : node->pull)
        if (st) (void)hipStreamDestroy(st);
    for (hipEvent_t ev : node->pulled)
        if (ev) (void)hipEventDestroy(ev);
    node->pull.clear();
    node->pulled.clear();
}

void free_root_side(crp_node *node)
{
    if (node->root < 0) return;
    (void)hipSetDevice(node->dev[(size_t)node->root].device);
    node->tables.free();
    (void)hipFree(node->d_map);
    node->d_map = nullptr;
    node->map_cap = 0;
    free_pull_streams(node);
    node->root = -1;
    node->have_gather = false;
}

void free_genome(crp_node *node)
{
    for (NodeDev &d : node->dev) {
        for (auto &sl : d.slots) {
            if (sl->arena) (void)crp_arena_destroy(sl->arena);
            sl->arena = nullptr;
            sl->piece0 = sl->n_pieces = 0;
        }
        d.n_slots = 0;
    }
    node->pieces.clear();
    node->arena_off.clear();
    node->n_contigs = 0;
    node->loaded = false;
    node->have_gather = false;
}

void free_slot_buffers(NodeDev &d, NodeSlot &sl)
{
    (void)hipSetDevice(d.device);
    (void)hipFree(sl.d_needles);
    (void)hipFree(sl.d_bounds);
    (void)hipFree(sl.d_map_self);
    if (sl.h_bounds) (void)hipHostFree(sl.h_bounds);
    for (int s = 0; s < 2; ++s) {
        (void)hipFree(sl.d_lpos[s]);
        (void)hipFree(sl.d_lo16[s]);
        (void)hipFree(sl.d_bstart[s]);
    }
}

// upload of one device's share, arena after arena; runs on a thread of its own
int load_device(crp_node *node, int k, const uint8_t *const *texts)
{
    NodeDev &d = node->dev[(size_t)k];
    crp_ctx *ctx = d.ctx;
    for (size_t j = 0; j < d.n_slots; ++j) {
        NodeSlot &sl = *d.slots[j];
        const size_t np = sl.n_pieces;
        const crp::Piece *pieces = node->pieces.data() + sl.piece0;
        uint64_t *offs = node->arena_off.data() + sl.piece0;
        std::vector<const uint8_t *> ptrs(np);
        std::vector<uint64_t> lens(np);
        uint64_t words = 0;
        for (size_t q = 0; q < np; ++q) {
            const crp::Piece &p = pieces[q];
            ptrs[q] = texts[p.contig] + p.text_lo;
            lens[q] = p.text_len;
            words += crp_arena_words_for(p.text_len);
        }
        int rc = crp_arena_create(ctx, crp_arena_words_total(words), &sl.arena);
        if (rc == CRP_OK) rc = crp_arena_add_contigs_ascii(sl.arena, ptrs.data(), lens.data(), np, offs);
        if (rc == CRP_OK) rc = crp_arena_seal(sl.arena);
        if (rc != CRP_OK) return rc;
        // the ownership needles of this arena, resident from now on, and its own piece map (begin[], then sub[]): what turns an
        // arena position of an owned row into the position inside its contig
        std::vector<uint32_t> needles(2 * np), map(2 * np);
        crp::piece_cuts(pieces, np, offs, needles.data(), map.data());
        CRP_HIP(ctx, hipSetDevice(ctx->device));
        rc = crp::grow(ctx, reinterpret_cast<void **>(&sl.d_needles), &sl.needles_cap, 2 * np, sizeof(uint32_t));
        if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&sl.d_bounds), &sl.bounds_cap, 4 * np, sizeof(uint32_t));
        if (rc != CRP_OK) return rc;
        if (sl.h_bounds_cap < 4 * np) {
            if (sl.h_bounds) (void)hipHostFree(sl.h_bounds);
            sl.h_bounds = nullptr;
            sl.h_bounds_cap = 0;
            CRP_HIP(ctx, hipHostMalloc(reinterpret_cast<void **>(&sl.h_bounds), 4 * np * sizeof(uint32_t), hipHostMallocDefault));
            sl.h_bounds_cap = 4 * np;
        }
        rc = crp::staged_h2d(ctx, sl.d_needles, needles.data(), 2 * np * sizeof(uint32_t));  // (never the runtime's path for pageable memory: crp_api.cpp)
        if (rc != CRP_OK) return rc;
        rc = crp::grow(ctx, reinterpret_cast<void **>(&sl.d_map_self), &sl.map_self_cap, 2 * np, sizeof(uint32_t));
        if (rc != CRP_OK) return rc;
        rc = crp::staged_h2d(ctx, sl.d_map_self, map.data(), 2 * np * sizeof(uint32_t));
        if (rc != CRP_OK) return rc;
        CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (`needles` and `map` leave scope)
        sl.n_buckets = crp::pos16_buckets_for(sl.arena->padded_words);
    }
    return CRP_OK;
}

// ---- RCCL: creation and every wait bounded
struct CommBoot {
    std::mutex m;
    std::condition_variable cv;
    bool done = false, abandoned = false;
    ncclResult_t st = ncclSuccess;
    std::vector<ncclComm_t> comms;
    std::vector<int> ids;
};

// RCCL communicators of the node (ncclCommInitAll), once.  The call has no time-out of its own and is known to hang where a
// node's fabric is unhealthy: it runs on a helper thread that is given comm_init_timeout_s; one that does not return in time is
// left behind (crp_node_comm_stuck) and the node goes on without RCCL.
bool ensure_comms(crp_node *node)
{
    if (!node->comms.empty()) return true;
    if (node->comms_tried) return false;
    node->comms_tried = true;
    const crp::Rccl *r = crp::rccl();
    if (!r) {
        node->comms_error = crp::rccl_load_error();
        return false;
    }
    const size_t n = node->dev.size();
    auto boot = std::make_shared<CommBoot>();
    boot->ids.resize(n);
    for (size_t k = 0; k < n; ++k) boot->ids[k] = node->dev[k].device;
    boot->comms.assign(n, nullptr);
    try {
        std::thread([boot, r, n] {
            const ncclResult_t st = r->CommInitAll(boot->comms.data(), (int)n, boot->ids.data());
            std::unique_lock<std::mutex> lk(boot->m);
            boot->st = st;
            boot->done = true;
            if (boot->abandoned) {  // nobody is waiting any more: what was created is given back
                lk.unlock();
                if (st == ncclSuccess)
                    for (ncclComm_t c : boot->comms)
                        if (c) (void)r->CommAbort(c);
                g_boot_stuck.fetch_sub(1);
                return;
            }
            lk.unlock();
            boot->cv.notify_all();
        }).detach();
    } catch (...) {
        node->comms_error = "ncclCommInitAll: no helper thread to be had";
        return false;
    }
    {
        std::unique_lock<std::mutex> lk(boot->m);
        const double limit = node->comm_init_timeout_s;
        if (limit > 0) boot->cv.wait_for(lk, std::chrono::duration<double>(limit), [&] { return boot->done; });
        else boot->cv.wait(lk, [&] { return boot->done; });
        if (!boot->done) {
            boot->abandoned = true;
            g_boot_stuck.fetch_add(1);
            char text[160];
            std::snprintf(text, sizeof text, "ncclCommInitAll did not return within %.0f s (CRP_NODE_COMM_INIT_TIMEOUT_S)", limit);
            node->comms_error = text;
            return false;
        }
    }
    if (boot->st != ncclSuccess) {
        node->comms_error = std::string("ncclCommInitAll: ") + r->GetErrorString(boot->st);
        return false;
    }
    node->comms = boot->comms;
    return true;
}

enum { WAIT_OK = 0, WAIT_TIMEOUT = 1, WAIT_ERROR = 2 };

// everything queued on `s` so far, waited for by polling an event: at most `seconds` (<= 0: plain synchronise)
int wait_bounded(crp_node *node, NodeDev &d, hipStream_t s, double seconds)
{
    hipError_t e = hipSetDevice(d.device);
    if (e == hipSuccess && seconds <= 0) e = hipStreamSynchronize(s);
    else if (e == hipSuccess) {
        e = hipEventRecord(d.waitev, s);
        const auto t0 = std::chrono::steady_clock::now();
        while (e == hipSuccess) {
            e = hipEventQuery(d.waitev);
            if (e == hipSuccess) break;
            if (e != hipErrorNotReady) break;
            (void)hipGetLastError();
            e = hipSuccess;
            const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (el > seconds) return WAIT_TIMEOUT;
            if (el > 0.002) ::usleep(el > 0.05 ? 1000 : 50);  // (the first two milliseconds are polled flat out: the exchange is timed)
        }
    }
    if (e != hipSuccess) {
        node->last_error = std::string("waiting for logical device ") + std::to_string(d.device) + ": " + hipGetErrorString(e);
        return WAIT_ERROR;
    }
    return WAIT_OK;
}

// A collective did not complete: the communicators are aborted (that is what lets the streams go), never used again, and
// every stream that may carry a piece of the collective is drained.  false: even that did not come back.
bool abort_comms(crp_node *node, const std::string &why)
{
    const crp::Rccl *r = crp::rccl();
    if (r)
        for (ncclComm_t c : node->comms)
            if (c) (void)r->CommAbort(c);
    node->comms.clear();
    node->comms_error = why;
    const double limit = std::max(10.0, node->collective_timeout_s);
    for (NodeDev &d : node->dev)
        if (wait_bounded(node, d, d.ctx->stream, limit) != WAIT_OK) {
            node->last_error = why + "; and after ncclCommAbort the stream of logical device " + std::to_string(&d - node->dev.data()) + " did not drain";
            return false;
        }
    return true;
}

std::string timeout_text(const crp_node *node, const char *stage)
{
    char text[256];
    std::snprintf(text, sizeof text, "%s did not complete within %.3g s (CRP_NODE_COLLECTIVE_TIMEOUT_S): the RCCL communicators were aborted", stage,
                  node->collective_timeout_s);
    return text;
}

// RCCL or not, for a step of `what`.  A device listed twice: RCCL refuses the clique, so it is not even asked -- unless it was
// asked for by name, which is how the tests put a loop-back double of librccl.so under this very code (and why a one-device
// node then still creates its communicator).  Where RCCL cannot be had the step goes without (crp_node_transport_note says
// why; crp_node_gather_stats reports the transport that ran) -- unless it was asked for by name: CRP_ERR_COMM.
int choose_transport(crp_node *node, int flags, const char *what, bool *use_rccl)
{
    *use_rccl = false;
    const bool by_name = node->transport_env == CRP_TRANSPORT_RCCL;
    if ((node->duplicates && !by_name && !node->try_rccl) || (flags & CRP_NODE_PEER_COPY) || node->transport_env == CRP_TRANSPORT_PEER_COPY) return CRP_OK;
    if (node->dev.size() < 2 && !by_name) return CRP_OK;
    *use_rccl = ensure_comms(node);
    if (*use_rccl || !by_name) return CRP_OK;
    node->last_error = std::string(what) + ": RCCL asked for (CRP_NODE_TRANSPORT=rccl) but unavailable: " + node->comms_error;
    return CRP_ERR_COMM;
}

// How a bounded wait on a collective ended.  One that ran out: the communicators are aborted and the stage named; unless
// RCCL was asked for by name, `again` then runs the step once more without RCCL, and its success keeps the message.
template <class F>
int after_collective(crp_node *node, int waited, const char *stage, const char *instead, F again)
{
    if (waited == WAIT_OK) return CRP_OK;
    if (waited == WAIT_ERROR) return CRP_ERR_HIP;
    const std::string why = timeout_text(node, stage);
    if (!abort_comms(node, why)) return CRP_ERR_COMM;
    node->last_error = why;
    if (node->transport_env == CRP_TRANSPORT_RCCL) return CRP_ERR_COMM;
    node->last_error += instead;
    const std::string keep = node->last_error;
    const int rc = again();
    if (rc == CRP_OK) node->last_error = keep;
    return rc;
}

// a group that was refused: nothing of it is on any stream, but the communicators are in an unknown state
int group_refused(crp_node *node, const char *what, ncclResult_t st)
{
    const std::string why = std::string(what) + crp::rccl()->GetErrorString(st);
    (void)abort_comms(node, why);
    node->last_error = why;
    return CRP_ERR_COMM;
}

// everything queued so far on every device that holds an arena
int sync_devices(crp_node *node)
{
    for (NodeDev &d : node->dev) {
        if (!d.n_slots) continue;
        NODE_HIP(node, hipSetDevice(d.device));
        NODE_HIP(node, hipStreamSynchronize(d.ctx->stream));
    }
    return CRP_OK;
}

}  // namespace

// One step on every device that holds an arena, each on a host thread of its own (the per-device calls of the C ABI
// block on their stream); returns the first failure.
template <class F>
static int on_every_device(crp_node *node, const char *what, F step)
{
    const int world = (int)node->dev.size();
    std::vector<int> rcs((size_t)world, CRP_OK);
    std::vector<std::thread> pool((size_t)world);
    auto guarded = [&](int k) {
        try {
            rcs[(size_t)k] = step(k);
        } catch (...) {
            rcs[(size_t)k] = CRP_ERR_NOMEM;
        }
    };
    int first = -1;
    for (int k = 0; k < world; ++k) {
        if (!node->dev[(size_t)k].n_slots) continue;
        if (first < 0) {
            first = k;  // (this thread takes the first one itself, below)
            continue;
        }
        try {
            pool[(size_t)k] = std::thread(guarded, k);
        } catch (...) {
            guarded(k);
        }
    }
    if (first >= 0) guarded(first);
    for (auto &t : pool)
        if (t.joinable()) t.join();
    for (int k = 0; k < world; ++k)
        if (rcs[(size_t)k] != CRP_OK) return dev_fail(node, k, rcs[(size_t)k], what);
    return CRP_OK;
}

extern "C" {

int crp_node_init(int n_devices, const int *device_ids, crp_node **out)
{
    if (!out || n_devices < 1 || n_devices > 64 || !device_ids) return CRP_ERR_INVALID;
    *out = nullptr;
    crp_node *node = new (std::nothrow) crp_node();
    if (!node) return CRP_ERR_NOMEM;
    try {
        node->dev.resize((size_t)n_devices);
    } catch (...) {
        delete node;
        return CRP_ERR_NOMEM;
    }
    for (int k = 0; k < n_devices; ++k) {
        NodeDev &d = node->dev[(size_t)k];
        d.device = device_ids[k];
        for (int j = 0; j < k; ++j)
            if (device_ids[j] == device_ids[k]) node->duplicates = true;
        int rc = crp_init(device_ids[k], &d.ctx);
        if (rc == CRP_OK && hipEventCreateWithFlags(&d.ready, hipEventDisableTiming) != hipSuccess) rc = CRP_ERR_HIP;
        if (rc == CRP_OK && hipEventCreateWithFlags(&d.waitev, hipEventDisableTiming) != hipSuccess) rc = CRP_ERR_HIP;
        if (rc != CRP_OK) {
            crp_node_destroy(node);
            return rc;
        }
    }
    // the root pulls from (and RCCL's point-to-point kernels write into) its peers' memory: open the doors once
    for (int a = 0; a < n_devices; ++a)
        for (int b = 0; b < n_devices; ++b) {
            const int da = device_ids[a], db = device_ids[b];
            int can = 0;
            if (da == db || hipDeviceCanAccessPeer(&can, da, db) != hipSuccess || !can) continue;
            if (hipSetDevice(da) == hipSuccess) (void)hipDeviceEnablePeerAccess(db, 0);  // (already enabled: fine)
        }
    (void)hipGetLastError();
    if (const char *e = std::getenv("CRP_NODE_TRANSPORT")) {
        if (!std::strcmp(e, "peer")) node->transport_env = CRP_TRANSPORT_PEER_COPY;
        else if (!std::strcmp(e, "rccl")) node->transport_env = CRP_TRANSPORT_RCCL;
        else if (!std::strcmp(e, "try")) node->try_rccl = true;
    }
    if (const char *e = std::getenv("CRP_NODE_SCAN_THREADS")) node->scan_threads_env = std::atoi(e) != 0;  // (tests: the threaded scan on one GPU)
    if (const char *e = std::getenv("CRP_TEST_NODE_MISCOUNT")) node->test_miscount = std::atoi(e);
    node->arena_words = crp_arena_max_words();
    // the same default as the process-per-GPU path's bootstrap (engine.Engine.comm_init, CROPSR_COMM_INIT_TIMEOUT_S)
    node->comm_init_timeout_s = env_seconds("CRP_NODE_COMM_INIT_TIMEOUT_S", env_seconds("CROPSR_COMM_INIT_TIMEOUT_S", 180.0));
    node->collective_timeout_s = env_seconds("CRP_NODE_COLLECTIVE_TIMEOUT_S", 300.0);
    *out = node;
    return CRP_OK;
}

int crp_node_destroy(crp_node *node)
{
    if (!node) return CRP_OK;
    for (auto &w : node->workers)
        if (w) w->leave();
    node->workers.clear();
    for (NodeDev &d : node->dev)
        if (d.ctx) (void)crp_synchronize(d.ctx);
    if (!node->comms.empty() && crp::rccl())
        for (ncclComm_t c : node->comms)
            if (c) (void)crp::rccl()->CommDestroy(c);
    node->comms.clear();
    free_root_side(node);
    free_genome(node);
    for (NodeDev &d : node->dev) {
        if (!d.ctx) continue;
        for (auto &sl : d.slots) free_slot_buffers(d, *sl);
        d.slots.clear();
        (void)hipSetDevice(d.device);
        if (d.ready) (void)hipEventDestroy(d.ready);
        if (d.waitev) (void)hipEventDestroy(d.waitev);
        (void)crp_destroy(d.ctx);
    }
    delete node;
    return CRP_OK;
}

const char *crp_node_last_error(const crp_node *node) { return node ? node->last_error.c_str() : ""; }

const char *crp_node_transport_note(const crp_node *node) { return node ? node->comms_error.c_str() : ""; }

int crp_node_comm_stuck(void) { return g_boot_stuck.load(); }

int crp_node_size(const crp_node *node) { return node ? (int)node->dev.size() : CRP_ERR_INVALID; }

crp_ctx *crp_node_ctx(crp_node *node, int k)
{
    return (node && k >= 0 && (size_t)k < node->dev.size()) ? node->dev[(size_t)k].ctx : nullptr;
}

int crp_node_arenas(const crp_node *node, int k)
{
    return (node && k >= 0 && (size_t)k < node->dev.size()) ? (int)node->dev[(size_t)k].n_slots : CRP_ERR_INVALID;
}

crp_arena *crp_node_arena_at(crp_node *node, int k, int j)
{
    if (!node || k < 0 || (size_t)k >= node->dev.size() || j < 0 || (size_t)j >= node->dev[(size_t)k].n_slots) return nullptr;
    return node->dev[(size_t)k].slots[(size_t)j]->arena;
}

crp_arena *crp_node_arena(crp_node *node, int k) { return crp_node_arena_at(node, k, 0); }

int crp_node_set_option(crp_node *node, int option, int64_t value)
{
    if (!node) return CRP_ERR_INVALID;
    switch (option) {
        case CRP_NODE_OPT_ARENA_WORDS:
            if (value == 0) value = (int64_t)crp_arena_max_words();
            // (room for one piece of 64 owned characters between two halos)
            if (value < (int64_t)crp::slice_words_min(CRP_HALO) || (uint64_t)value > crp_arena_max_words()) return CRP_ERR_INVALID;
            node->arena_words = (uint64_t)value;
            return CRP_OK;
        case CRP_NODE_OPT_COMM_INIT_TIMEOUT_MS: node->comm_init_timeout_s = (double)value / 1000.0; return CRP_OK;
        case CRP_NODE_OPT_COLLECTIVE_TIMEOUT_MS: node->collective_timeout_s = (double)value / 1000.0; return CRP_OK;
        default: return CRP_ERR_INVALID;
    }
}

static int node_load_impl(crp_node *node, const uint8_t *const *texts, const uint64_t *lens, uint64_t n)
{
    crp::Range roctx_range("crp: node load (cut + H2D + pack on every device)");
    if (!node || (n && (!texts || !lens))) return CRP_ERR_INVALID;
    for (uint64_t k = 0; k < n; ++k) {
        if (lens[k] && !texts[k]) return CRP_ERR_INVALID;
        if (lens[k] > 0xFFFFFFFFull) {  // the tables carry contig-local positions as 32 bits (like the reference's CSV consumers)
            node->last_error = "crp_node_load: contig " + std::to_string(k) + " has " + std::to_string(lens[k]) + " characters; positions are 32-bit";
            return CRP_ERR_CAPACITY;
        }
    }
    free_genome(node);
    const int world = (int)node->dev.size();
    try {
        // every device's share (crp_plan_shares), packed into as many arenas as it needs
        std::vector<crp::Piece> cut;
        crp::plan_shares(lens, n, world, 4096, CRP_HALO, cut);
        node->pieces.reserve(cut.size());
        for (size_t q = 0; q < cut.size();) {
            size_t n_run = 1;  // the pieces of one device follow each other
            while (q + n_run < cut.size() && cut[q + n_run].group == cut[q].group) ++n_run;
            NodeDev &d = node->dev[(size_t)cut[q].group];
            size_t at = node->pieces.size();
            crp::pack_pieces(&cut[q], n_run, lens, node->arena_words, CRP_HALO, node->pieces);
            for (; at < node->pieces.size(); ++at) {
                if (node->pieces[at].group == d.n_slots) {  // the device's next arena begins here
                    if (d.n_slots == d.slots.size()) d.slots.emplace_back(new NodeSlot());
                    d.slots[d.n_slots++]->piece0 = at;
                }
                d.slots[d.n_slots - 1]->n_pieces += 1;
            }
            q += n_run;
        }
        node->arena_off.assign(node->pieces.size(), 0);
        node->n_contigs = n;
        node->contig_counts.assign(2 * n, 0);
    } catch (...) {
        free_genome(node);
        return CRP_ERR_NOMEM;
    }
    // one host thread per device: its share crosses its own PCIe link while the others' cross theirs
    std::vector<int> rcs((size_t)world, CRP_OK);
    {
        std::vector<std::thread> pool((size_t)world);
        for (int k = 1; k < world; ++k) {
            try {
                pool[(size_t)k] = std::thread([node, k, texts, &rcs] {
                    try {
                        rcs[(size_t)k] = load_device(node, k, texts);
                    } catch (...) {
                        rcs[(size_t)k] = CRP_ERR_NOMEM;
                    }
                });
            } catch (...) {  // no thread to be had: this one does the share
                try {
                    rcs[(size_t)k] = load_device(node, k, texts);
                } catch (...) {
                    rcs[(size_t)k] = CRP_ERR_NOMEM;
                }
            }
        }
        try {
            rcs[0] = load_device(node, 0, texts);
        } catch (...) {
            rcs[0] = CRP_ERR_NOMEM;
        }
        for (auto &t : pool)
            if (t.joinable()) t.join();
    }
    for (int k = 0; k < world; ++k)
        if (rcs[(size_t)k] != CRP_OK) {
            const int rc = dev_fail(node, k, rcs[(size_t)k], "crp_node_load");
            const std::string keep = node->last_error;
            free_genome(node);
            node->last_error = keep;
            return rc;
        }
    node->loaded = true;
    return CRP_OK;
}

static int node_plan_impl(const crp_node *node, uint64_t *pieces, uint64_t cap, uint64_t *n_pieces)
{
    if (!node || !n_pieces || (cap && !pieces)) return CRP_ERR_INVALID;
    if (!node->loaded) return CRP_ERR_STATE;
    *n_pieces = node->pieces.size();
    if (node->pieces.size() > cap) return CRP_ERR_CAPACITY;
    for (size_t k = 0; k < node->dev.size(); ++k)
        for (size_t j = 0; j < node->dev[k].n_slots; ++j) {
            const NodeSlot &sl = *node->dev[k].slots[j];
            for (size_t q = sl.piece0; q < sl.piece0 + sl.n_pieces; ++q) {
                const crp::Piece &p = node->pieces[q];
                const uint64_t row[7] = {p.contig, p.start, p.end, k, node->arena_off[q], crp::owned_begin(p, 0), p.group};
                std::memcpy(pieces + 7 * q, row, sizeof row);
            }
        }
    return CRP_OK;
}

static int node_scan_score_impl(crp_node *node, int guide_len, int flags, uint64_t *n_plus, uint64_t *n_minus)
{
    crp::Range roctx_range("crp: node scan + score (all devices)");
    if (!node) return CRP_ERR_INVALID;
    if (!node->loaded) return CRP_ERR_STATE;
    node->have_gather = false;
    const int world = (int)node->dev.size();
    // every device's scan on its own host thread (NodeWorker); the calling thread takes the first device that has an arena
    if (node->workers.size() != (size_t)world) {
        try {
            node->workers.resize((size_t)world);
        } catch (...) {
            return CRP_ERR_NOMEM;
        }
    }
    int mine = -1;
    std::vector<char> posted((size_t)world, 0);
    // (a device listed more than once -- the rehearsal shape on a one-GPU box -- is scanned one logical device after the
    // other from this thread: N kernels launched at the same instant on ONE GPU only get in each other's way, their tiles'
    // look-backs waiting on workgroups that found no slot: 4 x 1.13 Gb took 2.32 ms that way against 1.64 ms one by one)
    const bool threaded = node->scan_threads_env >= 0 ? node->scan_threads_env == 1 : !node->duplicates;
    for (int k = 0; k < world && threaded; ++k) {
        NodeDev &d = node->dev[(size_t)k];
        if (!d.n_slots) continue;
        if (mine < 0) {
            mine = k;
            continue;
        }
        auto &w = node->workers[(size_t)k];
        if (!w) {
            try {
                w.reset(new NodeWorker());
                w->th = std::thread([p = w.get()] { p->loop(); });
            } catch (...) {
                w.reset();  // no thread to be had: this device is scanned from here, after the others were posted
                continue;
            }
        }
        w->post(&d, guide_len, flags);
        posted[(size_t)k] = 1;
    }
    int rc = CRP_OK;
    uint64_t tot[2] = {0, 0};
    for (int k = 0; k < world; ++k) {  // the first device, and any device without a thread
        NodeDev &d = node->dev[(size_t)k];
        if (!d.n_slots || posted[(size_t)k]) continue;
        uint64_t x[2] = {0, 0};
        const int rk = NodeWorker::scan_device(d, guide_len, flags, x);
        if (rk != CRP_OK && rc == CRP_OK) rc = dev_fail(node, k, rk, "crp_node_scan_score");
        tot[0] += x[0];
        tot[1] += x[1];
    }
    for (int k = 0; k < world; ++k) {
        if (!posted[(size_t)k]) continue;
        uint64_t n[2] = {0, 0};
        const int rk = node->workers[(size_t)k]->wait(n);
        if (rk != CRP_OK && rc == CRP_OK) rc = dev_fail(node, k, rk, "crp_node_scan_score");
        tot[0] += n[0];
        tot[1] += n[1];
    }
    if (rc != CRP_OK) return rc;
    if (n_plus) *n_plus = tot[0];
    if (n_minus) *n_minus = tot[1];
    return CRP_OK;
}

// ---- crp_node_gather, phase by phase.  What one gather carries from phase to phase (its results go into the node: total,
// contig_counts, bytes_to_root; none of them is read before have_gather is set again):
struct Gather {
    int root;
    crp::GatherCols cols;
    std::vector<SlotRef> act;
    std::vector<uint64_t> soff[2], boff[2];  // per slot: element offsets into the root's staging buffers
    std::vector<uint64_t> map_off;           // per slot: offset of its begin[] in d_map (sub[] follows)
    bool rccl = false;                       // the transport: one RCCL group, or the root's pull streams
    std::chrono::steady_clock::time_point t_call, t_x;
    NodeDev &R(crp_node *node) const { return node->dev[(size_t)root]; }
};

static inline uint64_t owned_rows(const NodeSlot &sl, int s) { return sl.last[s] - sl.first[s]; }

// ownership cuts: per arena and strand, the index of the first row at or after every needle; from them every slot's
// owned run, its place in the final tables, and the per-contig counts
static int gather_cuts(crp_node *node, Gather &g)
{
    for (const SlotRef &a : g.act) {
        NodeDev &d = node->dev[(size_t)a.k];
        NodeSlot &sl = *a.sl;
        const uint32_t nn = (uint32_t)(2 * sl.n_pieces);
        NODE_HIP(node, hipSetDevice(d.device));
        for (int s = 0; s < 2; ++s)
            NODE_HIP(node, crp::launch_lower_bound(d.ctx->stream, sl.arena->d_pos[s], sl.arena->n_hits[s], sl.d_needles, nn, sl.d_bounds + (size_t)s * nn));
        NODE_HIP(node, hipMemcpyAsync(sl.h_bounds, sl.d_bounds, 2 * (size_t)nn * sizeof(uint32_t), hipMemcpyDeviceToHost, d.ctx->stream));
    }
    const int rc = sync_devices(node);
    if (rc != CRP_OK) return rc;
    std::fill(node->contig_counts.begin(), node->contig_counts.end(), 0);
    node->total[0] = node->total[1] = 0;
    std::vector<uint32_t> counts;
    for (const SlotRef &a : g.act) {
        NodeSlot &sl = *a.sl;
        const size_t np = sl.n_pieces;
        counts.resize(np);
        for (int s = 0; s < 2; ++s) {
            // contiguous shares: only an arena's first piece has a left halo and only its last a right one, so its owned rows
            // are ONE run of each table
            if (!crp::owned_run(sl.h_bounds + (size_t)s * 2 * np, np, &sl.first[s], &sl.last[s], counts.data())) {
                node->last_error = "crp_node_gather: the owned rows of logical device " + std::to_string(a.k) + " are not one run";
                return CRP_ERR_STATE;
            }
            sl.foff[s] = node->total[s];
            for (size_t j = 0; j < np; ++j) node->contig_counts[2 * node->pieces[sl.piece0 + j].contig + (size_t)s] += counts[j];
            node->total[s] += owned_rows(sl, s);
        }
    }
    return CRP_OK;
}

// CRP_NODE_HOST_GATHER: nothing crosses xGMI.  Every device rebases the positions of its owned rows where they lie;
// crp_node_fetch then pulls every device's rows over that device's OWN PCIe link straight into their place in the
// caller's arrays -- N links instead of the root's one, for a consumer that lives on the host (the CSV writer).
static int gather_on_hosts(crp_node *node, Gather &g)
{
    g.t_x = std::chrono::steady_clock::now();
    node->bytes_to_root = 0;
    for (const SlotRef &a : g.act) {
        NodeDev &d = node->dev[(size_t)a.k];
        NodeSlot &sl = *a.sl;
        crp_ctx *ctx = d.ctx;
        NODE_HIP(node, hipSetDevice(d.device));
        const size_t np = sl.n_pieces;
        for (int s = 0; s < 2; ++s) {
            const uint64_t n = owned_rows(sl, s);
            const int rc = crp::grow(ctx, reinterpret_cast<void **>(&sl.d_lpos[s]), &sl.lpos_cap[s], n, sizeof(uint32_t));
            if (rc != CRP_OK) return dev_fail(node, a.k, rc, "crp_node_gather (rebased positions)");
            NODE_HIP(node, crp::launch_pos_rebase(ctx->stream, sl.arena->d_pos[s] + sl.first[s], n,
                                                  crp::PieceMap{sl.d_map_self, sl.d_map_self + np, (uint32_t)np}, sl.d_lpos[s]));
        }
    }
    return sync_devices(node);
}

// the root's side: final tables, staging, piece maps, pull streams.  The exchange is timed from its end.
static int gather_reserve_root(crp_node *node, Gather &g)
{
    const int world = (int)node->dev.size();
    if (node->root != g.root) free_root_side(node);
    node->root = g.root;
    crp_ctx *rctx = g.R(node).ctx;
    NODE_HIP(node, hipSetDevice(rctx->device));
    uint64_t lo_total[2] = {0, 0}, b_total[2] = {0, 0};
    for (int s = 0; s < 2; ++s) {
        g.soff[s].assign(g.act.size(), 0);
        g.boff[s].assign(g.act.size(), 0);
        for (const SlotRef &a : g.act) {
            if (a.k == g.root || !g.cols.pos16) continue;
            g.soff[s][a.flat] = lo_total[s];
            g.boff[s][a.flat] = b_total[s];
            lo_total[s] += round_up8(owned_rows(*a.sl, s));
            b_total[s] += a.sl->n_buckets;
        }
    }
    int rc = node->tables.reserve(rctx, node->total, lo_total, b_total, g.cols);
    if (rc != CRP_OK) return dev_fail(node, g.root, rc, "crp_node_gather (root's tables)");
    // piece maps: begin[] and sub[] per slot, one upload
    g.map_off.assign(g.act.size(), 0);
    node->h_map.resize(2 * node->pieces.size());
    for (const SlotRef &a : g.act) {
        const NodeSlot &sl = *a.sl;
        g.map_off[a.flat] = 2 * sl.piece0;
        crp::piece_cuts(node->pieces.data() + sl.piece0, sl.n_pieces, node->arena_off.data() + sl.piece0, nullptr, node->h_map.data() + 2 * sl.piece0);
    }
    rc = crp::grow(rctx, reinterpret_cast<void **>(&node->d_map), &node->map_cap, node->h_map.size(), sizeof(uint32_t));
    if (rc != CRP_OK) return dev_fail(node, g.root, rc, "crp_node_gather (piece maps)");
    if (!node->h_map.empty())
        NODE_HIP(node, hipMemcpyAsync(node->d_map, node->h_map.data(), node->h_map.size() * sizeof(uint32_t), hipMemcpyHostToDevice, rctx->stream));
    if (!g.rccl && node->pull.size() != (size_t)world) {
        free_pull_streams(node);
        node->pull.assign((size_t)world, nullptr);
        node->pulled.assign((size_t)world, nullptr);
        hipError_t e = hipSuccess;
        for (int k = 0; k < world && e == hipSuccess; ++k) {
            if (k == g.root) continue;
            e = hipStreamCreateWithFlags(&node->pull[(size_t)k], hipStreamNonBlocking);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&node->pulled[(size_t)k], hipEventDisableTiming);
        }
        if (e != hipSuccess) {  // (half a set would be taken for a whole one by the next gather)
            free_pull_streams(node);
            node->last_error = std::string("crp_node_gather (pull streams): ") + hipGetErrorString(e);
            return CRP_ERR_HIP;
        }
    }
    NODE_HIP(node, hipStreamSynchronize(rctx->stream));  // (the maps are in place; the exchange is timed from here)
    g.t_x = std::chrono::steady_clock::now();
    return CRP_OK;
}

// the peers' side: pack the positions of the owned rows; a peer's pull stream starts once the peer's side is in place
static int gather_pack_peers(crp_node *node, const Gather &g)
{
    for (const SlotRef &a : g.act) {
        if (a.k == g.root || !g.cols.pos16) continue;
        NodeDev &d = node->dev[(size_t)a.k];
        NodeSlot &sl = *a.sl;
        crp_ctx *ctx = d.ctx;
        NODE_HIP(node, hipSetDevice(d.device));
        for (int s = 0; s < 2; ++s) {
            const uint64_t n = owned_rows(sl, s);
            int rc = crp::grow(ctx, reinterpret_cast<void **>(&sl.d_lo16[s]), &sl.lo16_cap[s], round_up8(n), sizeof(uint16_t));
            if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&sl.d_bstart[s]), &sl.bstart_cap[s], sl.n_buckets, sizeof(uint32_t));
            if (rc != CRP_OK) return dev_fail(node, a.k, rc, "crp_node_gather (packed positions)");
            NODE_HIP(node, crp::launch_pos16_buckets(ctx->stream, sl.arena->d_pos[s], sl.arena->n_hits[s], sl.first[s], sl.last[s],
                                                     sl.d_bstart[s], sl.n_buckets));
            NODE_HIP(node, crp::launch_pos16_pack(ctx->stream, sl.arena->d_pos[s] + sl.first[s], n, sl.d_lo16[s]));
        }
    }
    for (size_t k = 0; k < node->dev.size() && !g.rccl; ++k) {
        NodeDev &d = node->dev[k];
        if ((int)k == g.root || !d.n_slots) continue;
        NODE_HIP(node, hipSetDevice(d.device));
        NODE_HIP(node, hipEventRecord(d.ready, d.ctx->stream));
        NODE_HIP(node, hipSetDevice(g.R(node).device));
        NODE_HIP(node, hipStreamWaitEvent(node->pull[k], d.ready, 0));
    }
    return CRP_OK;
}

// the exchange: every message of every peer's strands (crp::wire_msgs) as a send/recv pair inside ONE RCCL group, or as a
// copy on the root's pull stream for that peer
static int gather_exchange(crp_node *node, Gather &g)
{
    NodeDev &R = g.R(node);
    crp_ctx *rctx = R.ctx;
    const crp::Rccl *r = g.rccl ? crp::rccl() : nullptr;
    ncclResult_t st = ncclSuccess, st_end = ncclSuccess;
    int miscount = r ? node->test_miscount : 0;
    node->bytes_to_root = 0;
    if (r) st = r->GroupStart();
    for (const SlotRef &a : g.act) {
        if (st != ncclSuccess) break;
        if (a.k == g.root) continue;
        NodeDev &d = node->dev[(size_t)a.k];
        NodeSlot &sl = *a.sl;
        for (int s = 0; s < 2 && st == ncclSuccess; ++s) {
            const crp::GatherSrc src{sl.arena, sl.first[s], sl.d_lo16[s], sl.d_bstart[s]};
            const crp::GatherDst dst{&node->tables, sl.foff[s], g.soff[s][a.flat], g.boff[s][a.flat]};
            crp::WireMsg msg[crp::MAX_WIRE_MSGS];
            const int nm = crp::wire_msgs(g.cols, s, owned_rows(sl, s), sl.n_buckets, &src, &dst, msg);
            for (int m = 0; m < nm && st == ncclSuccess; ++m) {
                node->bytes_to_root += msg[m].bytes;
                if (r) {
                    uint64_t expect = msg[m].bytes;
                    if (miscount && expect > 8) {  // test hook (CRP_TEST_NODE_MISCOUNT): ONE receive of this gather is posted 8 bytes short
                        expect -= 8;
                        miscount = 0;
                    }
                    st = r->Send(msg[m].src, msg[m].bytes, ncclUint8, g.root, node->comms[(size_t)a.k], d.ctx->stream);
                    if (st == ncclSuccess) st = r->Recv(msg[m].dst, expect, ncclUint8, a.k, node->comms[(size_t)g.root], rctx->stream);
                } else {
                    NODE_HIP(node, hipSetDevice(R.device));
                    if (d.device == R.device)
                        NODE_HIP(node, hipMemcpyAsync(msg[m].dst, msg[m].src, msg[m].bytes, hipMemcpyDeviceToDevice, node->pull[(size_t)a.k]));
                    else
                        NODE_HIP(node, hipMemcpyPeerAsync(msg[m].dst, R.device, msg[m].src, d.device, msg[m].bytes, node->pull[(size_t)a.k]));
                }
            }
        }
    }
    if (r) st_end = r->GroupEnd();
    if (st != ncclSuccess || st_end != ncclSuccess) return group_refused(node, "crp_node_gather send/recv: ", st != ncclSuccess ? st : st_end);
    for (size_t k = 0; k < node->dev.size() && !r; ++k) {  // the root's stream goes on once every peer's rows have landed
        if ((int)k == g.root || !node->dev[k].n_slots) continue;
        NODE_HIP(node, hipSetDevice(R.device));
        NODE_HIP(node, hipEventRecord(node->pulled[k], node->pull[k]));
        NODE_HIP(node, hipStreamWaitEvent(rctx->stream, node->pulled[k], 0));
    }
    return CRP_OK;
}

// the root's side: expand / rebase into the final tables (its own rows never cross a link)
static int gather_expand(crp_node *node, const Gather &g)
{
    crp_ctx *rctx = g.R(node).ctx;
    NODE_HIP(node, hipSetDevice(rctx->device));
    for (const SlotRef &a : g.act) {
        NodeSlot &sl = *a.sl;
        const size_t np = sl.n_pieces;
        const crp::PieceMap map{node->d_map + g.map_off[a.flat], node->d_map + g.map_off[a.flat] + np, (uint32_t)np};
        for (int s = 0; s < 2; ++s) {
            const uint64_t n = owned_rows(sl, s);
            if (!n) continue;
            uint32_t *out = reinterpret_cast<uint32_t *>(node->tables.at(crp::COL_POS, s, sl.foff[s]));
            if (a.k == g.root) {
                NODE_HIP(node, crp::launch_pos_rebase(rctx->stream, sl.arena->d_pos[s] + sl.first[s], n, map, out));
                for (int i = 0; i < g.cols.n; ++i) {
                    const int c = g.cols.col[i];
                    if (c != crp::COL_POS)
                        NODE_HIP(node, hipMemcpyAsync(node->tables.at(c, s, sl.foff[s]), crp::col_src(g.cols, c, sl.arena, s, sl.first[s]),
                                                      n * crp::COL_BYTES[c], hipMemcpyDeviceToDevice, rctx->stream));
                }
            } else if (g.cols.pos16) {
                NODE_HIP(node, crp::launch_pos16_expand(rctx->stream, node->tables.d_lo16[s] + g.soff[s][a.flat], n,
                                                        node->tables.d_bstart[s] + g.boff[s][a.flat], sl.n_buckets, map, out));
            } else {
                NODE_HIP(node, crp::launch_pos_rebase(rctx->stream, out, n, map, out));  // in place: a thread rewrites the rows it read
            }
        }
    }
    return CRP_OK;
}

// the rows to the root over g's transport.  A grouped send/recv that does not complete in time is given up, and the rows
// move once more as device-to-device copies, everything sized and queued afresh.
static int gather_to_root(crp_node *node, Gather &g)
{
    int rc = gather_reserve_root(node, g);
    if (rc == CRP_OK) rc = gather_pack_peers(node, g);
    if (rc == CRP_OK) rc = gather_exchange(node, g);
    if (rc == CRP_OK) rc = gather_expand(node, g);
    if (rc != CRP_OK) return rc;
    // the receives, then the sends (they read the peers' tables: they must have left before the next scan) -- on RCCL every
    // wait has a bound
    const double bound = g.rccl ? node->collective_timeout_s : 0.0;
    int waited = wait_bounded(node, g.R(node), g.R(node).ctx->stream, bound);
    for (size_t k = 0; k < node->dev.size() && waited == WAIT_OK; ++k) {
        NodeDev &d = node->dev[k];
        if ((int)k != g.root && d.n_slots) waited = wait_bounded(node, d, d.ctx->stream, bound);
    }
    return after_collective(node, waited, "crp_node_gather: the grouped send/recv", "; device-to-device copies used instead", [&] {
        g.rccl = false;
        g.t_call = std::chrono::steady_clock::now();
        return gather_to_root(node, g);
    });
}

static int node_gather_impl(crp_node *node, int root, int flags)
{
    crp::Range roctx_range("crp: node gatherv");
    if (!node || root < 0 || (size_t)root >= node->dev.size() ||
        (flags & ~(CRP_GATHER_PRE | CRP_GATHER_POS16 | CRP_NODE_PEER_COPY | CRP_GATHER_OFFTARGET | CRP_GATHER_FEATURES | CRP_NODE_HOST_GATHER)))
        return CRP_ERR_INVALID;
    if (!node->loaded) return CRP_ERR_STATE;
    Gather g;
    g.root = root;
    g.cols = crp::gather_cols(flags);
    g.act = active_slots(node);
    for (const SlotRef &a : g.act)
        if (!crp::tables_present(g.cols, a.sl->arena)) {
            node->last_error = "crp_node_gather: logical device " + std::to_string(a.k) + " has no (matching) tables: scan first";
            return CRP_ERR_STATE;
        }
    node->have_gather = false;
    g.t_call = std::chrono::steady_clock::now();
    int rc = gather_cuts(node, g);
    const bool on_hosts = (flags & CRP_NODE_HOST_GATHER) != 0;
    if (rc == CRP_OK && on_hosts) rc = gather_on_hosts(node, g);
    if (rc == CRP_OK && !on_hosts) rc = choose_transport(node, flags, "crp_node_gather", &g.rccl);
    if (rc == CRP_OK && !on_hosts) rc = gather_to_root(node, g);
    if (rc != CRP_OK) return rc;
    node->ms_exchange = ms_since(g.t_x);
    node->ms_total = ms_since(g.t_call);
    node->transport = on_hosts ? CRP_TRANSPORT_HOST_LINKS : g.rccl ? CRP_TRANSPORT_RCCL : (node->dev.size() == 1 ? 0 : CRP_TRANSPORT_PEER_COPY);
    node->gflags = flags;
    node->have_gather = true;
    return CRP_OK;
}

static int node_offtarget_impl(crp_node *node, int guide_len, uint64_t *n_sites)
{
    crp::Range roctx_range("crp: node off-target seed scan");
    if (!node) return CRP_ERR_INVALID;
    if (!node->loaded) return CRP_ERR_STATE;
    const int world = (int)node->dev.size();
    for (const SlotRef &a : active_slots(node))
        if (!a.sl->arena->have_hits) {
            node->last_error = "crp_node_offtarget: scan first";
            return CRP_ERR_STATE;
        }
    node->have_gather = false;
    // 1. every device: its own sites into its own histogram -- a hit counts as a site on the device that OWNS it only
    std::vector<uint64_t> sites((size_t)world, 0);
    for (int k = 0; k < world; ++k) {  // (every device of the node takes part in the sum, with or without an arena)
        const int rc = crp_offtarget_reset(node->dev[(size_t)k].ctx);
        if (rc != CRP_OK) return dev_fail(node, k, rc, "crp_node_offtarget (reset)");
    }
    int rc = on_every_device(node, "crp_node_offtarget (sites)", [&](int k) {
        NodeDev &d = node->dev[(size_t)k];
        for (size_t j = 0; j < d.n_slots; ++j) {
            NodeSlot &sl = *d.slots[j];
            std::vector<uint64_t> own(2 * sl.n_pieces);
            for (size_t q = 0; q < sl.n_pieces; ++q) {
                const crp::Piece &p = node->pieces[sl.piece0 + q];
                own[2 * q] = crp::owned_begin(p, node->arena_off[sl.piece0 + q]);
                own[2 * q + 1] = own[2 * q] + (p.end - p.start);
            }
            uint64_t n = 0;
            const int r2 = crp_offtarget_add(sl.arena, guide_len, own.data(), sl.n_pieces, &n);
            if (r2 != CRP_OK) return r2;
            sites[(size_t)k] += n;
        }
        return (int)CRP_OK;
    });
    if (rc != CRP_OK) return rc;
    // 2. the histograms summed over the devices: RCCL all-reduce in one group, or through the first device
    if (world > 1) {
        bool use_rccl = false;
        rc = choose_transport(node, 0, "crp_node_offtarget", &use_rccl);
        if (rc != CRP_OK) return rc;
        if (use_rccl) {
            const crp::Rccl *r = crp::rccl();
            ncclResult_t st = r->GroupStart();
            for (int k = 0; k < world && st == ncclSuccess; ++k) {
                crp_ctx *ctx = node->dev[(size_t)k].ctx;
                st = r->AllReduce(ctx->d_ot_hist, ctx->d_ot_hist, crp::OT_HIST_ENTRIES, ncclUint32, ncclSum, node->comms[(size_t)k], ctx->stream);
            }
            const ncclResult_t st_end = r->GroupEnd();
            if (st != ncclSuccess || st_end != ncclSuccess) return group_refused(node, "crp_node_offtarget all-reduce: ", st != ncclSuccess ? st : st_end);
            int waited = WAIT_OK;
            for (int k = 0; k < world && waited == WAIT_OK; ++k) waited = wait_bounded(node, node->dev[(size_t)k], node->dev[(size_t)k].ctx->stream, node->collective_timeout_s);
            // (the histograms may be half summed: the whole step once more -- reset, sites, sum through device 0)
            if (waited != WAIT_OK)
                return after_collective(node, waited, "crp_node_offtarget: the histogram all-reduce", "; the histograms are summed through device 0 instead",
                                        [&] { return node_offtarget_impl(node, guide_len, n_sites); });
        } else {
            // device 0 collects: every other histogram is copied beside its own and added, then the sum goes back.  A device
            // without an arena has only QUEUED the zeroing of its histogram (crp_offtarget_reset): wait for every stream first
            for (int k = 0; k < world; ++k) {
                const int rk = crp_synchronize(node->dev[(size_t)k].ctx);
                if (rk != CRP_OK) return dev_fail(node, k, rk, "crp_node_offtarget (histograms ready)");
            }
            NodeDev &R = node->dev[0];
            crp_ctx *rctx = R.ctx;
            NODE_HIP(node, hipSetDevice(R.device));
            uint32_t *tmp = nullptr;  // (64 MiB of scratch for the length of this call)
            NODE_HIP(node, hipMalloc(reinterpret_cast<void **>(&tmp), crp::OT_HIST_ENTRIES * sizeof(uint32_t)));
            const size_t bytes = crp::OT_HIST_ENTRIES * sizeof(uint32_t);
            hipError_t e = hipSuccess;
            for (int k = 1; k < world && e == hipSuccess; ++k) {
                NodeDev &d = node->dev[(size_t)k];
                e = d.device == R.device ? hipMemcpyAsync(tmp, d.ctx->d_ot_hist, bytes, hipMemcpyDeviceToDevice, rctx->stream)
                                         : hipMemcpyPeerAsync(tmp, R.device, d.ctx->d_ot_hist, d.device, bytes, rctx->stream);
                if (e == hipSuccess) e = crp::launch_add_u32(rctx->stream, rctx->d_ot_hist, tmp, crp::OT_HIST_ENTRIES);
            }
            for (int k = 1; k < world && e == hipSuccess; ++k) {
                NodeDev &d = node->dev[(size_t)k];
                e = d.device == R.device ? hipMemcpyAsync(d.ctx->d_ot_hist, rctx->d_ot_hist, bytes, hipMemcpyDeviceToDevice, rctx->stream)
                                         : hipMemcpyPeerAsync(d.ctx->d_ot_hist, d.device, rctx->d_ot_hist, R.device, bytes, rctx->stream);
            }
            if (e == hipSuccess) e = hipStreamSynchronize(rctx->stream);
            (void)hipFree(tmp);
            if (e != hipSuccess) {
                node->last_error = std::string("crp_node_offtarget (histogram sum): ") + hipGetErrorString(e);
                return CRP_ERR_HIP;
            }
        }
    }
    // 3. every device: the Hamming-ball sums of the genome-wide histogram, then its own hits' counts (they stay in HBM)
    rc = on_every_device(node, "crp_node_offtarget (solve + counts)", [&](int k) {
        NodeDev &d = node->dev[(size_t)k];
        int r2 = crp_offtarget_solve(d.ctx);
        for (size_t j = 0; j < d.n_slots && r2 == CRP_OK; ++j) r2 = crp_offtarget_counts(d.slots[j]->arena, nullptr, nullptr);
        return r2;
    });
    if (rc != CRP_OK) return rc;
    if (n_sites) {
        *n_sites = 0;
        for (uint64_t v : sites) *n_sites += v;
    }
    return CRP_OK;
}

static int node_annotate_impl(crp_node *node, const crp_annotation *annotation, const uint64_t *seqid_of_contig, int dec)
{
    crp::Range roctx_range("crp: node annotation join");
    if (!node || !annotation || (node->n_contigs && !seqid_of_contig) || dec < 0) return CRP_ERR_INVALID;
    if (!node->loaded) return CRP_ERR_STATE;
    for (const SlotRef &a : active_slots(node))
        if (!a.sl->arena->have_hits) {
            node->last_error = "crp_node_annotate: scan first";
            return CRP_ERR_STATE;
        }
    node->have_gather = false;
    return on_every_device(node, "crp_node_annotate", [&](int k) {
        NodeDev &d = node->dev[(size_t)k];
        for (size_t j = 0; j < d.n_slots; ++j) {
            NodeSlot &sl = *d.slots[j];
            // the track of THIS arena: every text is a piece of a contig (with its halo), named by the contig's seqid
            std::vector<uint64_t> entries(4 * sl.n_pieces);
            for (size_t q = 0; q < sl.n_pieces; ++q) {
                const crp::Piece &p = node->pieces[sl.piece0 + q];
                const uint64_t e[4] = {seqid_of_contig[p.contig], p.text_lo, p.text_len, node->arena_off[sl.piece0 + q]};
                std::memcpy(&entries[4 * q], e, sizeof e);
            }
            uint64_t n = 0;
            int rc = crp_annotation_track(annotation, entries.data(), sl.n_pieces, dec, nullptr, nullptr, 0, &n);
            if (rc != CRP_OK && rc != CRP_ERR_CAPACITY) return rc;
            std::vector<uint32_t> points(n), ids(n);
            rc = crp_annotation_track(annotation, entries.data(), sl.n_pieces, dec, points.data(), ids.data(), n, &n);
            if (rc == CRP_OK) rc = crp_annotate_set_track(sl.arena, points.data(), ids.data(), n);
            if (rc == CRP_OK) rc = crp_annotate_lookup(sl.arena, nullptr, nullptr);
            if (rc != CRP_OK) return rc;
        }
        return (int)CRP_OK;
    });
}

// Columns of the last gather to the caller's arrays: out of the root's tables, or (CRP_NODE_HOST_GATHER) every device's
// owned rows over ITS link into their place, one host thread per device.
static int fetch_cols(crp_node *node, const crp::HostCol *want, int n_want, const char *what)
{
    if (node->gflags & CRP_NODE_HOST_GATHER) {
        const crp::GatherCols cols = crp::gather_cols(node->gflags);
        return on_every_device(node, (std::string(what) + " (host gather)").c_str(), [&](int k) {
            NodeDev &d = node->dev[(size_t)k];
            for (size_t j = 0; j < d.n_slots; ++j) {
                NodeSlot &sl = *d.slots[j];
                for (int s = 0; s < 2; ++s)
                    for (int i = 0; i < n_want; ++i) {
                        const int c = want[i].col;
                        const uint64_t n = owned_rows(sl, s);
                        if (!n || !want[i].host[s]) continue;
                        // (the positions of a host gather: rebased where they lie, gather_on_hosts)
                        const void *src = c == crp::COL_POS ? (const void *)sl.d_lpos[s] : crp::col_src(cols, c, sl.arena, s, sl.first[s]);
                        const int rc = crp::staged_d2h(d.ctx, static_cast<char *>(want[i].host[s]) + sl.foff[s] * crp::COL_BYTES[c], src, n * crp::COL_BYTES[c]);
                        if (rc != CRP_OK) return rc;
                    }
            }
            return crp_synchronize(d.ctx);
        });
    }
    crp_ctx *ctx = node->dev[(size_t)node->root].ctx;
    NODE_HIP(node, hipSetDevice(ctx->device));
    for (int s = 0; s < 2; ++s)
        for (int i = 0; i < n_want; ++i) {
            if (!want[i].host[s] || !node->total[s]) continue;
            const int rc = crp::staged_d2h(ctx, want[i].host[s], node->tables.d_col[s][want[i].col], node->total[s] * crp::COL_BYTES[want[i].col]);
            if (rc != CRP_OK) return dev_fail(node, node->root, rc, what);
        }
    NODE_HIP(node, hipStreamSynchronize(ctx->stream));
    return CRP_OK;
}

// the optional column that `flag` brought into the last gather
static int node_fetch_optional_impl(crp_node *node, int col, int flag, const char *what, uint32_t *plus, uint32_t *minus)
{
    if (!node) return CRP_ERR_INVALID;
    if (!node->have_gather || !(node->gflags & flag)) return CRP_ERR_STATE;
    const crp::HostCol want{col, {plus, minus}};
    return fetch_cols(node, &want, 1, what);
}

int crp_node_counts(const crp_node *node, uint64_t *per_contig, uint64_t *n_plus, uint64_t *n_minus)
{
    if (!node) return CRP_ERR_INVALID;
    if (!node->have_gather) return CRP_ERR_STATE;
    if (per_contig && !node->contig_counts.empty())
        std::memcpy(per_contig, node->contig_counts.data(), node->contig_counts.size() * sizeof(uint64_t));
    if (n_plus) *n_plus = node->total[0];
    if (n_minus) *n_minus = node->total[1];
    return CRP_OK;
}

static int node_count_scored_impl(crp_node *node, uint64_t *n_scored)
{
    if (!node || !n_scored) return CRP_ERR_INVALID;
    if (!node->have_gather) return CRP_ERR_STATE;
    const crp::GatherCols cols = crp::gather_cols(node->gflags);
    const bool on_hosts = (node->gflags & CRP_NODE_HOST_GATHER) != 0;
    *n_scored = 0;
    // the root counts its tables; after a host gather the rows are still on their devices and every device counts its owned runs
    for (size_t k = 0; k < node->dev.size(); ++k) {
        NodeDev &d = node->dev[k];
        if (on_hosts ? !d.n_slots : (int)k != node->root) continue;
        crp_ctx *c = d.ctx;
        NODE_HIP(node, hipSetDevice(d.device));
        NODE_HIP(node, hipMemsetAsync(c->d_scalar, 0, sizeof(uint64_t), c->stream));
        for (int s = 0; s < 2 && !on_hosts; ++s)
            NODE_HIP(node, crp::launch_count_scored(c->stream, static_cast<const double *>(node->tables.d_col[s][crp::COL_VALUE]), node->total[s], c->d_scalar));
        for (size_t j = 0; j < d.n_slots && on_hosts; ++j)
            for (int s = 0; s < 2; ++s) {
                const NodeSlot &sl = *d.slots[j];
                NODE_HIP(node, crp::launch_count_scored(c->stream, reinterpret_cast<const double *>(crp::col_src(cols, crp::COL_VALUE, sl.arena, s, sl.first[s])),
                                                        owned_rows(sl, s), c->d_scalar));
            }
        NODE_HIP(node, hipMemcpyAsync(c->h_scalar, c->d_scalar, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        NODE_HIP(node, hipStreamSynchronize(c->stream));
        *n_scored += c->h_scalar[0];
    }
    return CRP_OK;
}

static int node_fetch_impl(crp_node *node, uint32_t *pos_plus, double *score_plus, uint32_t *pos_minus, double *score_minus)
{
    crp::Range roctx_range("crp: node D2H tables");
    if (!node) return CRP_ERR_INVALID;
    if (!node->have_gather) return CRP_ERR_STATE;
    const crp::HostCol want[2] = {{crp::COL_POS, {pos_plus, pos_minus}}, {crp::COL_VALUE, {score_plus, score_minus}}};
    return fetch_cols(node, want, 2, "crp_node_fetch");
}

int crp_node_tables_device(crp_node *node, void **pos_plus, void **score_plus, void **pos_minus, void **score_minus)
{
    if (!node) return CRP_ERR_INVALID;
    if (!node->have_gather || (node->gflags & CRP_NODE_HOST_GATHER)) return CRP_ERR_STATE;  // (a host gather leaves no table on any one device)
    if (pos_plus) *pos_plus = node->tables.d_col[0][crp::COL_POS];
    if (score_plus) *score_plus = node->tables.d_col[0][crp::COL_VALUE];
    if (pos_minus) *pos_minus = node->tables.d_col[1][crp::COL_POS];
    if (score_minus) *score_minus = node->tables.d_col[1][crp::COL_VALUE];
    return CRP_OK;
}

int crp_node_gather_stats(const crp_node *node, double *ms_total, double *ms_exchange, uint64_t *bytes_to_root, int *transport)
{
    if (!node) return CRP_ERR_INVALID;
    if (!node->have_gather) return CRP_ERR_STATE;
    if (ms_total) *ms_total = node->ms_total;
    if (ms_exchange) *ms_exchange = node->ms_exchange;
    if (bytes_to_root) *bytes_to_root = node->bytes_to_root;
    if (transport) *transport = node->transport;
    return CRP_OK;
}


// The entry points above may allocate (vectors, strings, threads): nothing is allowed to throw across the C ABI.
#define CRP_NODE_GUARD(call)     \
    try {                        \
        return (call);           \
    } catch (...) {              \
        return CRP_ERR_NOMEM;    \
    }
int crp_node_load(crp_node *node, const uint8_t *const *texts, const uint64_t *lens, uint64_t n) { CRP_NODE_GUARD(node_load_impl(node, texts, lens, n)); }
int crp_node_plan(const crp_node *node, uint64_t *pieces, uint64_t cap, uint64_t *n_pieces) { CRP_NODE_GUARD(node_plan_impl(node, pieces, cap, n_pieces)); }
int crp_node_scan_score(crp_node *node, int guide_len, int flags, uint64_t *n_plus, uint64_t *n_minus) { CRP_NODE_GUARD(node_scan_score_impl(node, guide_len, flags, n_plus, n_minus)); }
int crp_node_gather(crp_node *node, int root, int flags) { CRP_NODE_GUARD(node_gather_impl(node, root, flags)); }
int crp_node_offtarget(crp_node *node, int guide_len, uint64_t *n_sites) { CRP_NODE_GUARD(node_offtarget_impl(node, guide_len, n_sites)); }
int crp_node_annotate(crp_node *node, const crp_annotation *annotation, const uint64_t *seqid_of_contig, int dec) { CRP_NODE_GUARD(node_annotate_impl(node, annotation, seqid_of_contig, dec)); }
int crp_node_fetch(crp_node *node, uint32_t *pos_plus, double *score_plus, uint32_t *pos_minus, double *score_minus) { CRP_NODE_GUARD(node_fetch_impl(node, pos_plus, score_plus, pos_minus, score_minus)); }
int crp_node_fetch_offtarget(crp_node *node, uint32_t *ot_plus, uint32_t *ot_minus) { CRP_NODE_GUARD(node_fetch_optional_impl(node, crp::COL_OT, CRP_GATHER_OFFTARGET, "crp_node_fetch_offtarget", ot_plus, ot_minus)); }
int crp_node_fetch_features(crp_node *node, uint32_t *feat_plus, uint32_t *feat_minus) { CRP_NODE_GUARD(node_fetch_optional_impl(node, crp::COL_FEAT, CRP_GATHER_FEATURES, "crp_node_fetch_features", feat_plus, feat_minus)); }
int crp_node_count_scored(crp_node *node, uint64_t *n_scored) { CRP_NODE_GUARD(node_count_scored_impl(node, n_scored)); }

}  // extern "C"
