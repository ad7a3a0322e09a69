// crp_comm.cpp -- the multi-GPU exchange of the path, on RCCL, inside the library.
//
// One process per GPU.  The scan itself needs no collective (contigs are independent,
// CROPSR.py:409); what crosses xGMI is
//   * crp_gather_hits      the final gatherv of the per-rank hit tables to a root.  RCCL has no
//                          gatherv primitive: ncclAllGather of the two counts, then
//                          ncclGroupStart / ncclSend (peers) | ncclRecv (root), one per column /
//                          ncclGroupEnd.  Every peer->root transfer rides its own point-to-point
//                          xGMI link, so the step is bounded by one link, not by a ring;
//   * crp_offtarget_reduce (crp_offtarget.hip) the all-reduce of the 64 MiB site histogram;
//   * crp_comm_barrier / crp_comm_allreduce_f64: bench fences and sums.
// librccl.so is loaded with dlopen on the first crp_comm_* call -- a single-GPU process never
// pays for it, and the library has no link-time dependency on RCCL.  The communicator's unique id is
// created here (rank 0) and carried to the other ranks by the host (cropsr_amd/rendezvous.py).
#include <dlfcn.h>

#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "crp_gather_cols.h"
#include "crp_internal.h"
#include "crp_rccl.h"
#include "crp_roctx.h"

namespace crp {

static Rccl g_rccl;
static std::once_flag g_rccl_once;

template <class F>
static bool bind(void *h, const char *name, F &fn)
{
    fn = reinterpret_cast<F>(dlsym(h, name));
    return fn != nullptr;
}

const Rccl *rccl()
{
    std::call_once(g_rccl_once, [] {
        const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        void *h = nullptr;
        for (const char *n : names)
            if ((h = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
        if (!h) {
            g_rccl.error = std::string("dlopen(librccl.so.1): ") + (dlerror() ? dlerror() : "not found");
            return;
        }
        Rccl &r = g_rccl;
        const bool ok = bind(h, "ncclGetUniqueId", r.GetUniqueId) && bind(h, "ncclCommInitRank", r.CommInitRank) &&
                        bind(h, "ncclCommInitAll", r.CommInitAll) &&
                        bind(h, "ncclCommDestroy", r.CommDestroy) && bind(h, "ncclCommAbort", r.CommAbort) &&
                        bind(h, "ncclAllGather", r.AllGather) && bind(h, "ncclAllReduce", r.AllReduce) &&
                        bind(h, "ncclSend", r.Send) && bind(h, "ncclRecv", r.Recv) &&
                        bind(h, "ncclGroupStart", r.GroupStart) && bind(h, "ncclGroupEnd", r.GroupEnd) &&
                        bind(h, "ncclGetErrorString", r.GetErrorString);
        if (!ok) {
            g_rccl.error = "librccl.so lacks a required symbol";
            return;
        }
        r.handle = h;
    });
    return g_rccl.handle ? &g_rccl : nullptr;
}

const std::string &rccl_load_error() { return g_rccl.error; }

}  // namespace crp

using crp::rccl;
using crp::Rccl;

struct crp_comm {
    ncclComm_t comm = nullptr;
    int rank = 0, world = 0;
    // scratch in HBM: counts (2 per rank) and small reductions
    uint64_t *d_counts = nullptr;  // 4 * world {n_plus, n_minus, status, position buckets} + world (second agreement round)
    double *d_small = nullptr;     // 64 doubles in, 64 out
    std::vector<uint64_t> counts;  // last gather: {n_plus, n_minus} per rank
    std::vector<uint64_t> raw;     // host copy of d_counts
    int test_fail = 0;             // test hook, environment CRP_TEST_GATHER_FAIL: 1 = the root's receive buffers
                                   // "do not fit", 2 = the last rank's arena "has no tables", 3 = the last rank sends
                                   // one row too few of its score column (a protocol error only a checking transport sees)
    // root's receive side of the last crp_gather_hits: column-wise, peers back to back in rank order; with
    // CRP_GATHER_POS16 its staging area takes the packed positions, peer after peer (every peer's rows at a multiple of 8)
    crp::GatherTables tables;
    // CRP_GATHER_POS16 (crp_gather.hip): a peer's packed positions and bucket starts
    uint16_t *d_lo16[2] = {nullptr, nullptr};
    uint32_t *d_bstart[2] = {nullptr, nullptr};
    uint64_t lo16_cap[2] = {0, 0}, bstart_cap[2] = {0, 0};
    uint64_t bytes_to_root = 0;  // of the last gather: what this rank sent (peer) or received (root)
    int gflags = 0;
    std::vector<uint64_t> goff[2];  // element offset of every rank's slice (root's own slice: unused)
    int groot = -1;
    crp_arena *garena = nullptr;    // root's own contribution stays in its arena
    bool have_gather = false;
};

#define CRP_NCCL(ctx, call)                                                                       \
    do {                                                                                          \
        ncclResult_t r__ = (call);                                                                \
        if (r__ != ncclSuccess) {                                                                 \
            (ctx)->last_error = std::string(#call) + ": " + rccl()->GetErrorString(r__);          \
            return CRP_ERR_COMM;                                                                  \
        }                                                                                         \
    } while (0)

namespace crp {

void comm_release(crp_ctx *ctx)
{
    crp_comm *c = ctx->comm;
    if (!c) return;
    if (c->comm && rccl()) (void)rccl()->CommDestroy(c->comm);
    (void)hipFree(c->d_counts);
    (void)hipFree(c->d_small);
    c->tables.free();
    for (int s = 0; s < 2; ++s) {
        (void)hipFree(c->d_lo16[s]);
        (void)hipFree(c->d_bstart[s]);
    }
    delete c;
    ctx->comm = nullptr;
}

// crp_arena_destroy: the root's own rows of the last gather lived in this arena
void comm_forget_arena(crp_ctx *ctx, const crp_arena *a)
{
    if (ctx->comm && ctx->comm->garena == a) {
        ctx->comm->garena = nullptr;
        ctx->comm->have_gather = false;
    }
}

int comm_world(const crp_ctx *ctx) { return ctx->comm ? ctx->comm->world : 0; }
int comm_rank(const crp_ctx *ctx) { return ctx->comm ? ctx->comm->rank : 0; }
uint64_t comm_gather_bytes(const crp_ctx *ctx) { return ctx->comm ? ctx->comm->bytes_to_root : 0; }

// used by crp_offtarget.hip: in-place sum of n uint32 over all ranks (no-op without a communicator)
int comm_allreduce_u32(crp_ctx *ctx, uint32_t *d_buf, uint64_t n)
{
    crp_comm *c = ctx->comm;
    if (!c || c->world == 1) return CRP_OK;
    CRP_NCCL(ctx, rccl()->AllReduce(d_buf, d_buf, n, ncclUint32, ncclSum, c->comm, ctx->stream));
    return CRP_OK;
}

}  // namespace crp

extern "C" {

int crp_comm_unique_id(uint8_t id[CRP_COMM_ID_BYTES])
{
    static_assert(CRP_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "unique id size");
    if (!id) return CRP_ERR_INVALID;
    const Rccl *r = rccl();
    if (!r) return CRP_ERR_COMM;
    ncclUniqueId u;
    if (r->GetUniqueId(&u) != ncclSuccess) return CRP_ERR_COMM;
    std::memcpy(id, u.internal, CRP_COMM_ID_BYTES);
    return CRP_OK;
}

int crp_comm_init(crp_ctx *ctx, const uint8_t id[CRP_COMM_ID_BYTES], int rank, int world)
{
    if (!ctx || !id || world < 1 || rank < 0 || rank >= world) return CRP_ERR_INVALID;
    if (ctx->comm) return CRP_ERR_STATE;
    const Rccl *r = rccl();
    if (!r) {
        ctx->last_error = crp::rccl_load_error();
        return CRP_ERR_COMM;
    }
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    crp_comm *c = new (std::nothrow) crp_comm();
    if (!c) return CRP_ERR_NOMEM;
    c->rank = rank;
    c->world = world;
    ctx->comm = c;
    ncclUniqueId u;
    std::memcpy(u.internal, id, CRP_COMM_ID_BYTES);
    ncclResult_t st = r->CommInitRank(&c->comm, world, u, rank);
    if (st != ncclSuccess) {
        ctx->last_error = std::string("ncclCommInitRank: ") + r->GetErrorString(st);
        c->comm = nullptr;
        crp::comm_release(ctx);
        return CRP_ERR_COMM;
    }
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&c->d_counts), 5 * (size_t)world * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&c->d_small), 128 * sizeof(double));
    if (e != hipSuccess) {
        ctx->last_error = std::string("communicator scratch: ") + hipGetErrorString(e);
        crp::comm_release(ctx);
        return CRP_ERR_NOMEM;
    }
    c->counts.assign(2 * (size_t)world, 0);
    c->raw.assign(5 * (size_t)world, 0);
    if (const char *e = std::getenv("CRP_TEST_GATHER_FAIL")) c->test_fail = std::atoi(e);
    return CRP_OK;
}

int crp_comm_destroy(crp_ctx *ctx)
{
    if (!ctx) return CRP_ERR_INVALID;
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    crp::comm_release(ctx);
    return CRP_OK;
}

int crp_comm_allreduce_f64(crp_ctx *ctx, double *values, int n, int op)
{
    if (!ctx || !values || n < 1 || n > 64 || (op != CRP_REDUCE_SUM && op != CRP_REDUCE_MAX)) return CRP_ERR_INVALID;
    crp_comm *c = ctx->comm;
    if (!c) return CRP_ERR_STATE;
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    CRP_HIP(ctx, hipMemcpyAsync(c->d_small, values, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    CRP_NCCL(ctx, rccl()->AllReduce(c->d_small, c->d_small + 64, (size_t)n, ncclDouble, op == CRP_REDUCE_SUM ? ncclSum : ncclMax,
                                    c->comm, ctx->stream));
    CRP_HIP(ctx, hipMemcpyAsync(values, c->d_small + 64, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CRP_OK;
}

int crp_comm_barrier(crp_ctx *ctx)
{
    double one = 1.0;
    return crp_comm_allreduce_f64(ctx, &one, 1, CRP_REDUCE_SUM);
}

// Every rank's status word of one agreement round -> this rank's return value: its own error if it has
// one, CRP_ERR_PEER if only others do, CRP_OK if nobody does.  The same words are seen by every rank (they
// come out of an all-gather), so all ranks leave the call together and none enters the next collective.
static int agreed_status(crp_ctx *ctx, const crp_comm *c, const uint64_t *status, size_t stride, int own, const char *what)
{
    int first_bad = -1;
    for (int p = 0; p < c->world; ++p)
        if (status[(size_t)p * stride] != 0 && first_bad < 0) first_bad = p;
    if (first_bad < 0) return CRP_OK;
    if (own != CRP_OK) return own;
    ctx->last_error = std::string("crp_gather_hits abandoned on every rank: rank ") + std::to_string(first_bad) + " reported '" +
                      crp_strerror(-(int)status[(size_t)first_bad * stride]) + "' " + what;
    return CRP_ERR_PEER;
}

int crp_gather_hits(crp_ctx *ctx, crp_arena *a, int root, int flags, uint64_t *counts_all)
{
    crp::Range roctx_range("crp: gatherv (RCCL)");
    if (!ctx) return CRP_ERR_INVALID;
    crp_comm *c = ctx->comm;
    if (!c) return CRP_ERR_STATE;
    // (arguments that are the same on every rank by contract: a bad one fails everywhere alike)
    if (root < 0 || root >= c->world || (flags & ~(CRP_GATHER_OFFTARGET | CRP_GATHER_PRE | CRP_GATHER_FEATURES | CRP_GATHER_POS16)))
        return CRP_ERR_INVALID;
    const crp::GatherCols cols = crp::gather_cols(flags);
    // What can differ from rank to rank -- the state of this rank's arena, the root's allocation -- is never
    // answered with an early return: a rank that left here alone would leave its peers inside a collective
    // that cannot complete.  Each rank's status travels WITH its counts, and everyone acts on all of them.
    int local = CRP_OK;
    if (a && (a->ctx != ctx || !crp::tables_present(cols, a))) local = CRP_ERR_STATE;
    if (c->test_fail == 2 && c->rank == c->world - 1) local = CRP_ERR_STATE;  // test hook (CRP_TEST_GATHER_FAIL)
    const Rccl *r = rccl();
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    c->have_gather = false;
    const bool ok_local = local == CRP_OK;
    const uint32_t my_buckets = ok_local && a ? crp::pos16_buckets_for(a->padded_words) : 0;
    const uint64_t mine[4] = {ok_local && a ? a->n_hits[0] : 0, ok_local && a ? a->n_hits[1] : 0, (uint64_t)(-local), my_buckets};
    const size_t W = (size_t)c->world;
    // 1. everyone learns every rank's two counts and its status
    CRP_HIP(ctx, hipMemcpyAsync(c->d_counts + 4 * c->rank, mine, sizeof mine, hipMemcpyHostToDevice, ctx->stream));
    CRP_NCCL(ctx, r->AllGather(c->d_counts + 4 * c->rank, c->d_counts, 4, ncclUint64, c->comm, ctx->stream));
    CRP_HIP(ctx, hipMemcpyAsync(c->raw.data(), c->d_counts, 4 * W * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<uint32_t> buckets(W);
    for (size_t p = 0; p < W; ++p) {
        c->counts[2 * p] = c->raw[4 * p];
        c->counts[2 * p + 1] = c->raw[4 * p + 1];
        buckets[p] = (uint32_t)c->raw[4 * p + 3];
    }
    if (counts_all) std::memcpy(counts_all, c->counts.data(), 2 * W * sizeof(uint64_t));
    int rc = agreed_status(ctx, c, c->raw.data() + 2, 4, local, "before the exchange (its arena has no tables to send)");
    if (rc != CRP_OK) return rc;
    // 2. the root sizes its receive buffers; whether that worked is agreed on as well (one more word per rank)
    int alloc = CRP_OK;
    std::vector<uint64_t> soff[2], boff[2];  // CRP_GATHER_POS16: every peer's place in the root's staging area
    if (c->rank == root) {
        uint64_t total[2] = {0, 0}, lo_total[2] = {0, 0}, b_total[2] = {0, 0};
        for (int s = 0; s < 2; ++s) {
            c->goff[s].assign(W, 0);
            soff[s].assign(W, 0);
            boff[s].assign(W, 0);
            for (int p = 0; p < c->world; ++p) {
                c->goff[s][(size_t)p] = total[s];
                soff[s][(size_t)p] = lo_total[s];
                boff[s][(size_t)p] = b_total[s];
                if (p == root) continue;
                total[s] += c->counts[2 * (size_t)p + s];
                if (!cols.pos16) continue;
                lo_total[s] += (c->counts[2 * (size_t)p + s] + 7) & ~(uint64_t)7;
                b_total[s] += buckets[(size_t)p];
            }
        }
        alloc = c->tables.reserve(ctx, total, lo_total, b_total, cols);
    } else if (cols.pos16 && a) {  // a peer's packed positions
        for (int s = 0; s < 2 && alloc == CRP_OK; ++s) {
            alloc = crp::grow(ctx, reinterpret_cast<void **>(&c->d_lo16[s]), &c->lo16_cap[s], (mine[s] + 7) & ~(uint64_t)7, sizeof(uint16_t));
            if (alloc == CRP_OK)
                alloc = crp::grow(ctx, reinterpret_cast<void **>(&c->d_bstart[s]), &c->bstart_cap[s], my_buckets, sizeof(uint32_t));
        }
    }
    if (c->rank == root && c->test_fail == 1) {  // test hook: as if the receive buffers did not fit
        alloc = CRP_ERR_NOMEM;
        ctx->last_error = "gatherv receive buffers: out of memory (injected by CRP_TEST_GATHER_FAIL)";
    }
    const uint64_t word = (uint64_t)(-alloc);
    uint64_t *d_status = c->d_counts + 4 * W;
    CRP_HIP(ctx, hipMemcpyAsync(d_status + c->rank, &word, sizeof word, hipMemcpyHostToDevice, ctx->stream));
    CRP_NCCL(ctx, r->AllGather(d_status + c->rank, d_status, 1, ncclUint64, c->comm, ctx->stream));
    CRP_HIP(ctx, hipMemcpyAsync(c->raw.data(), d_status, W * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    rc = agreed_status(ctx, c, c->raw.data(), 1, alloc, "while sizing the root's receive buffers");
    if (rc != CRP_OK) return rc;
    // 3. the tables: grouped point-to-point, peers -> root
    crp::prof_begin(ctx, CRP_K_GATHER);
    uint64_t moved = 0;
    if (cols.pos16 && c->rank != root && a)  // (on the stream the sends are queued on: packed before they read)
        for (int s = 0; s < 2; ++s) {
            CRP_HIP(ctx, crp::launch_pos16_buckets(ctx->stream, a->d_pos[s], mine[s], 0, mine[s], c->d_bstart[s], my_buckets));
            CRP_HIP(ctx, crp::launch_pos16_pack(ctx->stream, a->d_pos[s], mine[s], c->d_lo16[s]));
        }
    CRP_NCCL(ctx, r->GroupStart());
    ncclResult_t st = ncclSuccess;
    // (every message is counted in bytes, the same list on both sides: crp::wire_msgs)
    crp::WireMsg msg[crp::MAX_WIRE_MSGS];
    if (c->rank == root) {
        for (int p = 0; p < c->world && st == ncclSuccess; ++p) {
            if (p == root) continue;
            for (int s = 0; s < 2 && st == ncclSuccess; ++s) {
                const crp::GatherDst dst{&c->tables, c->goff[s][(size_t)p], soff[s][(size_t)p], boff[s][(size_t)p]};
                const int nm = crp::wire_msgs(cols, s, c->counts[2 * (size_t)p + s], buckets[(size_t)p], nullptr, &dst, msg);
                for (int m = 0; m < nm && st == ncclSuccess; ++m) {
                    moved += msg[m].bytes;
                    st = r->Recv(msg[m].dst, msg[m].bytes, ncclUint8, p, c->comm, ctx->stream);
                }
            }
        }
    } else {
        // test hook (CRP_TEST_GATHER_FAIL=3): the last rank's value column leaves one element short
        const uint64_t short_by = c->test_fail == 3 && c->rank == c->world - 1 ? sizeof(double) : 0;
        for (int s = 0; s < 2 && st == ncclSuccess; ++s) {
            const crp::GatherSrc src{a, 0, c->d_lo16[s], c->d_bstart[s]};
            const int nm = crp::wire_msgs(cols, s, mine[s], my_buckets, &src, nullptr, msg);
            for (int m = 0; m < nm && st == ncclSuccess; ++m) {
                moved += msg[m].bytes;
                st = r->Send(msg[m].src, msg[m].bytes - (msg[m].col == crp::COL_VALUE ? short_by : 0), ncclUint8, root, c->comm, ctx->stream);
            }
        }
    }
    const ncclResult_t st_end = r->GroupEnd();
    if (cols.pos16 && c->rank == root && st == ncclSuccess && st_end == ncclSuccess)  // packed -> the root's position tables
        for (int p = 0; p < c->world; ++p)
            for (int s = 0; s < 2 && p != root; ++s) {
                const uint64_t n = c->counts[2 * (size_t)p + s];
                CRP_HIP(ctx, crp::launch_pos16_expand(ctx->stream, c->tables.d_lo16[s] + soff[s][(size_t)p], n, c->tables.d_bstart[s] + boff[s][(size_t)p],
                                                      buckets[(size_t)p], crp::PieceMap{nullptr, nullptr, 0},
                                                      reinterpret_cast<uint32_t *>(c->tables.at(crp::COL_POS, s, c->goff[s][(size_t)p]))));
            }
    crp::prof_end(ctx, CRP_K_GATHER);
    if (st != ncclSuccess || st_end != ncclSuccess) {
        // not agreed on: the communicator is in an unknown state and the peers may be inside the exchange --
        // the caller must take the whole run down (cli.EngineResident.gather: Group.abort)
        ctx->last_error = std::string("gatherv send/recv: ") + r->GetErrorString(st != ncclSuccess ? st : st_end);
        return CRP_ERR_COMM;
    }
    // the sends read the arena's tables: they must have left before the caller may scan or destroy it
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    crp::prof_collect(ctx, CRP_K_GATHER);
    c->bytes_to_root = moved;
    c->groot = root;
    c->gflags = flags;
    c->garena = a;
    c->have_gather = true;
    return CRP_OK;
}

// Columns of rank `rank`'s slice of the last gather to the caller's arrays: the root's own rows never moved and come out
// of its arena, everyone else's out of the gathered tables at goff.
static int fetch_cols(crp_ctx *ctx, const crp_comm *c, int rank, const crp::HostCol *want, int n_want)
{
    const crp::GatherCols cols = crp::gather_cols(c->gflags);
    const bool own = rank == c->groot;
    for (int s = 0; s < 2; ++s)
        for (int i = 0; i < n_want; ++i) {
            const int col = want[i].col;
            const uint64_t n = c->counts[2 * (size_t)rank + s];
            if (!n || !want[i].host[s]) continue;
            if (own && (!c->garena || !(col == crp::COL_FEAT ? c->garena->have_feat : c->garena->have_hits))) return CRP_ERR_STATE;
            const void *d = own ? crp::col_src(cols, col, c->garena, s, 0) : c->tables.at(col, s, c->goff[s][(size_t)rank]);
            const int rc = crp::staged_d2h(ctx, want[i].host[s], d, n * crp::COL_BYTES[col]);
            if (rc != CRP_OK) return rc;
        }
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CRP_OK;
}

int crp_gathered_fetch(crp_ctx *ctx, int rank, uint32_t *pos_plus, double *score_plus, uint32_t *ot_plus,
                       uint32_t *pos_minus, double *score_minus, uint32_t *ot_minus)
{
    if (!ctx) return CRP_ERR_INVALID;
    crp_comm *c = ctx->comm;
    if (!c || !c->have_gather || c->rank != c->groot) return CRP_ERR_STATE;
    if (rank < 0 || rank >= c->world) return CRP_ERR_INVALID;
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    if ((ot_plus || ot_minus) && !(c->gflags & CRP_GATHER_OFFTARGET)) return CRP_ERR_STATE;
    const crp::HostCol want[3] = {{crp::COL_OT, {ot_plus, ot_minus}}, {crp::COL_POS, {pos_plus, pos_minus}}, {crp::COL_VALUE, {score_plus, score_minus}}};
    return fetch_cols(ctx, c, rank, want, 3);
}

int crp_gathered_fetch_features(crp_ctx *ctx, int rank, uint32_t *feat_plus, uint32_t *feat_minus)
{
    if (!ctx) return CRP_ERR_INVALID;
    crp_comm *c = ctx->comm;
    if (!c || !c->have_gather || c->rank != c->groot || !(c->gflags & CRP_GATHER_FEATURES)) return CRP_ERR_STATE;
    if (rank < 0 || rank >= c->world) return CRP_ERR_INVALID;
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    const crp::HostCol want{crp::COL_FEAT, {feat_plus, feat_minus}};
    return fetch_cols(ctx, c, rank, &want, 1);
}

}  // extern "C"
