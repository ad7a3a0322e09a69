// crp_gather_cols.h -- the row columns a gather moves, named ONCE for both multi-GPU paths (crp_node.cpp: one process
// over N GPUs; crp_comm.cpp: one process per GPU).  Everything that sizes, sends, receives, copies or fetches "the
// columns" walks the list built here, so a new per-hit column is added in this file alone: a COL_* with its bytes per
// row, its flag in gather_cols(), its arena pointer in col_src() and its readiness in tables_present().
#pragma once

#include "crp_internal.h"

namespace crp {

enum { COL_POS = 0, COL_VALUE = 1, COL_OT = 2, COL_FEAT = 3, N_COLS = 4 };  // wire order
constexpr uint64_t COL_BYTES[N_COLS] = {sizeof(uint32_t), sizeof(double), sizeof(uint4), sizeof(uint32_t)};

// the columns of one gather, from its CRP_GATHER_* flags
struct GatherCols {
    bool pre = false;    // COL_VALUE is the pre-score (d_pre), not the score
    bool pos16 = false;  // COL_POS crosses as 16-bit positions + bucket starts (crp_gather.hip)
    int n = 0;
    int col[N_COLS] = {0, 0, 0, 0};  // [0, n): the COL_* present, wire order
};

inline GatherCols gather_cols(int flags)
{
    GatherCols g;
    g.pre = (flags & CRP_GATHER_PRE) != 0;
    g.pos16 = (flags & CRP_GATHER_POS16) != 0;
    g.col[g.n++] = COL_POS;
    g.col[g.n++] = COL_VALUE;
    if (flags & CRP_GATHER_OFFTARGET) g.col[g.n++] = COL_OT;
    if (flags & CRP_GATHER_FEATURES) g.col[g.n++] = COL_FEAT;
    return g;
}

// column `c` of strand `s` in an arena's tables, from row `first` on
inline const char *col_src(const GatherCols &g, int c, const crp_arena *a, int s, uint64_t first)
{
    const void *p = c == COL_POS ? (const void *)a->d_pos[s]
                    : c == COL_VALUE ? (const void *)(g.pre ? a->d_pre[s] : a->d_score[s])
                    : c == COL_OT ? (const void *)a->d_ot_cnt[s]
                                  : (const void *)a->d_feat[s];
    return static_cast<const char *>(p) + first * COL_BYTES[c];
}

// does the arena hold current tables for every column?  (false: CRP_ERR_STATE)
inline bool tables_present(const GatherCols &g, const crp_arena *a)
{
    if (!a->have_hits || (g.pre && !a->have_pre)) return false;
    for (int i = 0; i < g.n; ++i) {
        if (g.col[i] == COL_OT && (!a->ctx->ot_solved || a->ot_epoch != a->ctx->ot_epoch || !a->d_ot_cnt[0])) return false;
        if (g.col[i] == COL_FEAT && !a->have_feat) return false;
    }
    return true;
}

// a fetch: column `col` of both strands to the caller's two arrays (either may be NULL)
struct HostCol {
    int col;
    void *host[2];
};

// The root's destination tables: per strand one buffer per column, and the staging area the packed positions of
// CRP_GATHER_POS16 arrive in (every peer's rows at a multiple of 8 elements).  Grow-only; they outlive the genome.
struct GatherTables {
    void *d_col[2][N_COLS] = {};
    uint64_t col_cap[2][N_COLS] = {};
    uint16_t *d_lo16[2] = {nullptr, nullptr};
    uint32_t *d_bstart[2] = {nullptr, nullptr};
    uint64_t lo16_cap[2] = {0, 0}, bstart_cap[2] = {0, 0};

    char *at(int c, int s, uint64_t row) const { return static_cast<char *>(d_col[s][c]) + row * COL_BYTES[c]; }

    // per strand: room for `rows` rows of every column of `g`, `lo16` staged positions and `buckets` staged bucket starts
    int reserve(crp_ctx *ctx, const uint64_t rows[2], const uint64_t lo16[2], const uint64_t buckets[2], const GatherCols &g)
    {
        for (int s = 0; s < 2; ++s) {
            int rc = CRP_OK;
            for (int i = 0; i < g.n && rc == CRP_OK; ++i)
                rc = grow(ctx, &d_col[s][g.col[i]], &col_cap[s][g.col[i]], rows[s], COL_BYTES[g.col[i]]);
            if (rc == CRP_OK && lo16[s]) rc = grow(ctx, reinterpret_cast<void **>(&d_lo16[s]), &lo16_cap[s], lo16[s], sizeof(uint16_t));
            if (rc == CRP_OK && buckets[s]) rc = grow(ctx, reinterpret_cast<void **>(&d_bstart[s]), &bstart_cap[s], buckets[s], sizeof(uint32_t));
            if (rc != CRP_OK) return rc;
        }
        return CRP_OK;
    }
    void free()  // (on the device the buffers live on)
    {
        for (int s = 0; s < 2; ++s) {
            for (int c = 0; c < N_COLS; ++c) (void)hipFree(d_col[s][c]);
            (void)hipFree(d_lo16[s]);
            (void)hipFree(d_bstart[s]);
        }
        *this = GatherTables();
    }
};

// ---- the wire: what one strand of one peer sends, message by message.  With CRP_GATHER_POS16: lo16, bucket starts,
// value, off-target, features; without: positions, value, off-target, features.  A strand with no rows sends nothing.
// The bytes a strand puts on the wire are the sum of its messages' `bytes` (bytes_to_root on both paths).
struct GatherSrc {  // the sender's side: its arena's owned rows from `first` on, and its packed positions
    const crp_arena *a;
    uint64_t first;
    const uint16_t *lo16;
    const uint32_t *bstart;
};
struct GatherDst {  // the root's side: the peer's place in the tables (rows) and in the staging area (elements)
    const GatherTables *t;
    uint64_t row, lo16_off, bstart_off;
};
struct WireMsg {
    int col;
    const void *src;  // nullptr where the caller gave no GatherSrc (the root of the process-per-GPU path)
    void *dst;        // nullptr where it gave no GatherDst (a peer of that path)
    uint64_t bytes;
};
constexpr int MAX_WIRE_MSGS = N_COLS + 1;

inline int wire_msgs(const GatherCols &g, int s, uint64_t rows, uint32_t buckets, const GatherSrc *src, const GatherDst *dst,
                     WireMsg out[MAX_WIRE_MSGS])
{
    int n = 0;
    for (int i = 0; i < g.n && rows; ++i) {
        const int c = g.col[i];
        if (c == COL_POS && g.pos16) {
            out[n++] = WireMsg{c, src ? src->lo16 : nullptr, dst ? dst->t->d_lo16[s] + dst->lo16_off : nullptr, rows * sizeof(uint16_t)};
            out[n++] = WireMsg{c, src ? src->bstart : nullptr, dst ? dst->t->d_bstart[s] + dst->bstart_off : nullptr, buckets * sizeof(uint32_t)};
        } else {
            out[n++] = WireMsg{c, src ? col_src(g, c, src->a, s, src->first) : nullptr, dst ? dst->t->at(c, s, dst->row) : nullptr, rows * COL_BYTES[c]};
        }
    }
    return n;
}

}  // namespace crp
