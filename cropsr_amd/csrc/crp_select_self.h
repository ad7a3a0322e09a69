// crp_select_self.h -- launch interface of crp_select_self.hip (guide selection for any nuclease: the K most specific
// guide sites of every gene, over the rows of a self-search handle), shared with its host side
// crp_select.cpp.  The items, the merge list, the partial lists and the merge kernel are crp_select.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crp_select.h"

struct crp_arena;
struct crp_search_self;

namespace crp {

// The candidates of a self-search handle in extraction order, and one result row each (crp_search_self.cpp).
struct SelfSelectRows {
    const uint32_t *hi, *lo;         // the oriented window's code bits (bit p = pattern position p; A=00 T=01 C=10 G=11)
    const uint32_t *pos;             // forward start | strand << 31
    const uint8_t *flag;             // 1: a guide site
    const uint32_t *counts;          // stride per candidate
    const unsigned long long *sum;   // hit_sum; null: an unscored handle
    const double *model;             // the on-target sum, NaN: none; null: the handle's model has not run
    uint32_t n;
    uint32_t stride;                 // M + 1
};

// The arena's annotation track as annot_lookup_kernel reads it, and the flag byte of every label-set string.
struct SelfSelectTrack {
    const uint32_t *points, *ids, *bucket;
    uint32_t last_bucket;
    const uint8_t *flags;            // null: no CDS filter
    uint32_t n_flags;
};

struct SelfSelectPredicate {
    unsigned long long max_hit_sum;  // read on a scored handle only
    uint32_t max_mm0;
    uint32_t T, cut;                 // the cut lies before pattern position `cut` of the oriented window: 1 .. T - 1
    uint32_t region;                 // the guide region's pattern positions
    uint32_t gc_min, gc_max, max_t_run;
    uint32_t seq_limits;             // 1: a GC or T-run limit is set (the code bits are read only then)
    int k;
    // the on-target model (crp_select_set_self_model; read by the kernel's model form only)
    double min_sum;                  // read when has_min
    uint32_t rank_model;             // 1: larger sum first (the key is self_select_model_key), a site without a sum fails
    uint32_t has_min;                // 1: a site passes only with a sum >= min_sum
};

// What crp_select_fetch_self copies: one entry per (gene, rank), all-ones where sel has no candidate.
struct SelfSelectGathered {
    uint32_t *pos, *hi, *lo, *counts;  // counts: stride per entry
    uint8_t *strand;
    unsigned long long *sum;
    double *model;                     // the on-target sum; NaN where sel has no candidate or the handle's model has not run
};

// run[g] = {first, end} of the candidates whose 64-position word can hold a start in [lo - T, hi] (a superset of the
// gene's rows; the exact test is the item kernel's)
hipError_t launch_select_self_bounds(hipStream_t s, const uint32_t *cand_pos, uint32_t n_cand, uint32_t T, const uint32_t *lo, const uint32_t *hi,
                                     uint32_t n_genes, uint2 *run);
// One wave per item: rows [first[0], first[0] + rows[0]) of the candidates (first[1], rows[1] are not read).  model: the
// kernel's form that reads rows.model (pred.rank_model or pred.has_min is set; rows.model is not null).
hipError_t launch_select_self_items(hipStream_t s, const SelfSelectRows &rows, const SelfSelectTrack &track, const SelfSelectPredicate &pred,
                                    const uint32_t *gene_lo, const uint32_t *gene_hi, const SelectItem *items, uint32_t n_items,
                                    const SelectPartials &part, const SelectResult &res, bool model);
// One lane per entry of sel (n_entries = genes x K).
hipError_t launch_select_self_gather(hipStream_t s, const SelfSelectRows &rows, const uint32_t *sel, uint64_t n_entries,
                                     const SelfSelectGathered &out);

// What a selection needs of a self-search handle (crp_search_self.cpp); *compared is false while the handle has not been the
// query of a compare on every segment 0 .. M.
struct SelfSelectHandle {
    SelfSelectRows rows;
    const struct ::crp_arena *arena;
    int T, pam_len, max_mm;
    bool pam3, scored;
    uint32_t region;
    uint64_t n;  // the candidates, uncut (rows.n is 32 bits)
};
void self_select_handle(const struct ::crp_search_self *s, SelfSelectHandle *out, bool *compared);

}  // namespace crp
