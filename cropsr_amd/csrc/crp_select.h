// crp_select.h -- launch interface of crp_select.hip (guide selection: the best K rows of every gene, DESIGN section
// 16), shared with its host side crp_select.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace crp {

constexpr int SELECT_WAVES = 4;                 // work items per workgroup: one wave each
constexpr uint32_t SELECT_NONE = 0xFFFFFFFFu;   // no row / an item that writes the gene's result itself
constexpr uint32_t SELECT_MAX_ITEMS = 1u << 20; // work items per launch

// The columns of one strand's table, as far as a run reads them (feat / counts / sum may be null).
struct SelectTable {
    const uint32_t *pos;
    const double *score;
    const uint32_t *feat;              // label-set ids (require_cds)
    const uint32_t *counts;            // joined self-search counts, `stride` per row: counts[0] is read
    const unsigned long long *sum;     // joined hit_sum
    const uint32_t *props;             // packed guide properties (property limits)
    const unsigned long long *repair;  // mh | oof << 32 of crp_repair_scores (repair limits)
    uint32_t n;
    const uint32_t *variants;          // packed variant counts of crp_variant_counts (variant limits)
    const unsigned long long *sites;   // in_guide | assay << 32 of crp_site_columns (site limits)
};

struct SelectPredicate {
    double min_score;
    unsigned long long max_hit_sum;
    uint32_t max_mm0;
    uint32_t stride;        // 0: no joined columns
    const uint8_t *flags;   // null: no CDS filter
    uint32_t n_flags;
    int k;
    // with SelectTable::props: gc_min <= gc <= gc_max, run <= max_run, t_run <= max_t_run, stem <= max_stem (each one byte)
    uint32_t gc_min, gc_max, max_run, max_t_run, max_stem;
    // with SelectTable::repair: mh >= min_mh and 100 oof >= min_oof_pct mh, and mh > 0 where min_oof_pct > 0
    uint32_t min_mh, min_oof_pct;
    // with SelectTable::variants: site <= max_var_site, guide <= max_var_guide, seed <= max_var_seed, pam <= max_var_pam (each one byte)
    uint32_t max_var_site, max_var_guide, max_var_seed, max_var_pam;
    // with SelectTable::sites: no enzyme of forbid_sites inside the guide, and -- need_assay != 0 -- an assay with one of need_assay's
    uint32_t forbid_sites, need_assay;
};

// One wave's work: rows [first[s], first[s] + rows[s]) of strand s's table, all inside gene `gene`'s runs.  slot ==
// SELECT_NONE: the item is the whole gene and writes its result; else it writes its partial list to that slot.
struct SelectItem {
    uint32_t gene, slot;
    uint32_t first[2], rows[2];
};

// A gene that was cut into several items: their slots are consecutive.
struct SelectMerge {
    uint32_t gene, slot, n_slots;
};

// The partial lists: k entries per slot (key = the score's bits, tie = cut site << 1 | strand, row = row | strand << 31;
// row SELECT_NONE: no entry) and two counts (rows in the gene, passing rows).
struct SelectPartials {
    unsigned long long *key;
    uint32_t *tie, *row, *cnt;
};

struct SelectResult {
    uint32_t *n_in, *n_pass, *sel;
};

// bounds[g] = {first '+' row with cut >= lo, first with cut > hi, the same for '-'}
hipError_t launch_select_bounds(hipStream_t s, const uint32_t *pos_plus, uint32_t n_plus, const uint32_t *pos_minus, uint32_t n_minus,
                                const uint32_t *lo, const uint32_t *hi, uint32_t n_genes, uint4 *bounds);
hipError_t launch_select_items(hipStream_t s, const SelectTable &plus, const SelectTable &minus, const SelectPredicate &pred,
                               const SelectItem *items, uint32_t n_items, const SelectPartials &part, const SelectResult &res);
hipError_t launch_select_merge(hipStream_t s, const SelectMerge *genes, uint32_t n_genes, int k, const SelectPartials &part,
                               const SelectResult &res);

// ---- guide pairs (crp_select_pairs.hip): the best KP deletion pairs of every gene ----------------
struct PairParams {
    int k;                   // KP
    uint32_t dmin, dmax;     // 1 <= dmin <= dmax <= 65 535
    uint32_t mask;           // orientation bits, bit sa * 2 + sb
    uint32_t frameshift;     // 1: D mod 3 != 0
};

// One wave's work: the a-rows [first[s], first[s] + rows[s]) of strand s's table, inside gene `gene`'s runs
// run[0] .. run[1] ('+') and run[2] .. run[3] ('-'), where its partners are looked for.  slot as SelectItem's.
struct PairItem {
    uint32_t gene, slot;
    uint32_t first[2], rows[2];
    uint32_t run[4];
};

// The partial lists: k entries per slot -- kmin / kmax (the smaller and the larger score's bits), tie = c_a << 32 | c_b,
// a / b (row | strand << 31; a SELECT_NONE: no entry) -- and per slot the passing a-rows and the qualifying pairs.
struct PairPartials {
    unsigned long long *kmin, *kmax, *tie;
    uint32_t *a, *b, *n_pass;
    unsigned long long *n_pairs;
};

struct PairResult {
    uint32_t *n_pass;             // per gene
    unsigned long long *n_pairs;  // per gene
    uint32_t *pairs;              // per gene k * 2: a then b
};

// key[row] = the score's bits where the row passes the predicate, else 0 (one lane per row)
hipError_t launch_pair_pass_key(hipStream_t s, const SelectTable &table, const SelectPredicate &pred, unsigned long long *key);
// evals[item] = partner rows the item streamed
hipError_t launch_pair_items(hipStream_t s, const uint32_t *pos_plus, const uint32_t *pos_minus, const unsigned long long *key_plus,
                             const unsigned long long *key_minus, const PairParams &pp, const PairItem *items, uint32_t n_items,
                             unsigned long long *evals, const PairPartials &part, const PairResult &res);
hipError_t launch_pair_merge(hipStream_t s, const SelectMerge *genes, uint32_t n_genes, int k, const PairPartials &part,
                             const PairResult &res);

}  // namespace crp
