// crp_select.cpp -- host side of the guide selection (include/cropsr_hip.h, crp_select_*): the
// handle, the checks of what a run needs to find in HBM, and the cut of the genes' runs into work items between the
// bounds kernel and the select launches (crp_select.hip).
#include <algorithm>
#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "crp_internal.h"
#include "crp_roctx.h"
#include "crp_search_self.h"
#include "crp_select.h"
#include "crp_select_coding.h"
#include "crp_select_edit.h"
#include "crp_select_family.h"
#include "crp_select_family_set.h"
#include "crp_select_pairs_distinct.h"
#include "crp_search_family.h"
#include "crp_select_self.h"
#include "crp_select_spaced.h"
#include "crp_select_splice.h"

struct crp_select {
    crp_arena *arena = nullptr;
    crp_ctx *ctx = nullptr;
    uint64_t n_genes = 0;
    uint64_t slice_rows = CRP_SELECT_DEFAULT_SLICE_ROWS;
    uint32_t *d_lo = nullptr, *d_hi = nullptr;
    uint4 *d_bounds = nullptr;
    uint8_t *d_flags = nullptr;
    uint64_t flags_cap = 0, n_flags = 0;
    bool have_flags = false;
    crp::SelectItem *d_items = nullptr;
    uint64_t items_cap = 0;
    crp::SelectMerge *d_merge = nullptr;
    uint64_t merge_cap = 0;
    crp::SelectPartials part = {};
    uint64_t part_entries_cap = 0, part_tie_cap = 0, part_row_cap = 0, part_cnt_cap = 0;
    crp::SelectResult res = {};  // n_in, n_pass: n_genes; sel: n_genes * k of the last run
    uint64_t sel_cap = 0;
    int k = 0;  // of the last successful run (0: none)
    bool have_prop_limits = false;
    crp_select_property_limits prop_limits = {};
    bool have_repair_limits = false;
    crp_select_repair_limits repair_limits = {};
    bool have_variant_limits = false;
    crp_select_variant_limits variant_limits = {};
    bool have_site_limits = false;
    uint32_t forbid_sites = 0, need_assay = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};
    double stats[9] = {};
    // guide pairs: buffers and results of crp_select_run_pairs, apart from the selection's
    uint64_t pair_slice_rows = CRP_SELECT_DEFAULT_PAIR_SLICE_ROWS;
    unsigned long long *d_pass_key[2] = {nullptr, nullptr};
    uint64_t pass_key_cap[2] = {0, 0};
    crp::PairItem *d_pair_items = nullptr;
    uint64_t pair_items_cap = 0;
    crp::SelectMerge *d_pair_merge = nullptr;
    uint64_t pair_merge_cap = 0;
    unsigned long long *d_pair_evals = nullptr;
    uint64_t pair_evals_cap = 0;
    crp::PairPartials pair_part = {};
    uint64_t pair_part_cap[7] = {};
    crp::PairResult pair_res = {};  // n_pass, n_pairs: n_genes; pairs: n_genes * kp * 2 of the last run
    uint64_t pair_res_cap[3] = {};
    int kp = 0;  // of the last successful crp_select_run_pairs (0: none)
    double pair_stats[8] = {};
    // coding position: the model of the handle's genes -- info, length, first (n_genes + 1), at, word,
    // cum -- the limits, and the queries and answers of crp_select_coding_eval
    uint32_t *d_cod[6] = {};
    uint64_t cod_cap[6] = {};
    bool have_coding = false;
    uint64_t coding_steps = 0;
    bool have_coding_limits = false;
    crp_select_coding_limits coding_limits = {};
    uint32_t *d_eval[4] = {};
    uint64_t eval_cap[4] = {};
    double coding_stats[3] = {};
    // base editing: the window and the limits of the selection, and what the last launches took
    bool have_edit_limits = false;
    crp_select_edit_window edit_window = {4, 8};
    crp_select_edit_limits edit_limits = {};
    double edit_stats[3] = {};
    // splice-site editing: window, editor and limits of the selection, and what the last launches took
    bool have_splice_limits = false;
    crp_select_edit_window splice_window = {4, 8};
    uint32_t splice_editor = CRP_EDITOR_CBE;
    crp_select_splice_limits splice_limits = {};
    double splice_stats[3] = {};
    // gene families: per gene its family and that family's size, the limits, the answers of the eval
    uint32_t *d_gene_family = nullptr, *d_family_size = nullptr;
    uint64_t gene_family_cap = 0, family_size_cap = 0;
    bool have_family = false, have_family_limits = false;
    crp_select_family_limits family_limits = {};
    unsigned long long *d_family_eval_sum = nullptr;
    uint64_t family_eval_sum_cap = 0;
    double family_stats[2] = {};
    // family sets: per gene its member bit, and the plan of crp_select_family_step -- the items of
    // the family genes, their proposals, the family -> item list -- with what it was built for
    uint32_t *d_gene_member = nullptr;
    uint64_t gene_member_cap = 0;
    bool have_members = false, set_plan_valid = false;
    crp::SelectItem *d_set_items = nullptr;
    crp::FamilyProposal *d_set_prop = nullptr, *d_set_best = nullptr;
    uint32_t *d_set_start = nullptr, *d_set_slots = nullptr;
    unsigned long long *d_set_covered = nullptr;
    uint64_t set_cap[6] = {};
    uint64_t set_items = 0, set_rows = 0, set_families = 0, set_plan_slice = 0, set_plan_hits[2] = {0, 0};
    crp_select_params set_plan_params = {};
    double set_stats[6] = {};
    // spaced selection: results and buffers of crp_select_run_spaced, apart from the selection's; the
    // pass keys are the pair path's (d_pass_key)
    crp::SpacedResult spaced_res = {};  // n_pass, n_spaced: n_genes; sel: n_genes * ks of the last run
    crp::SpacedRounds spaced_rounds = {};
    crp::SelectItem *d_spaced_items = nullptr;
    crp::SelectMerge *d_spaced_merge = nullptr;
    uint64_t spaced_cap[10] = {};
    int ks = 0;  // of the last successful crp_select_run_spaced (0: none)
    double spaced_stats[9] = {};
    // self selection: results and buffers of crp_select_run_self, apart from the selection's; the
    // items, the merge list and the partial lists are the selection's (scratch of one run)
    crp::SelectResult self_res = {};  // n_in, n_pass: n_genes; sel: n_genes * kself of the last run
    crp::SelfSelectGathered self_got = {};  // n_genes * kself entries, beside sel
    uint2 *d_self_run = nullptr;
    uint64_t self_cap[11] = {};
    uint64_t self_items_per_launch = crp::SELECT_MAX_ITEMS;
    bool self_rank_model = false, self_has_min = false;  // crp_select_set_self_model
    double self_min_sum = 0.0;
    int kself = 0;        // of the last successful crp_select_run_self (0: none)
    int self_stride = 0;  // M + 1 of that run's handle
    double self_stats[7] = {};
    // distinct pairs: results and buffers of crp_select_run_pairs_distinct, apart from the pair run's;
    // the pass keys are the pair path's (d_pass_key)
    crp::PairDistinctResult pd_res = {};  // n_pass, n_pairs, n_distinct: n_genes; pairs: n_genes * kpd * 2 of the last run
    crp::PairDistinctRounds pd_rounds = {};
    crp::PairItem *d_pd_items = nullptr;
    crp::SelectMerge *d_pd_merge = nullptr;
    unsigned long long *d_pd_evals = nullptr;
    uint64_t pd_cap[11] = {};
    uint64_t pd_items_per_launch = crp::SELECT_MAX_ITEMS;
    int kpd = 0;  // of the last successful crp_select_run_pairs_distinct (0: none)
    double pd_stats[12] = {};
};

namespace {

double elapsed(hipEvent_t a, hipEvent_t b)
{
    float ms = 0.f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.0;
}

int fail(crp_ctx *ctx, int rc, const std::string &text)
{
    ctx->last_error = text;
    return rc;
}

}  // namespace

namespace {

// What crp_select_run and crp_select_run_pairs ask of their arguments and of the arena (`who`: the caller's name).
int check_run(crp_select *s, const crp_select_params *p, crp_search_self *self, crp::SelfJoined *joined, const char *who_c)
{
    crp_ctx *ctx = s->ctx;
    crp_arena *a = s->arena;
    const std::string who = who_c;
    if (std::isnan(p->min_score)) return fail(ctx, CRP_ERR_INVALID, who + ": min_score is not a number");
    if (!a->have_hits || a->pend_guide_len != 20)
        return fail(ctx, CRP_ERR_STATE, who + ": the arena has no hit tables of guide length 20 (the ranking key exists only there)");
    if (p->require_cds && !s->have_flags) return fail(ctx, CRP_ERR_STATE, who + ": require_cds needs crp_select_set_flags");
    if (p->require_cds && !a->have_feat)
        return fail(ctx, CRP_ERR_STATE, who + ": require_cds needs the ids of a crp_annotate_lookup on the current tables");
    if (s->have_prop_limits && !a->have_props)
        return fail(ctx, CRP_ERR_STATE, who + ": property limits need the column of a crp_guide_properties on the current tables");
    if (s->have_repair_limits && !a->have_repair)
        return fail(ctx, CRP_ERR_STATE, who + ": repair limits need the column of a crp_repair_scores on the current tables");
    if (s->have_variant_limits && !a->have_variants)
        return fail(ctx, CRP_ERR_STATE, who + ": variant limits need the column of a crp_variant_counts on the current tables");
    if (s->have_site_limits && !a->have_site_col)
        return fail(ctx, CRP_ERR_STATE, who + ": site limits need the column of a crp_site_columns on the current tables");
    if (self) {
        if (!crp::self_joined(self, joined))
            return fail(ctx, CRP_ERR_STATE, who + ": the self-search handle has no joined columns (crp_search_self_join_hits)");
        if (joined->arena != a) return fail(ctx, CRP_ERR_INVALID, who + ": the self-search handle belongs to another arena");
        if (joined->rows[0] != a->n_hits[0] || joined->rows[1] != a->n_hits[1])
            return fail(ctx, CRP_ERR_STATE, who + ": the joined columns belong to an earlier scan's tables");
    }
    return CRP_OK;
}

// What crp_select_run_pairs and crp_select_run_pairs_distinct ask of their arguments, of the handle's limits and of the arena.
int check_pair_run(crp_select *s, const crp_select_params *p, const crp_select_pair_params *q, crp_search_self *self, crp::SelfJoined *joined,
                   const char *who_c)
{
    crp_ctx *ctx = s->ctx;
    const std::string who = who_c;
    if (q->k < 1 || q->k > CRP_SELECT_PAIRS_MAX_K)
        return fail(ctx, CRP_ERR_INVALID, who + ": k must be 1.." + std::to_string(CRP_SELECT_PAIRS_MAX_K) + ", not " + std::to_string(q->k));
    if (q->dmin < 1 || q->dmin > q->dmax || q->dmax > CRP_SELECT_PAIRS_MAX_DISTANCE)
        return fail(ctx, CRP_ERR_INVALID, who + ": the distances must be 1 <= dmin <= dmax <= " + std::to_string(CRP_SELECT_PAIRS_MAX_DISTANCE) +
                                              ", not " + std::to_string(q->dmin) + " and " + std::to_string(q->dmax));
    if (q->orientation_mask < 1 || q->orientation_mask > 0xFu)
        return fail(ctx, CRP_ERR_INVALID, who + ": the orientation mask must be 1..15, not " + std::to_string(q->orientation_mask));
    if (s->have_family_limits)
        return fail(ctx, CRP_ERR_UNSUPPORTED, who + ": family limits are relative to the gene and the pairs' eligibility key is per table row: "
                                                    "clear them (crp_select_set_family_limits(select, NULL)) for a pair selection");
    if (s->have_coding_limits)
        return fail(ctx, CRP_ERR_UNSUPPORTED, who + ": coding limits are relative to the gene and the pairs' eligibility key is per table row: "
                                                    "clear them (crp_select_set_coding_limits(select, NULL)) for a pair selection");
    if (s->have_edit_limits)
        return fail(ctx, CRP_ERR_UNSUPPORTED, who + ": edit limits are relative to the gene and the pairs' eligibility key is per table row: "
                                                    "clear them (crp_select_set_edit_limits(select, NULL, NULL)) for a pair selection");
    if (s->have_splice_limits)
        return fail(ctx, CRP_ERR_UNSUPPORTED, who + ": splice limits are relative to the gene and the pairs' eligibility key is per table row: "
                                                    "clear them (crp_select_set_splice_limits(select, NULL, 0, NULL)) for a pair selection");
    return check_run(s, p, self, joined, who_c);
}

// The two tables and the predicate of a run, as the kernels take them (k: the selection's K; the pair kernels do not read it).
void fill_predicate(const crp_select *s, const crp_select_params *p, bool with_self, const crp::SelfJoined &joined, int k,
                    crp::SelectTable tab[2], crp::SelectPredicate *pred_out)
{
    const crp_arena *a = s->arena;
    for (int t = 0; t < 2; ++t)
        tab[t] = crp::SelectTable{a->d_pos[t], a->d_score[t], p->require_cds ? a->d_feat[t] : nullptr, with_self ? joined.counts[t] : nullptr,
                                  with_self ? joined.sum[t] : nullptr, s->have_prop_limits ? a->d_props[t] : nullptr,
                                  s->have_repair_limits ? reinterpret_cast<const unsigned long long *>(a->d_repair[t]) : nullptr, (uint32_t)a->n_hits[t],
                                  s->have_variant_limits ? a->d_variants[t] : nullptr,
                                  s->have_site_limits ? reinterpret_cast<const unsigned long long *>(a->d_sites[t]) : nullptr};
    crp::SelectPredicate pred = {};
    pred.min_score = p->min_score;
    pred.max_hit_sum = p->max_hit_sum;
    pred.max_mm0 = p->max_mm0;
    pred.stride = with_self ? (uint32_t)joined.stride : 0u;
    pred.flags = p->require_cds ? s->d_flags : nullptr;
    pred.n_flags = (uint32_t)s->n_flags;
    pred.k = k;
    pred.gc_min = s->prop_limits.gc_min;
    pred.gc_max = s->prop_limits.gc_max;
    pred.max_run = s->prop_limits.max_run;
    pred.max_t_run = s->prop_limits.max_t_run;
    pred.max_stem = s->prop_limits.max_stem;
    pred.min_mh = s->repair_limits.min_mh;
    pred.min_oof_pct = s->repair_limits.min_oof_pct;
    pred.max_var_site = s->variant_limits.max_site;
    pred.max_var_guide = s->variant_limits.max_guide;
    pred.max_var_seed = s->variant_limits.max_seed;
    pred.max_var_pam = s->variant_limits.max_pam;
    pred.forbid_sites = s->forbid_sites;
    pred.need_assay = s->need_assay;
    *pred_out = pred;
}

// The joined plain and family columns of `self` and the handle's per-gene families, as the family kernels take them.
int family_columns(crp_select *s, crp_search_self *self, const char *who_c, crp::SelectFamily *out)
{
    crp_ctx *ctx = s->ctx;
    crp_arena *a = s->arena;
    const std::string who = who_c;
    if (!s->have_family) return fail(ctx, CRP_ERR_STATE, who + ": the handle has no families (crp_select_set_family)");
    crp::SelfJoined joined = {};
    crp::SelfFamilyJoined fj = {};
    if (!self || !crp::self_joined(self, &joined))
        return fail(ctx, CRP_ERR_STATE, who + ": families need a self-search handle with joined columns (crp_search_self_join_hits)");
    if (!crp::self_family_joined(self, &fj))
        return fail(ctx, CRP_ERR_STATE, who + ": the self-search handle has no joined family columns (crp_search_self_family_join_hits)");
    if (joined.arena != a) return fail(ctx, CRP_ERR_INVALID, who + ": the self-search handle belongs to another arena");
    for (int t = 0; t < 2; ++t)
        if (joined.rows[t] != a->n_hits[t] || fj.rows[t] != a->n_hits[t])
            return fail(ctx, CRP_ERR_STATE, who + ": the joined columns belong to an earlier scan's tables");
    for (int t = 0; t < 2; ++t) {
        out->counts[t] = joined.counts[t];
        out->sum[t] = joined.sum[t];
        out->fam_counts[t] = fj.counts[t];
        out->fam_sum[t] = fj.sum[t];
        out->fam_cover[t] = fj.cover[t];
        out->site_family[t] = fj.family[t];
    }
    out->stride = (uint32_t)joined.stride;
    out->gene_family = s->d_gene_family;
    out->gene_size = s->d_family_size;
    return CRP_OK;
}

// A window of protospacer positions 1 <= lo <= hi <= 20 (NULL: the default, 4 .. 8).
int check_window(crp_ctx *ctx, const crp_select_edit_window *w, const std::string &who, crp::EditWindow *out)
{
    *out = w ? crp::EditWindow{w->lo, w->hi} : crp::EditWindow{4u, 8u};
    if (out->lo < 1u || out->lo > out->hi || out->hi > crp::EDIT_GUIDE_LEN)
        return fail(ctx, CRP_ERR_INVALID, who + ": the window is 1 <= lo <= hi <= 20 in protospacer positions, not " + std::to_string(out->lo) +
                                              " and " + std::to_string(out->hi));
    return CRP_OK;
}

}  // namespace

extern "C" {

int crp_select_create(crp_arena *a, const uint32_t *lo, const uint32_t *hi, uint64_t n_genes, crp_select **out)
{
    if (!a || !out || (n_genes && (!lo || !hi)) || n_genes > 0x7fffffffull) return CRP_ERR_INVALID;
    *out = nullptr;
    if (!a->sealed) return CRP_ERR_STATE;
    crp_ctx *ctx = a->ctx;
    for (uint64_t g = 0; g < n_genes; ++g)
        if (lo[g] > hi[g] || hi[g] > 0x7fffffffu)
            return fail(ctx, CRP_ERR_INVALID, "crp_select_create: gene " + std::to_string(g) + " is no range of arena positions");
    crp_select *s = new (std::nothrow) crp_select();
    if (!s) return CRP_ERR_NOMEM;
    s->arena = a;
    s->ctx = ctx;
    s->n_genes = n_genes;
    int rc = CRP_OK;
    if (hipSetDevice(ctx->device) != hipSuccess || hipEventCreate(&s->ev[0]) != hipSuccess || hipEventCreate(&s->ev[1]) != hipSuccess)
        rc = fail(ctx, CRP_ERR_HIP, "crp_select_create: no HIP events");
    uint64_t cap = 0;
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_lo), &cap, n_genes, sizeof(uint32_t));
    cap = 0;
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_hi), &cap, n_genes, sizeof(uint32_t));
    cap = 0;
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_bounds), &cap, n_genes, sizeof(uint4));
    cap = 0;
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->res.n_in), &cap, n_genes, sizeof(uint32_t));
    cap = 0;
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->res.n_pass), &cap, n_genes, sizeof(uint32_t));
    if (rc == CRP_OK && n_genes) {
        rc = crp::staged_h2d(ctx, s->d_lo, lo, n_genes * sizeof(uint32_t));
        if (rc == CRP_OK) rc = crp::staged_h2d(ctx, s->d_hi, hi, n_genes * sizeof(uint32_t));
        if (rc == CRP_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = CRP_ERR_HIP;
    }
    if (rc != CRP_OK) {
        crp_select_destroy(s);
        return rc;
    }
    *out = s;
    return CRP_OK;
}

int crp_select_destroy(crp_select *s)
{
    if (!s) return CRP_OK;
    (void)hipSetDevice(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);
    void *bufs[] = {s->d_lo, s->d_hi, s->d_bounds, s->d_flags, s->d_items, s->d_merge, s->part.key, s->part.tie,
                    s->part.row, s->part.cnt, s->res.n_in, s->res.n_pass, s->res.sel, s->d_pass_key[0], s->d_pass_key[1], s->d_pair_items,
                    s->d_pair_merge, s->d_pair_evals, s->pair_part.kmin, s->pair_part.kmax, s->pair_part.tie, s->pair_part.a, s->pair_part.b,
                    s->pair_part.n_pass, s->pair_part.n_pairs, s->pair_res.n_pass, s->pair_res.n_pairs, s->pair_res.pairs,
                    s->d_cod[0], s->d_cod[1], s->d_cod[2], s->d_cod[3], s->d_cod[4], s->d_cod[5], s->d_eval[0], s->d_eval[1], s->d_eval[2],
                    s->d_eval[3], s->d_gene_family, s->d_family_size, s->d_family_eval_sum, s->d_gene_member, s->d_set_items, s->d_set_prop,
                    s->d_set_best, s->d_set_start, s->d_set_slots, s->d_set_covered, s->spaced_res.n_pass, s->spaced_res.n_spaced, s->spaced_res.sel,
                    s->spaced_rounds.cuts, s->spaced_rounds.last, s->spaced_rounds.prop, s->spaced_rounds.slot_pass, s->spaced_rounds.picked,
                    s->d_spaced_items, s->d_spaced_merge, s->self_res.n_in, s->self_res.n_pass, s->self_res.sel, s->self_got.pos,
                    s->self_got.hi, s->self_got.lo, s->self_got.counts, s->self_got.strand, s->self_got.sum, s->self_got.model, s->d_self_run,
                    s->pd_res.n_pass, s->pd_res.n_pairs, s->pd_res.n_distinct, s->pd_res.pairs, s->pd_rounds.prop, s->pd_rounds.slot_pass,
                    s->pd_rounds.slot_pairs, s->pd_rounds.picked, s->d_pd_items, s->d_pd_merge, s->d_pd_evals};
    for (void *p : bufs) (void)hipFree(p);
    for (hipEvent_t e : s->ev)
        if (e) (void)hipEventDestroy(e);
    delete s;
    return CRP_OK;
}

int crp_select_set_flags(crp_select *s, const uint8_t *flags, uint64_t n_flags)
{
    if (!s || (n_flags && !flags) || n_flags > 0xfffffffeull) return CRP_ERR_INVALID;
    crp_ctx *ctx = s->ctx;
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    s->have_flags = false;
    int rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_flags), &s->flags_cap, n_flags, 1);
    if (rc == CRP_OK && n_flags) rc = crp::staged_h2d(ctx, s->d_flags, flags, n_flags);
    if (rc != CRP_OK) return rc;
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->n_flags = n_flags;
    s->have_flags = true;
    return CRP_OK;
}

int crp_select_set_limits(crp_select *s, uint64_t slice_rows)
{
    if (!s) return CRP_ERR_INVALID;
    if (slice_rows && (slice_rows < CRP_SELECT_MIN_SLICE_ROWS || slice_rows > 0x40000000ull)) return CRP_ERR_INVALID;
    s->slice_rows = slice_rows ? slice_rows : CRP_SELECT_DEFAULT_SLICE_ROWS;
    s->set_plan_valid = false;
    return CRP_OK;
}

int crp_select_set_property_limits(crp_select *s, const crp_select_property_limits *limits)
{
    if (!s) return CRP_ERR_INVALID;
    s->have_prop_limits = limits != nullptr;
    if (limits) s->prop_limits = *limits;
    return CRP_OK;
}

int crp_select_set_repair_limits(crp_select *s, const crp_select_repair_limits *limits)
{
    if (!s) return CRP_ERR_INVALID;
    if (limits && limits->min_oof_pct > 100u)
        return fail(s->arena->ctx, CRP_ERR_INVALID,
                    "crp_select_set_repair_limits: min_oof_pct is a percentage 0..100, not " + std::to_string(limits->min_oof_pct));
    s->have_repair_limits = limits != nullptr;
    s->repair_limits = limits ? *limits : crp_select_repair_limits{};
    return CRP_OK;
}

int crp_select_set_variant_limits(crp_select *s, const crp_select_variant_limits *limits)
{
    if (!s) return CRP_ERR_INVALID;
    s->have_variant_limits = limits != nullptr;
    s->variant_limits = limits ? *limits : crp_select_variant_limits{};
    return CRP_OK;
}

int crp_select_set_site_limits(crp_select *s, uint32_t forbid_mask, uint32_t need_mask)
{
    if (!s) return CRP_ERR_INVALID;
    s->have_site_limits = forbid_mask != 0 || need_mask != 0;
    s->forbid_sites = forbid_mask;
    s->need_assay = need_mask;
    return CRP_OK;
}

int crp_select_run(crp_select *s, const crp_select_params *p, crp_search_self *self)
{
    crp::Range roctx_range("crp: guide selection");
    if (!s || !p) return CRP_ERR_INVALID;
    crp_ctx *ctx = s->ctx;
    crp_arena *a = s->arena;
    s->k = 0;
    if (p->k < 1 || p->k > CRP_SELECT_MAX_K)
        return fail(ctx, CRP_ERR_INVALID, "crp_select_run: k must be 1.." + std::to_string(CRP_SELECT_MAX_K) + ", not " + std::to_string(p->k));
    crp::SelfJoined joined = {};
    int rc = check_run(s, p, self, &joined, "crp_select_run");
    if (rc != CRP_OK) return rc;
    if (s->have_coding_limits && !s->have_coding)
        return fail(ctx, CRP_ERR_STATE, "crp_select_run: coding limits need the model of a crp_select_set_coding");
    if (s->have_edit_limits && s->have_coding_limits)
        return fail(ctx, CRP_ERR_UNSUPPORTED, "crp_select_run: edit limits and coding limits are two kernels' predicates: clear one of them "
                                              "(crp_select_set_coding_limits(select, NULL) or crp_select_set_edit_limits(select, NULL, NULL))");
    if (s->have_edit_limits && !s->have_coding)
        return fail(ctx, CRP_ERR_STATE, "crp_select_run: edit limits need the model of a crp_select_set_coding");
    if (s->have_splice_limits && s->have_coding_limits)
        return fail(ctx, CRP_ERR_UNSUPPORTED, "crp_select_run: splice limits and coding limits are two kernels' predicates: clear one of them "
                                              "(crp_select_set_coding_limits(select, NULL) or crp_select_set_splice_limits(select, NULL, 0, NULL))");
    if (s->have_splice_limits && s->have_edit_limits && s->splice_editor != CRP_EDITOR_CBE)
        return fail(ctx, CRP_ERR_UNSUPPORTED, "crp_select_run: an adenine editor writes no stop codon: clear the edit limits "
                                              "(crp_select_set_edit_limits(select, NULL, NULL)) or set the splice limits for CRP_EDITOR_CBE");
    if (s->have_splice_limits && !s->have_coding)
        return fail(ctx, CRP_ERR_STATE, "crp_select_run: splice limits need the model of a crp_select_set_coding");
    crp::SelectFamily family = {};
    if (s->have_family_limits) {
        if (s->have_coding_limits || s->have_edit_limits || s->have_splice_limits)
            return fail(ctx, CRP_ERR_UNSUPPORTED, "crp_select_run: family limits and coding, edit or splice limits are different kernels' "
                                                  "predicates: clear one of them (crp_select_set_family_limits(select, NULL))");
        rc = family_columns(s, self, "crp_select_run", &family);
        if (rc != CRP_OK) return rc;
    }
    s->family_stats[0] = 0;
    s->coding_stats[0] = 0;
    s->edit_stats[0] = 0;
    s->splice_stats[0] = 0;
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    const int k = p->k;
    const uint64_t G = s->n_genes;
    rc = crp::grow(ctx, reinterpret_cast<void **>(&s->res.sel), &s->sel_cap, G * k, sizeof(uint32_t));
    if (rc != CRP_OK) return rc;
    for (double &v : s->stats) v = 0;
    if (!G) {
        s->k = k;
        return CRP_OK;
    }
    // (a table has fewer rows than the arena positions: below 2^31)
    const uint32_t n_plus = (uint32_t)a->n_hits[0], n_minus = (uint32_t)a->n_hits[1];
    CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
    CRP_HIP(ctx, crp::launch_select_bounds(ctx->stream, a->d_pos[0], n_plus, a->d_pos[1], n_minus, s->d_lo, s->d_hi, (uint32_t)G, s->d_bounds));
    CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
    std::vector<uint4> bounds;
    std::vector<crp::SelectItem> items;
    std::vector<crp::SelectMerge> merges;
    uint64_t n_slots = 0, rows_covered = 0;
    try {
        bounds.resize(G);
        rc = crp::staged_d2h(ctx, bounds.data(), s->d_bounds, G * sizeof(uint4));
        if (rc != CRP_OK) return rc;
        CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        s->stats[0] = elapsed(s->ev[0], s->ev[1]);
        // every gene's rows -- its '+' run, then its '-' run -- in pieces of at most slice_rows rows; a gene without rows
        // still gets one (empty) item, which writes its zeros
        items.reserve(G + G / 8);
        for (uint64_t g = 0; g < G; ++g) {
            const uint4 b = bounds[g];
            if (b.x > b.y || b.y > n_plus || b.z > b.w || b.w > n_minus)
                return fail(ctx, CRP_ERR_HIP, "crp_select_run: the bounds of gene " + std::to_string(g) + " lie outside the tables");
            const uint64_t np = b.y - b.x, nm = b.w - b.z, total = np + nm;
            rows_covered += total;
            const uint64_t pieces = std::max<uint64_t>(1, (total + s->slice_rows - 1) / s->slice_rows);
            if (n_slots + pieces > 0xfffffff0ull || items.size() + pieces > 0xfffffff0ull) return CRP_ERR_UNSUPPORTED;
            if (pieces > 1) merges.push_back(crp::SelectMerge{(uint32_t)g, (uint32_t)n_slots, (uint32_t)pieces});
            for (uint64_t c = 0; c < pieces; ++c) {
                // rows [r0, r1) of the gene's concatenated runs
                const uint64_t r0 = c * s->slice_rows, r1 = std::min(total, r0 + s->slice_rows);
                const uint64_t p0 = std::min(r0, np), p1 = std::min(r1, np);
                const uint64_t m0 = std::max(r0, np) - np, m1 = std::max(r1, np) - np;
                crp::SelectItem it;
                it.gene = (uint32_t)g;
                it.slot = pieces > 1 ? (uint32_t)(n_slots + c) : crp::SELECT_NONE;
                it.first[0] = b.x + (uint32_t)p0;
                it.rows[0] = (uint32_t)(p1 - p0);
                it.first[1] = b.z + (uint32_t)m0;
                it.rows[1] = (uint32_t)(m1 - m0);
                items.push_back(it);
            }
            if (pieces > 1) n_slots += pieces;
        }
    } catch (const std::bad_alloc &) {
        return CRP_ERR_NOMEM;
    }
    rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_items), &s->items_cap, items.size(), sizeof(crp::SelectItem));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_merge), &s->merge_cap, merges.size(), sizeof(crp::SelectMerge));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->part.key), &s->part_entries_cap, n_slots * k, sizeof(uint64_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->part.tie), &s->part_tie_cap, n_slots * k, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->part.row), &s->part_row_cap, n_slots * k, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->part.cnt), &s->part_cnt_cap, n_slots * 2, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::staged_h2d(ctx, s->d_items, items.data(), items.size() * sizeof(crp::SelectItem));
    if (rc == CRP_OK && !merges.empty()) rc = crp::staged_h2d(ctx, s->d_merge, merges.data(), merges.size() * sizeof(crp::SelectMerge));
    if (rc != CRP_OK) return rc;
    crp::SelectTable tab[2];
    crp::SelectPredicate pred;
    fill_predicate(s, p, self != nullptr, joined, k, tab, &pred);
    const crp::SelectCoding coding = {s->d_cod[0], s->d_cod[1], s->d_cod[2], s->d_cod[3], s->d_cod[4], s->d_cod[5]};
    const crp::CodingLimits coding_lim = {s->coding_limits.min_pct, s->coding_limits.max_pct, s->coding_limits.min_transcripts_pct};
    const crp::FamilyLimits family_lim = {s->family_limits.max_hit_sum_outside, s->family_limits.max_mm0_outside, s->family_limits.min_members};
    const crp::EditPlanes edit_planes = {a->d_plane[0], a->d_plane[1], a->d_plane[3], a->padded_words};
    const crp::EditWindow edit_win = {s->edit_window.lo, s->edit_window.hi};
    const crp::EditLimits edit_lim = {s->edit_limits.min_pct, s->edit_limits.max_pct, s->edit_limits.max_targets};
    if (s->have_edit_limits) s->edit_stats[2] = (double)(edit_win.hi - edit_win.lo + 1u);
    // with splice limits the window is theirs, and edit limits set as well are the alternative under it (stop or splice)
    const crp::SpliceTest splice_test = {{s->splice_window.lo, s->splice_window.hi}, s->splice_editor,
                                         {s->splice_limits.min_pct, s->splice_limits.max_pct, s->splice_limits.max_targets, s->splice_limits.kinds},
                                         s->have_edit_limits ? 1u : 0u, edit_lim};
    if (s->have_splice_limits) s->splice_stats[2] = (double)(splice_test.window.hi - splice_test.window.lo + 1u);
    // the bounded-launch rule: at most 2^20 items a launch, each timed on its own
    for (uint64_t first = 0; first < items.size(); first += crp::SELECT_MAX_ITEMS) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(crp::SELECT_MAX_ITEMS, items.size() - first);
        CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
        if (s->have_splice_limits)
            CRP_HIP(ctx, crp::launch_select_items_splice(ctx->stream, tab[0], tab[1], pred, coding, edit_planes, splice_test, s->d_items + first, n, s->part,
                                                         s->res));
        else if (s->have_edit_limits)
            CRP_HIP(ctx, crp::launch_select_items_edit(ctx->stream, tab[0], tab[1], pred, coding, edit_planes, edit_win, edit_lim, s->d_items + first, n,
                                                       s->part, s->res));
        else if (s->have_coding_limits)
            CRP_HIP(ctx, crp::launch_select_items_coding(ctx->stream, tab[0], tab[1], pred, coding, coding_lim, s->d_items + first, n, s->part, s->res));
        else if (s->have_family_limits)
            CRP_HIP(ctx, crp::launch_select_items_family(ctx->stream, tab[0], tab[1], pred, family, family_lim, s->d_items + first, n, s->part, s->res));
        else
            CRP_HIP(ctx, crp::launch_select_items(ctx->stream, tab[0], tab[1], pred, s->d_items + first, n, s->part, s->res));
        CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
        CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const double ms = elapsed(s->ev[0], s->ev[1]);
        if (s->have_coding_limits) s->coding_stats[0] += ms;
        if (s->have_family_limits) s->family_stats[0] += ms;
        if (s->have_splice_limits) s->splice_stats[0] += ms;
        else if (s->have_edit_limits) s->edit_stats[0] += ms;
        s->stats[1] += ms;
        s->stats[4] += 1;
        s->stats[5] = std::max(s->stats[5], ms);
    }
    for (uint64_t first = 0; first < merges.size(); first += crp::SELECT_MAX_ITEMS) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(crp::SELECT_MAX_ITEMS, merges.size() - first);
        CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
        CRP_HIP(ctx, crp::launch_select_merge(ctx->stream, s->d_merge + first, n, k, s->part, s->res));
        CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
        CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        s->stats[2] += elapsed(s->ev[0], s->ev[1]);
    }
    s->stats[3] = (double)items.size();
    s->stats[6] = (double)rows_covered;
    // position + score, the label-set id under require_cds, with joined columns counts[0] and hit_sum, and the packed
    // properties under property limits, and the repair scores under repair limits
    s->stats[7] = 12.0 + (p->require_cds ? 4.0 : 0.0) + (self ? 12.0 : 0.0) + (s->have_prop_limits ? 4.0 : 0.0) + (s->have_repair_limits ? 8.0 : 0.0) +
                  (s->have_variant_limits ? 4.0 : 0.0) + (s->have_site_limits ? 8.0 : 0.0);
    s->stats[8] = (double)merges.size();
    s->k = k;
    return CRP_OK;
}

int crp_select_fetch(crp_select *s, uint32_t *n_in, uint32_t *n_pass, uint32_t *sel)
{
    if (!s) return CRP_ERR_INVALID;
    crp_ctx *ctx = s->ctx;
    if (!s->k) return fail(ctx, CRP_ERR_STATE, "crp_select_fetch: no crp_select_run has succeeded on this handle");
    if (!s->n_genes) return CRP_OK;
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = CRP_OK;
    if (n_in) rc = crp::staged_d2h(ctx, n_in, s->res.n_in, s->n_genes * sizeof(uint32_t));
    if (rc == CRP_OK && n_pass) rc = crp::staged_d2h(ctx, n_pass, s->res.n_pass, s->n_genes * sizeof(uint32_t));
    if (rc == CRP_OK && sel) rc = crp::staged_d2h(ctx, sel, s->res.sel, s->n_genes * s->k * sizeof(uint32_t));
    if (rc != CRP_OK) return rc;
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CRP_OK;
}

int crp_select_stats(const crp_select *s, double *out, int n)
{
    if (!s || (n && !out) || n < 0 || n > 9) return CRP_ERR_INVALID;
    for (int k = 0; k < n; ++k) out[k] = s->stats[k];
    return CRP_OK;
}

/* ---- guide pairs ---- */

int crp_select_set_pair_limits(crp_select *s, uint64_t pair_slice_rows)
{
    if (!s) return CRP_ERR_INVALID;
    if (pair_slice_rows && (pair_slice_rows < CRP_SELECT_MIN_PAIR_SLICE_ROWS || pair_slice_rows > 0x40000000ull)) return CRP_ERR_INVALID;
    s->pair_slice_rows = pair_slice_rows ? pair_slice_rows : CRP_SELECT_DEFAULT_PAIR_SLICE_ROWS;
    return CRP_OK;
}

int crp_select_run_pairs(crp_select *s, const crp_select_params *p, const crp_select_pair_params *q, crp_search_self *self)
{
    crp::Range roctx_range("crp: guide pairs");
    if (!s || !p || !q) return CRP_ERR_INVALID;
    crp_ctx *ctx = s->ctx;
    crp_arena *a = s->arena;
    s->kp = 0;
    const std::string who = "crp_select_run_pairs";
    crp::SelfJoined joined = {};
    int rc = check_pair_run(s, p, q, self, &joined, who.c_str());
    if (rc != CRP_OK) return rc;
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    const int k = q->k;
    const uint64_t G = s->n_genes;
    rc = crp::grow(ctx, reinterpret_cast<void **>(&s->pair_res.n_pass), &s->pair_res_cap[0], G, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->pair_res.n_pairs), &s->pair_res_cap[1], G, sizeof(uint64_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->pair_res.pairs), &s->pair_res_cap[2], G * k * 2, sizeof(uint32_t));
    if (rc != CRP_OK) return rc;
    for (double &v : s->pair_stats) v = 0;
    if (!G) {
        s->kp = k;
        return CRP_OK;
    }
    // (a table has fewer rows than the arena positions: below 2^31)
    const uint32_t n_plus = (uint32_t)a->n_hits[0], n_minus = (uint32_t)a->n_hits[1];
    crp::SelectTable tab[2];
    crp::SelectPredicate pred;
    fill_predicate(s, p, self != nullptr, joined, 0, tab, &pred);
    // the pass key of every row, once: the predicate apart from "in the gene" does not depend on the gene
    for (int t = 0; t < 2; ++t) {
        rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_pass_key[t]), &s->pass_key_cap[t], a->n_hits[t], sizeof(uint64_t));
        if (rc != CRP_OK) return rc;
    }
    CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
    for (int t = 0; t < 2; ++t) CRP_HIP(ctx, crp::launch_pair_pass_key(ctx->stream, tab[t], pred, s->d_pass_key[t]));
    CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
    CRP_HIP(ctx, crp::launch_select_bounds(ctx->stream, a->d_pos[0], n_plus, a->d_pos[1], n_minus, s->d_lo, s->d_hi, (uint32_t)G, s->d_bounds));
    std::vector<uint4> bounds;
    std::vector<crp::PairItem> items;
    std::vector<crp::SelectMerge> merges;
    std::vector<unsigned long long> host64;
    uint64_t n_slots = 0;
    try {
        bounds.resize(G);
        rc = crp::staged_d2h(ctx, bounds.data(), s->d_bounds, G * sizeof(uint4));
        if (rc != CRP_OK) return rc;
        CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        s->pair_stats[0] = elapsed(s->ev[0], s->ev[1]);
        // every gene's a-rows -- its '+' run, then its '-' run -- in pieces of at most pair_slice_rows rows; every piece
        // carries the gene's whole runs, where its partners are; a gene without rows still gets one (empty) item, which
        // writes its zeros
        items.reserve(G + G / 8);
        for (uint64_t g = 0; g < G; ++g) {
            const uint4 b = bounds[g];
            if (b.x > b.y || b.y > n_plus || b.z > b.w || b.w > n_minus)
                return fail(ctx, CRP_ERR_HIP, who + ": the bounds of gene " + std::to_string(g) + " lie outside the tables");
            const uint64_t np = b.y - b.x, nm = b.w - b.z, total = np + nm;
            const uint64_t pieces = std::max<uint64_t>(1, (total + s->pair_slice_rows - 1) / s->pair_slice_rows);
            if (n_slots + pieces > 0xfffffff0ull || items.size() + pieces > 0xfffffff0ull)
                return fail(ctx, CRP_ERR_UNSUPPORTED, who + ": more than 2^32 work items or slots (raise pair_slice_rows)");
            if (pieces > 1) merges.push_back(crp::SelectMerge{(uint32_t)g, (uint32_t)n_slots, (uint32_t)pieces});
            for (uint64_t c = 0; c < pieces; ++c) {
                // rows [r0, r1) of the gene's concatenated runs
                const uint64_t r0 = c * s->pair_slice_rows, r1 = std::min(total, r0 + s->pair_slice_rows);
                const uint64_t p0 = std::min(r0, np), p1 = std::min(r1, np);
                const uint64_t m0 = std::max(r0, np) - np, m1 = std::max(r1, np) - np;
                crp::PairItem it;
                it.gene = (uint32_t)g;
                it.slot = pieces > 1 ? (uint32_t)(n_slots + c) : crp::SELECT_NONE;
                it.first[0] = b.x + (uint32_t)p0;
                it.rows[0] = (uint32_t)(p1 - p0);
                it.first[1] = b.z + (uint32_t)m0;
                it.rows[1] = (uint32_t)(m1 - m0);
                it.run[0] = b.x;
                it.run[1] = b.y;
                it.run[2] = b.z;
                it.run[3] = b.w;
                items.push_back(it);
            }
            if (pieces > 1) n_slots += pieces;
        }
        host64.resize(std::max<uint64_t>(items.size(), G));
    } catch (const std::bad_alloc &) {
        return CRP_ERR_NOMEM;
    }
    crp::PairPartials &part = s->pair_part;
    rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_pair_items), &s->pair_items_cap, items.size(), sizeof(crp::PairItem));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_pair_merge), &s->pair_merge_cap, merges.size(), sizeof(crp::SelectMerge));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_pair_evals), &s->pair_evals_cap, items.size(), sizeof(uint64_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&part.kmin), &s->pair_part_cap[0], n_slots * k, sizeof(uint64_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&part.kmax), &s->pair_part_cap[1], n_slots * k, sizeof(uint64_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&part.tie), &s->pair_part_cap[2], n_slots * k, sizeof(uint64_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&part.a), &s->pair_part_cap[3], n_slots * k, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&part.b), &s->pair_part_cap[4], n_slots * k, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&part.n_pass), &s->pair_part_cap[5], n_slots, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&part.n_pairs), &s->pair_part_cap[6], n_slots, sizeof(uint64_t));
    if (rc == CRP_OK) rc = crp::staged_h2d(ctx, s->d_pair_items, items.data(), items.size() * sizeof(crp::PairItem));
    if (rc == CRP_OK && !merges.empty()) rc = crp::staged_h2d(ctx, s->d_pair_merge, merges.data(), merges.size() * sizeof(crp::SelectMerge));
    if (rc != CRP_OK) return rc;
    const crp::PairParams pp = {k, q->dmin, q->dmax, q->orientation_mask, q->frameshift ? 1u : 0u};
    // the bounded-launch rule: at most 2^20 items a launch, each timed on its own
    for (uint64_t first = 0; first < items.size(); first += crp::SELECT_MAX_ITEMS) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(crp::SELECT_MAX_ITEMS, items.size() - first);
        CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
        CRP_HIP(ctx, crp::launch_pair_items(ctx->stream, a->d_pos[0], a->d_pos[1], s->d_pass_key[0], s->d_pass_key[1], pp, s->d_pair_items + first,
                                            n, s->d_pair_evals + first, part, s->pair_res));
        CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
        CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const double ms = elapsed(s->ev[0], s->ev[1]);
        s->pair_stats[1] += ms;
        s->pair_stats[4] += 1;
        s->pair_stats[5] = std::max(s->pair_stats[5], ms);
    }
    for (uint64_t first = 0; first < merges.size(); first += crp::SELECT_MAX_ITEMS) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(crp::SELECT_MAX_ITEMS, merges.size() - first);
        CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
        CRP_HIP(ctx, crp::launch_pair_merge(ctx->stream, s->d_pair_merge + first, n, k, part, s->pair_res));
        CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
        CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        s->pair_stats[2] += elapsed(s->ev[0], s->ev[1]);
    }
    s->pair_stats[3] = (double)items.size();
    // the two totals: partner rows streamed (per item) and qualifying pairs (per gene), summed here
    rc = crp::staged_d2h(ctx, host64.data(), s->d_pair_evals, items.size() * sizeof(uint64_t));
    if (rc != CRP_OK) return rc;
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint64_t i = 0; i < items.size(); ++i) s->pair_stats[6] += (double)host64[i];
    rc = crp::staged_d2h(ctx, host64.data(), s->pair_res.n_pairs, G * sizeof(uint64_t));
    if (rc != CRP_OK) return rc;
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint64_t g = 0; g < G; ++g) s->pair_stats[7] += (double)host64[g];
    s->kp = k;
    return CRP_OK;
}

int crp_select_fetch_pairs(crp_select *s, uint32_t *n_pass, uint64_t *n_pairs, uint32_t *pairs)
{
    if (!s) return CRP_ERR_INVALID;
    crp_ctx *ctx = s->ctx;
    if (!s->kp) return fail(ctx, CRP_ERR_STATE, "crp_select_fetch_pairs: no crp_select_run_pairs has succeeded on this handle");
    if (!s->n_genes) return CRP_OK;
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = CRP_OK;
    if (n_pass) rc = crp::staged_d2h(ctx, n_pass, s->pair_res.n_pass, s->n_genes * sizeof(uint32_t));
    if (rc == CRP_OK && n_pairs) rc = crp::staged_d2h(ctx, n_pairs, s->pair_res.n_pairs, s->n_genes * sizeof(uint64_t));
    if (rc == CRP_OK && pairs) rc = crp::staged_d2h(ctx, pairs, s->pair_res.pairs, s->n_genes * s->kp * 2 * sizeof(uint32_t));
    if (rc != CRP_OK) return rc;
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CRP_OK;
}

int crp_select_pairs_stats(const crp_select *s, double *out, int n)
{
    if (!s || (n && !out) || n < 0 || n > 8) return CRP_ERR_INVALID;
    for (int k = 0; k < n; ++k) out[k] = s->pair_stats[k];
    return CRP_OK;
}

/* ---- distinct pairs ---- */

int crp_select_set_pair_distinct_limits(crp_select *s, uint64_t items_per_launch)
{
    if (!s || items_per_launch > crp::SELECT_MAX_ITEMS) return CRP_ERR_INVALID;
    s->pd_items_per_launch = items_per_launch ? items_per_launch : crp::SELECT_MAX_ITEMS;
    return CRP_OK;
}

int crp_select_run_pairs_distinct(crp_select *s, const crp_select_params *p, const crp_select_pair_params *q, crp_search_self *self)
{
    crp::Range roctx_range("crp: distinct guide pairs");
    if (!s || !p || !q) return CRP_ERR_INVALID;
    crp_ctx *ctx = s->ctx;
    crp_arena *a = s->arena;
    s->kpd = 0;
    const std::string who = "crp_select_run_pairs_distinct";
    crp::SelfJoined joined = {};
    int rc = check_pair_run(s, p, q, self, &joined, who.c_str());
    if (rc != CRP_OK) return rc;
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    const int k = q->k;
    const uint64_t G = s->n_genes;
    crp::PairDistinctResult &res = s->pd_res;
    crp::PairDistinctRounds &rounds = s->pd_rounds;
    rc = crp::grow(ctx, reinterpret_cast<void **>(&res.n_pass), &s->pd_cap[0], G, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&res.n_pairs), &s->pd_cap[1], G, sizeof(uint64_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&res.n_distinct), &s->pd_cap[2], G, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&res.pairs), &s->pd_cap[3], G * k * 2, sizeof(uint32_t));
    if (rc != CRP_OK) return rc;
    for (double &v : s->pd_stats) v = 0;
    if (!G) {
        s->kpd = k;
        return CRP_OK;
    }
    // (a table has fewer rows than the arena positions: below 2^31)
    const uint32_t n_plus = (uint32_t)a->n_hits[0], n_minus = (uint32_t)a->n_hits[1];
    crp::SelectTable tab[2];
    crp::SelectPredicate pred;
    fill_predicate(s, p, self != nullptr, joined, 0, tab, &pred);
    // the pass key of every row, once, in the pair path's buffers: this run writes them before it reads them
    for (int t = 0; t < 2; ++t) {
        rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_pass_key[t]), &s->pass_key_cap[t], a->n_hits[t], sizeof(uint64_t));
        if (rc != CRP_OK) return rc;
    }
    CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
    for (int t = 0; t < 2; ++t) CRP_HIP(ctx, crp::launch_pair_pass_key(ctx->stream, tab[t], pred, s->d_pass_key[t]));
    CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
    s->pd_stats[5] += 2;
    CRP_HIP(ctx, crp::launch_select_bounds(ctx->stream, a->d_pos[0], n_plus, a->d_pos[1], n_minus, s->d_lo, s->d_hi, (uint32_t)G, s->d_bounds));
    std::vector<uint4> bounds;
    std::vector<crp::PairItem> whole, pieces;
    std::vector<crp::SelectMerge> merges;
    std::vector<uint32_t> picked;
    std::vector<unsigned long long> host64;
    try {
        bounds.resize(G);
        rc = crp::staged_d2h(ctx, bounds.data(), s->d_bounds, G * sizeof(uint4));
        if (rc != CRP_OK) return rc;
        CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        s->pd_stats[0] = elapsed(s->ev[0], s->ev[1]);
        // crp_select_run_pairs' cut of every gene's a-rows into pieces of at most pair_slice_rows rows, each with the gene's
        // whole runs; the whole genes and the pieces of the cut genes in two lists, because only the pieces come back round
        // after round.  The runs are checked against the tables here, before anything reads through them
        whole.reserve(G);
        for (uint64_t g = 0; g < G; ++g) {
            const uint4 b = bounds[g];
            if (b.x > b.y || b.y > n_plus || b.z > b.w || b.w > n_minus)
                return fail(ctx, CRP_ERR_HIP, who + ": the bounds of gene " + std::to_string(g) + " lie outside the tables");
            const uint64_t np = b.y - b.x, nm = b.w - b.z, total = np + nm;
            const uint64_t n_pieces = std::max<uint64_t>(1, (total + s->pair_slice_rows - 1) / s->pair_slice_rows);
            if (pieces.size() + n_pieces > 0xfffffff0ull)
                return fail(ctx, CRP_ERR_UNSUPPORTED, who + ": more than 2^32 work items (raise pair_slice_rows)");
            if (n_pieces > 1) merges.push_back(crp::SelectMerge{(uint32_t)g, (uint32_t)pieces.size(), (uint32_t)n_pieces});
            for (uint64_t c = 0; c < n_pieces; ++c) {
                // rows [r0, r1) of the gene's concatenated runs
                const uint64_t r0 = c * s->pair_slice_rows, r1 = std::min(total, r0 + s->pair_slice_rows);
                const uint64_t p0 = std::min(r0, np), p1 = std::min(r1, np);
                const uint64_t m0 = std::max(r0, np) - np, m1 = std::max(r1, np) - np;
                crp::PairItem it;
                it.gene = (uint32_t)g;
                it.slot = n_pieces > 1 ? (uint32_t)pieces.size() : crp::SELECT_NONE;
                it.first[0] = b.x + (uint32_t)p0;
                it.rows[0] = (uint32_t)(p1 - p0);
                it.first[1] = b.z + (uint32_t)m0;
                it.rows[1] = (uint32_t)(m1 - m0);
                it.run[0] = b.x;
                it.run[1] = b.y;
                it.run[2] = b.z;
                it.run[3] = b.w;
                (n_pieces > 1 ? pieces : whole).push_back(it);
            }
        }
        picked.resize(merges.size());
        host64.resize(std::max<uint64_t>(whole.size() + pieces.size(), G));
    } catch (const std::bad_alloc &) {
        return CRP_ERR_NOMEM;
    }
    const uint64_t n_whole = whole.size(), n_pieces = pieces.size(), n_cut = merges.size(), per_launch = s->pd_items_per_launch;
    rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_pd_items), &s->pd_cap[4], n_whole + n_pieces, sizeof(crp::PairItem));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_pd_merge), &s->pd_cap[5], n_cut, sizeof(crp::SelectMerge));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_pd_evals), &s->pd_cap[6], n_whole + n_pieces, sizeof(uint64_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&rounds.prop), &s->pd_cap[7], n_pieces, sizeof(crp::PairProposal));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&rounds.slot_pass), &s->pd_cap[8], n_pieces, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&rounds.slot_pairs), &s->pd_cap[9], n_pieces, sizeof(uint64_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&rounds.picked), &s->pd_cap[10], n_cut, sizeof(uint32_t));
    if (rc == CRP_OK && n_whole) rc = crp::staged_h2d(ctx, s->d_pd_items, whole.data(), n_whole * sizeof(crp::PairItem));
    if (rc == CRP_OK && n_pieces) rc = crp::staged_h2d(ctx, s->d_pd_items + n_whole, pieces.data(), n_pieces * sizeof(crp::PairItem));
    if (rc == CRP_OK && n_cut) rc = crp::staged_h2d(ctx, s->d_pd_merge, merges.data(), n_cut * sizeof(crp::SelectMerge));
    if (rc != CRP_OK) return rc;
    const crp::PairParams pp = {k, q->dmin, q->dmax, q->orientation_mask, q->frameshift ? 1u : 0u};
    const auto timed = [&](double *sum) {
        const double ms = elapsed(s->ev[0], s->ev[1]);
        *sum += ms;
        s->pd_stats[5] += 1;
        s->pd_stats[6] = std::max(s->pd_stats[6], ms);
    };
    // the whole genes: every round inside one launch; the bounded-launch rule: at most 2^20 items a launch, each timed on its own
    for (uint64_t first = 0; first < n_whole; first += per_launch) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(per_launch, n_whole - first);
        CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
        CRP_HIP(ctx, crp::launch_pair_distinct_items(ctx->stream, a->d_pos[0], a->d_pos[1], s->d_pass_key[0], s->d_pass_key[1], pp, 0u,
                                                     s->d_pd_items + first, n, s->d_pd_evals + first, rounds, res));
        CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
        CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        timed(&s->pd_stats[1]);
    }
    // the cut genes: a step launch and a pick launch a round, until a round picks nothing
    for (uint32_t round = 0; n_cut && round < (uint32_t)k; ++round) {
        for (uint64_t first = 0; first < n_pieces; first += per_launch) {
            const uint32_t n = (uint32_t)std::min<uint64_t>(per_launch, n_pieces - first);
            CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
            CRP_HIP(ctx, crp::launch_pair_distinct_items(ctx->stream, a->d_pos[0], a->d_pos[1], s->d_pass_key[0], s->d_pass_key[1], pp, round,
                                                         s->d_pd_items + n_whole + first, n, s->d_pd_evals + n_whole + first, rounds, res));
            CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
            CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
            timed(&s->pd_stats[2]);
        }
        for (uint64_t first = 0; first < n_cut; first += per_launch) {
            const uint32_t n = (uint32_t)std::min<uint64_t>(per_launch, n_cut - first);
            CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
            CRP_HIP(ctx, crp::launch_pair_distinct_pick(ctx->stream, s->d_pd_merge + first, n, (uint32_t)first, k, round, rounds, res));
            CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
            CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
            timed(&s->pd_stats[3]);
        }
        s->pd_stats[4] += 1;
        rc = crp::staged_d2h(ctx, picked.data(), rounds.picked, n_cut * sizeof(uint32_t));
        if (rc != CRP_OK) return rc;
        CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (std::none_of(picked.begin(), picked.end(), [](uint32_t v) { return v != 0u; })) break;
    }
    s->pd_stats[7] = (double)(n_whole + n_pieces);
    s->pd_stats[8] = (double)n_cut;
    // the totals: partner rows streamed (per item, over all rounds), pairs taken and qualifying pairs (per gene), summed here
    rc = crp::staged_d2h(ctx, host64.data(), s->d_pd_evals, (n_whole + n_pieces) * sizeof(uint64_t));
    if (rc != CRP_OK) return rc;
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint64_t i = 0; i < n_whole + n_pieces; ++i) s->pd_stats[9] += (double)host64[i];
    rc = crp::staged_d2h(ctx, host64.data(), res.n_distinct, G * sizeof(uint32_t));
    if (rc != CRP_OK) return rc;
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint64_t g = 0; g < G; ++g) s->pd_stats[10] += (double)reinterpret_cast<const uint32_t *>(host64.data())[g];
    rc = crp::staged_d2h(ctx, host64.data(), res.n_pairs, G * sizeof(uint64_t));
    if (rc != CRP_OK) return rc;
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint64_t g = 0; g < G; ++g) s->pd_stats[11] += (double)host64[g];
    s->kpd = k;
    return CRP_OK;
}

int crp_select_fetch_pairs_distinct(crp_select *s, uint32_t *n_pass, uint64_t *n_pairs, uint32_t *n_distinct, uint32_t *pairs)
{
    if (!s) return CRP_ERR_INVALID;
    crp_ctx *ctx = s->ctx;
    if (!s->kpd)
        return fail(ctx, CRP_ERR_STATE, "crp_select_fetch_pairs_distinct: no crp_select_run_pairs_distinct has succeeded on this handle");
    if (!s->n_genes) return CRP_OK;
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = CRP_OK;
    if (n_pass) rc = crp::staged_d2h(ctx, n_pass, s->pd_res.n_pass, s->n_genes * sizeof(uint32_t));
    if (rc == CRP_OK && n_pairs) rc = crp::staged_d2h(ctx, n_pairs, s->pd_res.n_pairs, s->n_genes * sizeof(uint64_t));
    if (rc == CRP_OK && n_distinct) rc = crp::staged_d2h(ctx, n_distinct, s->pd_res.n_distinct, s->n_genes * sizeof(uint32_t));
    if (rc == CRP_OK && pairs) rc = crp::staged_d2h(ctx, pairs, s->pd_res.pairs, s->n_genes * s->kpd * 2 * sizeof(uint32_t));
    if (rc != CRP_OK) return rc;
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CRP_OK;
}

int crp_select_pairs_distinct_stats(const crp_select *s, double *out, int n)
{
    if (!s || (n && !out) || n < 0 || n > 12) return CRP_ERR_INVALID;
    for (int k = 0; k < n; ++k) out[k] = s->pd_stats[k];
    return CRP_OK;
}

/* ---- spaced selection ---- */

int crp_select_run_spaced(crp_select *s, const crp_select_params *p, uint32_t min_distance, crp_search_self *self)
{
    crp::Range roctx_range("crp: spaced selection");
    if (!s || !p) return CRP_ERR_INVALID;
    crp_ctx *ctx = s->ctx;
    crp_arena *a = s->arena;
    s->ks = 0;
    const std::string who = "crp_select_run_spaced";
    if (p->k < 1 || p->k > CRP_SELECT_MAX_K)
        return fail(ctx, CRP_ERR_INVALID, who + ": k must be 1.." + std::to_string(CRP_SELECT_MAX_K) + ", not " + std::to_string(p->k));
    if (min_distance > CRP_SELECT_MAX_SPACING)
        return fail(ctx, CRP_ERR_INVALID, who + ": the minimum distance must be 0.." + std::to_string(CRP_SELECT_MAX_SPACING) + " (cut sites lie below 2^31), not " +
                                              std::to_string(min_distance));
    if (s->have_family_limits)
        return fail(ctx, CRP_ERR_INVALID, who + ": family limits are relative to the gene and the spaced selection's eligibility key is per table row: "
                                                "clear them (crp_select_set_family_limits(select, NULL)) for a spaced selection");
    if (s->have_coding_limits)
        return fail(ctx, CRP_ERR_INVALID, who + ": coding limits are relative to the gene and the spaced selection's eligibility key is per table row: "
                                                "clear them (crp_select_set_coding_limits(select, NULL)) for a spaced selection");
    if (s->have_edit_limits)
        return fail(ctx, CRP_ERR_INVALID, who + ": edit limits are relative to the gene and the spaced selection's eligibility key is per table row: "
                                                "clear them (crp_select_set_edit_limits(select, NULL, NULL)) for a spaced selection");
    if (s->have_splice_limits)
        return fail(ctx, CRP_ERR_INVALID, who + ": splice limits are relative to the gene and the spaced selection's eligibility key is per table row: "
                                                "clear them (crp_select_set_splice_limits(select, NULL, 0, NULL)) for a spaced selection");
    crp::SelfJoined joined = {};
    int rc = check_run(s, p, self, &joined, who.c_str());
    if (rc != CRP_OK) return rc;
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    const int k = p->k;
    const uint64_t G = s->n_genes;
    crp::SpacedResult &res = s->spaced_res;
    crp::SpacedRounds &rounds = s->spaced_rounds;
    rc = crp::grow(ctx, reinterpret_cast<void **>(&res.n_pass), &s->spaced_cap[0], G, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&res.n_spaced), &s->spaced_cap[1], G, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&res.sel), &s->spaced_cap[2], G * k, sizeof(uint32_t));
    if (rc != CRP_OK) return rc;
    for (double &v : s->spaced_stats) v = 0;
    if (!G) {
        s->ks = k;
        return CRP_OK;
    }
    // (a table has fewer rows than the arena positions: below 2^31)
    const uint32_t n_plus = (uint32_t)a->n_hits[0], n_minus = (uint32_t)a->n_hits[1];
    crp::SelectTable tab[2];
    crp::SelectPredicate pred;
    fill_predicate(s, p, self != nullptr, joined, 0, tab, &pred);
    // the pass key of every row, once, in the pair path's buffers: the rounds then read position and key, 12 bytes a row
    for (int t = 0; t < 2; ++t) {
        rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_pass_key[t]), &s->pass_key_cap[t], a->n_hits[t], sizeof(uint64_t));
        if (rc != CRP_OK) return rc;
    }
    CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
    for (int t = 0; t < 2; ++t) CRP_HIP(ctx, crp::launch_pair_pass_key(ctx->stream, tab[t], pred, s->d_pass_key[t]));
    CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
    s->spaced_stats[5] += 2;
    CRP_HIP(ctx, crp::launch_select_bounds(ctx->stream, a->d_pos[0], n_plus, a->d_pos[1], n_minus, s->d_lo, s->d_hi, (uint32_t)G, s->d_bounds));
    std::vector<uint4> bounds;
    std::vector<crp::SelectItem> whole, pieces;
    std::vector<crp::SelectMerge> merges;
    std::vector<uint32_t> picked;
    try {
        bounds.resize(G);
        rc = crp::staged_d2h(ctx, bounds.data(), s->d_bounds, G * sizeof(uint4));
        if (rc != CRP_OK) return rc;
        CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        s->spaced_stats[0] = elapsed(s->ev[0], s->ev[1]);
        // crp_select_run's cut of the genes' rows into items of at most slice_rows rows; the whole genes and the pieces of
        // the cut genes in two lists, because only the pieces come back round after round
        whole.reserve(G);
        for (uint64_t g = 0; g < G; ++g) {
            const uint4 b = bounds[g];
            if (b.x > b.y || b.y > n_plus || b.z > b.w || b.w > n_minus)
                return fail(ctx, CRP_ERR_HIP, who + ": the bounds of gene " + std::to_string(g) + " lie outside the tables");
            const uint64_t np = b.y - b.x, nm = b.w - b.z, total = np + nm;
            const uint64_t n_pieces = std::max<uint64_t>(1, (total + s->slice_rows - 1) / s->slice_rows);
            if (pieces.size() + n_pieces > 0xfffffff0ull) return fail(ctx, CRP_ERR_UNSUPPORTED, who + ": more than 2^32 work items (raise slice_rows)");
            if (n_pieces > 1) merges.push_back(crp::SelectMerge{(uint32_t)g, (uint32_t)pieces.size(), (uint32_t)n_pieces});
            for (uint64_t c = 0; c < n_pieces; ++c) {
                // rows [r0, r1) of the gene's concatenated runs
                const uint64_t r0 = c * s->slice_rows, r1 = std::min(total, r0 + s->slice_rows);
                const uint64_t p0 = std::min(r0, np), p1 = std::min(r1, np);
                const uint64_t m0 = std::max(r0, np) - np, m1 = std::max(r1, np) - np;
                crp::SelectItem it;
                it.gene = (uint32_t)g;
                it.slot = n_pieces > 1 ? (uint32_t)pieces.size() : crp::SELECT_NONE;
                it.first[0] = b.x + (uint32_t)p0;
                it.rows[0] = (uint32_t)(p1 - p0);
                it.first[1] = b.z + (uint32_t)m0;
                it.rows[1] = (uint32_t)(m1 - m0);
                (n_pieces > 1 ? pieces : whole).push_back(it);
            }
        }
        picked.resize(merges.size());
    } catch (const std::bad_alloc &) {
        return CRP_ERR_NOMEM;
    }
    const uint64_t n_whole = whole.size(), n_pieces = pieces.size(), n_cut = merges.size();
    rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_spaced_items), &s->spaced_cap[3], n_whole + n_pieces, sizeof(crp::SelectItem));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_spaced_merge), &s->spaced_cap[4], n_cut, sizeof(crp::SelectMerge));
    if (rc == CRP_OK && n_cut) rc = crp::grow(ctx, reinterpret_cast<void **>(&rounds.cuts), &s->spaced_cap[5], G * k, sizeof(uint32_t));
    if (rc == CRP_OK && n_cut) rc = crp::grow(ctx, reinterpret_cast<void **>(&rounds.last), &s->spaced_cap[6], G, sizeof(crp::SpacedProposal));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&rounds.prop), &s->spaced_cap[7], n_pieces, sizeof(crp::SpacedProposal));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&rounds.slot_pass), &s->spaced_cap[8], n_pieces, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&rounds.picked), &s->spaced_cap[9], n_cut, sizeof(uint32_t));
    if (rc == CRP_OK && n_whole) rc = crp::staged_h2d(ctx, s->d_spaced_items, whole.data(), n_whole * sizeof(crp::SelectItem));
    if (rc == CRP_OK && n_pieces) rc = crp::staged_h2d(ctx, s->d_spaced_items + n_whole, pieces.data(), n_pieces * sizeof(crp::SelectItem));
    if (rc == CRP_OK && n_cut) rc = crp::staged_h2d(ctx, s->d_spaced_merge, merges.data(), n_cut * sizeof(crp::SelectMerge));
    if (rc != CRP_OK) return rc;
    const auto timed = [&](double *sum) {
        const double ms = elapsed(s->ev[0], s->ev[1]);
        *sum += ms;
        s->spaced_stats[5] += 1;
        s->spaced_stats[6] = std::max(s->spaced_stats[6], ms);
    };
    // the whole genes: every round inside one launch; the bounded-launch rule: at most 2^20 items a launch, each timed on its own
    for (uint64_t first = 0; first < n_whole; first += crp::SELECT_MAX_ITEMS) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(crp::SELECT_MAX_ITEMS, n_whole - first);
        CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
        CRP_HIP(ctx, crp::launch_spaced_items(ctx->stream, a->d_pos[0], a->d_pos[1], s->d_pass_key[0], s->d_pass_key[1], k, min_distance, 0u,
                                              s->d_spaced_items + first, n, rounds, res));
        CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
        CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        timed(&s->spaced_stats[1]);
    }
    // the cut genes: a step launch and a pick launch a round, until a round picks nothing
    for (uint32_t round = 0; n_cut && round < (uint32_t)k; ++round) {
        for (uint64_t first = 0; first < n_pieces; first += crp::SELECT_MAX_ITEMS) {
            const uint32_t n = (uint32_t)std::min<uint64_t>(crp::SELECT_MAX_ITEMS, n_pieces - first);
            CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
            CRP_HIP(ctx, crp::launch_spaced_items(ctx->stream, a->d_pos[0], a->d_pos[1], s->d_pass_key[0], s->d_pass_key[1], k, min_distance, round,
                                                  s->d_spaced_items + n_whole + first, n, rounds, res));
            CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
            CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
            timed(&s->spaced_stats[2]);
        }
        for (uint64_t first = 0; first < n_cut; first += crp::SELECT_MAX_ITEMS) {
            const uint32_t n = (uint32_t)std::min<uint64_t>(crp::SELECT_MAX_ITEMS, n_cut - first);
            CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
            CRP_HIP(ctx, crp::launch_spaced_pick(ctx->stream, s->d_spaced_merge + first, n, (uint32_t)first, k, round, rounds, res));
            CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
            CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
            timed(&s->spaced_stats[3]);
        }
        s->spaced_stats[4] += 1;
        rc = crp::staged_d2h(ctx, picked.data(), rounds.picked, n_cut * sizeof(uint32_t));
        if (rc != CRP_OK) return rc;
        CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (std::none_of(picked.begin(), picked.end(), [](uint32_t v) { return v != 0u; })) break;
    }
    s->spaced_stats[7] = (double)(n_whole + n_pieces);
    s->spaced_stats[8] = (double)n_cut;
    s->ks = k;
    return CRP_OK;
}

int crp_select_fetch_spaced(crp_select *s, uint32_t *n_pass, uint32_t *n_spaced, uint32_t *sel)
{
    if (!s) return CRP_ERR_INVALID;
    crp_ctx *ctx = s->ctx;
    if (!s->ks) return fail(ctx, CRP_ERR_STATE, "crp_select_fetch_spaced: no crp_select_run_spaced has succeeded on this handle");
    if (!s->n_genes) return CRP_OK;
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = CRP_OK;
    if (n_pass) rc = crp::staged_d2h(ctx, n_pass, s->spaced_res.n_pass, s->n_genes * sizeof(uint32_t));
    if (rc == CRP_OK && n_spaced) rc = crp::staged_d2h(ctx, n_spaced, s->spaced_res.n_spaced, s->n_genes * sizeof(uint32_t));
    if (rc == CRP_OK && sel) rc = crp::staged_d2h(ctx, sel, s->spaced_res.sel, s->n_genes * s->ks * sizeof(uint32_t));
    if (rc != CRP_OK) return rc;
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CRP_OK;
}

int crp_select_spaced_stats(const crp_select *s, double *out, int n)
{
    if (!s || (n && !out) || n < 0 || n > 9) return CRP_ERR_INVALID;
    for (int k = 0; k < n; ++k) out[k] = s->spaced_stats[k];
    return CRP_OK;
}

/* ---- self selection ---- */

int crp_select_set_self_limits(crp_select *s, uint64_t items_per_launch)
{
    if (!s || items_per_launch > crp::SELECT_MAX_ITEMS) return CRP_ERR_INVALID;
    s->self_items_per_launch = items_per_launch ? items_per_launch : crp::SELECT_MAX_ITEMS;
    return CRP_OK;
}

int crp_select_set_self_model(crp_select *s, int rank_by_model, int has_min, double min_sum)
{
    if (!s) return CRP_ERR_INVALID;
    if (has_min && std::isnan(min_sum)) return fail(s->ctx, CRP_ERR_INVALID, "crp_select_set_self_model: min_sum is not a number");
    s->self_rank_model = rank_by_model != 0;
    s->self_has_min = has_min != 0;
    s->self_min_sum = has_min ? min_sum : 0.0;
    return CRP_OK;
}

int crp_select_run_self(crp_select *s, const crp_select_self_params *p, crp_search_self *self)
{
    crp::Range roctx_range("crp: self selection");
    if (!s || !p || !self) return CRP_ERR_INVALID;
    crp_ctx *ctx = s->ctx;
    crp_arena *a = s->arena;
    s->kself = 0;
    const std::string who = "crp_select_run_self";
    if (p->k < 1 || p->k > CRP_SELECT_MAX_K)
        return fail(ctx, CRP_ERR_INVALID, who + ": k must be 1.." + std::to_string(CRP_SELECT_MAX_K) + ", not " + std::to_string(p->k));
    crp::SelfSelectHandle h = {};
    bool compared = false;
    crp::self_select_handle(self, &h, &compared);
    if (h.arena != a) return fail(ctx, CRP_ERR_INVALID, who + ": the self-search handle belongs to another arena");
    if (!compared)
        return fail(ctx, CRP_ERR_STATE, who + ": the self-search handle has not been through the compare of every segment 0.." +
                                            std::to_string(h.max_mm) + " (crp_search_self_order, crp_search_self_compare)");
    const bool by_model = s->self_rank_model || s->self_has_min;
    if (by_model && !h.rows.model)
        return fail(ctx, CRP_ERR_STATE, who + ": ranking or bounding by the on-target model needs the handle's model run first "
                                              "(crp_search_self_set_model, crp_search_self_run_model)");
    if (p->cut_offset < 1 || p->cut_offset > h.T - 1)
        return fail(ctx, CRP_ERR_INVALID, who + ": the cut offset must be 1.." + std::to_string(h.T - 1) + " (pattern positions), not " +
                                              std::to_string(p->cut_offset));
    if (p->require_cds && !s->have_flags) return fail(ctx, CRP_ERR_STATE, who + ": require_cds needs crp_select_set_flags");
    if (p->require_cds && !a->have_track) return fail(ctx, CRP_ERR_STATE, who + ": require_cds needs a track on the arena (crp_annotate_set_track)");
    if (p->gc_min > p->gc_max)
        return fail(ctx, CRP_ERR_INVALID, who + ": gc_min " + std::to_string(p->gc_min) + " is above gc_max " + std::to_string(p->gc_max));
    if (h.n > 0xfffffffeull) return fail(ctx, CRP_ERR_UNSUPPORTED, who + ": more than 2^32 - 2 candidates: a candidate index is 32 bits");
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    const int k = p->k;
    const uint64_t G = s->n_genes, stride = (uint64_t)h.max_mm + 1;
    int rc = crp::grow(ctx, reinterpret_cast<void **>(&s->self_res.n_in), &s->self_cap[0], G, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->self_res.n_pass), &s->self_cap[1], G, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->self_res.sel), &s->self_cap[2], G * k, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->self_got.pos), &s->self_cap[3], G * k, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->self_got.hi), &s->self_cap[4], G * k, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->self_got.lo), &s->self_cap[5], G * k, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->self_got.counts), &s->self_cap[6], G * k * stride, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->self_got.strand), &s->self_cap[7], G * k, sizeof(uint8_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->self_got.sum), &s->self_cap[8], G * k, sizeof(uint64_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_self_run), &s->self_cap[9], G, sizeof(uint2));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->self_got.model), &s->self_cap[10], G * k, sizeof(double));
    if (rc != CRP_OK) return rc;
    for (double &v : s->self_stats) v = 0;
    s->self_stride = (int)stride;
    if (!G) {
        s->kself = k;
        return CRP_OK;
    }
    const uint32_t n_cand = h.rows.n;
    CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
    CRP_HIP(ctx, crp::launch_select_self_bounds(ctx->stream, h.rows.pos, n_cand, (uint32_t)h.T, s->d_lo, s->d_hi, (uint32_t)G, s->d_self_run));
    CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
    std::vector<uint2> runs;
    std::vector<crp::SelectItem> items;
    std::vector<crp::SelectMerge> merges;
    uint64_t n_slots = 0, rows_covered = 0;
    try {
        runs.resize(G);
        rc = crp::staged_d2h(ctx, runs.data(), s->d_self_run, G * sizeof(uint2));
        if (rc != CRP_OK) return rc;
        CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        s->self_stats[0] = elapsed(s->ev[0], s->ev[1]);
        // every gene's run in pieces of at most slice_rows candidates; a gene without rows still gets one (empty) item,
        // which writes its zeros
        items.reserve(G + G / 8);
        for (uint64_t g = 0; g < G; ++g) {
            const uint2 b = runs[g];
            if (b.x > b.y || b.y > n_cand) return fail(ctx, CRP_ERR_HIP, who + ": the run of gene " + std::to_string(g) + " lies outside the candidates");
            const uint64_t total = b.y - b.x;
            rows_covered += total;
            const uint64_t pieces = std::max<uint64_t>(1, (total + s->slice_rows - 1) / s->slice_rows);
            if (n_slots + pieces > 0xfffffff0ull || items.size() + pieces > 0xfffffff0ull)
                return fail(ctx, CRP_ERR_UNSUPPORTED, who + ": more than 2^32 work items or slots (raise slice_rows)");
            if (pieces > 1) merges.push_back(crp::SelectMerge{(uint32_t)g, (uint32_t)n_slots, (uint32_t)pieces});
            for (uint64_t c = 0; c < pieces; ++c) {
                const uint64_t r0 = c * s->slice_rows, r1 = std::min(total, r0 + s->slice_rows);
                crp::SelectItem it;
                it.gene = (uint32_t)g;
                it.slot = pieces > 1 ? (uint32_t)(n_slots + c) : crp::SELECT_NONE;
                it.first[0] = b.x + (uint32_t)r0;
                it.rows[0] = (uint32_t)(r1 - r0);
                it.first[1] = 0;
                it.rows[1] = 0;
                items.push_back(it);
            }
            if (pieces > 1) n_slots += pieces;
        }
    } catch (const std::bad_alloc &) {
        return CRP_ERR_NOMEM;
    }
    rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_items), &s->items_cap, items.size(), sizeof(crp::SelectItem));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_merge), &s->merge_cap, merges.size(), sizeof(crp::SelectMerge));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->part.key), &s->part_entries_cap, n_slots * k, sizeof(uint64_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->part.tie), &s->part_tie_cap, n_slots * k, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->part.row), &s->part_row_cap, n_slots * k, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->part.cnt), &s->part_cnt_cap, n_slots * 2, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::staged_h2d(ctx, s->d_items, items.data(), items.size() * sizeof(crp::SelectItem));
    if (rc == CRP_OK && !merges.empty()) rc = crp::staged_h2d(ctx, s->d_merge, merges.data(), merges.size() * sizeof(crp::SelectMerge));
    if (rc != CRP_OK) return rc;
    const uint32_t G_letters = (uint32_t)(h.T - h.pam_len);
    crp::SelfSelectPredicate pred = {};
    pred.max_hit_sum = p->max_hit_sum;
    pred.max_mm0 = p->max_mm0;
    pred.T = (uint32_t)h.T;
    pred.cut = (uint32_t)p->cut_offset;
    pred.region = h.region;
    pred.gc_min = p->gc_min;
    pred.gc_max = p->gc_max;
    pred.max_t_run = p->max_t_run;
    pred.seq_limits = (p->gc_min > 0 || p->gc_max < G_letters || p->max_t_run < G_letters) ? 1u : 0u;
    pred.k = k;
    pred.min_sum = s->self_min_sum;
    pred.rank_model = s->self_rank_model ? 1u : 0u;
    pred.has_min = s->self_has_min ? 1u : 0u;
    crp::SelfSelectTrack track = {};
    if (p->require_cds) {
        track.points = a->d_ann_points;
        track.ids = a->d_ann_ids;
        track.bucket = a->d_ann_bucket;
        track.last_bucket = (uint32_t)(a->n_ann_entries - 2);
        track.flags = s->d_flags;
        track.n_flags = (uint32_t)s->n_flags;
    }
    // the bounded-launch rule: at most self_items_per_launch (2^20) items a launch, each timed on its own
    for (uint64_t first = 0; first < items.size(); first += s->self_items_per_launch) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(s->self_items_per_launch, items.size() - first);
        CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
        CRP_HIP(ctx, crp::launch_select_self_items(ctx->stream, h.rows, track, pred, s->d_lo, s->d_hi, s->d_items + first, n, s->part, s->self_res,
                                                   by_model));
        CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
        CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        s->self_stats[1] += elapsed(s->ev[0], s->ev[1]);
        s->self_stats[4] += 1;
    }
    for (uint64_t first = 0; first < merges.size(); first += crp::SELECT_MAX_ITEMS) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(crp::SELECT_MAX_ITEMS, merges.size() - first);
        CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
        CRP_HIP(ctx, crp::launch_select_merge(ctx->stream, s->d_merge + first, n, k, s->part, s->self_res));
        CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
        CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        s->self_stats[2] += elapsed(s->ev[0], s->ev[1]);
    }
    CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
    CRP_HIP(ctx, crp::launch_select_self_gather(ctx->stream, h.rows, s->self_res.sel, G * k, s->self_got));
    CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->self_stats[3] = elapsed(s->ev[0], s->ev[1]);
    s->self_stats[5] = (double)items.size();
    s->self_stats[6] = (double)rows_covered;
    s->kself = k;
    return CRP_OK;
}

int crp_select_fetch_self(crp_select *s, uint32_t *n_in, uint32_t *n_pass, uint32_t *sel, uint32_t *arena_pos, uint8_t *strand, uint32_t *hi,
                          uint32_t *lo, uint32_t *counts, uint64_t *hit_sum)
{
    if (!s) return CRP_ERR_INVALID;
    crp_ctx *ctx = s->ctx;
    if (!s->kself) return fail(ctx, CRP_ERR_STATE, "crp_select_fetch_self: no crp_select_run_self has succeeded on this handle");
    if (!s->n_genes) return CRP_OK;
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t G = s->n_genes, E = G * s->kself;
    int rc = CRP_OK;
    if (n_in) rc = crp::staged_d2h(ctx, n_in, s->self_res.n_in, G * sizeof(uint32_t));
    if (rc == CRP_OK && n_pass) rc = crp::staged_d2h(ctx, n_pass, s->self_res.n_pass, G * sizeof(uint32_t));
    if (rc == CRP_OK && sel) rc = crp::staged_d2h(ctx, sel, s->self_res.sel, E * sizeof(uint32_t));
    if (rc == CRP_OK && arena_pos) rc = crp::staged_d2h(ctx, arena_pos, s->self_got.pos, E * sizeof(uint32_t));
    if (rc == CRP_OK && strand) rc = crp::staged_d2h(ctx, strand, s->self_got.strand, E * sizeof(uint8_t));
    if (rc == CRP_OK && hi) rc = crp::staged_d2h(ctx, hi, s->self_got.hi, E * sizeof(uint32_t));
    if (rc == CRP_OK && lo) rc = crp::staged_d2h(ctx, lo, s->self_got.lo, E * sizeof(uint32_t));
    if (rc == CRP_OK && counts) rc = crp::staged_d2h(ctx, counts, s->self_got.counts, E * s->self_stride * sizeof(uint32_t));
    if (rc == CRP_OK && hit_sum) rc = crp::staged_d2h(ctx, hit_sum, s->self_got.sum, E * sizeof(uint64_t));
    if (rc != CRP_OK) return rc;
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CRP_OK;
}

int crp_select_fetch_self_model(crp_select *s, double *model_sum)
{
    if (!s) return CRP_ERR_INVALID;
    crp_ctx *ctx = s->ctx;
    if (!s->kself) return fail(ctx, CRP_ERR_STATE, "crp_select_fetch_self_model: no crp_select_run_self has succeeded on this handle");
    if (!s->n_genes || !model_sum) return CRP_OK;
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    const int rc = crp::staged_d2h(ctx, model_sum, s->self_got.model, s->n_genes * s->kself * sizeof(double));
    if (rc != CRP_OK) return rc;
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CRP_OK;
}

int crp_select_self_stats(const crp_select *s, double *out, int n)
{
    if (!s || (n && !out) || n < 0 || n > 7) return CRP_ERR_INVALID;
    for (int k = 0; k < n; ++k) out[k] = s->self_stats[k];
    return CRP_OK;
}

/* ---- coding position ---- */

int crp_select_set_coding(crp_select *s, const uint32_t *info, const uint32_t *length, const uint64_t *first, uint64_t n_rows, const uint32_t *at,
                          const uint32_t *word, const uint32_t *cum, uint64_t n_steps)
{
    if (!s) return CRP_ERR_INVALID;
    crp_ctx *ctx = s->ctx;
    const std::string who = "crp_select_set_coding";
    if (!n_rows && !info && !length && !first && !n_steps) {
        s->have_coding = false;
        return CRP_OK;
    }
    if (n_rows != s->n_genes)
        return fail(ctx, CRP_ERR_INVALID, who + ": the model has " + std::to_string(n_rows) + " rows and the handle " + std::to_string(s->n_genes) + " genes");
    if (!first || (n_rows && (!info || !length)) || (n_steps && (!at || !word || !cum)) || n_steps > 0xfffffff0ull) return CRP_ERR_INVALID;
    s->have_coding = false;
    std::vector<uint32_t> first32;
    try {
        first32.resize(n_rows + 1);
    } catch (const std::bad_alloc &) {
        return CRP_ERR_NOMEM;
    }
    // what the kernels rely on: every row's steps lie inside the arrays, and its change points ascend
    for (uint64_t g = 0; g <= n_rows; ++g) {
        if (first[g] > n_steps || (g && first[g] < first[g - 1]) || (g == n_rows && first[g] != n_steps) || (!g && first[g] != 0))
            return fail(ctx, CRP_ERR_INVALID, who + ": first does not ascend from 0 to n_steps at row " + std::to_string(g));
        first32[g] = (uint32_t)first[g];
    }
    for (uint64_t g = 0; g < n_rows; ++g)
        for (uint64_t k = first[g] + 1; k < first[g + 1]; ++k)
            if (at[k] <= at[k - 1]) return fail(ctx, CRP_ERR_INVALID, who + ": the change points of row " + std::to_string(g) + " do not ascend");
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    const void *src[6] = {info, length, first32.data(), at, word, cum};
    const uint64_t count[6] = {n_rows, n_rows, n_rows + 1, n_steps, n_steps, n_steps};
    int rc = CRP_OK;
    for (int j = 0; j < 6 && rc == CRP_OK; ++j) {
        rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_cod[j]), &s->cod_cap[j], count[j], sizeof(uint32_t));
        if (rc == CRP_OK && count[j]) rc = crp::staged_h2d(ctx, s->d_cod[j], src[j], count[j] * sizeof(uint32_t));
    }
    if (rc != CRP_OK) return rc;
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->coding_steps = n_steps;
    s->coding_stats[2] = (double)n_steps;
    s->have_coding = true;
    return CRP_OK;
}

int crp_select_set_coding_limits(crp_select *s, const crp_select_coding_limits *limits)
{
    if (!s) return CRP_ERR_INVALID;
    if (limits && (limits->min_pct > limits->max_pct || limits->max_pct > 100u || limits->min_transcripts_pct > 100u))
        return fail(s->ctx, CRP_ERR_INVALID,
                    "crp_select_set_coding_limits: percentages 0..100 with min_pct <= max_pct, not " + std::to_string(limits->min_pct) + ", " +
                        std::to_string(limits->max_pct) + " and " + std::to_string(limits->min_transcripts_pct));
    s->have_coding_limits = limits != nullptr;
    s->coding_limits = limits ? *limits : crp_select_coding_limits{};
    return CRP_OK;
}

int crp_select_coding_eval(crp_select *s, const uint32_t *gene_row, const uint32_t *packed_row, uint64_t n, uint32_t *off, uint32_t *cover)
{
    if (!s || (n && (!gene_row || !packed_row || !off || !cover)) || n > 0x7fffffffull) return CRP_ERR_INVALID;
    crp_ctx *ctx = s->ctx;
    crp_arena *a = s->arena;
    const std::string who = "crp_select_coding_eval";
    if (!s->have_coding) return fail(ctx, CRP_ERR_STATE, who + ": the handle has no model (crp_select_set_coding)");
    if (!a->have_hits) return fail(ctx, CRP_ERR_STATE, who + ": the arena has no hit tables");
    for (uint64_t q = 0; q < n; ++q) {
        if (gene_row[q] >= s->n_genes)
            return fail(ctx, CRP_ERR_INVALID, who + ": query " + std::to_string(q) + " names gene " + std::to_string(gene_row[q]) + " of " + std::to_string(s->n_genes));
        if ((packed_row[q] & 0x7FFFFFFFu) >= a->n_hits[packed_row[q] >> 31])
            return fail(ctx, CRP_ERR_INVALID, who + ": query " + std::to_string(q) + " names a row outside its table");
    }
    s->coding_stats[1] = 0;
    if (!n) return CRP_OK;
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = CRP_OK;
    for (int j = 0; j < 4 && rc == CRP_OK; ++j) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_eval[j]), &s->eval_cap[j], n, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::staged_h2d(ctx, s->d_eval[0], gene_row, n * sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::staged_h2d(ctx, s->d_eval[1], packed_row, n * sizeof(uint32_t));
    if (rc != CRP_OK) return rc;
    const crp::SelectCoding coding = {s->d_cod[0], s->d_cod[1], s->d_cod[2], s->d_cod[3], s->d_cod[4], s->d_cod[5]};
    CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
    CRP_HIP(ctx, crp::launch_coding_eval(ctx->stream, a->d_pos[0], a->d_pos[1], coding, s->d_eval[0], s->d_eval[1], (uint32_t)n, s->d_eval[2],
                                         s->d_eval[3]));
    CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
    rc = crp::staged_d2h(ctx, off, s->d_eval[2], n * sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::staged_d2h(ctx, cover, s->d_eval[3], n * sizeof(uint32_t));
    if (rc != CRP_OK) return rc;
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->coding_stats[1] = elapsed(s->ev[0], s->ev[1]);
    return CRP_OK;
}

int crp_select_coding_stats(const crp_select *s, double *out, int n)
{
    if (!s || (n && !out) || n < 0 || n > 3) return CRP_ERR_INVALID;
    for (int k = 0; k < n; ++k) out[k] = s->coding_stats[k];
    return CRP_OK;
}

/* ---- gene families ---- */

int crp_select_set_family(crp_select *s, const uint32_t *gene_family, const uint32_t *family_size, uint64_t n_genes)
{
    if (!s) return CRP_ERR_INVALID;
    crp_ctx *ctx = s->ctx;
    s->have_family = false;
    s->have_members = false;  // (the member bits belong to the families: section 24)
    s->set_plan_valid = false;
    if (!gene_family && !family_size && !n_genes) return CRP_OK;
    if (!gene_family || !family_size) return CRP_ERR_INVALID;
    if (n_genes != s->n_genes)
        return fail(ctx, CRP_ERR_INVALID, "crp_select_set_family: " + std::to_string(n_genes) + " genes for a handle of " + std::to_string(s->n_genes));
    for (uint64_t g = 0; g < n_genes; ++g)
        if (!family_size[g])
            return fail(ctx, CRP_ERR_INVALID, "crp_select_set_family: gene " + std::to_string(g) + " has a family of size 0 (a gene in no family has 1)");
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_gene_family), &s->gene_family_cap, n_genes, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_family_size), &s->family_size_cap, n_genes, sizeof(uint32_t));
    if (rc == CRP_OK && n_genes) rc = crp::staged_h2d(ctx, s->d_gene_family, gene_family, n_genes * sizeof(uint32_t));
    if (rc == CRP_OK && n_genes) rc = crp::staged_h2d(ctx, s->d_family_size, family_size, n_genes * sizeof(uint32_t));
    if (rc != CRP_OK) return rc;
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->have_family = true;
    return CRP_OK;
}

int crp_select_set_family_limits(crp_select *s, const crp_select_family_limits *limits)
{
    if (!s) return CRP_ERR_INVALID;
    if (limits && limits->min_members != CRP_SELECT_ALL_MEMBERS && limits->min_members > 64u)
        return fail(s->ctx, CRP_ERR_INVALID, "crp_select_set_family_limits: a family has at most 64 members, not " + std::to_string(limits->min_members));
    s->have_family_limits = limits != nullptr;
    s->family_limits = limits ? *limits : crp_select_family_limits{};
    return CRP_OK;
}

int crp_select_family_eval(crp_select *s, crp_search_self *self, const uint32_t *gene_row, const uint32_t *packed_row, uint64_t n,
                           uint32_t *outside_mm0, uint64_t *outside_hit_sum, uint32_t *members_hit, uint32_t *family_size, uint64_t *fam_cover)
{
    if (!s || (n && (!gene_row || !packed_row || !outside_mm0 || !outside_hit_sum || !members_hit || !family_size || !fam_cover)) ||
        n > 0x7fffffffull)
        return CRP_ERR_INVALID;
    crp_ctx *ctx = s->ctx;
    crp_arena *a = s->arena;
    const std::string who = "crp_select_family_eval";
    if (!a->have_hits) return fail(ctx, CRP_ERR_STATE, who + ": the arena has no hit tables");
    crp::SelectFamily family = {};
    int rc = family_columns(s, self, who.c_str(), &family);
    if (rc != CRP_OK) return rc;
    for (uint64_t q = 0; q < n; ++q) {
        if (gene_row[q] >= s->n_genes)
            return fail(ctx, CRP_ERR_INVALID, who + ": query " + std::to_string(q) + " names gene " + std::to_string(gene_row[q]) + " of " + std::to_string(s->n_genes));
        if ((packed_row[q] & 0x7FFFFFFFu) >= a->n_hits[packed_row[q] >> 31])
            return fail(ctx, CRP_ERR_INVALID, who + ": query " + std::to_string(q) + " names a row outside its table");
    }
    s->family_stats[1] = 0;
    if (!n) return CRP_OK;
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    for (int j = 0; j < 4 && rc == CRP_OK; ++j) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_eval[j]), &s->eval_cap[j], 2 * n, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_family_eval_sum), &s->family_eval_sum_cap, 2 * n, sizeof(uint64_t));
    if (rc == CRP_OK) rc = crp::staged_h2d(ctx, s->d_eval[0], gene_row, n * sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::staged_h2d(ctx, s->d_eval[1], packed_row, n * sizeof(uint32_t));
    if (rc != CRP_OK) return rc;
    // (the eval buffers hold 2 n words each here: d_eval[2] carries outside_mm0 and, behind it, family_size)
    uint32_t *d_mm0 = s->d_eval[2], *d_hit = s->d_eval[3], *d_size = s->d_eval[2] + n;
    CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
    CRP_HIP(ctx, crp::launch_family_eval(ctx->stream, family, s->d_eval[0], s->d_eval[1], (uint32_t)n, d_mm0, s->d_family_eval_sum, d_hit, d_size,
                                         s->d_family_eval_sum + n));
    CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
    rc = crp::staged_d2h(ctx, outside_mm0, d_mm0, n * sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::staged_d2h(ctx, outside_hit_sum, s->d_family_eval_sum, n * sizeof(uint64_t));
    if (rc == CRP_OK) rc = crp::staged_d2h(ctx, members_hit, d_hit, n * sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::staged_d2h(ctx, family_size, d_size, n * sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::staged_d2h(ctx, fam_cover, s->d_family_eval_sum + n, n * sizeof(uint64_t));
    if (rc != CRP_OK) return rc;
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->family_stats[1] = elapsed(s->ev[0], s->ev[1]);
    return CRP_OK;
}

int crp_select_family_stats(const crp_select *s, double *out, int n)
{
    if (!s || (n && !out) || n < 0 || n > 2) return CRP_ERR_INVALID;
    for (int k = 0; k < n; ++k) out[k] = s->family_stats[k];
    return CRP_OK;
}

/* ---- family sets ---- */

int crp_select_set_family_members(crp_select *s, const uint32_t *gene_member, uint64_t n_genes)
{
    if (!s) return CRP_ERR_INVALID;
    crp_ctx *ctx = s->ctx;
    const std::string who = "crp_select_set_family_members";
    s->have_members = false;
    s->set_plan_valid = false;
    if (!gene_member && !n_genes) return CRP_OK;
    if (!gene_member) return CRP_ERR_INVALID;
    if (!s->have_family) return fail(ctx, CRP_ERR_STATE, who + ": the handle has no families (crp_select_set_family)");
    if (n_genes != s->n_genes)
        return fail(ctx, CRP_ERR_INVALID, who + ": " + std::to_string(n_genes) + " genes for a handle of " + std::to_string(s->n_genes));
    for (uint64_t g = 0; g < n_genes; ++g)
        if (gene_member[g] >= 64u)
            return fail(ctx, CRP_ERR_INVALID, who + ": gene " + std::to_string(g) + " is member " + std::to_string(gene_member[g]) +
                                                  " of its family (a family has at most 64)");
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_gene_member), &s->gene_member_cap, n_genes, sizeof(uint32_t));
    if (rc == CRP_OK && n_genes) rc = crp::staged_h2d(ctx, s->d_gene_member, gene_member, n_genes * sizeof(uint32_t));
    if (rc != CRP_OK) return rc;
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->have_members = true;
    return CRP_OK;
}

namespace {

// The plan of crp_select_family_step: the bounds kernel's runs of the genes that have a family, cut at slice_rows as the
// selection's items are, and per family the list of its items (CSR).  Built once per handle, tables and parameter set.
int build_set_plan(crp_select *s, const crp_select_params *p, uint64_t n_families, const std::string &who)
{
    crp_ctx *ctx = s->ctx;
    crp_arena *a = s->arena;
    const uint64_t G = s->n_genes;
    const uint32_t n_plus = (uint32_t)a->n_hits[0], n_minus = (uint32_t)a->n_hits[1];
    std::vector<uint4> bounds;
    std::vector<uint32_t> family, start, slots;
    std::vector<crp::SelectItem> items;
    uint64_t rows_covered = 0;
    try {
        bounds.resize(G);
        family.resize(G);
        start.assign(n_families + 1, 0u);
        if (G) {
            CRP_HIP(ctx, crp::launch_select_bounds(ctx->stream, a->d_pos[0], n_plus, a->d_pos[1], n_minus, s->d_lo, s->d_hi, (uint32_t)G, s->d_bounds));
            int rc = crp::staged_d2h(ctx, bounds.data(), s->d_bounds, G * sizeof(uint4));
            if (rc == CRP_OK) rc = crp::staged_d2h(ctx, family.data(), s->d_gene_family, G * sizeof(uint32_t));
            if (rc != CRP_OK) return rc;
            CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        for (uint64_t g = 0; g < G; ++g) {
            if (family[g] == crp::SELECT_NONE) continue;
            if (family[g] >= n_families)
                return fail(ctx, CRP_ERR_INVALID, who + ": gene " + std::to_string(g) + " has family " + std::to_string(family[g]) + " of " +
                                                      std::to_string(n_families));
            const uint4 b = bounds[g];
            if (b.x > b.y || b.y > n_plus || b.z > b.w || b.w > n_minus)
                return fail(ctx, CRP_ERR_HIP, who + ": the bounds of gene " + std::to_string(g) + " lie outside the tables");
            const uint64_t np = b.y - b.x, nm = b.w - b.z, total = np + nm;
            if (!total) continue;  // (no row, no candidate)
            rows_covered += total;
            const uint64_t pieces = (total + s->slice_rows - 1) / s->slice_rows;
            if (items.size() + pieces > 0xfffffff0ull) return fail(ctx, CRP_ERR_UNSUPPORTED, who + ": more than 2^32 work items (raise slice_rows)");
            for (uint64_t c = 0; c < pieces; ++c) {
                // rows [r0, r1) of the gene's concatenated runs
                const uint64_t r0 = c * s->slice_rows, r1 = std::min(total, r0 + s->slice_rows);
                const uint64_t p0 = std::min(r0, np), p1 = std::min(r1, np);
                const uint64_t m0 = std::max(r0, np) - np, m1 = std::max(r1, np) - np;
                crp::SelectItem it;
                it.gene = (uint32_t)g;
                it.slot = (uint32_t)items.size();
                it.first[0] = b.x + (uint32_t)p0;
                it.rows[0] = (uint32_t)(p1 - p0);
                it.first[1] = b.z + (uint32_t)m0;
                it.rows[1] = (uint32_t)(m1 - m0);
                items.push_back(it);
                ++start[family[g] + 1];
            }
        }
        for (uint64_t f = 0; f < n_families; ++f) start[f + 1] += start[f];
        slots.resize(items.size());
        std::vector<uint32_t> at(start.begin(), start.end() - 1);
        for (uint64_t i = 0; i < items.size(); ++i) slots[at[family[items[i].gene]]++] = (uint32_t)i;
    } catch (const std::bad_alloc &) {
        return CRP_ERR_NOMEM;
    }
    int rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_set_items), &s->set_cap[0], items.size(), sizeof(crp::SelectItem));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_set_prop), &s->set_cap[1], items.size(), sizeof(crp::FamilyProposal));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_set_best), &s->set_cap[2], n_families, sizeof(crp::FamilyProposal));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_set_start), &s->set_cap[3], n_families + 1, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_set_slots), &s->set_cap[4], items.size(), sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_set_covered), &s->set_cap[5], n_families, sizeof(uint64_t));
    if (rc == CRP_OK && !items.empty()) rc = crp::staged_h2d(ctx, s->d_set_items, items.data(), items.size() * sizeof(crp::SelectItem));
    if (rc == CRP_OK && !items.empty()) rc = crp::staged_h2d(ctx, s->d_set_slots, slots.data(), slots.size() * sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::staged_h2d(ctx, s->d_set_start, start.data(), start.size() * sizeof(uint32_t));
    if (rc != CRP_OK) return rc;
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->set_items = items.size();
    s->set_rows = rows_covered;
    s->set_families = n_families;
    s->set_plan_slice = s->slice_rows;
    s->set_plan_hits[0] = a->n_hits[0];
    s->set_plan_hits[1] = a->n_hits[1];
    s->set_plan_params = *p;
    s->set_plan_valid = true;
    s->set_stats[5] += 1;
    return CRP_OK;
}

bool same_params(const crp_select_params &a, const crp_select_params &b)
{
    return a.min_score == b.min_score && a.max_hit_sum == b.max_hit_sum && a.max_mm0 == b.max_mm0 && a.k == b.k && a.require_cds == b.require_cds;
}

}  // namespace

int crp_select_family_step(crp_select *s, const crp_select_params *p, crp_search_self *self, const uint64_t *covered, uint64_t n_families,
                           crp_family_step_best *best)
{
    crp::Range roctx_range("crp: family set step");
    if (!s || !p || (n_families && (!covered || !best)) || n_families > 0x7fffffffull) return CRP_ERR_INVALID;
    crp_ctx *ctx = s->ctx;
    crp_arena *a = s->arena;
    const std::string who = "crp_select_family_step";
    if (s->have_coding_limits || s->have_edit_limits || s->have_splice_limits)
        return fail(ctx, CRP_ERR_UNSUPPORTED, who + ": the family step and coding, edit or splice limits are different kernels' predicates: "
                                                    "clear them (one kernel per predicate)");
    crp::SelfJoined joined = {};
    int rc = check_run(s, p, self, &joined, who.c_str());
    if (rc != CRP_OK) return rc;
    crp::SelectFamily family = {};
    rc = family_columns(s, self, who.c_str(), &family);
    if (rc != CRP_OK) return rc;
    if (!s->have_members) return fail(ctx, CRP_ERR_STATE, who + ": the handle has no member bits (crp_select_set_family_members)");
    s->set_stats[0] = s->set_stats[1] = 0;
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    if (!s->set_plan_valid || s->set_families != n_families || s->set_plan_slice != s->slice_rows || s->set_plan_hits[0] != a->n_hits[0] ||
        s->set_plan_hits[1] != a->n_hits[1] || !same_params(s->set_plan_params, *p)) {
        s->set_plan_valid = false;
        rc = build_set_plan(s, p, n_families, who);
        if (rc != CRP_OK) return rc;
    }
    s->set_stats[2] = (double)s->set_items;
    s->set_stats[3] = (double)s->set_rows;
    // the selection's columns (crp_select_stats) and, per row, site_family, fam_cover, fam_counts[0] and fam_sum
    s->set_stats[4] = 24.0 + (p->require_cds ? 4.0 : 0.0) + (s->have_prop_limits ? 4.0 : 0.0) + (s->have_repair_limits ? 8.0 : 0.0) +
                      (s->have_variant_limits ? 4.0 : 0.0) + (s->have_site_limits ? 8.0 : 0.0) + 24.0;
    if (!n_families) return CRP_OK;
    rc = crp::staged_h2d(ctx, s->d_set_covered, covered, n_families * sizeof(uint64_t));
    if (rc != CRP_OK) return rc;
    crp::SelectTable tab[2];
    crp::SelectPredicate pred;
    fill_predicate(s, p, true, joined, 1, tab, &pred);
    // without family limits: bounds that every row meets
    const crp::FamilyLimits lim = s->have_family_limits
                                      ? crp::FamilyLimits{s->family_limits.max_hit_sum_outside, s->family_limits.max_mm0_outside, s->family_limits.min_members}
                                      : crp::FamilyLimits{~0ull, 0xFFFFFFFFu, 0u};
    // the bounded-launch rule: at most 2^20 items a launch
    CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
    for (uint64_t first = 0; first < s->set_items; first += crp::SELECT_MAX_ITEMS) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(crp::SELECT_MAX_ITEMS, s->set_items - first);
        CRP_HIP(ctx, crp::launch_family_set_step(ctx->stream, tab[0], tab[1], pred, family, lim, s->d_gene_member, s->d_set_covered, s->d_set_items + first,
                                                 n, s->d_set_prop + first));
    }
    CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->set_stats[0] = elapsed(s->ev[0], s->ev[1]);
    CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
    CRP_HIP(ctx, crp::launch_family_set_pick(ctx->stream, s->d_set_prop, s->d_set_start, s->d_set_slots, (uint32_t)n_families, s->d_set_best));
    CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
    static_assert(sizeof(crp_family_step_best) == sizeof(crp::FamilyProposal), "one record");
    rc = crp::staged_d2h(ctx, best, s->d_set_best, n_families * sizeof(crp::FamilyProposal));
    if (rc != CRP_OK) return rc;
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->set_stats[1] = elapsed(s->ev[0], s->ev[1]);
    return CRP_OK;
}

int crp_select_family_step_stats(const crp_select *s, double *out, int n)
{
    if (!s || (n && !out) || n < 0 || n > 6) return CRP_ERR_INVALID;
    for (int k = 0; k < n; ++k) out[k] = s->set_stats[k];
    return CRP_OK;
}

/* ---- base editing ---- */

int crp_select_set_edit_limits(crp_select *s, const crp_select_edit_window *window, const crp_select_edit_limits *limits)
{
    if (!s) return CRP_ERR_INVALID;
    if (!limits) {
        s->have_edit_limits = false;
        s->edit_limits = crp_select_edit_limits{};
        return CRP_OK;
    }
    crp::EditWindow w;
    const int rc = check_window(s->ctx, window, "crp_select_set_edit_limits", &w);
    if (rc != CRP_OK) return rc;
    if (limits->min_pct > limits->max_pct || limits->max_pct > 100u)
        return fail(s->ctx, CRP_ERR_INVALID, "crp_select_set_edit_limits: percentages 0..100 with min_pct <= max_pct, not " +
                                                 std::to_string(limits->min_pct) + " and " + std::to_string(limits->max_pct));
    s->edit_window = crp_select_edit_window{w.lo, w.hi};
    s->edit_limits = *limits;
    s->have_edit_limits = true;
    return CRP_OK;
}

int crp_select_edit_eval(crp_select *s, const crp_select_edit_window *window, const uint32_t *gene_row, const uint32_t *packed_row, uint64_t n,
                         uint32_t *counts, uint32_t *stop_off)
{
    if (!s || (n && (!gene_row || !packed_row || !counts || !stop_off)) || n > 0x7fffffffull) return CRP_ERR_INVALID;
    crp_ctx *ctx = s->ctx;
    crp_arena *a = s->arena;
    const std::string who = "crp_select_edit_eval";
    crp::EditWindow w;
    int rc = check_window(ctx, window, who, &w);
    if (rc != CRP_OK) return rc;
    if (!s->have_coding) return fail(ctx, CRP_ERR_STATE, who + ": the handle has no model (crp_select_set_coding)");
    if (!a->have_hits || a->pend_guide_len != (int)crp::EDIT_GUIDE_LEN)
        return fail(ctx, CRP_ERR_STATE, who + ": the arena has no hit tables of guide length 20 (the window counts protospacer positions of 20)");
    for (uint64_t q = 0; q < n; ++q) {
        if (gene_row[q] >= s->n_genes)
            return fail(ctx, CRP_ERR_INVALID, who + ": query " + std::to_string(q) + " names gene " + std::to_string(gene_row[q]) + " of " + std::to_string(s->n_genes));
        if ((packed_row[q] & 0x7FFFFFFFu) >= a->n_hits[packed_row[q] >> 31])
            return fail(ctx, CRP_ERR_INVALID, who + ": query " + std::to_string(q) + " names a row outside its table");
    }
    s->edit_stats[1] = 0;
    if (!n) return CRP_OK;
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    for (int j = 0; j < 4 && rc == CRP_OK; ++j) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_eval[j]), &s->eval_cap[j], n, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::staged_h2d(ctx, s->d_eval[0], gene_row, n * sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::staged_h2d(ctx, s->d_eval[1], packed_row, n * sizeof(uint32_t));
    if (rc != CRP_OK) return rc;
    const crp::SelectCoding coding = {s->d_cod[0], s->d_cod[1], s->d_cod[2], s->d_cod[3], s->d_cod[4], s->d_cod[5]};
    const crp::EditPlanes planes = {a->d_plane[0], a->d_plane[1], a->d_plane[3], a->padded_words};
    CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
    CRP_HIP(ctx, crp::launch_edit_eval(ctx->stream, a->d_pos[0], a->d_pos[1], coding, planes, w, s->d_eval[0], s->d_eval[1], (uint32_t)n, s->d_eval[2],
                                       s->d_eval[3]));
    CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
    rc = crp::staged_d2h(ctx, counts, s->d_eval[2], n * sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::staged_d2h(ctx, stop_off, s->d_eval[3], n * sizeof(uint32_t));
    if (rc != CRP_OK) return rc;
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->edit_stats[1] = elapsed(s->ev[0], s->ev[1]);
    s->edit_stats[2] = (double)(w.hi - w.lo + 1u);
    return CRP_OK;
}

int crp_select_edit_stats(const crp_select *s, double *out, int n)
{
    if (!s || (n && !out) || n < 0 || n > 3) return CRP_ERR_INVALID;
    for (int k = 0; k < n; ++k) out[k] = s->edit_stats[k];
    return CRP_OK;
}

/* ---- splice-site editing ---- */

int crp_select_set_splice_limits(crp_select *s, const crp_select_edit_window *window, uint32_t editor, const crp_select_splice_limits *limits)
{
    if (!s) return CRP_ERR_INVALID;
    if (!limits) {
        s->have_splice_limits = false;
        s->splice_limits = crp_select_splice_limits{};
        return CRP_OK;
    }
    const std::string who = "crp_select_set_splice_limits";
    crp::EditWindow w;
    const int rc = check_window(s->ctx, window, who, &w);
    if (rc != CRP_OK) return rc;
    if (editor != CRP_EDITOR_CBE && editor != CRP_EDITOR_ABE)
        return fail(s->ctx, CRP_ERR_INVALID, who + ": the editor is CRP_EDITOR_CBE or CRP_EDITOR_ABE, not " + std::to_string(editor));
    if (limits->min_pct > limits->max_pct || limits->max_pct > 100u)
        return fail(s->ctx, CRP_ERR_INVALID, who + ": percentages 0..100 with min_pct <= max_pct, not " + std::to_string(limits->min_pct) + " and " +
                                                 std::to_string(limits->max_pct));
    if (limits->kinds < 1u || limits->kinds > (CRP_SPLICE_DONOR | CRP_SPLICE_ACCEPTOR))
        return fail(s->ctx, CRP_ERR_INVALID, who + ": kinds is CRP_SPLICE_DONOR, CRP_SPLICE_ACCEPTOR or both, not " + std::to_string(limits->kinds));
    s->splice_window = crp_select_edit_window{w.lo, w.hi};
    s->splice_editor = editor;
    s->splice_limits = *limits;
    s->have_splice_limits = true;
    return CRP_OK;
}

int crp_select_splice_eval(crp_select *s, const crp_select_edit_window *window, uint32_t editor, const uint32_t *gene_row, const uint32_t *packed_row,
                           uint64_t n, uint32_t *counts, uint32_t *off)
{
    if (!s || (n && (!gene_row || !packed_row || !counts || !off)) || n > 0x3fffffffull) return CRP_ERR_INVALID;
    crp_ctx *ctx = s->ctx;
    crp_arena *a = s->arena;
    const std::string who = "crp_select_splice_eval";
    crp::EditWindow w;
    int rc = check_window(ctx, window, who, &w);
    if (rc != CRP_OK) return rc;
    if (editor != CRP_EDITOR_CBE && editor != CRP_EDITOR_ABE)
        return fail(ctx, CRP_ERR_INVALID, who + ": the editor is CRP_EDITOR_CBE or CRP_EDITOR_ABE, not " + std::to_string(editor));
    if (!s->have_coding) return fail(ctx, CRP_ERR_STATE, who + ": the handle has no model (crp_select_set_coding)");
    if (!a->have_hits || a->pend_guide_len != (int)crp::EDIT_GUIDE_LEN)
        return fail(ctx, CRP_ERR_STATE, who + ": the arena has no hit tables of guide length 20 (the window counts protospacer positions of 20)");
    for (uint64_t q = 0; q < n; ++q) {
        if (gene_row[q] >= s->n_genes)
            return fail(ctx, CRP_ERR_INVALID, who + ": query " + std::to_string(q) + " names gene " + std::to_string(gene_row[q]) + " of " + std::to_string(s->n_genes));
        if ((packed_row[q] & 0x7FFFFFFFu) >= a->n_hits[packed_row[q] >> 31])
            return fail(ctx, CRP_ERR_INVALID, who + ": query " + std::to_string(q) + " names a row outside its table");
    }
    s->splice_stats[1] = 0;
    if (!n) return CRP_OK;
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    // (the offs are two words a query: d_eval[3] holds 2 n)
    for (int j = 0; j < 4 && rc == CRP_OK; ++j)
        rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_eval[j]), &s->eval_cap[j], j == 3 ? 2 * n : n, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::staged_h2d(ctx, s->d_eval[0], gene_row, n * sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::staged_h2d(ctx, s->d_eval[1], packed_row, n * sizeof(uint32_t));
    if (rc != CRP_OK) return rc;
    const crp::SelectCoding coding = {s->d_cod[0], s->d_cod[1], s->d_cod[2], s->d_cod[3], s->d_cod[4], s->d_cod[5]};
    const crp::EditPlanes planes = {a->d_plane[0], a->d_plane[1], a->d_plane[3], a->padded_words};
    CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
    CRP_HIP(ctx, crp::launch_splice_eval(ctx->stream, a->d_pos[0], a->d_pos[1], coding, planes, w, editor, s->d_eval[0], s->d_eval[1], (uint32_t)n,
                                         s->d_eval[2], s->d_eval[3]));
    CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
    rc = crp::staged_d2h(ctx, counts, s->d_eval[2], n * sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::staged_d2h(ctx, off, s->d_eval[3], 2 * n * sizeof(uint32_t));
    if (rc != CRP_OK) return rc;
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->splice_stats[1] = elapsed(s->ev[0], s->ev[1]);
    s->splice_stats[2] = (double)(w.hi - w.lo + 1u);
    return CRP_OK;
}

int crp_select_splice_stats(const crp_select *s, double *out, int n)
{
    if (!s || (n && !out) || n < 0 || n > 3) return CRP_ERR_INVALID;
    for (int k = 0; k < n; ++k) out[k] = s->splice_stats[k];
    return CRP_OK;
}

}  // extern "C"
