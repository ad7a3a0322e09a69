// crp_search_self.cpp -- host side of the self search (include/cropsr_hip.h crp_search_self_*; kernels in
// crp_search_self.hip, extraction kernels of crp_search.hip; DESIGN section 15, Self search).
//
// create   validates the two patterns, extracts every candidate of the arena into HBM (count + emit, one chunk: the
//          self search is not chunked, a budget too small is CRP_ERR_CAPACITY with the size it takes), flags the guide
//          sites and zeroes one result row per candidate.
// order    segment j: key + histogram kernel, bucket starts by a prefix sum on the host (which also keeps the bucket
//          sizes: they are the work plan), scatter kernel.  One ordering is held at a time.
// compare  guide sites of one handle against the candidates of another (or the same) in their current orderings, which
//          must be of the same segment: per bucket, tiles of SELF_TILE queries x slices of candidates, cut into
//          launches of at most pairs_per_launch pairs.  Hits add into the query handle's rows.
// join     the rows of the guide sites onto the hit tables of the arena's last scan (CSV join): one
//          launch per strand, the joined columns stay on the handle.
// families (kernels in crp_search_family.hip) the family genes of the arena on the handle: assign gives
//          every candidate its owner, compare fills a second row per guide site from the candidates of its own family
//          (work planned from the genes' runs: tiles of SELF_TILE queries x slices of a member's run), join hands those
//          rows to the hit tables like the plain ones.
// model    (kernel in crp_ontarget.hip) a position-specific linear on-target model on the handle: set_model
//          uploads its tables, run_model leaves one f64 sum per candidate (NaN where a candidate is no guide site or its
//          window holds a non-base), fetch_model returns the guide sites' sums in fetch's order.  It needs no compare.
// A genome of several arenas is every ordered pair of handles, segment by segment (cropsr_amd/search.py: search_self).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "crp_internal.h"
#include "crp_ontarget.h"
#include "crp_search_family.h"
#include "crp_search_self.h"
#include "crp_select_self.h"

namespace {

constexpr uint64_t kPairsPerLaunch = 1ull << 36;  // the bound the given-guides compare keeps
constexpr uint64_t kItemsPerLaunch = 1ull << 20;  // work items one upload holds
constexpr uint32_t kSliceMin = 2048;              // candidates per slice of a bucket, at least
constexpr uint32_t kSlicesMax = 64;               // slices per bucket, at most: a huge bucket is tiles x 64 workgroups
constexpr uint64_t kMaxCands = (1ull << 32) - 2 * crp::SELF_PAD;
constexpr uint64_t kFamilyItemsPerLaunch = kItemsPerLaunch / 2;  // a family item is two uint4 of the same upload
constexpr uint32_t kFamilySliceFloor = crp::SELF_UNROLL;          // the smallest slice crp_search_self_family_set_limits takes

uint32_t iupac_set(char c)  // bit = code: A=0 T=1 C=2 G=3
{
    switch (c | 0x20) {
        case 'a': return 1;
        case 't': return 2;
        case 'c': return 4;
        case 'g': return 8;
        case 'r': return 1 | 8;
        case 'y': return 4 | 2;
        case 's': return 4 | 8;
        case 'w': return 1 | 2;
        case 'k': return 8 | 2;
        case 'm': return 1 | 4;
        case 'b': return 4 | 8 | 2;
        case 'd': return 1 | 8 | 2;
        case 'h': return 1 | 4 | 2;
        case 'v': return 1 | 4 | 8;
        case 'n': return 15;
        default: return 0;
    }
}

uint32_t complement_set(uint32_t s) { return ((s & 1) << 1) | ((s & 2) >> 1) | ((s & 4) << 1) | ((s & 8) >> 1); }

double elapsed(hipEvent_t a, hipEvent_t b)
{
    float ms = 0.f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.0;
}

}  // namespace

struct crp_search_self {
    crp_arena *arena = nullptr;
    crp_ctx *ctx = nullptr;
    crp::SearchSets sets = {};
    crp::SelfGuideRule rule = {};
    int T = 0, pam_len = 0, max_mm = 0;
    bool pam3 = true;
    int seg_shift[crp::SELF_MAX_MM + 1] = {}, seg_len[crp::SELF_MAX_MM + 1] = {};
    uint64_t n_plus = 0, n_minus = 0, n = 0, n_guides = 0, bytes = 0;
    uint64_t pairs_per_launch = kPairsPerLaunch;
    // device
    uint32_t *d_cand = nullptr;   // 4 x n (SoA): hi, lo, nb, pos
    uint8_t *d_flag = nullptr;    // n: a guide site
    uint32_t *d_key = nullptr;    // n: the current segment's key
    uint32_t *d_order = nullptr;  // 4 x (n + SELF_PAD): hi, lo, nb, idx of the current ordering
    uint32_t *d_hist = nullptr;   // 2 x max keys: histogram, cursors
    uint32_t *d_counts = nullptr;            // n x (max_mm + 1)
    unsigned long long *d_hit_sum = nullptr;  // n
    crp::SearchValueState value;  // crp_search_self_set_scheme / crp_search_self_set_pair_scheme
    uint4 *d_items = nullptr;
    // the current ordering
    int segment = -1;
    std::vector<uint32_t> hist, start;  // per key: entries, first slot
    uint32_t compared = 0;  // bit j: a crp_search_self_compare with this handle's guide sites as queries has run on segment j
    hipEvent_t ev[2] = {nullptr, nullptr};
    double ms_extract = 0, ms_order = 0, ms_compare = 0, ms_longest = 0;
    uint64_t n_compare = 0, n_order = 0, pairs = 0;
    // the joined columns of the last crp_search_self_join_hits, in hit-table order: [0] = '+', [1] = '-'
    uint32_t *d_join_counts[2] = {nullptr, nullptr};
    unsigned long long *d_join_sum[2] = {nullptr, nullptr};
    uint64_t join_counts_cap[2] = {0, 0}, join_sum_cap[2] = {0, 0};
    bool have_join = false;
    uint64_t join_rows[2] = {0, 0};  // the tables' rows at the time of the join
    double ms_join = 0;
    // gene families: crp_search_self_set_families .. crp_search_self_family_join_hits
    uint64_t budget = 0;
    std::vector<crp::FamilyRow> fam_rows;       // the arena's family genes, GFF order
    std::vector<uint32_t> fam_by_family;        // row indices ordered by (family, row)
    std::vector<uint2> fam_run;                 // per row: its candidates' run, after assign
    int fam_cover_mm = 0;
    bool fam_set = false, fam_assigned = false, fam_have_join = false;
    uint64_t fam_bytes = 0, fam_pairs_per_launch = kPairsPerLaunch, fam_pairs = 0, fam_launches = 0;
    uint32_t fam_slice_min = kSliceMin;
    double ms_fam_assign = 0, ms_fam_compare = 0, ms_fam_join = 0;
    crp::FamilyRow *d_fam_rows = nullptr;
    uint2 *d_fam_run = nullptr;
    uint32_t *d_fam_tag = nullptr, *d_fam_family = nullptr, *d_fam_counts = nullptr;
    unsigned long long *d_fam_sum = nullptr, *d_fam_cover = nullptr;
    uint32_t *d_fjoin_counts[2] = {nullptr, nullptr}, *d_fjoin_family[2] = {nullptr, nullptr};
    unsigned long long *d_fjoin_sum[2] = {nullptr, nullptr}, *d_fjoin_cover[2] = {nullptr, nullptr};
    uint64_t fjoin_cap[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    uint64_t fjoin_rows[2] = {0, 0};  // the tables' rows at the time of the family join
    // the on-target model: crp_search_self_set_model .. crp_search_self_model_stats
    crp::ModelShape model = {};
    bool model_set = false, model_run = false;
    double *d_model_table = nullptr;  // MODEL_TABLE: single, pair, gc
    double *d_model = nullptr;        // n: the sums, in extraction order
    uint64_t model_bytes = 0;
    double ms_model = 0;

    crp::FamilyCands family_cands() const { return crp::FamilyCands{d_cand, d_cand + n, d_cand + 2 * n, d_fam_tag}; }
    void free_families()
    {
        (void)hipFree(d_fam_rows);
        (void)hipFree(d_fam_run);
        (void)hipFree(d_fam_tag);
        (void)hipFree(d_fam_family);
        (void)hipFree(d_fam_counts);
        (void)hipFree(d_fam_sum);
        (void)hipFree(d_fam_cover);
        d_fam_rows = nullptr;
        d_fam_run = nullptr;
        d_fam_tag = d_fam_family = d_fam_counts = nullptr;
        d_fam_sum = d_fam_cover = nullptr;
        bytes -= fam_bytes;
        fam_bytes = 0;
        fam_rows.clear();
        fam_by_family.clear();
        fam_run.clear();
        fam_set = fam_assigned = fam_have_join = false;
    }

    crp::SearchCands cands() const { return crp::SearchCands{d_cand, d_cand + n, d_cand + 2 * n, d_cand + 3 * n}; }
    crp::SelfOrder order() const
    {
        const uint64_t m = n + crp::SELF_PAD;
        return crp::SelfOrder{d_order, d_order + m, d_order + 2 * m, d_order + 3 * m};
    }
    uint64_t max_keys() const { return 2ull << (2 * crp::SELF_MAX_SEG_LETTERS); }
};

namespace {

int extract(crp_search_self *s, uint64_t budget, uint64_t *needed)
{
    crp_ctx *ctx = s->ctx;
    crp_arena *a = s->arena;
    const crp::Planes pl{{a->d_plane[0], a->d_plane[1], a->d_plane[2], a->d_plane[3]}};
    const uint64_t n_blocks = (a->used_words + crp::SEARCH_WORDS - 1) / crp::SEARCH_WORDS;
    std::vector<uint2> cnt(n_blocks);
    uint2 *d_cnt = nullptr;
    uint32_t *d_off = nullptr;
    int rc = CRP_OK;
    const auto fail = [&](hipError_t e, const char *what) {
        ctx->last_error = std::string(what) + ": " + hipGetErrorString(e);
        rc = e == hipErrorOutOfMemory ? CRP_ERR_NOMEM : CRP_ERR_HIP;
    };
    hipError_t e = hipSuccess;
    if (n_blocks) {
        e = hipMalloc(reinterpret_cast<void **>(&d_cnt), n_blocks * sizeof(uint2));
        if (e == hipSuccess) e = hipEventRecord(s->ev[0], ctx->stream);
        if (e == hipSuccess) e = crp::launch_search_count(ctx->stream, pl, a->used_words, s->sets, d_cnt);
        if (e == hipSuccess) e = hipEventRecord(s->ev[1], ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(cnt.data(), d_cnt, n_blocks * sizeof(uint2), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        (void)hipFree(d_cnt);
        if (e != hipSuccess) {
            fail(e, "crp_search_self_create (count)");
            return rc;
        }
        s->ms_extract += elapsed(s->ev[0], s->ev[1]);
    }
    std::vector<uint32_t> off(n_blocks);
    uint64_t total = 0;
    for (uint64_t b = 0; b < n_blocks; ++b) {
        off[b] = (uint32_t)total;
        total += (uint64_t)cnt[b].x + cnt[b].y;
        s->n_plus += cnt[b].x;
        s->n_minus += cnt[b].y;
    }
    if (total > kMaxCands) return CRP_ERR_UNSUPPORTED;
    s->n = total;
    // what the handle holds per candidate: 16 B of fields, 16 B of the current ordering, key, flag, one result row
    const uint64_t row = 4ull * (s->max_mm + 1) + 8;
    s->bytes = total * (16 + 16 + 4 + 1 + row) + 16ull * crp::SELF_PAD + 2 * s->max_keys() * sizeof(uint32_t) +
               kItemsPerLaunch * sizeof(uint4);
    if (needed) *needed = s->bytes;
    if (s->bytes > budget) return CRP_ERR_CAPACITY;
    const uint64_t n1 = std::max<uint64_t>(total, 1);
    CRP_HIP(ctx, hipMalloc(reinterpret_cast<void **>(&s->d_cand), n1 * 16));
    CRP_HIP(ctx, hipMalloc(reinterpret_cast<void **>(&s->d_flag), n1));
    CRP_HIP(ctx, hipMalloc(reinterpret_cast<void **>(&s->d_key), n1 * 4));
    CRP_HIP(ctx, hipMalloc(reinterpret_cast<void **>(&s->d_order), (total + crp::SELF_PAD) * 16));
    CRP_HIP(ctx, hipMalloc(reinterpret_cast<void **>(&s->d_hist), 2 * s->max_keys() * sizeof(uint32_t)));
    CRP_HIP(ctx, hipMalloc(reinterpret_cast<void **>(&s->d_counts), n1 * 4 * (s->max_mm + 1)));
    CRP_HIP(ctx, hipMalloc(reinterpret_cast<void **>(&s->d_hit_sum), n1 * 8));
    CRP_HIP(ctx, hipMalloc(reinterpret_cast<void **>(&s->d_items), kItemsPerLaunch * sizeof(uint4)));
    CRP_HIP(ctx, hipMemsetAsync(s->d_order, 0, (total + crp::SELF_PAD) * 16, ctx->stream));  // (the pad is read, never used)
    CRP_HIP(ctx, hipMemsetAsync(s->d_counts, 0, n1 * 4 * (s->max_mm + 1), ctx->stream));
    CRP_HIP(ctx, hipMemsetAsync(s->d_hit_sum, 0, n1 * 8, ctx->stream));
    unsigned long long *d_ng = reinterpret_cast<unsigned long long *>(s->d_hist);  // (free until the first ordering)
    CRP_HIP(ctx, hipMemsetAsync(d_ng, 0, sizeof(unsigned long long), ctx->stream));
    if (total) {
        CRP_HIP(ctx, hipMalloc(reinterpret_cast<void **>(&d_off), n_blocks * sizeof(uint32_t)));
        e = hipMemcpyAsync(d_off, off.data(), n_blocks * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipEventRecord(s->ev[0], ctx->stream);
        if (e == hipSuccess)
            e = crp::launch_search_emit(ctx->stream, pl, a->used_words, s->sets, 0, (uint32_t)n_blocks, d_off, s->cands());
        if (e == hipSuccess) e = crp::launch_self_flag(ctx->stream, s->cands(), (uint32_t)total, s->rule, s->d_flag, d_ng);
        if (e == hipSuccess) e = hipEventRecord(s->ev[1], ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // (off is read until here)
        (void)hipFree(d_off);
        if (e != hipSuccess) {
            fail(e, "crp_search_self_create (emit)");
            return rc;
        }
        s->ms_extract += elapsed(s->ev[0], s->ev[1]);
    }
    unsigned long long ng = 0;
    CRP_HIP(ctx, hipMemcpy(&ng, d_ng, sizeof(ng), hipMemcpyDeviceToHost));
    s->n_guides = ng;
    return CRP_OK;
}

}  // namespace

namespace crp {

bool self_joined(const crp_search_self *s, SelfJoined *out)
{
    if (!s || !s->have_join) return false;
    for (int k = 0; k < 2; ++k) {
        out->counts[k] = s->d_join_counts[k];
        out->sum[k] = s->d_join_sum[k];
        out->rows[k] = s->join_rows[k];
    }
    out->stride = s->max_mm + 1;
    out->arena = s->arena;
    return true;
}

void self_select_handle(const crp_search_self *s, SelfSelectHandle *out, bool *compared)
{
    const SearchCands c = s->cands();
    out->rows = SelfSelectRows{c.hi, c.lo, c.pos, s->d_flag, s->d_counts, s->value.any() ? s->d_hit_sum : nullptr,
                               s->model_run ? s->d_model : nullptr, (uint32_t)s->n, (uint32_t)s->max_mm + 1u};
    out->arena = s->arena;
    out->T = s->T;
    out->pam_len = s->pam_len;
    out->max_mm = s->max_mm;
    out->pam3 = s->pam3;
    out->scored = s->value.any();
    out->region = s->rule.region;
    out->n = s->n;
    *compared = s->compared == (2u << s->max_mm) - 1u;
}

bool self_family_joined(const crp_search_self *s, SelfFamilyJoined *out)
{
    if (!s || !s->fam_have_join) return false;
    for (int k = 0; k < 2; ++k) {
        out->counts[k] = s->d_fjoin_counts[k];
        out->sum[k] = s->d_fjoin_sum[k];
        out->cover[k] = s->d_fjoin_cover[k];
        out->family[k] = s->d_fjoin_family[k];
        out->rows[k] = s->fjoin_rows[k];
    }
    return true;
}

}  // namespace crp

extern "C" {

int crp_search_self_create(crp_arena *a, const char *pattern, const char *guide_pattern, int T, int pam_len, int max_mm, uint64_t budget,
                           uint64_t *needed_bytes, crp_search_self **out)
{
    if (!a || !pattern || !out) return CRP_ERR_INVALID;
    *out = nullptr;
    if (needed_bytes) *needed_bytes = 0;
    if (!guide_pattern) guide_pattern = pattern;
    if (T < 2 || T > CRP_SEARCH_MAX_T || max_mm < 0 || max_mm > CRP_SEARCH_SELF_MAX_MM) return CRP_ERR_UNSUPPORTED;
    if (pam_len < 1 || pam_len >= T) return CRP_ERR_INVALID;
    crp::SearchSets sets = {};
    sets.T = T;
    for (int o = 0; o < T; ++o) {
        const uint32_t sp = iupac_set(pattern[o]), sm = iupac_set(pattern[T - 1 - o]);
        if (!sp || !sm || !iupac_set(guide_pattern[o])) return CRP_ERR_INVALID;
        sets.plus[o >> 4] |= (uint64_t)sp << ((o & 15) * 4);
        sets.minus[o >> 4] |= (uint64_t)complement_set(sm) << ((o & 15) * 4);
    }
    // the guide region: all N on one side of the PAM, in both patterns
    const int G = T - pam_len;
    const auto all_n = [&](int lo, int hi) {
        for (int p = lo; p < hi; ++p)
            if (iupac_set(pattern[p]) != 15 || iupac_set(guide_pattern[p]) != 15) return false;
        return true;
    };
    const bool pam3 = all_n(0, G);
    if (!pam3 && !all_n(pam_len, T)) return CRP_ERR_INVALID;
    if (G < max_mm + 1) return CRP_ERR_UNSUPPORTED;
    const int glo = pam3 ? 0 : pam_len;
    crp::SelfGuideRule rule = {};
    rule.region = (G == 32 ? ~0u : (1u << G) - 1u) << glo;
    for (int p = pam3 ? G : 0; p < (pam3 ? T : pam_len); ++p) {
        const uint32_t sc = iupac_set(pattern[p]), sg = iupac_set(guide_pattern[p]);
        if (sg & ~sc) return CRP_ERR_INVALID;  // a guide site must be a candidate
        if (sg != sc) {
            rule.pos[rule.n] = (uint8_t)p;
            rule.set[rule.n] = (uint8_t)sg;
            ++rule.n;
        }
    }
    if (!a->sealed) return CRP_ERR_STATE;
    crp_ctx *ctx = a->ctx;
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    crp_search_self *s = new (std::nothrow) crp_search_self;
    if (!s) return CRP_ERR_NOMEM;
    s->arena = a;
    s->ctx = ctx;
    s->sets = sets;
    s->rule = rule;
    s->T = T;
    s->pam_len = pam_len;
    s->max_mm = max_mm;
    s->pam3 = pam3;
    // M + 1 segments from the region's first position, as even as they come, each at most SELF_MAX_SEG_LETTERS long
    int at = glo;
    for (int j = 0; j <= max_mm; ++j) {
        const int len = std::min(crp::SELF_MAX_SEG_LETTERS, G / (max_mm + 1) + (j < G % (max_mm + 1) ? 1 : 0));
        s->seg_shift[j] = at;
        s->seg_len[j] = len;
        at += len;
    }
    int rc = CRP_OK;
    for (int k = 0; k < 2 && rc == CRP_OK; ++k)
        if (hipEventCreate(&s->ev[k]) != hipSuccess) rc = CRP_ERR_HIP;
    s->budget = budget ? budget : CRP_SEARCH_SELF_DEFAULT_BUDGET;
    if (rc == CRP_OK) rc = extract(s, s->budget, needed_bytes);
    if (rc != CRP_OK) {
        crp_search_self_destroy(s);
        return rc;
    }
    *out = s;
    return CRP_OK;
}

int crp_search_self_destroy(crp_search_self *s)
{
    if (!s) return CRP_ERR_INVALID;
    (void)hipSetDevice(s->ctx->device);
    (void)hipFree(s->d_cand);
    (void)hipFree(s->d_flag);
    (void)hipFree(s->d_key);
    (void)hipFree(s->d_order);
    (void)hipFree(s->d_hist);
    (void)hipFree(s->d_counts);
    (void)hipFree(s->d_hit_sum);
    s->value.free();
    (void)hipFree(s->d_items);
    (void)hipFree(s->d_model_table);
    (void)hipFree(s->d_model);
    s->free_families();
    for (int k = 0; k < 2; ++k) {
        (void)hipFree(s->d_join_counts[k]);
        (void)hipFree(s->d_join_sum[k]);
        (void)hipFree(s->d_fjoin_counts[k]);
        (void)hipFree(s->d_fjoin_family[k]);
        (void)hipFree(s->d_fjoin_sum[k]);
        (void)hipFree(s->d_fjoin_cover[k]);
    }
    for (hipEvent_t e : s->ev)
        if (e) (void)hipEventDestroy(e);
    delete s;
    return CRP_OK;
}

int crp_search_self_set_limits(crp_search_self *s, uint64_t pairs_per_launch)
{
    if (!s) return CRP_ERR_INVALID;
    s->pairs_per_launch = pairs_per_launch ? std::min(pairs_per_launch, kPairsPerLaunch) : kPairsPerLaunch;
    return CRP_OK;
}

int crp_search_self_set_scheme(crp_search_self *s, const double *factor, int n_factor, const double *shape)
{
    if (!s) return CRP_ERR_INVALID;
    if (!factor) {
        s->value.clear();
        return CRP_OK;
    }
    if (n_factor != s->T - s->pam_len) return CRP_ERR_INVALID;
    return s->value.set_scheme(s->ctx, s->T, factor, n_factor, s->pam3, shape);
}

int crp_search_self_set_pair_scheme(crp_search_self *s, const double *pair, int n_factor, const int *pam_offsets, int n_pam_offsets,
                                    const double *pam)
{
    if (!s) return CRP_ERR_INVALID;
    if (!pair) {
        s->value.clear();
        return CRP_OK;
    }
    if (n_factor != s->T - s->pam_len) return CRP_ERR_INVALID;
    return s->value.set_pair(s->ctx, s->sets, pair, n_factor, s->pam3, pam_offsets, n_pam_offsets, pam);
}

int crp_search_self_sizes(const crp_search_self *s, uint64_t *n_plus, uint64_t *n_minus, uint64_t *n_guides)
{
    if (!s) return CRP_ERR_INVALID;
    if (n_plus) *n_plus = s->n_plus;
    if (n_minus) *n_minus = s->n_minus;
    if (n_guides) *n_guides = s->n_guides;
    return CRP_OK;
}

int crp_search_self_order(crp_search_self *s, int segment)
{
    if (!s || segment < 0 || segment > s->max_mm) return CRP_ERR_INVALID;
    crp_ctx *ctx = s->ctx;
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    s->segment = -1;
    const int len = s->seg_len[segment];
    const uint64_t keys = 2ull << (2 * len);
    s->hist.assign(keys, 0);
    s->start.assign(keys, 0);
    if (s->n) {
        uint32_t *d_cursor = s->d_hist + s->max_keys();
        CRP_HIP(ctx, hipMemsetAsync(s->d_hist, 0, keys * sizeof(uint32_t), ctx->stream));
        CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
        CRP_HIP(ctx, crp::launch_self_key(ctx->stream, s->cands(), (uint32_t)s->n, s->d_flag, s->seg_shift[segment], len, s->d_key, s->d_hist));
        CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
        CRP_HIP(ctx, hipMemcpyAsync(s->hist.data(), s->d_hist, keys * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        s->ms_order += elapsed(s->ev[0], s->ev[1]);
        uint64_t at = 0;
        for (uint64_t k = 0; k < keys; ++k) {
            s->start[k] = (uint32_t)at;
            at += s->hist[k];
        }
        if (at > s->n) {  // (cannot be: every candidate has at most one key)
            ctx->last_error = "crp_search_self_order: histogram larger than the candidate list";
            return CRP_ERR_HIP;
        }
        const crp::SelfOrder o = s->order();
        CRP_HIP(ctx, hipMemcpyAsync(d_cursor, s->start.data(), keys * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
        CRP_HIP(ctx, crp::launch_self_scatter(ctx->stream, s->cands(), (uint32_t)s->n, s->d_key, s->rule.region, d_cursor,
                                              const_cast<uint32_t *>(o.hi), const_cast<uint32_t *>(o.lo), const_cast<uint32_t *>(o.nb),
                                              const_cast<uint32_t *>(o.idx)));
        CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
        CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        s->ms_order += elapsed(s->ev[0], s->ev[1]);
        s->n_order += 2;
    }
    s->segment = segment;
    return CRP_OK;
}

int crp_search_self_compare(crp_search_self *q, crp_search_self *c)
{
    if (!q || !c) return CRP_ERR_INVALID;
    if (q->ctx != c->ctx || q->T != c->T || q->pam_len != c->pam_len || q->max_mm != c->max_mm || q->rule.region != c->rule.region)
        return CRP_ERR_INVALID;
    if (q->segment < 0 || q->segment != c->segment) return CRP_ERR_STATE;
    crp_ctx *ctx = q->ctx;
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    crp::SelfCompare cmp = {};
    cmp.n_before = q->segment;
    cmp.max_mm = q->max_mm;
    cmp.skip_same = q == c;
    for (int j = 0; j < q->segment; ++j) cmp.before[j] = ((1u << q->seg_len[j]) - 1u) << q->seg_shift[j];
    const crp::SearchScore score = q->value.score(q->d_hit_sum);
    const crp::SearchScore *sc = q->value.have_scheme ? &score : nullptr;
    // under a pair table the candidates' PAM letters are read from the candidates' handle: its fields, through its ordering
    const crp::SearchPair pair = q->value.pair(q->d_hit_sum);
    std::vector<uint4> items;
    uint64_t pairs = 0;
    const auto flush = [&]() -> int {
        if (items.empty()) return CRP_OK;
        CRP_HIP(ctx, hipMemcpy(q->d_items, items.data(), items.size() * sizeof(uint4), hipMemcpyHostToDevice));
        CRP_HIP(ctx, hipEventRecord(q->ev[0], ctx->stream));
        if (q->value.have_pair)
            CRP_HIP(ctx, crp::launch_self_pair_compare(ctx->stream, q->order(), c->order(), c->cands(), q->d_items, (uint32_t)items.size(), cmp,
                                                       q->d_counts, pair));
        else
            CRP_HIP(ctx, crp::launch_self_compare(ctx->stream, q->order(), c->order(), q->d_items, (uint32_t)items.size(), cmp, q->d_counts, sc));
        CRP_HIP(ctx, hipEventRecord(q->ev[1], ctx->stream));
        CRP_HIP(ctx, hipEventSynchronize(q->ev[1]));
        const double ms = elapsed(q->ev[0], q->ev[1]);
        q->ms_compare += ms;
        q->ms_longest = std::max(q->ms_longest, ms);
        q->n_compare += 1;
        q->pairs += pairs;
        items.clear();
        pairs = 0;
        return CRP_OK;
    };
    const uint64_t buckets = q->hist.size() / 2;
    for (uint64_t b = 0; b < buckets; ++b) {
        const uint32_t nq = q->hist[2 * b], nc = c->hist[2 * b] + c->hist[2 * b + 1];
        if (!nq || !nc) continue;
        const uint32_t slices = std::min<uint32_t>(kSlicesMax, (nc + kSliceMin - 1) / kSliceMin);
        const uint32_t per = ((nc + slices - 1) / slices + crp::SELF_UNROLL - 1) / crp::SELF_UNROLL * crp::SELF_UNROLL;
        for (uint32_t t = 0; t < nq; t += crp::SELF_TILE) {
            const uint32_t tq = std::min<uint32_t>(crp::SELF_TILE, nq - t);
            for (uint32_t c0 = 0; c0 < nc; c0 += per) {
                const uint32_t tc = std::min(per, nc - c0);
                const uint64_t p = (uint64_t)tq * tc;
                if (!items.empty() && (pairs + p > q->pairs_per_launch || items.size() >= kItemsPerLaunch)) {
                    const int rc = flush();
                    if (rc != CRP_OK) return rc;
                }
                items.push_back(make_uint4(q->start[2 * b] + t, tq, c->start[2 * b] + c0, tc));
                pairs += p;
            }
        }
    }
    const int rc = flush();
    if (rc == CRP_OK) q->compared |= 1u << q->segment;
    return rc;
}

int crp_search_self_fetch(crp_search_self *s, uint32_t *arena_pos, uint8_t *strand, uint32_t *hi, uint32_t *lo, uint32_t *counts,
                          uint64_t *hit_sum, uint64_t cap)
{
    if (!s) return CRP_ERR_INVALID;
    if (cap < s->n_guides) return CRP_ERR_CAPACITY;
    crp_ctx *ctx = s->ctx;
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const uint64_t chunk = 1ull << 22, stride = (uint64_t)s->max_mm + 1;
    std::vector<uint8_t> flag(chunk);
    std::vector<uint32_t> w(chunk), cnt(counts ? chunk * stride : 0);
    std::vector<uint64_t> hs(hit_sum ? chunk : 0);
    const crp::SearchCands c = s->cands();
    uint64_t k = 0;
    for (uint64_t i0 = 0; i0 < s->n; i0 += chunk) {
        const uint64_t m = std::min(chunk, s->n - i0);
        CRP_HIP(ctx, hipMemcpy(flag.data(), s->d_flag + i0, m, hipMemcpyDeviceToHost));
        const uint64_t k0 = k;
        const auto column = [&](const uint32_t *src, auto put) -> int {
            CRP_HIP(ctx, hipMemcpy(w.data(), src + i0, m * sizeof(uint32_t), hipMemcpyDeviceToHost));
            uint64_t kk = k0;
            for (uint64_t i = 0; i < m; ++i)
                if (flag[i]) put(kk++, w[i]);
            return CRP_OK;
        };
        int rc = CRP_OK;
        if (arena_pos || strand)
            rc = column(c.pos, [&](uint64_t kk, uint32_t v) {
                if (arena_pos) arena_pos[kk] = v & 0x7fffffffu;
                if (strand) strand[kk] = (uint8_t)(v >> 31);
            });
        if (rc == CRP_OK && hi) rc = column(c.hi, [&](uint64_t kk, uint32_t v) { hi[kk] = v; });
        if (rc == CRP_OK && lo) rc = column(c.lo, [&](uint64_t kk, uint32_t v) { lo[kk] = v; });
        if (rc != CRP_OK) return rc;
        if (counts) CRP_HIP(ctx, hipMemcpy(cnt.data(), s->d_counts + i0 * stride, m * stride * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (hit_sum) CRP_HIP(ctx, hipMemcpy(hs.data(), s->d_hit_sum + i0, m * sizeof(uint64_t), hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < m; ++i) {
            if (!flag[i]) continue;
            if (counts) std::memcpy(counts + k * stride, cnt.data() + i * stride, stride * sizeof(uint32_t));
            if (hit_sum) hit_sum[k] = hs[i];
            ++k;
        }
    }
    return k == s->n_guides ? CRP_OK : CRP_ERR_HIP;
}

int crp_search_self_join_hits(crp_search_self *s, int guide_len, uint32_t *counts_plus, uint64_t *hit_sum_plus, uint32_t *counts_minus,
                              uint64_t *hit_sum_minus)
{
    if (!s) return CRP_ERR_INVALID;
    crp_ctx *ctx = s->ctx;
    crp_arena *a = s->arena;
    s->have_join = false;
    if (s->T != guide_len + 3) {
        ctx->last_error = "crp_search_self_join_hits: a pattern of " + std::to_string(s->T) + " letters does not join hits of guide length " +
                          std::to_string(guide_len) + " (pattern_len must be guide_len + 3)";
        return CRP_ERR_INVALID;
    }
    if (!s->pam3 || s->pam_len != 3) {
        ctx->last_error = "crp_search_self_join_hits: the handle's PAM must be the pattern's last 3 letters";
        return CRP_ERR_INVALID;
    }
    if (!a->have_hits || a->pend_guide_len != guide_len) {
        ctx->last_error = "crp_search_self_join_hits: the arena has no hit tables of guide length " + std::to_string(guide_len);
        return CRP_ERR_INVALID;
    }
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t stride = (uint64_t)s->max_mm + 1;
    for (int k = 0; k < 2; ++k) {
        int rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_join_counts[k]), &s->join_counts_cap[k], a->n_hits[k] * stride, sizeof(uint32_t));
        if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_join_sum[k]), &s->join_sum_cap[k], a->n_hits[k], sizeof(uint64_t));
        if (rc != CRP_OK) return rc;
    }
    const unsigned long long *sums = s->value.any() ? s->d_hit_sum : nullptr;  // an unscored handle joins counts only
    CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
    for (int k = 0; k < 2; ++k)  // (a table has fewer rows than the arena positions: below 2^31)
        CRP_HIP(ctx, crp::launch_self_join(ctx->stream, a->d_pos[k], (uint32_t)a->n_hits[k], k, guide_len, s->cands(), (uint32_t)s->n, s->d_flag,
                                           s->d_counts, sums, s->max_mm, s->d_join_counts[k], s->d_join_sum[k]));
    CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->ms_join += elapsed(s->ev[0], s->ev[1]);
    s->have_join = true;
    s->join_rows[0] = a->n_hits[0];
    s->join_rows[1] = a->n_hits[1];
    uint32_t *hc[2] = {counts_plus, counts_minus};
    uint64_t *hs[2] = {hit_sum_plus, hit_sum_minus};
    for (int k = 0; k < 2; ++k) {
        const uint64_t n = a->n_hits[k];
        if (!n) continue;
        int rc = CRP_OK;
        if (hc[k]) rc = crp::staged_d2h(ctx, hc[k], s->d_join_counts[k], n * stride * sizeof(uint32_t));
        if (rc == CRP_OK && hs[k]) rc = crp::staged_d2h(ctx, hs[k], s->d_join_sum[k], n * sizeof(uint64_t));
        if (rc != CRP_OK) return rc;
    }
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CRP_OK;
}

int crp_search_self_join_device(crp_search_self *s, void **counts_plus, void **hit_sum_plus, void **counts_minus, void **hit_sum_minus)
{
    if (!s) return CRP_ERR_INVALID;
    if (!s->have_join) return CRP_ERR_STATE;
    if (counts_plus) *counts_plus = s->d_join_counts[0];
    if (hit_sum_plus) *hit_sum_plus = s->d_join_sum[0];
    if (counts_minus) *counts_minus = s->d_join_counts[1];
    if (hit_sum_minus) *hit_sum_minus = s->d_join_sum[1];
    return CRP_OK;
}

int crp_search_self_stats(const crp_search_self *s, double *out, int n)
{
    if (!s || (n && !out) || n < 0 || n > 9) return CRP_ERR_INVALID;
    const double v[9] = {s->ms_extract, s->ms_order, s->ms_compare, (double)s->n_compare, s->ms_longest,
                         (double)s->pairs, (double)s->bytes, (double)s->n_order, s->ms_join};
    for (int k = 0; k < n; ++k) out[k] = v[k];
    return CRP_OK;
}

// ---- on-target model ---------------------------------------------------------------------------

int crp_search_self_set_model(crp_search_self *s, int window, int left, double intercept, const double *single, const double *pair,
                              const double *gc, int n_gc)
{
    if (!s) return CRP_ERR_INVALID;
    crp_ctx *ctx = s->ctx;
    const std::string who = "crp_search_self_set_model";
    const auto refuse = [&](const std::string &text) {
        ctx->last_error = who + ": " + text;
        return CRP_ERR_INVALID;
    };
    const int G = s->T - s->pam_len;
    if (window < 1 || window > crp::MODEL_MAX_W)
        return refuse("a window of 1.." + std::to_string(crp::MODEL_MAX_W) + " letters is scored, not " + std::to_string(window));
    if (left < 0 || left >= window)
        return refuse("left must be 0.." + std::to_string(window - 1) + " (the window holds at least pattern position 0), not " +
                      std::to_string(left));
    if (gc && n_gc != G + 1)
        return refuse("the gc table has " + std::to_string(n_gc) + " weights, the guide region " + std::to_string(G) + " letters (" +
                      std::to_string(G + 1) + " counts)");
    // terms not given are 0.0; the device always reads full tables
    std::vector<double> table(crp::MODEL_TABLE, 0.0);
    const auto copy = [&](const double *src, int n, int at) {
        for (int i = 0; src && i < n; ++i) {
            if (!std::isfinite(src[i])) return false;
            table[at + i] = src[i];
        }
        return true;
    };
    if (!std::isfinite(intercept)) return refuse("the intercept is not a finite number");
    if (!copy(single, window * 4, 0)) return refuse("a single-letter weight is not a finite number");
    if (!copy(pair, (window - 1) * 16, crp::MODEL_SINGLE)) return refuse("a pair weight is not a finite number");
    if (!copy(gc, G + 1, crp::MODEL_SINGLE + crp::MODEL_PAIR)) return refuse("a gc weight is not a finite number");
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    if (!s->d_model_table) {
        const uint64_t n1 = std::max<uint64_t>(s->n, 1);
        const uint64_t add = n1 * sizeof(double) + crp::MODEL_TABLE * sizeof(double);
        if (s->bytes + add > s->budget) {
            ctx->last_error = who + ": the handle with a model column needs " + std::to_string(s->bytes + add) +
                              " bytes of device memory: more than the budget of " + std::to_string(s->budget);
            return CRP_ERR_CAPACITY;
        }
        double *tab = nullptr, *col = nullptr;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&tab), crp::MODEL_TABLE * sizeof(double));
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&col), n1 * sizeof(double));
        if (e != hipSuccess) {
            (void)hipFree(tab);
            ctx->last_error = who + ": " + hipGetErrorString(e);
            return e == hipErrorOutOfMemory ? CRP_ERR_NOMEM : CRP_ERR_HIP;
        }
        s->d_model_table = tab;
        s->d_model = col;
        s->model_bytes = add;
        s->bytes += add;
    }
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (an earlier run of the model has read the table)
    s->model_set = s->model_run = false;
    CRP_HIP(ctx, hipMemcpy(s->d_model_table, table.data(), crp::MODEL_TABLE * sizeof(double), hipMemcpyHostToDevice));
    s->model = crp::ModelShape{window, left, s->T, s->rule.region, intercept};
    s->model_set = true;
    return CRP_OK;
}

int crp_search_self_run_model(crp_search_self *s)
{
    if (!s) return CRP_ERR_INVALID;
    crp_ctx *ctx = s->ctx;
    crp_arena *a = s->arena;
    if (!s->model_set) {
        ctx->last_error = "crp_search_self_run_model: no model on the handle (crp_search_self_set_model)";
        return CRP_ERR_STATE;
    }
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    s->model_run = false;
    const crp::SearchCands c = s->cands();
    const crp::ModelPlanes planes{a->d_plane[0], a->d_plane[1], a->d_plane[3], a->padded_words};
    CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
    CRP_HIP(ctx, crp::launch_self_model(ctx->stream, c.pos, c.hi, s->d_flag, (uint32_t)s->n, planes, s->model, s->d_model_table, s->d_model));
    CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->ms_model = elapsed(s->ev[0], s->ev[1]);
    s->model_run = true;
    return CRP_OK;
}

int crp_search_self_fetch_model(crp_search_self *s, double *sum, uint64_t cap)
{
    if (!s || !sum) return CRP_ERR_INVALID;
    crp_ctx *ctx = s->ctx;
    if (!s->model_run) {
        ctx->last_error = "crp_search_self_fetch_model: the handle's model has not been run (crp_search_self_run_model)";
        return CRP_ERR_STATE;
    }
    if (cap < s->n_guides) return CRP_ERR_CAPACITY;
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const uint64_t chunk = 1ull << 22, m1 = std::min(chunk, std::max<uint64_t>(s->n, 1));
    std::vector<uint8_t> flag(m1);
    std::vector<double> v(m1);
    uint64_t k = 0;
    for (uint64_t i0 = 0; i0 < s->n; i0 += chunk) {
        const uint64_t m = std::min(chunk, s->n - i0);
        CRP_HIP(ctx, hipMemcpy(flag.data(), s->d_flag + i0, m, hipMemcpyDeviceToHost));
        CRP_HIP(ctx, hipMemcpy(v.data(), s->d_model + i0, m * sizeof(double), hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < m; ++i) {
            if (!flag[i]) continue;
            if (k >= cap) return CRP_ERR_HIP;  // (cannot be: the flags were counted at create)
            sum[k++] = v[i];
        }
    }
    return k == s->n_guides ? CRP_OK : CRP_ERR_HIP;
}

int crp_search_self_model_stats(const crp_search_self *s, double *out, int n)
{
    if (!s || (n && !out) || n < 0 || n > 2) return CRP_ERR_INVALID;
    if (!s->model_run) return CRP_ERR_STATE;
    const double v[2] = {s->ms_model, (double)s->n};
    for (int k = 0; k < n; ++k) out[k] = v[k];
    return CRP_OK;
}

// ---- gene families ----------------------------------------------------------------------------

int crp_search_self_set_families(crp_search_self *s, const uint32_t *lo, const uint32_t *hi, const uint32_t *family, const uint32_t *member,
                                 uint64_t n_rows, int cover_mm)
{
    if (!s) return CRP_ERR_INVALID;
    crp_ctx *ctx = s->ctx;
    if (n_rows && (!lo || !hi || !family || !member)) return CRP_ERR_INVALID;
    if (!s->pam3 || s->pam_len != 3) {
        ctx->last_error = "crp_search_self_set_families: the handle's PAM must be the pattern's last 3 letters (the cut-site rule is that geometry's)";
        return CRP_ERR_INVALID;
    }
    if (cover_mm < 0 || cover_mm > s->max_mm) {
        ctx->last_error = "crp_search_self_set_families: cover limit " + std::to_string(cover_mm) + " is outside 0.." + std::to_string(s->max_mm);
        return CRP_ERR_INVALID;
    }
    if (n_rows >= crp::FAMILY_NO_ROW) return CRP_ERR_UNSUPPORTED;
    for (uint64_t r = 0; r < n_rows; ++r) {
        if (member[r] >= (uint32_t)crp::FAMILY_MAX_MEMBERS) {
            ctx->last_error = "crp_search_self_set_families: member bit " + std::to_string(member[r]) + " of row " + std::to_string(r) +
                              ": a family has at most " + std::to_string(crp::FAMILY_MAX_MEMBERS) + " members";
            return CRP_ERR_INVALID;
        }
        if (family[r] == crp::FAMILY_NONE) {
            ctx->last_error = "crp_search_self_set_families: family id 0xFFFFFFFF of row " + std::to_string(r) + " means no family";
            return CRP_ERR_INVALID;
        }
    }
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->free_families();
    if (!n_rows && !lo) return CRP_OK;  // families taken off the handle
    const uint64_t stride = (uint64_t)s->max_mm + 1;
    const uint64_t add = s->n * (4 * stride + 8 + 8 + 4 + 4) + n_rows * (sizeof(crp::FamilyRow) + sizeof(uint2));
    if (s->bytes + add > s->budget) {
        ctx->last_error = "crp_search_self_set_families: the handle with families needs " + std::to_string(s->bytes + add) +
                          " bytes of device memory: more than the budget of " + std::to_string(s->budget);
        return CRP_ERR_CAPACITY;
    }
    const uint64_t n1 = std::max<uint64_t>(s->n, 1), r1 = std::max<uint64_t>(n_rows, 1);
    s->fam_bytes = add;
    s->bytes += add;
    s->fam_rows.resize(n_rows);
    for (uint64_t r = 0; r < n_rows; ++r) s->fam_rows[r] = crp::FamilyRow{lo[r], hi[r], family[r], member[r]};
    s->fam_by_family.resize(n_rows);
    for (uint64_t r = 0; r < n_rows; ++r) s->fam_by_family[r] = (uint32_t)r;
    std::stable_sort(s->fam_by_family.begin(), s->fam_by_family.end(),
                     [&](uint32_t a, uint32_t b) { return s->fam_rows[a].family < s->fam_rows[b].family; });
    int rc = CRP_OK;
    const auto alloc = [&](void **p, uint64_t bytes) {
        if (rc != CRP_OK) return;
        const hipError_t e = hipMalloc(p, bytes);
        if (e != hipSuccess) {
            ctx->last_error = std::string("crp_search_self_set_families: ") + hipGetErrorString(e);
            rc = e == hipErrorOutOfMemory ? CRP_ERR_NOMEM : CRP_ERR_HIP;
        }
    };
    alloc(reinterpret_cast<void **>(&s->d_fam_rows), r1 * sizeof(crp::FamilyRow));
    alloc(reinterpret_cast<void **>(&s->d_fam_run), r1 * sizeof(uint2));
    alloc(reinterpret_cast<void **>(&s->d_fam_tag), n1 * 4);
    alloc(reinterpret_cast<void **>(&s->d_fam_family), n1 * 4);
    alloc(reinterpret_cast<void **>(&s->d_fam_counts), n1 * 4 * stride);
    alloc(reinterpret_cast<void **>(&s->d_fam_sum), n1 * 8);
    alloc(reinterpret_cast<void **>(&s->d_fam_cover), n1 * 8);
    if (rc == CRP_OK && n_rows &&
        hipMemcpy(s->d_fam_rows, s->fam_rows.data(), n_rows * sizeof(crp::FamilyRow), hipMemcpyHostToDevice) != hipSuccess) {
        ctx->last_error = "crp_search_self_set_families: upload of the family rows failed";
        rc = CRP_ERR_HIP;
    }
    if (rc != CRP_OK) {
        s->free_families();
        return rc;
    }
    s->fam_cover_mm = cover_mm;
    s->fam_set = true;
    return CRP_OK;
}

int crp_search_self_family_set_limits(crp_search_self *s, uint64_t pairs_per_launch, uint32_t slice_min)
{
    if (!s) return CRP_ERR_INVALID;
    s->fam_pairs_per_launch = pairs_per_launch ? std::min(pairs_per_launch, kPairsPerLaunch) : kPairsPerLaunch;
    s->fam_slice_min = slice_min ? std::max(slice_min, kFamilySliceFloor) : kSliceMin;
    return CRP_OK;
}

int crp_search_self_family_assign(crp_search_self *s)
{
    if (!s) return CRP_ERR_INVALID;
    crp_ctx *ctx = s->ctx;
    if (!s->fam_set) {
        ctx->last_error = "crp_search_self_family_assign: no families on the handle (crp_search_self_set_families)";
        return CRP_ERR_STATE;
    }
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    s->fam_assigned = s->fam_have_join = false;
    const uint64_t stride = (uint64_t)s->max_mm + 1, n1 = std::max<uint64_t>(s->n, 1);
    const uint32_t n_rows = (uint32_t)s->fam_rows.size(), n = (uint32_t)s->n;
    const crp::SearchCands c = s->cands();
    CRP_HIP(ctx, hipMemsetAsync(s->d_fam_tag, 0xFF, n1 * 4, ctx->stream));  // no owner
    CRP_HIP(ctx, hipMemsetAsync(s->d_fam_counts, 0, n1 * 4 * stride, ctx->stream));
    CRP_HIP(ctx, hipMemsetAsync(s->d_fam_sum, 0, n1 * 8, ctx->stream));
    CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
    CRP_HIP(ctx, crp::launch_family_bounds(ctx->stream, s->d_fam_rows, n_rows, c.pos, n, s->T, s->d_fam_run));
    CRP_HIP(ctx, crp::launch_family_assign(ctx->stream, s->d_fam_rows, n_rows, s->d_fam_run, c.pos, s->T, s->d_fam_tag));
    CRP_HIP(ctx, crp::launch_family_finish(ctx->stream, s->d_fam_rows, s->d_flag, n, s->d_fam_tag, s->d_fam_family, s->d_fam_cover));
    CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
    s->fam_run.assign(n_rows, make_uint2(0, 0));
    if (n_rows) CRP_HIP(ctx, hipMemcpyAsync(s->fam_run.data(), s->d_fam_run, n_rows * sizeof(uint2), hipMemcpyDeviceToHost, ctx->stream));
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->ms_fam_assign += elapsed(s->ev[0], s->ev[1]);
    for (const uint2 &r : s->fam_run)
        if (r.x > r.y || r.y > s->n) {  // (cannot be: both ends come from one search over n candidates)
            ctx->last_error = "crp_search_self_family_assign: a run outside the candidate list";
            return CRP_ERR_HIP;
        }
    s->fam_assigned = true;
    return CRP_OK;
}

int crp_search_self_family_compare(crp_search_self *q, crp_search_self *c)
{
    if (!q || !c) return CRP_ERR_INVALID;
    if (q->ctx != c->ctx || q->T != c->T || q->pam_len != c->pam_len || q->max_mm != c->max_mm || q->rule.region != c->rule.region)
        return CRP_ERR_INVALID;
    crp_ctx *ctx = q->ctx;
    if (!q->fam_assigned || !c->fam_assigned) {
        ctx->last_error = "crp_search_self_family_compare: both handles need crp_search_self_family_assign first";
        return CRP_ERR_STATE;
    }
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    crp::FamilyCompare cmp = {};
    cmp.region = q->rule.region;
    cmp.max_mm = q->max_mm;
    cmp.cover_mm = q->fam_cover_mm;
    cmp.same = q == c;
    const crp::SearchScore score = q->value.score(nullptr);
    const crp::SearchPair pair = q->value.pair(nullptr);
    std::vector<uint4> items;
    uint64_t pairs = 0;
    const auto flush = [&]() -> int {
        if (items.empty()) return CRP_OK;
        CRP_HIP(ctx, hipMemcpy(q->d_items, items.data(), items.size() * sizeof(uint4), hipMemcpyHostToDevice));
        CRP_HIP(ctx, hipEventRecord(q->ev[0], ctx->stream));
        CRP_HIP(ctx, crp::launch_family_compare(ctx->stream, q->family_cands(), c->family_cands(), q->d_items, (uint32_t)(items.size() / 2), cmp,
                                                q->d_fam_counts, q->d_fam_sum, q->d_fam_cover, q->value.have_scheme ? &score : nullptr,
                                                q->value.have_pair ? &pair : nullptr));
        CRP_HIP(ctx, hipEventRecord(q->ev[1], ctx->stream));
        CRP_HIP(ctx, hipEventSynchronize(q->ev[1]));
        q->ms_fam_compare += elapsed(q->ev[0], q->ev[1]);
        q->fam_launches += 1;
        q->fam_pairs += pairs;
        items.clear();
        pairs = 0;
        return CRP_OK;
    };
    // the candidates' rows by family: [first, end) of c->fam_by_family per family id met in q
    const auto &order = c->fam_by_family;
    for (uint32_t a = 0; a < q->fam_rows.size(); ++a) {
        const uint2 qr = q->fam_run[a];
        if (qr.x == qr.y) continue;
        const uint32_t fam = q->fam_rows[a].family;
        auto at = std::lower_bound(order.begin(), order.end(), fam, [&](uint32_t r, uint32_t f) { return c->fam_rows[r].family < f; });
        for (; at != order.end() && c->fam_rows[*at].family == fam; ++at) {
            const uint32_t b = *at;
            const uint2 cr = c->fam_run[b];
            const uint32_t nc = cr.y - cr.x;
            if (!nc) continue;
            const uint32_t slices = std::min<uint32_t>(kSlicesMax, std::max<uint32_t>(1, nc / q->fam_slice_min));
            const uint32_t per = ((nc + slices - 1) / slices + crp::SELF_UNROLL - 1) / crp::SELF_UNROLL * crp::SELF_UNROLL;
            for (uint32_t t = qr.x; t < qr.y; t += crp::SELF_TILE) {
                const uint32_t tq = std::min<uint32_t>(crp::SELF_TILE, qr.y - t);
                for (uint32_t c0 = 0; c0 < nc; c0 += per) {
                    const uint32_t tc = std::min(per, nc - c0);
                    const uint64_t p = (uint64_t)tq * tc;
                    if (!items.empty() && (pairs + p > q->fam_pairs_per_launch || items.size() / 2 >= kFamilyItemsPerLaunch)) {
                        const int rc = flush();
                        if (rc != CRP_OK) return rc;
                    }
                    items.push_back(make_uint4(t, tq, cr.x + c0, tc));
                    items.push_back(make_uint4(a, b, c->fam_rows[b].member, 0));
                    pairs += p;
                }
            }
        }
    }
    return flush();
}

int crp_search_self_family_fetch(crp_search_self *s, uint32_t *owner, uint32_t *family, uint32_t *counts, uint64_t *sum, uint64_t *cover,
                                 uint64_t cap)
{
    if (!s) return CRP_ERR_INVALID;
    crp_ctx *ctx = s->ctx;
    if (!s->fam_assigned) {
        ctx->last_error = "crp_search_self_family_fetch: no assigned families on the handle";
        return CRP_ERR_STATE;
    }
    if (cap < s->n_guides) return CRP_ERR_CAPACITY;
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const uint64_t chunk = 1ull << 22, stride = (uint64_t)s->max_mm + 1;
    const uint64_t m1 = std::min(chunk, std::max<uint64_t>(s->n, 1));
    std::vector<uint32_t> tag(m1), fam(family ? m1 : 0), cnt(counts ? m1 * stride : 0);
    std::vector<uint64_t> sm(sum ? m1 : 0), cv(cover ? m1 : 0);
    uint64_t k = 0;
    for (uint64_t i0 = 0; i0 < s->n; i0 += chunk) {
        const uint64_t m = std::min(chunk, s->n - i0);
        CRP_HIP(ctx, hipMemcpy(tag.data(), s->d_fam_tag + i0, m * 4, hipMemcpyDeviceToHost));
        if (family) CRP_HIP(ctx, hipMemcpy(fam.data(), s->d_fam_family + i0, m * 4, hipMemcpyDeviceToHost));
        if (counts) CRP_HIP(ctx, hipMemcpy(cnt.data(), s->d_fam_counts + i0 * stride, m * stride * 4, hipMemcpyDeviceToHost));
        if (sum) CRP_HIP(ctx, hipMemcpy(sm.data(), s->d_fam_sum + i0, m * 8, hipMemcpyDeviceToHost));
        if (cover) CRP_HIP(ctx, hipMemcpy(cv.data(), s->d_fam_cover + i0, m * 8, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < m; ++i) {
            if (!(tag[i] & crp::FAMILY_GUIDE)) continue;
            if (k >= cap) return CRP_ERR_HIP;  // (cannot be: the tags carry the guide flags)
            const uint32_t row = tag[i] & crp::FAMILY_NO_ROW;
            if (owner) owner[k] = row == crp::FAMILY_NO_ROW ? crp::FAMILY_NONE : row;
            if (family) family[k] = fam[i];
            if (counts) std::memcpy(counts + k * stride, cnt.data() + i * stride, stride * sizeof(uint32_t));
            if (sum) sum[k] = sm[i];
            if (cover) cover[k] = cv[i];
            ++k;
        }
    }
    return k == s->n_guides ? CRP_OK : CRP_ERR_HIP;
}

int crp_search_self_family_join_hits(crp_search_self *s, int guide_len, uint32_t *counts_plus, uint64_t *sum_plus, uint64_t *cover_plus,
                                     uint32_t *family_plus, uint32_t *counts_minus, uint64_t *sum_minus, uint64_t *cover_minus,
                                     uint32_t *family_minus)
{
    if (!s) return CRP_ERR_INVALID;
    uint32_t *const counts[2] = {counts_plus, counts_minus}, *const family[2] = {family_plus, family_minus};
    uint64_t *const sum[2] = {sum_plus, sum_minus}, *const cover[2] = {cover_plus, cover_minus};
    crp_ctx *ctx = s->ctx;
    crp_arena *a = s->arena;
    s->fam_have_join = false;
    if (!s->fam_assigned) {
        ctx->last_error = "crp_search_self_family_join_hits: no assigned families on the handle";
        return CRP_ERR_STATE;
    }
    if (s->T != guide_len + 3) {
        ctx->last_error = "crp_search_self_family_join_hits: a pattern of " + std::to_string(s->T) +
                          " letters does not join hits of guide length " + std::to_string(guide_len);
        return CRP_ERR_INVALID;
    }
    if (!a->have_hits || a->pend_guide_len != guide_len) {
        ctx->last_error = "crp_search_self_family_join_hits: the arena has no hit tables of guide length " + std::to_string(guide_len);
        return CRP_ERR_INVALID;
    }
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t stride = (uint64_t)s->max_mm + 1;
    for (int k = 0; k < 2; ++k) {
        int rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_fjoin_counts[k]), &s->fjoin_cap[k][0], a->n_hits[k] * stride, sizeof(uint32_t));
        if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_fjoin_sum[k]), &s->fjoin_cap[k][1], a->n_hits[k], sizeof(uint64_t));
        if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_fjoin_cover[k]), &s->fjoin_cap[k][2], a->n_hits[k], sizeof(uint64_t));
        if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_fjoin_family[k]), &s->fjoin_cap[k][3], a->n_hits[k], sizeof(uint32_t));
        if (rc != CRP_OK) return rc;
    }
    CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
    for (int k = 0; k < 2; ++k)
        CRP_HIP(ctx, crp::launch_family_join(ctx->stream, a->d_pos[k], (uint32_t)a->n_hits[k], k, guide_len, s->cands().pos, (uint32_t)s->n,
                                             s->d_fam_tag, s->d_fam_family, s->d_fam_counts, s->d_fam_sum, s->d_fam_cover, s->max_mm,
                                             s->d_fjoin_counts[k], s->d_fjoin_sum[k], s->d_fjoin_cover[k], s->d_fjoin_family[k]));
    CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->ms_fam_join += elapsed(s->ev[0], s->ev[1]);
    s->fam_have_join = true;
    s->fjoin_rows[0] = a->n_hits[0];
    s->fjoin_rows[1] = a->n_hits[1];
    for (int k = 0; k < 2; ++k) {
        const uint64_t n = a->n_hits[k];
        if (!n) continue;
        int rc = CRP_OK;
        if (counts[k]) rc = crp::staged_d2h(ctx, counts[k], s->d_fjoin_counts[k], n * stride * sizeof(uint32_t));
        if (rc == CRP_OK && sum[k]) rc = crp::staged_d2h(ctx, sum[k], s->d_fjoin_sum[k], n * sizeof(uint64_t));
        if (rc == CRP_OK && cover[k]) rc = crp::staged_d2h(ctx, cover[k], s->d_fjoin_cover[k], n * sizeof(uint64_t));
        if (rc == CRP_OK && family[k]) rc = crp::staged_d2h(ctx, family[k], s->d_fjoin_family[k], n * sizeof(uint32_t));
        if (rc != CRP_OK) return rc;
    }
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CRP_OK;
}

int crp_search_self_family_stats(const crp_search_self *s, double *out, int n)
{
    if (!s || (n && !out) || n < 0 || n > 6) return CRP_ERR_INVALID;
    const double v[6] = {s->ms_fam_assign, s->ms_fam_compare, (double)s->fam_pairs, (double)s->fam_launches, (double)s->fam_bytes, s->ms_fam_join};
    for (int k = 0; k < n; ++k) out[k] = v[k];
    return CRP_OK;
}

}  // extern "C"
