// crp_search.cpp -- host side of the off-target search of given guides (include/cropsr_hip.h crp_search_*; kernels in
// crp_search.hip).
//
// create   validates the pattern, counts the candidates of every workgroup of the arena (one launch) and plans the
//          chunks: consecutive workgroups whose candidates fit the budget.
// run      per chunk: extraction (skipped when the one chunk of the plan is still in HBM from an earlier run), then the
//          compare in query batches of at most Kind::pairs_per_launch() pairs and kBatchQueries queries per launch.  The
//          site list is copied back and sorted by (query, arena position, strand): the atomics' order never reaches the
//          caller.  crp_search_run and crp_search_run_bulge are the same run of different kinds: plain, or a DNA or RNA
//          bulge on a handle whose pattern is the window pattern of that bulge (Bulges).  The kind
//          picks the compare kernel, the pairs per launch, the query limit and the site word and sort-key layout.
//          crp_search_run_scored is the plain kind with the scoring compare: per-query sums of hit values under the
//          handle's scheme (crp_search_set_scheme; DESIGN section 15, Specificity score), zeroed with the counts at the
//          start of every pass, so a repeated pass does not add a hit twice.  With a pair table instead of a scheme
//          (crp_search_set_pair_scheme; DESIGN section 15, Pair tables) the same call runs search_pair_compare_kernel.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "crp_internal.h"
#include "crp_search.h"

namespace {

constexpr uint64_t kCandBytes = 16;                   // hi, lo, nb, pos
constexpr uint64_t kPairsPerLaunch = 1ull << 36;      // ~7e10 pairs: a few ms at the issue floor, ~10-20 ms as measured
constexpr uint64_t kBatchQueries = 4096;              // and at most this many queries, i.e. loop trips per lane, when candidates are few
constexpr uint64_t kMinChunk = crp::SEARCH_WORDS * 64 * 2;  // one workgroup's most candidates (all-N pattern)
constexpr uint64_t kMaxChunk = 1ull << 31;            // chunk-relative offsets are 32-bit
constexpr uint64_t kSiteStart = 1ull << 20;           // device site slots of a first run (grows to what a run needs)
constexpr uint64_t kMaxQueries = 1ull << 28;          // query index << 4 | mismatches in 32 bits
constexpr uint64_t kBulgePairsPerLaunch = 1ull << 35;  // the bulge compare costs about twice the VALU per pair
constexpr uint64_t kMaxBulgeQueries = 1ull << 23;     // query index << 9 | placement << 4 | mismatches in 32 bits

// base set of an IUPAC letter (bit = code: A=0 T=1 C=2 G=3), 0 = not a letter of the pattern alphabet
uint32_t iupac_set(char c)
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

// The kind of a run: plain (dna = rna = 0) or a DNA or an RNA bulge of that size.  It decides the compare kernel, the
// pairs per launch, the query limit and the layout of the site word and the sort key: a bulge kind carries the bulge's
// placement (at_bits() bits) between the strand and the mismatches.
struct Kind {
    int dna = 0, rna = 0;
    enum Value { NONE, SCHEME, PAIR } value = NONE;  // (plain kind only) what the compare sums per query, and under which table
    bool bulge() const { return dna || rna; }
    bool scored() const { return value != NONE; }
    int at_bits() const { return bulge() ? 5 : 0; }
    uint64_t pairs_per_launch() const { return bulge() ? kBulgePairsPerLaunch : kPairsPerLaunch; }
    uint64_t max_queries() const { return bulge() ? kMaxBulgeQueries : kMaxQueries; }
};

// One site: the kernels' site word is {query << (4 + at_bits) | placement << 4 | mismatches, strand << 31 | pos}; the
// sort key packs query, arena position, strand, bulge_at and mismatches from the top bit down (36 + at_bits bits below
// the query), so that sorted keys order the sites by query, position and strand.
struct Site {
    uint64_t query, pos, strand, at, mm;
};

uint64_t pack_key(const Site &x, Kind k)
{
    const int b = k.at_bits();
    return x.query << (36 + b) | x.pos << (5 + b) | x.strand << (4 + b) | x.at << 4 | x.mm;
}

Site unpack_key(uint64_t key, Kind k)
{
    const int b = k.at_bits();
    return Site{key >> (36 + b), (key >> (5 + b)) & 0x7fffffffu, (key >> (4 + b)) & 1, (key >> 4) & ((1u << b) - 1), key & 15};
}

}  // namespace

namespace crp {

namespace {

bool in_unit(double v) { return std::isfinite(v) && v >= 0.0 && v <= 1.0; }

// a laid-out table to the device, allocated on first use
int upload(crp_ctx *ctx, double **d, const double *tab, size_t bytes)
{
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    if (!*d) CRP_HIP(ctx, hipMalloc(reinterpret_cast<void **>(d), bytes));
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (no run of this handle's stream is in flight, but say so)
    CRP_HIP(ctx, hipMemcpy(*d, tab, bytes, hipMemcpyHostToDevice));
    return CRP_OK;
}

uint32_t factor_region(int T, int n_factor, bool pam3)
{
    const uint32_t low = n_factor == 32 ? ~0u : (1u << n_factor) - 1u;
    return pam3 ? low : low << (T - n_factor);
}

}  // namespace

bool search_scheme_layout(int T, const double *factor, int n_factor, bool pam3, const double *shape, double *tab)
{
    if (!shape || n_factor < 1 || n_factor > T) return false;
    if (!std::all_of(factor, factor + n_factor, in_unit) || !std::all_of(shape, shape + CRP_SEARCH_SHAPE_DOUBLES, in_unit)) return false;
    std::fill(tab, tab + SEARCH_SCORE_WALK, 1.0);
    for (int g = 0; g < n_factor; ++g) tab[pam3 ? g : g + 32 - T] = factor[g];
    std::copy(shape, shape + CRP_SEARCH_SHAPE_DOUBLES, tab + SEARCH_SCORE_WALK);
    return true;
}

int SearchValueState::set_scheme(crp_ctx *ctx, int T, const double *factor, int n_factor, bool pam3, const double *shape)
{
    double tab[SEARCH_SCORE_TAB];
    if (!search_scheme_layout(T, factor, n_factor, pam3, shape, tab)) return CRP_ERR_INVALID;
    const int rc = upload(ctx, &d_scheme, tab, sizeof(tab));
    if (rc != CRP_OK) return rc;
    region = factor_region(T, n_factor, pam3);
    rev = pam3 ? 0 : 1;
    have_scheme = true;
    have_pair = false;
    return CRP_OK;
}

int SearchValueState::set_pair(crp_ctx *ctx, const SearchSets &sets, const double *pair, int n_factor, bool pam3, const int *pam_offsets,
                               int n_pam_offsets, const double *pam)
{
    double tab[SEARCH_PAIR_TAB];
    uint32_t pos = 0;
    if (!search_pair_layout(sets, pair, n_factor, pam3, pam_offsets, n_pam_offsets, pam, tab, &pos)) return CRP_ERR_INVALID;
    const int rc = upload(ctx, &d_pair, tab, sizeof(tab));
    if (rc != CRP_OK) return rc;
    region = factor_region(sets.T, n_factor, pam3);
    rev = pam3 ? 0 : 1;
    n_pam = n_pam_offsets;
    pam_pos = pos;
    have_pair = true;
    have_scheme = false;
    return CRP_OK;
}

void SearchValueState::free()
{
    (void)hipFree(d_scheme);
    (void)hipFree(d_pair);
    d_scheme = d_pair = nullptr;
    clear();
}

bool search_pair_layout(const SearchSets &sets, const double *pair, int n_factor, bool pam3, const int *pam_offsets, int n_pam_offsets,
                        const double *pam, double *tab, uint32_t *pam_pos)
{
    const int T = sets.T;
    if (!pair || n_factor < 1 || n_factor > T || n_pam_offsets < 0 || n_pam_offsets > SEARCH_PAIR_MAX_PAM) return false;
    if (n_pam_offsets && (!pam_offsets || !pam)) return false;
    const int P = T - n_factor, glo = pam3 ? 0 : P;
    const auto set_at = [&](int o) { return (uint32_t)(sets.plus[o >> 4] >> ((o & 15) * 4)) & 15u; };
    for (int p = glo; p < glo + n_factor; ++p)
        if (set_at(p) != 15u) return false;
    static const int dev[4] = {0, 2, 3, 1};  // A, C, G, T in the planes' coding (A=00 T=01 C=10 G=11)
    std::fill(tab, tab + SEARCH_PAIR_WALK * 16, 1.0);
    std::fill(tab + SEARCH_PAIR_WALK * 16, tab + SEARCH_PAIR_TAB, 0.0);
    // the walk order of search_scheme_layout: bit g of the mask (PAM on the 3' side), bit g + 32 - T of the reversed mask
    for (int g = 0; g < n_factor; ++g)
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) {
                if (a == b) continue;
                const double v = pair[(g * 4 + a) * 4 + b];
                if (!in_unit(v)) return false;
                tab[(pam3 ? g : g + 32 - T) * 16 + (dev[a] << 2 | dev[b])] = v;
            }
    *pam_pos = 0;
    for (int k = 0; k < n_pam_offsets; ++k) {
        const int off = pam_offsets[k];
        if (off < 0 || off >= P || (k && off <= pam_offsets[k - 1])) return false;
        const int p = pam3 ? n_factor + off : off;
        if (set_at(p) == 15u) return false;  // an N of the pattern: the site may hold a non-base there
        *pam_pos |= (uint32_t)p << (8 * k);
    }
    const int n_pam = 1 << (2 * n_pam_offsets);
    for (int i = 0; i < n_pam; ++i) {
        if (!n_pam_offsets) {
            tab[SEARCH_PAIR_WALK * 16] = 1.0;
            break;
        }
        if (!in_unit(pam[i])) return false;
        int at = 0;
        for (int k = 0; k < n_pam_offsets; ++k) at = at << 2 | dev[(i >> (2 * (n_pam_offsets - 1 - k))) & 3];
        tab[SEARCH_PAIR_WALK * 16 + at] = pam[i];
    }
    return true;
}

}  // namespace crp

struct crp_search {
    crp_arena *arena = nullptr;
    crp_ctx *ctx = nullptr;
    crp::SearchSets sets = {};
    uint64_t n_plus = 0, n_minus = 0;
    std::vector<uint2> block_cnt;  // per extraction workgroup: {'+', '-'} candidates
    uint64_t budget = CRP_SEARCH_DEFAULT_BUDGET;
    uint64_t batch_queries = kBatchQueries;  // crp_search_set_limits
    uint64_t site_start = kSiteStart;
    // plan: chunk c covers workgroups [chunk_first[c], chunk_first[c + 1]) with chunk_n[c] candidates
    std::vector<uint32_t> chunk_first;
    std::vector<uint64_t> chunk_n;
    bool planned = false;
    uint32_t *d_block_off = nullptr;  // per workgroup: first candidate, relative to its chunk
    uint64_t block_off_cap = 0;
    uint32_t *d_cand = nullptr;  // 4 x cand_cap uint32 (SoA)
    uint64_t cand_cap = 0;
    int cached_chunk = -1;  // the chunk whose candidates d_cand holds
    // run
    uint4 *d_queries = nullptr;
    uint64_t q_cap = 0;
    uint32_t *d_counts = nullptr;
    uint64_t counts_cap = 0;
    uint2 *d_sites = nullptr;
    uint64_t sites_cap = 0;
    unsigned long long *d_ctr = nullptr;
    crp::SearchValueState value;  // crp_search_set_scheme / crp_search_set_pair_scheme
    unsigned long long *d_hit_sum = nullptr;
    uint64_t hit_sum_cap = 0;
    std::vector<uint64_t> keys;  // sites of the last successful run, as pack_key of its kind
    bool have_sites = false;
    Kind keys_kind;              // the kind of the last run
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    double ms_extract = 0, ms_compare = 0;
    uint64_t n_extract = 0, n_compare = 0;

    crp::SearchCands cands() const
    {
        return crp::SearchCands{d_cand, d_cand + cand_cap, d_cand + 2 * cand_cap, d_cand + 3 * cand_cap};
    }
};

namespace {

double elapsed(hipEvent_t a, hipEvent_t b)
{
    float ms = 0.f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.0;
}

int plan(crp_search *s)
{
    crp_ctx *ctx = s->ctx;
    const uint64_t cap = std::min(kMaxChunk, std::max(kMinChunk, s->budget / kCandBytes));
    const uint32_t n_blocks = (uint32_t)s->block_cnt.size();
    std::vector<uint32_t> off(n_blocks);
    s->chunk_first.assign(1, 0);
    s->chunk_n.clear();
    uint64_t cur = 0, biggest = 0;
    for (uint32_t b = 0; b < n_blocks; ++b) {
        const uint64_t n = (uint64_t)s->block_cnt[b].x + s->block_cnt[b].y;
        if (cur + n > cap) {
            s->chunk_first.push_back(b);
            s->chunk_n.push_back(cur);
            biggest = std::max(biggest, cur);
            cur = 0;
        }
        off[b] = (uint32_t)cur;
        cur += n;
    }
    s->chunk_first.push_back(n_blocks);
    s->chunk_n.push_back(cur);
    biggest = std::max(biggest, cur);
    if (n_blocks) {
        int rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_block_off), &s->block_off_cap, n_blocks, sizeof(uint32_t));
        if (rc != CRP_OK) return rc;
        CRP_HIP(ctx, hipMemcpy(s->d_block_off, off.data(), n_blocks * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    // the candidate buffer holds the biggest chunk, exactly (not grow(): its slack would leave the budget)
    if (s->cand_cap < biggest || s->cand_cap > std::max<uint64_t>(biggest, 1) * 2) {
        (void)hipFree(s->d_cand);
        s->d_cand = nullptr;
        s->cand_cap = 0;
        if (biggest) {
            CRP_HIP(ctx, hipMalloc(reinterpret_cast<void **>(&s->d_cand), biggest * kCandBytes));
            s->cand_cap = biggest;
        }
    }
    s->cached_chunk = -1;
    s->planned = true;
    return CRP_OK;
}

// the compare kernel of `kind` over the cached chunk's n candidates and queries [q0, q0 + nq)
hipError_t compare(crp_search *s, Kind kind, uint32_t n, uint32_t q0, uint32_t nq, int max_mm, uint64_t site_cap)
{
    const hipStream_t st = s->ctx->stream;
    const crp::SearchCands c = s->cands();
    if (kind.value == Kind::PAIR)
        return crp::launch_search_pair_compare(st, c, n, s->d_queries, q0, nq, max_mm, s->d_counts, s->d_sites, site_cap, s->d_ctr,
                                               s->value.pair(s->d_hit_sum));
    if (kind.value == Kind::SCHEME)
        return crp::launch_search_score_compare(st, c, n, s->d_queries, q0, nq, max_mm, s->d_counts, s->d_sites, site_cap, s->d_ctr,
                                                s->value.score(s->d_hit_sum));
    if (kind.bulge())
        return crp::launch_search_bulge_compare(st, c, n, s->d_queries, q0, nq, max_mm, kind.dna, kind.rna, s->d_counts, s->d_sites, site_cap,
                                                s->d_ctr);
    return crp::launch_search_compare(st, c, n, s->d_queries, q0, nq, max_mm, s->d_counts, s->d_sites, site_cap, s->d_ctr);
}

// one pass over every chunk with the compare kernel of `kind`: counts and sites accumulate on the device
int run_pass(crp_search *s, uint32_t n_queries, int max_mm, uint64_t dev_sites, Kind kind)
{
    crp_ctx *ctx = s->ctx;
    crp_arena *a = s->arena;
    const crp::Planes pl{{a->d_plane[0], a->d_plane[1], a->d_plane[2], a->d_plane[3]}};
    CRP_HIP(ctx, hipMemsetAsync(s->d_counts, 0, (size_t)n_queries * (max_mm + 1) * sizeof(uint32_t), ctx->stream));
    CRP_HIP(ctx, hipMemsetAsync(s->d_ctr, 0, sizeof(unsigned long long), ctx->stream));
    if (kind.scored()) CRP_HIP(ctx, hipMemsetAsync(s->d_hit_sum, 0, (size_t)n_queries * sizeof(unsigned long long), ctx->stream));
    const int n_chunks = (int)s->chunk_n.size();
    for (int c = 0; c < n_chunks; ++c) {
        const uint64_t n = s->chunk_n[c];
        if (!n) continue;
        const bool extract = s->cached_chunk != c;
        CRP_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
        if (extract) {
            s->cached_chunk = -1;
            CRP_HIP(ctx, crp::launch_search_emit(ctx->stream, pl, a->used_words, s->sets, s->chunk_first[c],
                                                 s->chunk_first[c + 1] - s->chunk_first[c], s->d_block_off, s->cands()));
        }
        CRP_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
        const uint64_t pairs = kind.pairs_per_launch();
        const uint32_t batch = (uint32_t)std::max<uint64_t>(1, std::min({(uint64_t)n_queries, pairs / n, s->batch_queries}));
        uint64_t launches = 0;
        for (uint32_t q0 = 0; q0 < n_queries; q0 += batch) {
            const uint32_t nq = std::min(batch, n_queries - q0);
            CRP_HIP(ctx, compare(s, kind, (uint32_t)n, q0, nq, max_mm, dev_sites));
            ++launches;
        }
        CRP_HIP(ctx, hipEventRecord(s->ev[2], ctx->stream));
        CRP_HIP(ctx, hipEventSynchronize(s->ev[2]));
        if (extract) {
            s->cached_chunk = c;
            s->ms_extract += elapsed(s->ev[0], s->ev[1]);
            s->n_extract += 1;
        }
        s->ms_compare += elapsed(s->ev[1], s->ev[2]);
        s->n_compare += launches;
    }
    return CRP_OK;
}

}  // namespace

extern "C" {

int crp_search_create(crp_arena *a, const char *pattern, int T, crp_search **out)
{
    if (!a || !pattern || !out) return CRP_ERR_INVALID;
    *out = nullptr;
    if (T < 1 || T > CRP_SEARCH_MAX_T) return CRP_ERR_UNSUPPORTED;
    crp::SearchSets sets = {};
    sets.T = T;
    for (int o = 0; o < T; ++o) {
        const uint32_t sp = iupac_set(pattern[o]), sm = iupac_set(pattern[T - 1 - o]);
        if (!sp || !sm) return CRP_ERR_INVALID;
        sets.plus[o >> 4] |= (uint64_t)sp << ((o & 15) * 4);
        sets.minus[o >> 4] |= (uint64_t)complement_set(sm) << ((o & 15) * 4);
    }
    if (!a->sealed) return CRP_ERR_STATE;
    crp_ctx *ctx = a->ctx;
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    crp_search *s = new (std::nothrow) crp_search;
    if (!s) return CRP_ERR_NOMEM;
    s->arena = a;
    s->ctx = ctx;
    s->sets = sets;
    int rc = CRP_OK;
    for (int k = 0; k < 3 && rc == CRP_OK; ++k)
        if (hipEventCreate(&s->ev[k]) != hipSuccess) rc = CRP_ERR_HIP;
    const uint64_t n_blocks = (a->used_words + crp::SEARCH_WORDS - 1) / crp::SEARCH_WORDS;
    uint2 *d_cnt = nullptr;
    if (rc == CRP_OK && n_blocks) {
        s->block_cnt.resize(n_blocks);
        const crp::Planes pl{{a->d_plane[0], a->d_plane[1], a->d_plane[2], a->d_plane[3]}};
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&d_cnt), n_blocks * sizeof(uint2));
        if (e == hipSuccess) e = hipEventRecord(s->ev[0], ctx->stream);
        if (e == hipSuccess) e = crp::launch_search_count(ctx->stream, pl, a->used_words, sets, d_cnt);
        if (e == hipSuccess) e = hipEventRecord(s->ev[1], ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(s->block_cnt.data(), d_cnt, n_blocks * sizeof(uint2), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            ctx->last_error = std::string("crp_search_create: ") + hipGetErrorString(e);
            rc = e == hipErrorOutOfMemory ? CRP_ERR_NOMEM : CRP_ERR_HIP;
        } else {
            s->ms_extract += elapsed(s->ev[0], s->ev[1]);
            s->n_extract += 1;
        }
        (void)hipFree(d_cnt);
    }
    for (const uint2 &c : s->block_cnt) {
        s->n_plus += c.x;
        s->n_minus += c.y;
    }
    if (rc != CRP_OK) {
        crp_search_destroy(s);
        return rc;
    }
    *out = s;
    return CRP_OK;
}

int crp_search_destroy(crp_search *s)
{
    if (!s) return CRP_ERR_INVALID;
    (void)hipSetDevice(s->ctx->device);
    (void)hipFree(s->d_block_off);
    (void)hipFree(s->d_cand);
    (void)hipFree(s->d_queries);
    (void)hipFree(s->d_counts);
    (void)hipFree(s->d_sites);
    (void)hipFree(s->d_ctr);
    s->value.free();
    (void)hipFree(s->d_hit_sum);
    for (hipEvent_t e : s->ev)
        if (e) (void)hipEventDestroy(e);
    delete s;
    return CRP_OK;
}

int crp_search_set_budget(crp_search *s, uint64_t bytes)
{
    if (!s) return CRP_ERR_INVALID;
    s->budget = bytes ? bytes : CRP_SEARCH_DEFAULT_BUDGET;
    s->planned = false;
    return CRP_OK;
}

int crp_search_set_limits(crp_search *s, uint64_t batch_queries, uint64_t first_site_slots)
{
    if (!s) return CRP_ERR_INVALID;
    s->batch_queries = batch_queries ? batch_queries : kBatchQueries;
    s->site_start = first_site_slots ? first_site_slots : kSiteStart;
    return CRP_OK;
}

int crp_search_set_scheme(crp_search *s, const double *factor, int n_factor, int pam_side, const double *shape)
{
    if (!s) return CRP_ERR_INVALID;
    if (!factor) {
        s->value.clear();
        return CRP_OK;
    }
    if (pam_side != CRP_SEARCH_PAM_3PRIME && pam_side != CRP_SEARCH_PAM_5PRIME) return CRP_ERR_INVALID;
    return s->value.set_scheme(s->ctx, s->sets.T, factor, n_factor, pam_side == CRP_SEARCH_PAM_3PRIME, shape);
}

int crp_search_set_pair_scheme(crp_search *s, const double *pair, int n_factor, int pam_side, const int *pam_offsets, int n_pam_offsets,
                               const double *pam)
{
    if (!s) return CRP_ERR_INVALID;
    if (!pair) {
        s->value.clear();
        return CRP_OK;
    }
    if (pam_side != CRP_SEARCH_PAM_3PRIME && pam_side != CRP_SEARCH_PAM_5PRIME) return CRP_ERR_INVALID;
    return s->value.set_pair(s->ctx, s->sets, pair, n_factor, pam_side == CRP_SEARCH_PAM_3PRIME, pam_offsets, n_pam_offsets, pam);
}

int crp_search_candidates(const crp_search *s, uint64_t *n_plus, uint64_t *n_minus)
{
    if (!s) return CRP_ERR_INVALID;
    if (n_plus) *n_plus = s->n_plus;
    if (n_minus) *n_minus = s->n_minus;
    return CRP_OK;
}

}  // extern "C"

namespace {

// queries (n_queries x T letters of ACGTN) -> {hi, lo, compare mask, 0} per query; false on another letter
bool encode_queries(const char *queries, uint64_t n_queries, int T, std::vector<uint4> &enc)
{
    enc.resize(n_queries);
    for (uint64_t q = 0; q < n_queries; ++q) {
        uint32_t h = 0, l = 0, m = 0;
        for (int p = 0; p < T; ++p) {
            uint32_t code;
            switch (queries[q * T + p] | 0x20) {
                case 'a': code = 0; break;
                case 't': code = 1; break;
                case 'c': code = 2; break;
                case 'g': code = 3; break;
                case 'n': continue;
                default: return false;
            }
            h |= (code >> 1) << p;
            l |= (code & 1) << p;
            m |= 1u << p;
        }
        enc[q] = make_uint4(h, l, m, 0);
    }
    return true;
}

// the capacity protocol over encoded queries of one kind; span_first: per query, what bulge_at counts from
int run_encoded(crp_search *s, const std::vector<uint4> &enc, Kind kind, const std::vector<uint8_t> &span_first, int max_mm,
                uint64_t site_cap, uint32_t *counts, uint64_t *n_sites, uint64_t *hit_sum)
{
    const uint64_t n_queries = enc.size();
    s->have_sites = false;
    s->keys.clear();
    *n_sites = 0;
    crp_ctx *ctx = s->ctx;
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = CRP_OK;
    if (!s->planned && (rc = plan(s)) != CRP_OK) return rc;
    const uint64_t n_counts = n_queries * (uint64_t)(max_mm + 1);
    if (!n_queries) {  // nothing to compare: an empty, fetchable list
        s->have_sites = true;
        return CRP_OK;
    }
    if ((rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_queries), &s->q_cap, n_queries, sizeof(uint4))) != CRP_OK) return rc;
    if ((rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_counts), &s->counts_cap, n_counts, sizeof(uint32_t))) != CRP_OK) return rc;
    if (!s->d_ctr) CRP_HIP(ctx, hipMalloc(reinterpret_cast<void **>(&s->d_ctr), sizeof(unsigned long long)));
    if (kind.scored() &&
        (rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_hit_sum), &s->hit_sum_cap, n_queries, sizeof(unsigned long long))) != CRP_OK)
        return rc;
    uint64_t dev_sites = std::min(site_cap, std::max(s->sites_cap, s->site_start));
    if (dev_sites && (rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_sites), &s->sites_cap, dev_sites, sizeof(uint2))) != CRP_OK)
        return rc;
    CRP_HIP(ctx, hipMemcpyAsync(s->d_queries, enc.data(), n_queries * sizeof(uint4), hipMemcpyHostToDevice, ctx->stream));
    unsigned long long total = 0;
    for (int pass = 0; pass < 2; ++pass) {
        if ((rc = run_pass(s, (uint32_t)n_queries, max_mm, dev_sites, kind)) != CRP_OK) return rc;
        CRP_HIP(ctx, hipMemcpy(&total, s->d_ctr, sizeof(total), hipMemcpyDeviceToHost));
        if (total <= dev_sites || total > site_cap) break;
        // more sites than the device list had room for, fewer than the caller's: once more with room for all of them
        dev_sites = total;
        if ((rc = crp::grow(ctx, reinterpret_cast<void **>(&s->d_sites), &s->sites_cap, dev_sites, sizeof(uint2))) != CRP_OK)
            return rc;
    }
    if (counts) CRP_HIP(ctx, hipMemcpy(counts, s->d_counts, n_counts * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (kind.scored()) CRP_HIP(ctx, hipMemcpy(hit_sum, s->d_hit_sum, n_queries * sizeof(uint64_t), hipMemcpyDeviceToHost));
    *n_sites = total;
    if (total > site_cap) return CRP_ERR_CAPACITY;
    std::vector<uint2> raw(total);
    if (total) CRP_HIP(ctx, hipMemcpy(raw.data(), s->d_sites, total * sizeof(uint2), hipMemcpyDeviceToHost));
    s->keys.resize(total);
    const int b = kind.at_bits();
    for (uint64_t k = 0; k < total; ++k) {
        const uint64_t q = raw[k].x >> (4 + b), at = ((raw[k].x >> 4) & ((1u << b) - 1)) - span_first[q];
        s->keys[k] = pack_key(Site{q, raw[k].y & 0x7fffffffu, raw[k].y >> 31, at, raw[k].x & 15}, kind);
    }
    std::sort(s->keys.begin(), s->keys.end());
    s->keys_kind = kind;
    s->have_sites = true;
    return CRP_OK;
}

// crp_search_run(_bulge) past the checks of its own arguments; span: per query, the first and last letter of its span
// (bulge kinds only)
int run_kind(crp_search *s, const char *queries, uint64_t n_queries, Kind kind, const uint8_t *span, int max_mm, uint64_t site_cap,
             uint32_t *counts, uint64_t *n_sites, uint64_t *hit_sum = nullptr)
{
    if (max_mm < 0 || max_mm > CRP_SEARCH_MAX_MM || n_queries >= kind.max_queries()) return CRP_ERR_UNSUPPORTED;
    const int T = s->sets.T - kind.dna + kind.rna;  // the query's length
    if (T < 1 || T > CRP_SEARCH_MAX_T) return CRP_ERR_UNSUPPORTED;
    std::vector<uint4> enc;
    if (!encode_queries(queries, n_queries, T, enc)) return CRP_ERR_INVALID;
    if (kind.scored())  // a base outside the guide region would mismatch where no factor is
        for (const uint4 &q : enc)
            if (q.z & ~s->value.region) return CRP_ERR_INVALID;
    std::vector<uint8_t> span_first(n_queries);  // (0 for a plain run: its sites have no placement)
    if (kind.bulge())
        for (uint64_t q = 0; q < n_queries; ++q) {
            const int first = span[2 * q], last = span[2 * q + 1];
            // placements: first < s <= last (DNA), first < s and s + size - 1 < last (RNA)
            const int s_min = first + 1, s_max = last - kind.rna;
            if (last >= T || s_min > s_max) return CRP_ERR_INVALID;
            enc[q].w = (uint32_t)s_min | (uint32_t)s_max << 8;
            span_first[q] = (uint8_t)first;
        }
    return run_encoded(s, enc, kind, span_first, max_mm, site_cap, counts, n_sites, hit_sum);
}

}  // namespace

extern "C" {

int crp_search_run(crp_search *s, const char *queries, uint64_t n_queries, int max_mm, uint64_t site_cap, uint32_t *counts,
                   uint64_t *n_sites)
{
    if (!s || !n_sites || (n_queries && !queries)) return CRP_ERR_INVALID;
    return run_kind(s, queries, n_queries, Kind{}, nullptr, max_mm, site_cap, counts, n_sites);
}

int crp_search_run_scored(crp_search *s, const char *queries, uint64_t n_queries, int max_mm, uint64_t site_cap, uint32_t *counts,
                          uint64_t *n_sites, uint64_t *hit_sum)
{
    if (!s || !n_sites || (n_queries && (!queries || !hit_sum))) return CRP_ERR_INVALID;
    if (!s->value.any()) return CRP_ERR_STATE;
    Kind kind;
    kind.value = s->value.have_pair ? Kind::PAIR : Kind::SCHEME;
    return run_kind(s, queries, n_queries, kind, nullptr, max_mm, site_cap, counts, n_sites, hit_sum);
}

int crp_search_run_bulge(crp_search *s, const char *queries, uint64_t n_queries, int kind, int size, const uint8_t *span, int max_mm,
                         uint64_t site_cap, uint32_t *counts, uint64_t *n_sites)
{
    if (!s || !n_sites || (n_queries && (!queries || !span))) return CRP_ERR_INVALID;
    if (kind != CRP_SEARCH_BULGE_DNA && kind != CRP_SEARCH_BULGE_RNA) return CRP_ERR_INVALID;
    if (size < 1 || size > CRP_SEARCH_MAX_BULGE) return CRP_ERR_UNSUPPORTED;
    const bool dna = kind == CRP_SEARCH_BULGE_DNA;
    return run_kind(s, queries, n_queries, Kind{dna ? size : 0, dna ? 0 : size}, span, max_mm, site_cap, counts, n_sites);
}

int crp_search_fetch(const crp_search *s, uint32_t *query, uint32_t *arena_pos, uint8_t *strand, uint8_t *mismatches, uint64_t cap)
{
    return crp_search_fetch_bulge(s, query, arena_pos, strand, mismatches, nullptr, cap);
}

int crp_search_fetch_bulge(const crp_search *s, uint32_t *query, uint32_t *arena_pos, uint8_t *strand, uint8_t *mismatches,
                           uint8_t *bulge_at, uint64_t cap)
{
    if (!s) return CRP_ERR_INVALID;
    if (!s->have_sites) return CRP_ERR_STATE;
    if (cap < s->keys.size()) return CRP_ERR_CAPACITY;
    for (uint64_t k = 0; k < s->keys.size(); ++k) {
        const Site x = unpack_key(s->keys[k], s->keys_kind);
        if (query) query[k] = (uint32_t)x.query;
        if (arena_pos) arena_pos[k] = (uint32_t)x.pos;
        if (strand) strand[k] = (uint8_t)x.strand;
        if (mismatches) mismatches[k] = (uint8_t)x.mm;
        if (bulge_at) bulge_at[k] = (uint8_t)x.at;
    }
    return CRP_OK;
}

int crp_search_stats(const crp_search *s, double *out, int n)
{
    if (!s || (n && !out) || n < 0 || n > 6) return CRP_ERR_INVALID;
    const double v[6] = {s->ms_extract, s->ms_compare, (double)s->n_extract, (double)s->n_compare,
                         s->planned ? (double)s->chunk_n.size() : 0.0, (double)(s->cand_cap * kCandBytes)};
    for (int k = 0; k < n; ++k) out[k] = v[k];
    return CRP_OK;
}

}  // extern "C"
