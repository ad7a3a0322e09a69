// crp_variants.hip -- variant counts of every kept hit (include/cropsr_hip.h states the definition,
// tests/variant_reference.py restates it twice).  Not in the reference, opt-in.
//
// The arena's variant track is two ascending uint32 arrays of one length: starts (every s') and ends1 (every e' + 1), the
// closed intervals [s', e'] of arena positions a cultivar's alleles replace (e' >= s' - 1: an insertion is empty).  The
// variants that touch a closed window [a, b] are #(starts <= b) - #(ends1 <= a): a difference of two RANKS.  Per row four
// windows -- site, guide, seed, pam -- share their ends, so five ranks make all four counts:
//
//   '+' row, match index i     starts <= {i - 1, i + 2}              ends1 <= {i - l, i - S, i + 1}
//   '-' row, match index j     starts <= {j + 1, j + 2 + S, j + 2 + l}   ends1 <= {j, j + 3}
//
// A rank is read the way the annotation join reads its track (crp_annotate.hip): a bucket index per array (entry b: the
// values below b << 11; built on the GPU when the track is set), two neighbouring entries of it, and a binary search over
// the values inside the bucket -- correct for any fill, a dense population VCF's thousands included.  The queries of one
// row lie within 53 positions of each other and ascend, so a later search of the same array starts from the earlier
// rank.  One lane per four rows, both tables in one launch (annot_lookup_kernel's scheme): 16-byte non-temporal loads of
// the positions, 16-byte non-temporal stores of the packed words; the track and its indices stay in the caches.  No
// atomics, no LDS, no scratch.  4 B in and 4 B out per row of table traffic; bound: the dependent loads of the searches.
#include <algorithm>

#include "crp_internal.h"
#include "crp_roctx.h"

namespace crp {

constexpr int VAR_SHIFT = 11;  // one bucket = 2 048 arena positions (crp_annotate.hip's ANN_SHIFT)
constexpr int VAR_ROWS = 4;    // table rows per lane
constexpr int VAR_MAX_GUIDE = 50;
typedef uint32_t var_u32x4 __attribute__((ext_vector_type(4)));

// bucket[b] = number of values below b << VAR_SHIFT; the last entry is n whatever the values are, so that the last
// bucket takes every query at or beyond its start
__global__ __launch_bounds__(BLOCK) void variant_bucket_kernel(const uint32_t *__restrict__ starts, const uint32_t *__restrict__ ends1,
                                                               uint32_t n, uint32_t *__restrict__ bucket_s, uint32_t *__restrict__ bucket_e,
                                                               uint32_t n_entries)
{
    const uint32_t b = blockIdx.x * BLOCK + threadIdx.x;
    if (b >= n_entries) return;
    const uint64_t key = (uint64_t)b << VAR_SHIFT;
    for (int which = 0; which < 2; ++which) {
        const uint32_t *__restrict__ v = which ? ends1 : starts;
        uint32_t lo = 0, hi = n;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (v[mid] < key) lo = mid + 1;
            else hi = mid;
        }
        (which ? bucket_e : bucket_s)[b] = b + 1 == n_entries ? n : lo;
    }
}

struct VarTrack {
    const uint32_t *starts, *ends1;
    const uint32_t *bucket_s, *bucket_e;
    uint32_t last_bucket;
};

// #(v <= q), not below `from` (a rank of the same array at a query <= q)
__device__ __forceinline__ uint32_t var_rank(const uint32_t *__restrict__ v, const uint32_t *__restrict__ bucket, uint32_t last_bucket,
                                             uint32_t q, uint32_t from)
{
    const uint32_t b = min(q >> VAR_SHIFT, last_bucket);
    uint32_t lo = max(bucket[b], from), hi = bucket[b + 1];
    while (lo < hi) {  // v[lo..hi) lie inside the bucket: how many of them are <= q
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (v[mid] <= q) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint32_t var_pack(uint32_t site, uint32_t guide, uint32_t seed, uint32_t pam)
{
    return min(site, 255u) | min(guide, 255u) << 8 | min(seed, 255u) << 16 | min(pam, 255u) << 24;
}

__device__ __forceinline__ uint32_t var_plus(uint32_t i, uint32_t l, uint32_t S, const VarTrack &t)
{
    // (the scan keeps i - l >= 5; a position below l is treated as 0 and not as a wrapped one)
    const uint32_t a_site = i >= l ? i - l : 0u, a_seed = i >= S ? i - S : 0u;
    const uint32_t s_guide = var_rank(t.starts, t.bucket_s, t.last_bucket, i - (i ? 1u : 0u), 0u);  // starts <= i - 1
    const uint32_t s_site = var_rank(t.starts, t.bucket_s, t.last_bucket, i + 2u, s_guide);         // starts <= i + 2
    const uint32_t e_site = var_rank(t.ends1, t.bucket_e, t.last_bucket, a_site, 0u);               // ends1 <= i - l
    const uint32_t e_seed = var_rank(t.ends1, t.bucket_e, t.last_bucket, a_seed, e_site);           // ends1 <= i - S
    const uint32_t e_pam = var_rank(t.ends1, t.bucket_e, t.last_bucket, i + 1u, e_seed);            // ends1 <= i + 1
    return var_pack(s_site - e_site, s_guide - e_site, s_guide - e_seed, s_site - e_pam);
}

__device__ __forceinline__ uint32_t var_minus(uint32_t j, uint32_t l, uint32_t S, const VarTrack &t)
{
    const uint32_t s_pam = var_rank(t.starts, t.bucket_s, t.last_bucket, j + 1u, 0u);            // starts <= j + 1
    const uint32_t s_seed = var_rank(t.starts, t.bucket_s, t.last_bucket, j + 2u + S, s_pam);    // starts <= j + 2 + S
    const uint32_t s_site = var_rank(t.starts, t.bucket_s, t.last_bucket, j + 2u + l, s_seed);   // starts <= j + 2 + l
    const uint32_t e_site = var_rank(t.ends1, t.bucket_e, t.last_bucket, j, 0u);                 // ends1 <= j
    const uint32_t e_guide = var_rank(t.ends1, t.bucket_e, t.last_bucket, j + 3u, e_site);       // ends1 <= j + 3
    return var_pack(s_site - e_site, s_site - e_guide, s_seed - e_guide, s_pam - e_site);
}

struct VarTable {
    const uint32_t *pos;
    uint32_t *out;
    uint64_t n;
};

// One launch for both tables: the first blocks_plus workgroups walk the '+' table, the others the '-' table.
__global__ __launch_bounds__(BLOCK) void variant_counts_kernel(VarTable plus, VarTable minus, uint32_t blocks_plus, VarTrack track, uint32_t l,
                                                               uint32_t S)
{
    const bool is_minus = blockIdx.x >= blocks_plus;  // (uniform per workgroup)
    const VarTable t = is_minus ? minus : plus;
    const uint64_t first = ((uint64_t)(blockIdx.x - (is_minus ? blocks_plus : 0u)) * BLOCK + threadIdx.x) * VAR_ROWS;
    if (first >= t.n) return;
    if (first + VAR_ROWS <= t.n) {
        // the tables are read once and the column written once: keep them out of the way of the track and its indices
        const var_u32x4 p = __builtin_nontemporal_load(reinterpret_cast<const var_u32x4 *>(t.pos + first));
        var_u32x4 c;
        if (is_minus) {
            c.x = var_minus(p.x, l, S, track);
            c.y = var_minus(p.y, l, S, track);
            c.z = var_minus(p.z, l, S, track);
            c.w = var_minus(p.w, l, S, track);
        } else {
            c.x = var_plus(p.x, l, S, track);
            c.y = var_plus(p.y, l, S, track);
            c.z = var_plus(p.z, l, S, track);
            c.w = var_plus(p.w, l, S, track);
        }
        __builtin_nontemporal_store(c, reinterpret_cast<var_u32x4 *>(t.out + first));
    } else {
        for (uint64_t r = first; r < t.n; ++r) t.out[r] = is_minus ? var_minus(t.pos[r], l, S, track) : var_plus(t.pos[r], l, S, track);
    }
}

}  // namespace crp

extern "C" {

int crp_variant_set_track(crp_arena *a, const uint32_t *starts, const uint32_t *ends1, uint64_t n)
{
    crp::Range roctx_range("crp: variant track");
    if (!a || (n && (!starts || !ends1)) || n > 0x7fffffffull) return CRP_ERR_INVALID;
    if (!a->sealed) return CRP_ERR_STATE;
    crp_ctx *ctx = a->ctx;
    for (uint64_t k = 0; k < n; ++k)
        if (starts[k] > 0x7fffffffu || ends1[k] > 0x7fffffffu || (k && (starts[k] < starts[k - 1] || ends1[k] < ends1[k - 1]))) {
            ctx->last_error = "crp_variant_set_track: starts and ends1 are each ascending and below 2^31; element " + std::to_string(k) + " is not";
            return CRP_ERR_INVALID;
        }
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    a->have_var_track = false;
    a->have_variants = false;
    uint64_t cap_s = a->var_cap, cap_e = a->var_cap;
    int rc = crp::grow(ctx, reinterpret_cast<void **>(&a->d_var_starts), &cap_s, n, sizeof(uint32_t));
    if (rc == CRP_OK) rc = crp::grow(ctx, reinterpret_cast<void **>(&a->d_var_ends1), &cap_e, n, sizeof(uint32_t));
    if (rc != CRP_OK) {
        a->var_cap = 0;
        return rc;
    }
    a->var_cap = std::min(cap_s, cap_e);
    // one entry per bucket of the arena's positions, plus the end of the last bucket
    const uint64_t n_entries = ((a->padded_words * 64) >> crp::VAR_SHIFT) + 2;
    for (int s = 0; s < 2; ++s) {
        rc = crp::grow(ctx, reinterpret_cast<void **>(&a->d_var_bucket[s]), &a->var_bucket_cap[s], n_entries, sizeof(uint32_t));
        if (rc != CRP_OK) return rc;
    }
    if (n) {
        rc = crp::staged_h2d(ctx, a->d_var_starts, starts, n * sizeof(uint32_t));
        if (rc == CRP_OK) rc = crp::staged_h2d(ctx, a->d_var_ends1, ends1, n * sizeof(uint32_t));
        if (rc != CRP_OK) return rc;
    }
    hipLaunchKernelGGL(crp::variant_bucket_kernel, dim3((uint32_t)((n_entries + crp::BLOCK - 1) / crp::BLOCK)), dim3(crp::BLOCK), 0, ctx->stream,
                       a->d_var_starts, a->d_var_ends1, (uint32_t)n, a->d_var_bucket[0], a->d_var_bucket[1], (uint32_t)n_entries);
    CRP_HIP(ctx, hipGetLastError());
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    a->n_var = n;
    a->n_var_entries = n_entries;
    a->have_var_track = true;
    return CRP_OK;
}

int crp_variant_counts(crp_arena *a, int seed_len, uint32_t *plus, uint32_t *minus)
{
    crp::Range roctx_range("crp: variant counts");
    if (!a) return CRP_ERR_INVALID;
    crp_ctx *ctx = a->ctx;
    if (!a->have_hits) {
        ctx->last_error = "crp_variant_counts: the arena has no hit tables (crp_scan_score)";
        return CRP_ERR_STATE;
    }
    const int l = a->pend_guide_len;
    if (l < 1 || l > crp::VAR_MAX_GUIDE) {
        ctx->last_error = "crp_variant_counts: the tables were scanned at guide length " + std::to_string(l) + ": a guide of 1.." +
                          std::to_string(crp::VAR_MAX_GUIDE) + " letters has windows";
        return CRP_ERR_INVALID;
    }
    if (seed_len < 1 || seed_len > l) {
        ctx->last_error = "crp_variant_counts: the seed is 1.." + std::to_string(l) + " letters of the guide, not " + std::to_string(seed_len);
        return CRP_ERR_INVALID;
    }
    if (!a->have_var_track) {
        ctx->last_error = "crp_variant_counts: the arena has no variant track (crp_variant_set_track)";
        return CRP_ERR_STATE;
    }
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    a->have_variants = false;
    for (int s = 0; s < 2; ++s) {
        const int rc = crp::grow(ctx, reinterpret_cast<void **>(&a->d_variants[s]), &a->variants_cap[s], a->n_hits[s], sizeof(uint32_t));
        if (rc != CRP_OK) return rc;
    }
    for (hipEvent_t &e : a->ev_variants)
        if (!e) CRP_HIP(ctx, hipEventCreate(&e));
    const uint64_t per_block = (uint64_t)crp::BLOCK * crp::VAR_ROWS;
    const uint32_t bp = (uint32_t)((a->n_hits[0] + per_block - 1) / per_block), bm = (uint32_t)((a->n_hits[1] + per_block - 1) / per_block);
    const crp::VarTable tp{a->d_pos[0], a->d_variants[0], a->n_hits[0]};
    const crp::VarTable tm{a->d_pos[1], a->d_variants[1], a->n_hits[1]};
    const crp::VarTrack track{a->d_var_starts, a->d_var_ends1, a->d_var_bucket[0], a->d_var_bucket[1], (uint32_t)(a->n_var_entries - 2)};
    CRP_HIP(ctx, hipEventRecord(a->ev_variants[0], ctx->stream));
    if (bp + bm)
        hipLaunchKernelGGL(crp::variant_counts_kernel, dim3(bp + bm), dim3(crp::BLOCK), 0, ctx->stream, tp, tm, bp, track, (uint32_t)l,
                           (uint32_t)seed_len);
    CRP_HIP(ctx, hipGetLastError());
    CRP_HIP(ctx, hipEventRecord(a->ev_variants[1], ctx->stream));
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    a->variants_ms = hipEventElapsedTime(&ms, a->ev_variants[0], a->ev_variants[1]) == hipSuccess ? ms : 0.0;
    a->variants_seed = seed_len;
    a->have_variants = true;
    uint32_t *host[2] = {plus, minus};
    for (int s = 0; s < 2; ++s)
        if (host[s] && a->n_hits[s]) {
            const int rc = crp::staged_d2h(ctx, host[s], a->d_variants[s], a->n_hits[s] * sizeof(uint32_t));
            if (rc != CRP_OK) return rc;
        }
    return CRP_OK;
}

int crp_variant_counts_stats(const crp_arena *a, double *out, int n)
{
    if (!a || (n && !out) || n < 0 || n > 5) return CRP_ERR_INVALID;
    if (!a->have_variants) return CRP_ERR_STATE;
    const double v[5] = {a->variants_ms, (double)(a->n_hits[0] + a->n_hits[1]), (double)a->pend_guide_len, (double)a->variants_seed,
                         (double)a->n_var};
    for (int k = 0; k < n; ++k) out[k] = v[k];
    return CRP_OK;
}

}  // extern "C"
