// crp_search_self.hip -- the self search (Self search): every guide site of an arena against every
// candidate site, without visiting all pairs.
//
// Two windows within M mismatches agree exactly, on bases, in at least one of the first M + 1 segments of the guide
// region.  So, per segment j:
//
//   order    a counting sort of the candidates by their 2-bit codes over segment j (self_key_kernel: key and
//            histogram; the host turns the histogram into bucket starts; self_scatter_kernel: one slot per candidate
//            through a cursor per key).  A bucket's guide sites come first: they are its queries.
//   compare  per bucket its guide sites against its candidates, all pairs.  One query per lane, in registers with its
//            M + 1 counters and its sum; the candidates of a slice are wave-uniform (scalar loads of 8 words per field).
//            Per pair: popc((h ^ qh) | (l ^ ql) | nb) <= M over fields masked to the guide region when the ordering was
//            written.  The no-hit loop has no atomics and no memory traffic of its own; a hit is counted only if its
//            mask is non-zero in every segment before j (else that segment's bucket has counted it), and a lane adds
//            its row to the result once, at the end of its slice.
//
// The CSV join (CSV join; self_join_kernel) hands the rows to the hits of a scan: one lane per hit of
// a strand's table, a binary search for the hit's site among the candidates in extraction order, the row copied.
//
// Only vector stores and vector atomics, like the rest of the library.
#include "crp_search_self.h"

namespace crp {

namespace {

__global__ __launch_bounds__(BLOCK) void self_flag_kernel(SearchCands c, uint32_t n, SelfGuideRule rule, uint8_t *__restrict__ flag,
                                                          unsigned long long *__restrict__ n_guides)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    bool guide = false;
    if (i < n) {
        const uint32_t h = c.hi[i], l = c.lo[i], nb = c.nb[i];
        guide = (nb & rule.region) == 0;
        for (int k = 0; k < rule.n; ++k) {  // (wave-uniform trip count)
            const int p = rule.pos[k];
            const uint32_t code = ((h >> p) & 1u) << 1 | ((l >> p) & 1u);
            guide = guide && !((nb >> p) & 1u) && ((rule.set[k] >> code) & 1u);
        }
        flag[i] = guide ? 1 : 0;
    }
    const uint64_t bal = __ballot(guide);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(n_guides, (unsigned long long)__popcll(bal));
}

__global__ __launch_bounds__(BLOCK) void self_key_kernel(SearchCands c, uint32_t n, const uint8_t *__restrict__ flag, int shift, int len,
                                                         uint32_t *__restrict__ key, uint32_t *__restrict__ hist)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t m = (1u << len) - 1u;
    const uint32_t h = (c.hi[i] >> shift) & m, l = (c.lo[i] >> shift) & m, nb = (c.nb[i] >> shift) & m;
    uint32_t k = SELF_NO_KEY;
    if (!nb) {
        k = ((h << len | l) << 1) | (flag[i] ? 0u : 1u);
        atomicAdd(&hist[k], 1u);
    }
    key[i] = k;
}

__global__ __launch_bounds__(BLOCK) void self_scatter_kernel(SearchCands c, uint32_t n, const uint32_t *__restrict__ key, uint32_t region,
                                                             uint32_t *__restrict__ cursor, uint32_t *__restrict__ hi,
                                                             uint32_t *__restrict__ lo, uint32_t *__restrict__ nb, uint32_t *__restrict__ idx)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = key[i];
    if (k == SELF_NO_KEY) return;
    const uint32_t slot = atomicAdd(&cursor[k], 1u);  // (< n: the cursors start at the prefix sums of the histogram)
    hi[slot] = c.hi[i] & region;
    lo[slot] = c.lo[i] & region;
    nb[slot] = c.nb[i] & region;
    idx[slot] = i;
}

// What a counted pair of 1 .. max_mm mismatches is worth: the compare's one template parameter.  of() gets the pair's
// mismatch mask (not 0) and number of mismatches, the query's fields, the candidate's (masked to the guide region, like
// the query's) and the candidate's entry of its ordering; add() gets a lane's sum at the end of its slice.
struct SelfNoValue {  // counts only
    __device__ __forceinline__ uint32_t of(uint32_t, int, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) const { return 0; }
    __device__ __forceinline__ void add(uint32_t, unsigned long long) const {}
};

struct SelfSchemeValue {  // hit_value, as the given-guides search has it
    SearchScore sc;
    __device__ __forceinline__ uint32_t of(uint32_t mask, int mm, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) const
    {
        return hit_value(mask, mm, sc);
    }
    __device__ __forceinline__ void add(uint32_t row, unsigned long long sum) const
    {
        if (sum) atomicAdd(&sc.hit_sum[row], sum);
    }
};

// Under a pair table (Pair tables).  The ordering's fields are masked to the guide region, which is
// all a mismatch's two letters need; the candidate's PAM letters come, on the hit path only, from its unmasked fields in
// extraction order (f_hi, f_lo of the candidates' handle) through the ordering's row index c_idx.  The candidate is
// wave-uniform, so that gather and the PAM value are scalar loads.
struct SelfPairValue {
    SearchPair sp;
    const uint32_t *__restrict__ c_idx, *__restrict__ f_hi, *__restrict__ f_lo;
    __device__ __forceinline__ uint32_t of(uint32_t mask, int, uint32_t qh, uint32_t ql, uint32_t ch, uint32_t cl, uint32_t cn, uint32_t at) const
    {
        if (mask & cn) return 0;  // a non-base at a mismatching position: counted, worth nothing
        const uint32_t row = c_idx[at];  // (an entry of the ordering, its index below the handle's n)
        return search_pair_value(search_pair_walk(mask, ch, cl, qh, ql, sp), search_pair_pam(f_hi[row], f_lo[row], sp));
    }
    __device__ __forceinline__ void add(uint32_t row, unsigned long long sum) const
    {
        if (sum) atomicAdd(&sp.hit_sum[row], sum);
    }
};

// The compare of the three kernels below: one query per lane, scalar candidate loads, the no-hit loop, and for a wave
// with a hit the segment test, the counters and the value.
template <class Value>
__device__ __forceinline__ void self_compare(const uint32_t *q_hi, const uint32_t *q_lo, const uint32_t *q_idx, const uint32_t *c_hi,
                                             const uint32_t *c_lo, const uint32_t *c_nb, const uint4 *items, SelfCompare cmp, uint32_t *counts,
                                             Value value)
{
    const uint4 it = items[blockIdx.x];  // wave-uniform: {first query, queries, first candidate, candidates}
    const bool have = threadIdx.x < it.y;
    const uint32_t qi = it.x + threadIdx.x;
    const uint32_t qh = have ? q_hi[qi] : 0u, ql = have ? q_lo[qi] : 0u;
    const int lim = have ? cmp.max_mm : -1;  // a lane without a query never hits
    const uint32_t self = cmp.skip_same ? qi : ~0u;
    uint32_t cnt[SELF_MAX_MM + 1] = {};
    unsigned long long sum = 0;
    const uint32_t end = it.z + it.w;
    // 8 consecutive words per field and trip: one scalar load each (the words behind `end` belong to the next slice or the
    // pad).  The pointers are stepped, not formed from i: their first use is then before the loop, and so is the wait for
    // the kernel arguments they come from.
    const uint32_t *ph = c_hi + it.z, *pl = c_lo + it.z, *pn = c_nb + it.z;
    for (uint32_t i = it.z; i < end; i += SELF_UNROLL, ph += SELF_UNROLL, pl += SELF_UNROLL, pn += SELF_UNROLL) {
        int mm[SELF_UNROLL];
        bool any = false;
#pragma unroll
        for (int k = 0; k < SELF_UNROLL; ++k) {
            mm[k] = __popc(xor_or(qh, ph[k], xor_or(ql, pl[k], pn[k])));
            any |= mm[k] <= lim;
        }
        if (__builtin_expect(any, 0)) {
#pragma unroll
            for (int k = 0; k < SELF_UNROLL; ++k) {
                if (mm[k] > lim || i + k >= end || i + k == self) continue;
                const uint32_t mask = xor_or(qh, ph[k], xor_or(ql, pl[k], pn[k]));
                bool first = true;  // no earlier segment's bucket holds this pair
#pragma unroll
                for (int s = 0; s < SELF_MAX_MM; ++s)  // (| and &=, not || and &&: nothing to skip, and it compiles to scalar mask logic)
                    first &= (s >= cmp.n_before) | ((mask & cmp.before[s]) != 0u);
                if (!first) continue;
#pragma unroll
                for (int n = 0; n <= SELF_MAX_MM; ++n) cnt[n] += mm[k] == n ? 1u : 0u;
                if (mm[k] > 0) sum += value.of(mask, mm[k], qh, ql, ph[k], pl[k], pn[k], i + k);
            }
        }
    }
    if (!have) return;
    const uint32_t row = q_idx[qi];
    const uint32_t stride = (uint32_t)cmp.max_mm + 1;
#pragma unroll
    for (int n = 0; n <= SELF_MAX_MM; ++n)
        if (n <= cmp.max_mm && cnt[n]) atomicAdd(&counts[(uint64_t)row * stride + n], cnt[n]);
    value.add(row, sum);
}

template <bool SCORED>
__global__ __launch_bounds__(SELF_TILE) void search_self_compare_kernel(const uint32_t *__restrict__ q_hi, const uint32_t *__restrict__ q_lo,
                                                                        const uint32_t *__restrict__ q_idx,
                                                                        const uint32_t *__restrict__ c_hi, const uint32_t *__restrict__ c_lo,
                                                                        const uint32_t *__restrict__ c_nb, const uint4 *__restrict__ items,
                                                                        SelfCompare cmp, uint32_t *__restrict__ counts, SearchScore sc)
{
    if (SCORED)
        self_compare(q_hi, q_lo, q_idx, c_hi, c_lo, c_nb, items, cmp, counts, SelfSchemeValue{sc});
    else
        self_compare(q_hi, q_lo, q_idx, c_hi, c_lo, c_nb, items, cmp, counts, SelfNoValue{});
}

__global__ __launch_bounds__(SELF_TILE) void search_self_pair_compare_kernel(const uint32_t *__restrict__ q_hi, const uint32_t *__restrict__ q_lo,
                                                                             const uint32_t *__restrict__ q_idx,
                                                                             const uint32_t *__restrict__ c_hi, const uint32_t *__restrict__ c_lo,
                                                                             const uint32_t *__restrict__ c_nb, const uint32_t *__restrict__ c_idx,
                                                                             const uint32_t *__restrict__ f_hi, const uint32_t *__restrict__ f_lo,
                                                                             const uint4 *__restrict__ items, SelfCompare cmp,
                                                                             uint32_t *__restrict__ counts, SearchPair sp)
{
    self_compare(q_hi, q_lo, q_idx, c_hi, c_lo, c_nb, items, cmp, counts, SelfPairValue{sp, c_idx, f_hi, f_lo});
}

// Extraction order as one ascending word: candidates come by 64-position word, within a word the '+' starts ascending
// and then the '-' starts (search_emit_kernel), so (word, strand, bit) ascends with the index.  pos = start | strand << 31
// with start < 2^31: the key has 32 bits.
__device__ __forceinline__ uint32_t join_key(uint32_t pos) { return ((pos & 0x7fffffc0u) << 1) | ((pos >> 31) << 6) | (pos & 63u); }

// One lane per hit of one strand's table (ascending arena match indices): '+' hit i has the site at forward start
// i - guide_len, '-' hit j the site at j.  The site's row, if it is a guide site of the handle, goes to the hit's
// columns; every other hit gets all-ones.  Reads only; writes its own slots only.
__global__ __launch_bounds__(BLOCK) void self_join_kernel(const uint32_t *__restrict__ hit_pos, uint32_t n_hits, uint32_t strand, uint32_t guide_len,
                                                          const uint32_t *__restrict__ cand_pos, uint32_t n_cand,
                                                          const uint8_t *__restrict__ flag, const uint32_t *__restrict__ counts,
                                                          const unsigned long long *__restrict__ hit_sum, uint32_t stride,
                                                          uint32_t *__restrict__ out_counts, unsigned long long *__restrict__ out_sum)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_hits) return;
    const uint32_t p = hit_pos[i];
    uint32_t row = n_cand;  // none
    if (strand || p >= guide_len) {
        const uint32_t site = (strand ? p : p - guide_len) | strand << 31;
        const uint32_t key = join_key(site);
        uint32_t lo = 0, hi = n_cand;  // the first candidate whose key is not below the site's
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (join_key(cand_pos[mid]) < key)
                lo = mid + 1;
            else
                hi = mid;
        }
        if (lo < n_cand && cand_pos[lo] == site && flag[lo]) row = lo;
    }
    const bool joined = row < n_cand;
#pragma unroll
    for (uint32_t n = 0; n <= (uint32_t)SELF_MAX_MM; ++n)
        if (n < stride) out_counts[(uint64_t)i * stride + n] = joined ? counts[(uint64_t)row * stride + n] : 0xFFFFFFFFu;
    out_sum[i] = joined && hit_sum ? hit_sum[row] : ~0ull;
}

inline uint32_t blocks_for(uint32_t n) { return (uint32_t)(((uint64_t)n + BLOCK - 1) / BLOCK); }

}  // namespace

hipError_t launch_self_flag(hipStream_t s, const SearchCands &c, uint32_t n, const SelfGuideRule &rule, uint8_t *flag,
                            unsigned long long *n_guides)
{
    if (!n) return hipSuccess;
    self_flag_kernel<<<dim3(blocks_for(n)), dim3(BLOCK), 0, s>>>(c, n, rule, flag, n_guides);
    return hipGetLastError();
}

hipError_t launch_self_key(hipStream_t s, const SearchCands &c, uint32_t n, const uint8_t *flag, int shift, int len, uint32_t *key,
                           uint32_t *hist)
{
    if (!n) return hipSuccess;
    self_key_kernel<<<dim3(blocks_for(n)), dim3(BLOCK), 0, s>>>(c, n, flag, shift, len, key, hist);
    return hipGetLastError();
}

hipError_t launch_self_scatter(hipStream_t s, const SearchCands &c, uint32_t n, const uint32_t *key, uint32_t region, uint32_t *cursor,
                               uint32_t *hi, uint32_t *lo, uint32_t *nb, uint32_t *idx)
{
    if (!n) return hipSuccess;
    self_scatter_kernel<<<dim3(blocks_for(n)), dim3(BLOCK), 0, s>>>(c, n, key, region, cursor, hi, lo, nb, idx);
    return hipGetLastError();
}

hipError_t launch_self_join(hipStream_t s, const uint32_t *hit_pos, uint32_t n_hits, int strand, int guide_len, const SearchCands &c, uint32_t n_cand,
                            const uint8_t *flag, const uint32_t *counts, const unsigned long long *hit_sum, int max_mm, uint32_t *out_counts,
                            unsigned long long *out_sum)
{
    if (!n_hits) return hipSuccess;
    self_join_kernel<<<dim3(blocks_for(n_hits)), dim3(BLOCK), 0, s>>>(hit_pos, n_hits, (uint32_t)strand, (uint32_t)guide_len, c.pos, n_cand, flag,
                                                                      counts, hit_sum, (uint32_t)max_mm + 1, out_counts, out_sum);
    return hipGetLastError();
}

hipError_t launch_self_compare(hipStream_t s, const SelfOrder &q, const SelfOrder &c, const uint4 *items, uint32_t n_items,
                               const SelfCompare &cmp, uint32_t *counts, const SearchScore *score)
{
    if (!n_items) return hipSuccess;
    if (score)
        search_self_compare_kernel<true><<<dim3(n_items), dim3(SELF_TILE), 0, s>>>(q.hi, q.lo, q.idx, c.hi, c.lo, c.nb, items, cmp, counts,
                                                                                  *score);
    else
        search_self_compare_kernel<false><<<dim3(n_items), dim3(SELF_TILE), 0, s>>>(q.hi, q.lo, q.idx, c.hi, c.lo, c.nb, items, cmp, counts,
                                                                                   SearchScore{nullptr, 0, nullptr});
    return hipGetLastError();
}

hipError_t launch_self_pair_compare(hipStream_t s, const SelfOrder &q, const SelfOrder &c, const SearchCands &c_fields, const uint4 *items,
                                    uint32_t n_items, const SelfCompare &cmp, uint32_t *counts, const SearchPair &pair)
{
    if (!n_items) return hipSuccess;
    search_self_pair_compare_kernel<<<dim3(n_items), dim3(SELF_TILE), 0, s>>>(q.hi, q.lo, q.idx, c.hi, c.lo, c.nb, c.idx, c_fields.hi,
                                                                              c_fields.lo, items, cmp, counts, pair);
    return hipGetLastError();
}

}  // namespace crp
