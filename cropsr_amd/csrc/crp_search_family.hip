// crp_search_family.hip -- gene families on a self-search handle.
//
// The self search counts, per guide site, every near copy in the genome.  In a polyploid most of those copies are the
// gene's own homeologs, which a knock-out guide is meant to cut.  With a family table the handle also says WHERE:
//
//   bounds   one lane per family gene: a binary search of the candidates' positions (extraction order, join_key as in the
//            CSV join) for the run of candidates whose 64-position word can hold a site that cuts in the gene.
//   assign   over each gene's run, the candidates whose cut site lies in the gene take the smallest gene row as their
//            owner (vector atomicMin); one pass then turns the owner into a tag (owner | guide site << 31), writes the
//            owner's family and starts the cover word with the owner's own bit.
//   compare  per item the guide sites owned by member a (a tile of its run, one query per lane, in registers with its
//            M + 1 counters, its sum and one cover bit) against the candidates owned by member b (a slice of its run,
//            wave-uniform: scalar loads of 8 words per field and of the tags).  Per pair popc((h ^ qh) | (l ^ ql) | nb)
//            <= M over the fields masked to the guide region; the value of a hit is the self search's.  A lane adds its
//            row once, at the end of its item (vector atomicAdd, 64-bit vector atomicOr for the cover bit).
//   join     the family columns onto the hit tables, by the key search of the CSV join.
//
// Only vector stores and vector atomics, like the rest of the library.
#include "crp_search_family.h"

namespace crp {

namespace {

// Extraction order as one ascending word (crp_search_self.hip states the same): (64-position word, strand, bit).
__device__ __forceinline__ uint32_t family_key(uint32_t pos) { return ((pos & 0x7fffffc0u) << 1) | ((pos >> 31) << 6) | (pos & 63u); }

// The first candidate whose key is not below `key` (64 bits: one word past the last one does not wrap).
__device__ __forceinline__ uint32_t family_lower(const uint32_t *__restrict__ cand_pos, uint32_t n, uint64_t key)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if ((uint64_t)family_key(cand_pos[mid]) < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(BLOCK) void family_bounds_kernel(const FamilyRow *__restrict__ rows, uint32_t n_rows,
                                                              const uint32_t *__restrict__ cand_pos, uint32_t n_cand, int d,
                                                              uint2 *__restrict__ run)
{
    const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= n_rows) return;
    const FamilyRow g = rows[r];
    // '+' starts lo - d .. hi - d, '-' starts lo .. hi (d = T - 6 may be negative for a tiny guide)
    const int64_t first = max((int64_t)0, min((int64_t)g.lo, (int64_t)g.lo - d));
    const int64_t last = max((int64_t)g.hi, (int64_t)g.hi - d);
    uint2 out = make_uint2(0, 0);
    if (g.lo <= g.hi && last >= 0) {
        out.x = family_lower(cand_pos, n_cand, (uint64_t)(first >> 6) << 7);
        out.y = family_lower(cand_pos, n_cand, ((uint64_t)(last >> 6) + 1) << 7);
    }
    run[r] = out;
}

__global__ __launch_bounds__(BLOCK) void family_assign_kernel(const FamilyRow *__restrict__ rows, const uint2 *__restrict__ run,
                                                              const uint32_t *__restrict__ cand_pos, int d, uint32_t *__restrict__ owner)
{
    const uint32_t r = blockIdx.x;  // (one workgroup per family gene)
    const FamilyRow g = rows[r];
    const uint2 span = run[r];
    for (uint32_t c = span.x + threadIdx.x; c < span.y; c += BLOCK) {
        const uint32_t p = cand_pos[c];
        const int64_t cut = (p >> 31) ? (int64_t)(p & 0x7fffffffu) : (int64_t)p + d;
        if (cut >= (int64_t)g.lo && cut <= (int64_t)g.hi) atomicMin(&owner[c], r);
    }
}

__global__ __launch_bounds__(BLOCK) void family_finish_kernel(const FamilyRow *__restrict__ rows, const uint8_t *__restrict__ flag,
                                                              uint32_t n_cand, uint32_t *__restrict__ owner_tag,
                                                              uint32_t *__restrict__ family, unsigned long long *__restrict__ cover)
{
    const uint32_t c = blockIdx.x * BLOCK + threadIdx.x;
    if (c >= n_cand) return;
    const uint32_t o = owner_tag[c];
    const bool owned = o != FAMILY_NONE, guide = flag[c] != 0;
    uint32_t fam = FAMILY_NONE, member = 0;
    if (owned) {
        fam = rows[o].family;
        member = rows[o].member;
    }
    owner_tag[c] = (owned ? o : FAMILY_NO_ROW) | (guide ? FAMILY_GUIDE : 0u);
    family[c] = fam;
    cover[c] = owned && guide ? 1ull << member : 0ull;
}

// What a counted pair of 1 .. max_mm mismatches is worth.  of() gets the mismatch mask (not 0), the number of
// mismatches, the query's masked fields and the candidate's fields, masked and as extracted.
struct FamilyNoValue {
    __device__ __forceinline__ uint32_t of(uint32_t, int, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) const { return 0; }
};

struct FamilySchemeValue {
    SearchScore sc;
    __device__ __forceinline__ uint32_t of(uint32_t mask, int mm, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) const
    {
        return hit_value(mask, mm, sc);
    }
};

struct FamilyPairValue {  // as the self search under a pair table: the PAM letters from the unmasked fields
    SearchPair sp;
    __device__ __forceinline__ uint32_t of(uint32_t mask, int, uint32_t qh, uint32_t ql, uint32_t ch, uint32_t cl, uint32_t cn, uint32_t fh,
                                           uint32_t fl) const
    {
        if (mask & cn) return 0;  // a non-base at a mismatching position: counted, worth nothing
        return search_pair_value(search_pair_walk(mask, ch, cl, qh, ql, sp), search_pair_pam(fh, fl, sp));
    }
};

template <class Value>
__global__ __launch_bounds__(SELF_TILE) void search_family_compare_kernel(FamilyCands q, FamilyCands c, const uint4 *__restrict__ items,
                                                                          FamilyCompare cmp, uint32_t *__restrict__ counts,
                                                                          unsigned long long *__restrict__ sums,
                                                                          unsigned long long *__restrict__ cover, Value value)
{
    const uint4 it = items[2 * blockIdx.x];      // wave-uniform: {first query, queries, first candidate, candidates}
    const uint4 ow = items[2 * blockIdx.x + 1];  // {owner row of the queries, owner row of the candidates, its member bit, 0}
    const uint32_t qi = it.x + threadIdx.x;
    bool have = threadIdx.x < it.y;
    if (have) have = q.tag[qi] == (ow.x | FAMILY_GUIDE);  // a guide site that a owns
    const uint32_t region = cmp.region;
    const uint32_t qh = have ? q.hi[qi] & region : 0u, ql = have ? q.lo[qi] & region : 0u;
    const int lim = have ? cmp.max_mm : -1;  // a lane without a query never hits
    const uint32_t self = cmp.same ? qi : ~0u;
    uint32_t cnt[SELF_MAX_MM + 1] = {};
    unsigned long long sum = 0;
    bool cov = false;
    const uint32_t end = it.z + it.w;

    // one candidate (wave-uniform i, fields fh / fl / fn as extracted, its tag) against the lane's query
    const auto hit = [&](uint32_t i, uint32_t fh, uint32_t fl, uint32_t fn, uint32_t tag) {
        if ((tag & FAMILY_NO_ROW) != ow.y || i == self) return;  // (scalar: not b's, or the site itself)
        const uint32_t ch = fh & region, cl = fl & region, cn = fn & region;
        const uint32_t mask = xor_or(qh, ch, xor_or(ql, cl, cn));
        const int mm = __popc(mask);
        if (mm > lim) return;
#pragma unroll
        for (int n = 0; n <= SELF_MAX_MM; ++n) cnt[n] += mm == n ? 1u : 0u;
        if (mm > 0) sum += value.of(mask, mm, qh, ql, ch, cl, cn, fh, fl);
        cov |= (tag & FAMILY_GUIDE) != 0u && mm <= cmp.cover_mm;
    };

    uint32_t i = it.z;
    const uint32_t *ph = c.hi + i, *pl = c.lo + i, *pn = c.nb + i, *pt = c.tag + i;
    // 8 consecutive words per field and trip, all of them inside the slice: one scalar load each
    for (; i + SELF_UNROLL <= end; i += SELF_UNROLL, ph += SELF_UNROLL, pl += SELF_UNROLL, pn += SELF_UNROLL, pt += SELF_UNROLL) {
        bool any = false;
#pragma unroll
        for (int k = 0; k < SELF_UNROLL; ++k) {
            const int mm = __popc(xor_or(qh, ph[k] & region, xor_or(ql, pl[k] & region, pn[k] & region)));
            any |= mm <= ((pt[k] & FAMILY_NO_ROW) == ow.y ? lim : -1);
        }
        if (__builtin_expect(any, 0)) {
#pragma unroll
            for (int k = 0; k < SELF_UNROLL; ++k) hit(i + k, ph[k], pl[k], pn[k], pt[k]);
        }
    }
    for (; i < end; ++i, ++ph, ++pl, ++pn, ++pt) hit(i, *ph, *pl, *pn, *pt);  // (the slice's last 0 .. 7)

    if (!have) return;
    const uint32_t stride = (uint32_t)cmp.max_mm + 1;
#pragma unroll
    for (int n = 0; n <= SELF_MAX_MM; ++n)
        if (n <= cmp.max_mm && cnt[n]) atomicAdd(&counts[(uint64_t)qi * stride + n], cnt[n]);
    if (sum) atomicAdd(&sums[qi], sum);
    if (cov) atomicOr(&cover[qi], 1ull << (ow.z & 63u));
}

// One lane per hit of one strand's table, the key search of self_join_kernel; reads only, writes its own slots only.
__global__ __launch_bounds__(BLOCK) void family_join_kernel(const uint32_t *__restrict__ hit_pos, uint32_t n_hits, uint32_t strand,
                                                            uint32_t guide_len, const uint32_t *__restrict__ cand_pos, uint32_t n_cand,
                                                            const uint32_t *__restrict__ tag, const uint32_t *__restrict__ family,
                                                            const uint32_t *__restrict__ counts, const unsigned long long *__restrict__ sum,
                                                            const unsigned long long *__restrict__ cover, uint32_t stride,
                                                            uint32_t *__restrict__ out_counts, unsigned long long *__restrict__ out_sum,
                                                            unsigned long long *__restrict__ out_cover, uint32_t *__restrict__ out_family)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_hits) return;
    const uint32_t p = hit_pos[i];
    uint32_t row = n_cand;  // none
    if (strand || p >= guide_len) {
        const uint32_t site = (strand ? p : p - guide_len) | strand << 31;
        const uint32_t at = family_lower(cand_pos, n_cand, family_key(site));
        if (at < n_cand && cand_pos[at] == site && (tag[at] & FAMILY_GUIDE)) row = at;
    }
    const bool joined = row < n_cand;
#pragma unroll
    for (uint32_t n = 0; n <= (uint32_t)SELF_MAX_MM; ++n)
        if (n < stride) out_counts[(uint64_t)i * stride + n] = joined ? counts[(uint64_t)row * stride + n] : 0xFFFFFFFFu;
    out_sum[i] = joined ? sum[row] : ~0ull;
    out_cover[i] = joined ? cover[row] : 0ull;
    out_family[i] = joined ? family[row] : FAMILY_NONE;
}

inline uint32_t blocks_for(uint32_t n) { return (uint32_t)(((uint64_t)n + BLOCK - 1) / BLOCK); }

}  // namespace

hipError_t launch_family_bounds(hipStream_t s, const FamilyRow *rows, uint32_t n_rows, const uint32_t *cand_pos, uint32_t n_cand, int T,
                                uint2 *run)
{
    if (!n_rows) return hipSuccess;
    family_bounds_kernel<<<dim3(blocks_for(n_rows)), dim3(BLOCK), 0, s>>>(rows, n_rows, cand_pos, n_cand, T - 6, run);
    return hipGetLastError();
}

hipError_t launch_family_assign(hipStream_t s, const FamilyRow *rows, uint32_t n_rows, const uint2 *run, const uint32_t *cand_pos, int T,
                                uint32_t *owner)
{
    if (!n_rows) return hipSuccess;
    family_assign_kernel<<<dim3(n_rows), dim3(BLOCK), 0, s>>>(rows, run, cand_pos, T - 6, owner);
    return hipGetLastError();
}

hipError_t launch_family_finish(hipStream_t s, const FamilyRow *rows, const uint8_t *flag, uint32_t n_cand, uint32_t *owner_tag,
                                uint32_t *family, unsigned long long *cover)
{
    if (!n_cand) return hipSuccess;
    family_finish_kernel<<<dim3(blocks_for(n_cand)), dim3(BLOCK), 0, s>>>(rows, flag, n_cand, owner_tag, family, cover);
    return hipGetLastError();
}

hipError_t launch_family_compare(hipStream_t s, const FamilyCands &q, const FamilyCands &c, const uint4 *items, uint32_t n_items,
                                 const FamilyCompare &cmp, uint32_t *counts, unsigned long long *sum, unsigned long long *cover,
                                 const SearchScore *score, const SearchPair *pair)
{
    if (!n_items) return hipSuccess;
    const dim3 grid(n_items), block(SELF_TILE);
    if (pair)
        search_family_compare_kernel<<<grid, block, 0, s>>>(q, c, items, cmp, counts, sum, cover, FamilyPairValue{*pair});
    else if (score)
        search_family_compare_kernel<<<grid, block, 0, s>>>(q, c, items, cmp, counts, sum, cover, FamilySchemeValue{*score});
    else
        search_family_compare_kernel<<<grid, block, 0, s>>>(q, c, items, cmp, counts, sum, cover, FamilyNoValue{});
    return hipGetLastError();
}

hipError_t launch_family_join(hipStream_t s, const uint32_t *hit_pos, uint32_t n_hits, int strand, int guide_len, const uint32_t *cand_pos,
                              uint32_t n_cand, const uint32_t *tag, const uint32_t *family, const uint32_t *counts,
                              const unsigned long long *sum, const unsigned long long *cover, int max_mm, uint32_t *out_counts,
                              unsigned long long *out_sum, unsigned long long *out_cover, uint32_t *out_family)
{
    if (!n_hits) return hipSuccess;
    family_join_kernel<<<dim3(blocks_for(n_hits)), dim3(BLOCK), 0, s>>>(hit_pos, n_hits, (uint32_t)strand, (uint32_t)guide_len, cand_pos, n_cand,
                                                                        tag, family, counts, sum, cover, (uint32_t)max_mm + 1, out_counts,
                                                                        out_sum, out_cover, out_family);
    return hipGetLastError();
}

}  // namespace crp
