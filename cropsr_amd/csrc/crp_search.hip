// crp_search.hip -- the off-target search of given guides: every site of the arena that fits a
// PAM pattern of T <= 32 letters, on both strands, compared with every query guide; the sites within M mismatches are
// appended to a list and counted per (query, mismatches).
//
// Two phases, both on the arena's bit-planes:
//
//   extraction  one thread per 64-bit plane word = 64 forward starts.  For every window offset o the planes are
//               funnel-shifted by o, so bit b of the shifted word is the character at start 64 w + b + o; a start is a
//               '+' candidate when the character at every offset is in the pattern letter's base set, a '-' candidate
//               when it is in the complemented set of the letter at T - 1 - o, and for both when no character of the
//               window is void (outside every contig: a site never spans two contigs).  A count pass sizes the output
//               per workgroup; the emit pass writes each candidate's oriented window as three 32-bit fields (bit-reversed,
//               with `lo` flipped for '-').
//   compare     candidates in registers, SEARCH_CPL per lane; the queries of a batch are wave-uniform (scalar loads).
//               Per pair: popc(((h ^ qh) | (l ^ ql) | nb) & qm) <= M.  Hits are rare: a wave ballots them and reserves
//               its slots with one atomic.  The bulge compare (DNA or RNA bulge of one size) takes, per pair, the best
//               placement of the bulge inside the query's span; see search_bulge_compare_kernel.  The plain compare is
//               written once (compare<Value>) and instantiated with three values of a hit: none (search_compare_kernel),
//               the hit's value under a weighting scheme, added to a per-query sum (search_score_compare_kernel), and
//               its value under a pair table, values per base pair and per PAM (search_pair_compare_kernel).
//
// Only vector stores and vector atomics, like the rest of the library.
#include "crp_search.h"

namespace crp {

namespace {

__device__ __forceinline__ uint64_t fsh(uint64_t x0, uint64_t x1, int o)  // bits o .. o + 63 of x1:x0 (0 <= o < 64)
{
    return o ? (x0 >> o) | (x1 << (64 - o)) : x0;
}

__device__ __forceinline__ uint32_t set_at(const uint64_t s[2], int o) { return (uint32_t)(s[o >> 4] >> ((o & 15) * 4)) & 15u; }

// starts whose character at this offset is a base of `set` (ac: a base at all; codes A=00 T=01 C=10 G=11)
__device__ __forceinline__ uint64_t in_set(uint32_t set, uint64_t h, uint64_t l, uint64_t ac)
{
    uint64_t m = 0;
    if (set & 1u) m |= ~h & ~l;
    if (set & 2u) m |= ~h & l;
    if (set & 4u) m |= h & ~l;
    if (set & 8u) m |= h & l;
    return m & ac;
}

struct Words {
    uint64_t hi[2], lo[2], ac[2], vd[2];  // word w and w + 1 of hi, lo, ac and the void mask
};

__device__ __forceinline__ Words load_words(const Planes &pl, uint64_t w, uint64_t used_words)
{
    Words x;
    for (int k = 0; k < 2; ++k) {
        const uint64_t ww = w + k;
        if (ww < used_words) {
            const uint64_t h = pl.plane[0][ww], l = pl.plane[1][ww], u = pl.plane[2][ww], a = pl.plane[3][ww];
            x.hi[k] = h;
            x.lo[k] = l;
            x.ac[k] = a;
            x.vd[k] = h & l & ~u & ~a;
        } else {  // past the last contig's separator: void
            x.hi[k] = x.lo[k] = x.vd[k] = ~0ull;
            x.ac[k] = 0;
        }
    }
    return x;
}

// the '+' and '-' candidate starts of one word
__device__ __forceinline__ void window_masks(const Words &x, const SearchSets &ss, uint64_t &plus, uint64_t &minus)
{
    uint64_t p = ~0ull, m = ~0ull, bad = 0;
    for (int o = 0; o < ss.T; ++o) {
        const uint64_t h = fsh(x.hi[0], x.hi[1], o), l = fsh(x.lo[0], x.lo[1], o), a = fsh(x.ac[0], x.ac[1], o);
        bad |= fsh(x.vd[0], x.vd[1], o);
        const uint32_t sp = set_at(ss.plus, o), sm = set_at(ss.minus, o);  // (wave-uniform)
        if (sp != 15u) p &= in_set(sp, h, l, a);
        if (sm != 15u) m &= in_set(sm, h, l, a);
    }
    plus = p & ~bad;
    minus = m & ~bad;
}

__global__ __launch_bounds__(SEARCH_WORDS) void search_count_kernel(Planes pl, uint64_t used_words, SearchSets ss, uint2 *__restrict__ block_cnt)
{
    __shared__ uint32_t sum[2];
    if (threadIdx.x < 2) sum[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t w = (uint64_t)blockIdx.x * SEARCH_WORDS + threadIdx.x;
    uint64_t plus = 0, minus = 0;
    if (w < used_words) window_masks(load_words(pl, w, used_words), ss, plus, minus);
    // wave totals first, then one LDS atomic per wave and strand
    uint32_t np = __popcll(plus), nm = __popcll(minus);
    for (int d = 32; d >= 1; d >>= 1) {
        np += __shfl_xor(np, d);
        nm += __shfl_xor(nm, d);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&sum[0], np);
        atomicAdd(&sum[1], nm);
    }
    __syncthreads();
    if (threadIdx.x == 0) block_cnt[blockIdx.x] = make_uint2(sum[0], sum[1]);
}

__device__ __forceinline__ uint32_t brev_t(uint32_t x, int T) { return __builtin_bitreverse32(x) >> (32 - T); }

__global__ __launch_bounds__(SEARCH_WORDS) void search_emit_kernel(Planes pl, uint64_t used_words, SearchSets ss, uint32_t block_first,
                                                                   const uint32_t *__restrict__ block_off, SearchCands out)
{
    __shared__ uint32_t scan[SEARCH_WORDS];
    const uint32_t blk = block_first + blockIdx.x;
    const uint64_t w = (uint64_t)blk * SEARCH_WORDS + threadIdx.x;
    uint64_t plus = 0, minus = 0;
    Words x = {};
    if (w < used_words) {
        x = load_words(pl, w, used_words);
        window_masks(x, ss, plus, minus);
    }
    // exclusive prefix of the per-thread counts over the workgroup (Hillis-Steele in LDS)
    const uint32_t mine = __popcll(plus) + __popcll(minus);
    scan[threadIdx.x] = mine;
    __syncthreads();
    for (int d = 1; d < SEARCH_WORDS; d <<= 1) {
        const uint32_t v = threadIdx.x >= (uint32_t)d ? scan[threadIdx.x - d] : 0u;
        __syncthreads();
        scan[threadIdx.x] += v;
        __syncthreads();
    }
    if (!mine) return;
    uint32_t k = block_off[blk] + scan[threadIdx.x] - mine;
    const int T = ss.T;
    const uint32_t tmask = T == 32 ? ~0u : (1u << T) - 1u;
    const uint32_t base = (uint32_t)(w * 64);  // arena positions are < 2^31
    for (int s = 0; s < 2; ++s) {
        uint64_t bits = s ? minus : plus;
        while (bits) {
            const int b = __builtin_ctzll(bits);
            bits &= bits - 1;
            uint32_t h = (uint32_t)fsh(x.hi[0], x.hi[1], b) & tmask;
            uint32_t l = (uint32_t)fsh(x.lo[0], x.lo[1], b) & tmask;
            uint32_t nb = ~(uint32_t)fsh(x.ac[0], x.ac[1], b) & tmask;
            if (s) {  // oriented '-' window: position p is the complement of forward offset T - 1 - p
                h = brev_t(h, T);
                l = brev_t(l, T) ^ tmask;
                nb = brev_t(nb, T);
            }
            out.hi[k] = h;
            out.lo[k] = l;
            out.nb[k] = nb;
            out.pos[k] = (base + (uint32_t)b) | ((uint32_t)s << 31);
            ++k;
        }
    }
}

__device__ __forceinline__ uint32_t lane_rank(uint64_t mask)  // set bits of mask below this lane
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// Appends the wave's hits to the site list: one ballot, the leader reserves the wave's slots with one atomic.  A hit
// counts for (qi, mm) and, while there is room, stores its site word with the candidate's position.  pos is read only
// for a hit (loading it outside the branch changes the register allocation).
__device__ __forceinline__ void append_hits(bool hit, uint32_t qi, int mm, uint32_t word, const uint32_t *pos, uint32_t stride,
                                            uint32_t *__restrict__ counts, uint2 *__restrict__ sites, uint64_t site_cap,
                                            unsigned long long *__restrict__ site_ctr)
{
    const uint64_t bal = __ballot(hit);
    if (!bal) return;
    const int leader = __builtin_ctzll(bal);
    unsigned long long slot = 0;
    if ((int)(threadIdx.x & 63) == leader) slot = atomicAdd(site_ctr, (unsigned long long)__popcll(bal));
    slot = __shfl(slot, leader);
    if (hit) {
        slot += lane_rank(bal);
        atomicAdd(&counts[(uint64_t)qi * stride + mm], 1u);
        if (slot < site_cap) sites[slot] = make_uint2(word, *pos);
    }
}

// What a hit of 1 .. max_mm mismatches is worth: the compare's one template parameter.  add() gets the lane's mismatch
// mask (not 0), its candidate's oriented fields, the query's and the number of mismatches.
struct NoValue {  // counts and sites only
    __device__ __forceinline__ void add(uint32_t, uint32_t, uint32_t, uint32_t, const uint4 &, uint32_t, int) const {}
};

// The hit's value under a weighting scheme, added to hit_sum[q] with one 64-bit vector atomic.  The queries of a scored
// run have no base outside the guide region (checked on the host), so every bit of the mask has a factor.
struct SchemeValue {
    SearchScore sc;
    __device__ __forceinline__ void add(uint32_t mask, uint32_t, uint32_t, uint32_t, const uint4 &, uint32_t qi, int mm) const
    {
        atomicAdd(&sc.hit_sum[qi], (unsigned long long)hit_value(mask, mm, sc));
    }
};

// The hit's value under a pair table (Pair tables): the lane has the candidate's oriented fields, PAM
// positions included, and the query's in hand: per set bit of its mask it looks up the pair value of the two letters,
// then the value of the site's PAM letters.  The table is read on this path only.
struct PairValue {
    SearchPair sp;
    __device__ __forceinline__ void add(uint32_t mask, uint32_t h, uint32_t l, uint32_t nb, const uint4 &q, uint32_t qi, int) const
    {
        if (mask & nb) return;  // a non-base where the query has a base: counted, worth nothing
        const uint32_t v = search_pair_value(search_pair_walk(mask, h, l, q.x, q.y, sp), search_pair_pam(h, l, sp));
        atomicAdd(&sp.hit_sum[qi], (unsigned long long)v);
    }
};

// The compare of the three kernels below: SEARCH_CPL candidates per lane in registers, the no-hit loop over the batch's
// queries, and for a wave with a hit the append and the value.
template <class Value>
__device__ __forceinline__ void compare(SearchCands c, uint32_t n, const uint4 *queries, uint32_t q0, uint32_t nq, int max_mm, uint32_t *counts,
                                        uint2 *sites, uint64_t site_cap, unsigned long long *site_ctr, Value value)
{
    const uint32_t first = blockIdx.x * (BLOCK * SEARCH_CPL) + threadIdx.x;
    uint32_t h[SEARCH_CPL], l[SEARCH_CPL], nb[SEARCH_CPL];
    int lim[SEARCH_CPL];  // max_mm, or -1 past the end: a lane without a candidate never hits
#pragma unroll
    for (int j = 0; j < SEARCH_CPL; ++j) {
        const uint32_t i = first + j * BLOCK;
        const bool ok = i < n;
        h[j] = ok ? c.hi[i] : 0u;
        nb[j] = ok ? c.nb[i] : 0u;
        l[j] = ok ? c.lo[i] : 0u;  // (after nb: the loop's first instruction then needs the last load, one s_waitcnt instead of two)
        lim[j] = ok ? max_mm : -1;
    }
    const uint32_t stride = (uint32_t)max_mm + 1;
    for (uint32_t qi = q0; qi < q0 + nq; ++qi) {
        const uint4 q = queries[qi];  // wave-uniform
        int mm[SEARCH_CPL];
        bool any = false;
#pragma unroll
        for (int j = 0; j < SEARCH_CPL; ++j) {
            mm[j] = __popc(((h[j] ^ q.x) | (l[j] ^ q.y) | nb[j]) & q.z);  // (the compiler's xor + or3, not xor_or: as measured)
            any |= mm[j] <= lim[j];
        }
        if (__builtin_expect(any, 0)) {
#pragma unroll
            for (int j = 0; j < SEARCH_CPL; ++j) {
                const bool hit = mm[j] <= lim[j];
                append_hits(hit, qi, mm[j], qi << 4 | (uint32_t)mm[j], c.pos + (first + j * BLOCK), stride, counts, sites, site_cap,
                            site_ctr);
                if (hit && mm[j] > 0) value.add(((h[j] ^ q.x) | (l[j] ^ q.y) | nb[j]) & q.z, h[j], l[j], nb[j], q, qi, mm[j]);
            }
        }
    }
}

__global__ __launch_bounds__(BLOCK) void search_compare_kernel(SearchCands c, uint32_t n, const uint4 *__restrict__ queries, uint32_t q0,
                                                               uint32_t nq, int max_mm, uint32_t *__restrict__ counts,
                                                               uint2 *__restrict__ sites, uint64_t site_cap,
                                                               unsigned long long *__restrict__ site_ctr)
{
    compare(c, n, queries, q0, nq, max_mm, counts, sites, site_cap, site_ctr, NoValue{});
}

__global__ __launch_bounds__(BLOCK) void search_score_compare_kernel(SearchCands c, uint32_t n, const uint4 *__restrict__ queries, uint32_t q0,
                                                                     uint32_t nq, int max_mm, uint32_t *__restrict__ counts,
                                                                     uint2 *__restrict__ sites, uint64_t site_cap,
                                                                     unsigned long long *__restrict__ site_ctr, SearchScore sc)
{
    compare(c, n, queries, q0, nq, max_mm, counts, sites, site_cap, site_ctr, SchemeValue{sc});
}

__global__ __launch_bounds__(BLOCK) void search_pair_compare_kernel(SearchCands c, uint32_t n, const uint4 *__restrict__ queries, uint32_t q0,
                                                                    uint32_t nq, int max_mm, uint32_t *__restrict__ counts,
                                                                    uint2 *__restrict__ sites, uint64_t site_cap,
                                                                    unsigned long long *__restrict__ site_ctr, SearchPair sp)
{
    compare(c, n, queries, q0, nq, max_mm, counts, sites, site_cap, site_ctr, PairValue{sp});
}

// mismatch mask of a window's fields against a query's, over the window's positions
__device__ __forceinline__ uint32_t mism(uint32_t h, uint32_t l, uint32_t nb, uint32_t qh, uint32_t ql) { return xor_or(h, qh, xor_or(l, ql, nb)); }

// Bulge compare (Bulges).  Candidates are the windows of one bulge kind: T + d characters for a DNA
// bulge of d, T - r for an RNA bulge of r, T the query length.  Per pair two mismatch masks over the query positions:
// m0 against the window as it is (query i with window i) and m1 against the window moved by the bulge (query i with
// window i + d, or i - r): the shifted fields h1, l1, nb1 are formed once per candidate.  For a placement s,
//   mm(s) = popc(m0 & lo(s)) + popc(m1 & ~lo(s + r))      (r = 0 for a DNA bulge; bits s .. s + r - 1 are unpaired)
// with s in [s_min, s_max], the query's split limits.  a = m0 below s_max, m1 above, and b = m0 below s_min, m1
// above, give mm(s) = popc(a & lo(s)) + popc(b & ~lo(s + r)) for every such s, and every bit of a & b is counted in
// mm(s) unless it is one of the r unpaired ones: popc(a & b & qm) - r <= mm(s).  Pairs pass that bound rarely at small
// M; only a wave with a survivor scans s (wave-uniform bounds) for the minimum and the smallest s that reaches it.
__global__ __launch_bounds__(BLOCK) void search_bulge_compare_kernel(SearchCands c, uint32_t n, const uint4 *__restrict__ queries,
                                                                     uint32_t q0, uint32_t nq, int max_mm, int dna, int rna,
                                                                     uint32_t *__restrict__ counts, uint2 *__restrict__ sites,
                                                                     uint64_t site_cap, unsigned long long *__restrict__ site_ctr)
{
    const uint32_t first = blockIdx.x * (BLOCK * SEARCH_CPL) + threadIdx.x;
    uint32_t h[SEARCH_CPL], l[SEARCH_CPL], nb[SEARCH_CPL], h1[SEARCH_CPL], l1[SEARCH_CPL], nb1[SEARCH_CPL];
    int lim[SEARCH_CPL];  // max_mm + r, or -1 past the end
#pragma unroll
    for (int j = 0; j < SEARCH_CPL; ++j) {
        const uint32_t i = first + j * BLOCK;
        const bool ok = i < n;
        h[j] = ok ? c.hi[i] : 0u;
        l[j] = ok ? c.lo[i] : 0u;
        nb[j] = ok ? c.nb[i] : 0u;
        h1[j] = (h[j] >> dna) << rna;  // (one of dna, rna is 0)
        l1[j] = (l[j] >> dna) << rna;
        nb1[j] = (nb[j] >> dna) << rna;
        lim[j] = ok ? max_mm + rna : -1;
    }
    const uint32_t stride = (uint32_t)max_mm + 1;
    for (uint32_t qi = q0; qi < q0 + nq; ++qi) {
        const uint4 q = queries[qi];  // wave-uniform: {hi, lo, compare mask, s_min | s_max << 8}
        const int s_min = (int)(q.w & 255u), s_max = (int)((q.w >> 8) & 255u);
        const uint32_t la = (1u << s_max) - 1u, lb = (1u << s_min) - 1u;
        int bound[SEARCH_CPL];
        bool any = false;
#pragma unroll
        for (int j = 0; j < SEARCH_CPL; ++j) {
            const uint32_t m0 = mism(h[j], l[j], nb[j], q.x, q.y), m1 = mism(h1[j], l1[j], nb1[j], q.x, q.y);
            const uint32_t a = (m0 & la) | (m1 & ~la), b = (m0 & lb) | (m1 & ~lb);
            bound[j] = __popc(a & b & q.z);
            any |= bound[j] <= lim[j];
        }
        if (__builtin_expect(any, 0)) {
#pragma unroll
            for (int j = 0; j < SEARCH_CPL; ++j) {
                const bool cand = bound[j] <= lim[j];
                if (!__ballot(cand)) continue;
                int best = SEARCH_MAX_T + 1, at = s_min;
                if (cand) {
                    const uint32_t m0 = mism(h[j], l[j], nb[j], q.x, q.y), m1 = mism(h1[j], l1[j], nb1[j], q.x, q.y);
                    const uint32_t a = ((m0 & la) | (m1 & ~la)) & q.z, b = ((m0 & lb) | (m1 & ~lb)) & q.z;
                    int mm = __popc(a & lb) + __popc(b & ~((1u << (s_min + rna)) - 1u));
                    best = mm;
                    for (int s = s_min; s < s_max; ++s) {  // mm(s + 1) - mm(s) = a_s - b_(s + r)
                        mm += (int)((a >> s) & 1u) - (int)((b >> (s + rna)) & 1u);
                        if (mm < best) {
                            best = mm;
                            at = s + 1;
                        }
                    }
                }
                append_hits(cand && best <= max_mm, qi, best, qi << 9 | (uint32_t)at << 4 | (uint32_t)best, c.pos + (first + j * BLOCK),
                            stride, counts, sites, site_cap, site_ctr);
            }
        }
    }
}

}  // namespace

hipError_t launch_search_count(hipStream_t s, const Planes &pl, uint64_t used_words, const SearchSets &sets, uint2 *block_cnt)
{
    const uint64_t blocks = (used_words + SEARCH_WORDS - 1) / SEARCH_WORDS;
    if (!blocks) return hipSuccess;
    search_count_kernel<<<dim3((uint32_t)blocks), dim3(SEARCH_WORDS), 0, s>>>(pl, used_words, sets, block_cnt);
    return hipGetLastError();
}

hipError_t launch_search_emit(hipStream_t s, const Planes &pl, uint64_t used_words, const SearchSets &sets, uint32_t block_first,
                              uint32_t n_blocks, const uint32_t *block_off, SearchCands out)
{
    if (!n_blocks) return hipSuccess;
    search_emit_kernel<<<dim3(n_blocks), dim3(SEARCH_WORDS), 0, s>>>(pl, used_words, sets, block_first, block_off, out);
    return hipGetLastError();
}

// workgroups of a compare kernel over n candidates: BLOCK lanes of SEARCH_CPL candidates each
static uint32_t compare_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + BLOCK * SEARCH_CPL - 1) / (BLOCK * SEARCH_CPL)); }

hipError_t launch_search_compare(hipStream_t s, const SearchCands &c, uint32_t n, const uint4 *queries, uint32_t q0, uint32_t nq,
                                 int max_mm, uint32_t *counts, uint2 *sites, uint64_t site_cap, unsigned long long *site_ctr)
{
    if (!n || !nq) return hipSuccess;
    search_compare_kernel<<<dim3(compare_blocks(n)), dim3(BLOCK), 0, s>>>(c, n, queries, q0, nq, max_mm, counts, sites, site_cap, site_ctr);
    return hipGetLastError();
}

hipError_t launch_search_score_compare(hipStream_t s, const SearchCands &c, uint32_t n, const uint4 *queries, uint32_t q0, uint32_t nq,
                                       int max_mm, uint32_t *counts, uint2 *sites, uint64_t site_cap, unsigned long long *site_ctr,
                                       const SearchScore &score)
{
    if (!n || !nq) return hipSuccess;
    search_score_compare_kernel<<<dim3(compare_blocks(n)), dim3(BLOCK), 0, s>>>(c, n, queries, q0, nq, max_mm, counts, sites, site_cap,
                                                                                site_ctr, score);
    return hipGetLastError();
}

hipError_t launch_search_pair_compare(hipStream_t s, const SearchCands &c, uint32_t n, const uint4 *queries, uint32_t q0, uint32_t nq,
                                      int max_mm, uint32_t *counts, uint2 *sites, uint64_t site_cap, unsigned long long *site_ctr,
                                      const SearchPair &pair)
{
    if (!n || !nq) return hipSuccess;
    search_pair_compare_kernel<<<dim3(compare_blocks(n)), dim3(BLOCK), 0, s>>>(c, n, queries, q0, nq, max_mm, counts, sites, site_cap,
                                                                               site_ctr, pair);
    return hipGetLastError();
}

hipError_t launch_search_bulge_compare(hipStream_t s,const SearchCands &c, uint32_t n, const uint4 *queries, uint32_t q0, uint32_t nq,
                                       int max_mm, int dna, int rna, uint32_t *counts, uint2 *sites, uint64_t site_cap,
                                       unsigned long long *site_ctr)
{
    if (!n || !nq) return hipSuccess;
    search_bulge_compare_kernel<<<dim3(compare_blocks(n)), dim3(BLOCK), 0, s>>>(c, n, queries, q0, nq, max_mm, dna, rna, counts, sites,
                                                                                site_cap, site_ctr);
    return hipGetLastError();
}

}  // namespace crp
