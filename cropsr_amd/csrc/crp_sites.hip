// crp_sites.hip -- restriction sites of an enzyme set: cloning-safe guides and cut-site assays (DESIGN.md section 27;
// include/cropsr_hip.h states the definition, tests/site_reference.py restates it twice).  Not in the reference, opt-in.
//
// An enzyme is a recognition motif of 4 .. 16 IUPAC letters; it OCCURS at arena position q when the letters s[q : q + m]
// are bases and lie in the sets of the motif's letters, or of its reverse complement's.  Three steps:
//
//   planes   site_planes_kernel, one lane per plane word: occ[e][w] bit p = enzyme e occurs at 64 w + p.  Bit-parallel
//            shift-AND over the four one-hot base planes of the word and of its successor (the halo: m <= 16).  The enzyme
//            loop, the letter loop and the letter's set are wave-uniform (scalar loads of the enzyme table): the "is this
//            base in the set" selects are uniform branches.  No LDS, no atomics.
//   ranks    rank[e][w] = occurrences of e below 64 w: popcount, then an exclusive scan per enzyme in three launches
//            (chunk sums, a scan of the sums, the fill).  rank(x) = rank[e][x >> 6] + popc(occ[e][x >> 6] & lowmask(x & 63)).
//   columns  site_columns_kernel, one lane per table row, both tables in one launch (guide_properties_kernel's scheme):
//            per enzyme one 64-bit window of its occurrence plane answers "inside the guide" and "across the cut"; only a
//            row with a site across its cut asks two ranks for the amplicon's count.  One 8-byte store per row.
#include <algorithm>
#include <string>
#include <vector>

#include "crp_internal.h"
#include "crp_roctx.h"
#include "crp_sites.h"

namespace crp {

namespace {

typedef unsigned long long site_u64;

// a value every lane holds alike, moved to scalar registers: what branches on it is a uniform branch
__device__ __forceinline__ uint32_t site_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ site_u64 site_uniform(site_u64 v)
{
    return (site_u64)site_uniform((uint32_t)v) | (site_u64)site_uniform((uint32_t)(v >> 32)) << 32;
}

// the one-hot base planes of a word and of its successor: index = the set's bit (0 A, 1 C, 2 G, 3 T)
struct SiteBases {
    site_u64 cur[4], next[4];
};

// bit p: letters p + k, k < len, are bases in the sets of `motif` (nibble k)
__device__ __forceinline__ site_u64 site_match(site_u64 motif, uint32_t len, const SiteBases &b)
{
    site_u64 acc = ~0ull;
    for (uint32_t k = 0; k < len; ++k) {
        const uint32_t set = (uint32_t)(motif >> (4u * k)) & 15u;  // (uniform)
        site_u64 p0 = 0, p1 = 0;
        if (set & 1u) { p0 |= b.cur[0]; p1 |= b.next[0]; }
        if (set & 2u) { p0 |= b.cur[1]; p1 |= b.next[1]; }
        if (set & 4u) { p0 |= b.cur[2]; p1 |= b.next[2]; }
        if (set & 8u) { p0 |= b.cur[3]; p1 |= b.next[3]; }
        acc &= k ? (p0 >> k) | (p1 << (64u - k)) : p0;
    }
    return acc;
}

}  // namespace

__global__ __launch_bounds__(BLOCK) void site_planes_kernel(SitePlanes pl, const SiteEnzyme *__restrict__ enzymes, uint32_t n_enzymes,
                                                            site_u64 *__restrict__ occ)
{
    const uint64_t w = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (w >= pl.n_words) return;
    const bool more = w + 1 < pl.n_words;  // a word at or beyond the planes reads as zero
    const site_u64 ac0 = pl.ac[w], hi0 = pl.hi[w], lo0 = pl.lo[w];
    const site_u64 ac1 = more ? pl.ac[w + 1] : 0ull, hi1 = more ? pl.hi[w + 1] : 0ull, lo1 = more ? pl.lo[w + 1] : 0ull;
    SiteBases b;  // (hi, lo): A = 00, T = 01, C = 10, G = 11
    b.cur[0] = ac0 & ~hi0 & ~lo0;
    b.cur[1] = ac0 & hi0 & ~lo0;
    b.cur[2] = ac0 & hi0 & lo0;
    b.cur[3] = ac0 & ~hi0 & lo0;
    b.next[0] = ac1 & ~hi1 & ~lo1;
    b.next[1] = ac1 & hi1 & ~lo1;
    b.next[2] = ac1 & hi1 & lo1;
    b.next[3] = ac1 & ~hi1 & lo1;
    for (uint32_t e = 0; e < n_enzymes; ++e) {
        const site_u64 fwd = site_uniform(enzymes[e].fwd), rev = site_uniform(enzymes[e].rev);
        const uint32_t len = site_uniform(enzymes[e].len), palindrome = site_uniform(enzymes[e].palindrome);
        site_u64 hit = site_match(fwd, len, b);
        if (!palindrome) hit |= site_match(rev, len, b);
        occ[(uint64_t)e * pl.n_words + w] = hit;
    }
}

namespace {

// exclusive prefix of v over the workgroup's BLOCK lanes; *total = the workgroup's sum.  lds: BLOCK / 64 values.
__device__ __forceinline__ uint32_t site_block_scan(uint32_t v, uint32_t *lds, uint32_t *total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d, 64);
        if (lane >= (uint32_t)d) inc += up;
    }
    if (lane == 63u) lds[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t k = 0; k < BLOCK / 64; ++k) {
        const uint32_t s = lds[k];
        if (k < wave) before += s;
        all += s;
    }
    __syncthreads();  // (the next call writes lds again)
    *total = all;
    return before + inc - v;
}

// the popcounts of a lane's SITE_RANK_WORDS words of one enzyme's plane; words at or beyond n_words count nothing
__device__ __forceinline__ void site_lane_counts(const site_u64 *__restrict__ plane, uint64_t n_words, uint64_t first, uint32_t *c)
{
    for (int j = 0; j < SITE_RANK_WORDS; ++j) c[j] = first + j < n_words ? (uint32_t)__popcll(plane[first + j]) : 0u;
}

}  // namespace

// grid (chunks, enzymes): chunk_sum[e][chunk] = occurrences of e inside the chunk
__global__ __launch_bounds__(BLOCK) void site_rank_sums_kernel(const site_u64 *__restrict__ occ, uint64_t n_words, uint32_t n_chunks,
                                                               uint32_t *__restrict__ chunk_sum)
{
    __shared__ uint32_t lds[BLOCK / 64];
    const uint32_t e = blockIdx.y;
    uint32_t c[SITE_RANK_WORDS];
    site_lane_counts(occ + (uint64_t)e * n_words, n_words, (uint64_t)blockIdx.x * SITE_CHUNK + (uint64_t)threadIdx.x * SITE_RANK_WORDS, c);
    uint32_t v = 0, total;
    for (int j = 0; j < SITE_RANK_WORDS; ++j) v += c[j];
    (void)site_block_scan(v, lds, &total);
    if (threadIdx.x == 0) chunk_sum[(uint64_t)e * n_chunks + blockIdx.x] = total;
}

// one workgroup per enzyme: chunk_sum[e][.] becomes its own exclusive scan; rank[e][n_words] = the enzyme's total
__global__ __launch_bounds__(BLOCK) void site_rank_scan_kernel(uint32_t *__restrict__ chunk_sum, uint32_t n_chunks, uint64_t n_words,
                                                               uint32_t *__restrict__ rank)
{
    __shared__ uint32_t lds[BLOCK / 64];
    const uint32_t e = blockIdx.x;
    uint32_t *__restrict__ sums = chunk_sum + (uint64_t)e * n_chunks;
    uint32_t carry = 0;
    for (uint32_t first = 0; first < n_chunks; first += BLOCK) {
        const uint32_t k = first + threadIdx.x;
        const uint32_t v = k < n_chunks ? sums[k] : 0u;
        uint32_t total;
        const uint32_t ex = site_block_scan(v, lds, &total);
        if (k < n_chunks) sums[k] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) rank[(uint64_t)e * (n_words + 1) + n_words] = carry;
}

// grid (chunks, enzymes): rank[e][w] for the chunk's words, from the scanned chunk sums
__global__ __launch_bounds__(BLOCK) void site_rank_fill_kernel(const site_u64 *__restrict__ occ, uint64_t n_words, uint32_t n_chunks,
                                                               const uint32_t *__restrict__ chunk_sum, uint32_t *__restrict__ rank)
{
    __shared__ uint32_t lds[BLOCK / 64];
    const uint32_t e = blockIdx.y;
    const uint64_t first = (uint64_t)blockIdx.x * SITE_CHUNK + (uint64_t)threadIdx.x * SITE_RANK_WORDS;
    uint32_t c[SITE_RANK_WORDS];
    site_lane_counts(occ + (uint64_t)e * n_words, n_words, first, c);
    uint32_t v = 0, total;
    for (int j = 0; j < SITE_RANK_WORDS; ++j) v += c[j];
    uint32_t r = chunk_sum[(uint64_t)e * n_chunks + blockIdx.x] + site_block_scan(v, lds, &total);
    uint32_t *__restrict__ out = rank + (uint64_t)e * (n_words + 1);
    for (int j = 0; j < SITE_RANK_WORDS; ++j) {
        if (first + j < n_words) out[first + j] = r;
        r += c[j];
    }
}

namespace {

// bits [lo, lo + n) of a 64-bit value; n <= 0: none.  0 <= lo, lo + n <= 64, n <= 63.
__device__ __forceinline__ site_u64 site_bits(long long lo, long long n) { return n > 0 ? (~0ull >> (64 - n)) << lo : 0ull; }

// occurrences of the enzyme whose plane and rank row these are at positions below x, 0 <= x <= 64 n_words
__device__ __forceinline__ uint32_t site_rank(const site_u64 *__restrict__ plane, const uint32_t *__restrict__ rank, uint64_t n_words,
                                              long long x)
{
    const uint64_t w = (uint64_t)x >> 6;
    const uint32_t bits = (uint32_t)x & 63u;
    uint32_t r = rank[w];
    if (bits && w < n_words) r += (uint32_t)__popcll(plane[w] & ~(~0ull << bits));
    return r;
}

}  // namespace

// One launch for both tables: the first blocks_plus workgroups walk the '+' table, the others the '-' table.
__global__ __launch_bounds__(BLOCK) void site_columns_kernel(SiteTable plus, SiteTable minus, uint32_t blocks_plus, SiteIndex ix, int l, int flank)
{
    const bool is_minus = blockIdx.x >= blocks_plus;  // (uniform per workgroup)
    const SiteTable t = is_minus ? minus : plus;
    const uint64_t row = (uint64_t)(blockIdx.x - (is_minus ? blocks_plus : 0u)) * BLOCK + threadIdx.x;
    if (row >= t.n) return;
    const long long pos = (long long)t.pos[row];
    const long long c = is_minus ? pos + 6 : pos - 3;   // the cut boundary: letters c - 1 and c lie around the cut
    const long long g0 = is_minus ? pos + 3 : pos - l;  // the guide window [g0, g0 + l)
    // the text that contains c: the last one that starts at or below c, if c lies below its end
    uint32_t lo = 0, hi = ix.n_texts;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((long long)ix.text_start[mid] <= c) lo = mid + 1;
        else hi = mid;
    }
    long long a_lo = 0, a_hi = 0;  // the amplicon [a_lo, a_hi); empty where no text contains c
    if (lo) {
        const long long t0 = (long long)ix.text_start[lo - 1], t1 = (long long)ix.text_end[lo - 1];
        if (c < t1) {
            a_lo = max(c - (long long)flank, t0);
            a_hi = min(c + (long long)flank, t1);
        }
    }
    // one 64-bit window of an occurrence plane holds every start inside the guide and every start of a site across the
    // cut: it begins at min(g0, c - 15) and both ranges end within 62 positions of that
    const long long base = max(0ll, min(g0, c - (long long)(SITE_MAX_MOTIF - 1)));
    const uint64_t wb = (uint64_t)base >> 6;
    const uint32_t sh = (uint32_t)base & 63u;
    const bool in0 = wb < ix.n_words, in1 = sh && wb + 1 < ix.n_words;
    uint32_t in_guide = 0, assay = 0;
    for (uint32_t e = 0; e < ix.n_enzymes; ++e) {
        const long long m = (long long)site_uniform(ix.enzymes[e].len);
        const site_u64 *__restrict__ plane = ix.occ + (uint64_t)e * ix.n_words;
        const site_u64 x0 = in0 ? plane[wb] : 0ull, x1 = in1 ? plane[wb + 1] : 0ull;
        const site_u64 win = sh ? (x0 >> sh) | (x1 << (64u - sh)) : x0;  // bit k: an occurrence at base + k
        // inside the guide: g0 <= q and q + m <= g0 + l
        const long long g_lo = max(g0, base);
        if (win & site_bits(g_lo - base, g0 + l - m + 1 - g_lo)) in_guide |= 1u << e;
        // across the cut: c - m + 1 <= q <= c - 1
        const long long s_lo = max(c - m + 1, base);
        if (win & site_bits(s_lo - base, c - s_lo)) {
            // the amplicon: a_lo <= q and q + m <= a_hi
            const long long q_hi = a_hi - m + 1;
            if (q_hi > a_lo) {
                const uint32_t *__restrict__ rk = ix.rank + (uint64_t)e * (ix.n_words + 1);
                if (site_rank(plane, rk, ix.n_words, q_hi) - site_rank(plane, rk, ix.n_words, a_lo) == 1u) assay |= 1u << e;
            }
        }
    }
    t.out[row] = (site_u64)in_guide | (site_u64)assay << 32;
}

hipError_t launch_site_planes(hipStream_t s, const SitePlanes &planes, const SiteEnzyme *enzymes, uint32_t n_enzymes, unsigned long long *occ)
{
    if (!planes.n_words) return hipSuccess;
    hipLaunchKernelGGL(site_planes_kernel, dim3((uint32_t)((planes.n_words + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, planes, enzymes, n_enzymes, occ);
    return hipGetLastError();
}

hipError_t launch_site_ranks(hipStream_t s, const unsigned long long *occ, uint64_t n_words, uint32_t n_enzymes, uint32_t *chunk_sum,
                             uint32_t *rank)
{
    const uint32_t n_chunks = (uint32_t)((n_words + SITE_CHUNK - 1) / SITE_CHUNK);
    if (n_chunks) {
        hipLaunchKernelGGL(site_rank_sums_kernel, dim3(n_chunks, n_enzymes), dim3(BLOCK), 0, s, occ, n_words, n_chunks, chunk_sum);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(site_rank_scan_kernel, dim3(n_enzymes), dim3(BLOCK), 0, s, chunk_sum, n_chunks, n_words, rank);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !n_chunks) return e;
    hipLaunchKernelGGL(site_rank_fill_kernel, dim3(n_chunks, n_enzymes), dim3(BLOCK), 0, s, occ, n_words, n_chunks, chunk_sum, rank);
    return hipGetLastError();
}

hipError_t launch_site_columns(hipStream_t s, const SiteTable &plus, const SiteTable &minus, const SiteIndex &index, int guide_len, int flank)
{
    const uint32_t bp = (uint32_t)((plus.n + BLOCK - 1) / BLOCK), bm = (uint32_t)((minus.n + BLOCK - 1) / BLOCK);
    if (!(bp + bm)) return hipSuccess;
    hipLaunchKernelGGL(site_columns_kernel, dim3(bp + bm), dim3(BLOCK), 0, s, plus, minus, bp, index, guide_len, flank);
    return hipGetLastError();
}

// the set of bases an IUPAC letter stands for (bit 0 A, 1 C, 2 G, 3 T); 0: not a letter of the alphabet
static uint32_t site_letter_set(char ch)
{
    switch (ch >= 'a' && ch <= 'z' ? ch - 32 : ch) {
    case 'A': return 1;
    case 'C': return 2;
    case 'G': return 4;
    case 'T': case 'U': return 8;
    case 'R': return 1 | 4;
    case 'Y': return 2 | 8;
    case 'S': return 2 | 4;
    case 'W': return 1 | 8;
    case 'K': return 4 | 8;
    case 'M': return 1 | 2;
    case 'B': return 2 | 4 | 8;
    case 'D': return 1 | 4 | 8;
    case 'H': return 1 | 2 | 8;
    case 'V': return 1 | 2 | 4;
    case 'N': return 15;
    default: return 0;
    }
}

// the complement of a set: A <-> T, C <-> G
static uint32_t site_complement(uint32_t set) { return (set & 1) << 3 | (set & 2) << 1 | (set & 4) >> 1 | (set & 8) >> 3; }

static void site_free(crp_arena *a)
{
    (void)hipFree(a->d_site_occ);
    (void)hipFree(a->d_site_rank);
    (void)hipFree(a->d_site_chunk);
    a->d_site_occ = nullptr;
    a->d_site_rank = a->d_site_chunk = nullptr;
    a->site_index_bytes = a->site_alloc_enzymes = a->site_alloc_words = 0;
}

}  // namespace crp

extern "C" {

int crp_sites_set_enzymes(crp_arena *a, uint64_t n, const char *const *motifs, const uint32_t *lens, const uint32_t *text_starts,
                          const uint32_t *text_ends, uint64_t n_texts)
{
    crp::Range roctx_range("crp: restriction site planes");
    if (!a) return CRP_ERR_INVALID;
    crp_ctx *ctx = a->ctx;
    const std::string who = "crp_sites_set_enzymes: ";
    auto refuse = [&](const std::string &text) {
        ctx->last_error = who + text;
        return CRP_ERR_INVALID;
    };
    if (!a->sealed) {
        ctx->last_error = who + "the arena is not sealed";
        return CRP_ERR_STATE;
    }
    if (n < 1 || n > (uint64_t)crp::SITE_MAX_ENZYMES)
        return refuse("an enzyme set has 1.." + std::to_string(crp::SITE_MAX_ENZYMES) + " enzymes, not " + std::to_string(n));
    if (!motifs || !lens || (n_texts && (!text_starts || !text_ends))) return refuse("a null array");
    crp::SiteEnzyme table[crp::SITE_MAX_ENZYMES] = {};
    uint32_t m_max = 0;
    for (uint64_t e = 0; e < n; ++e) {
        const uint32_t m = lens[e];
        if (m < (uint32_t)crp::SITE_MIN_MOTIF || m > (uint32_t)crp::SITE_MAX_MOTIF || !motifs[e])
            return refuse("a motif has " + std::to_string(crp::SITE_MIN_MOTIF) + ".." + std::to_string(crp::SITE_MAX_MOTIF) + " letters; enzyme " +
                          std::to_string(e) + " has " + std::to_string(m));
        for (uint32_t k = 0; k < m; ++k) {
            const uint32_t set = crp::site_letter_set(motifs[e][k]);
            if (!set)
                return refuse("enzyme " + std::to_string(e) + ", letter " + std::to_string(k) + ": not one of the IUPAC letters ACGTRYSWKMBDHVN");
            table[e].fwd |= (unsigned long long)set << (4 * k);
            table[e].rev |= (unsigned long long)crp::site_complement(set) << (4 * (m - 1 - k));
        }
        table[e].len = m;
        table[e].palindrome = table[e].fwd == table[e].rev;
        m_max = std::max(m_max, m);
    }
    const uint64_t n_words = a->used_words, n_pos = n_words * 64;
    if (n_texts > 0xffffffffull) return refuse("too many texts");
    for (uint64_t k = 0; k < n_texts; ++k)
        if (text_starts[k] >= text_ends[k] || text_ends[k] > n_pos || (k && text_starts[k] < text_ends[k - 1]))
            return refuse("the text bounds ascend, do not overlap and lie inside the arena's " + std::to_string(n_pos) + " positions; text " +
                          std::to_string(k) + " does not");
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    a->have_sites = false;
    a->have_site_col = false;
    // 12 B per plane word and enzyme: the occurrence plane's 8 and the rank's 4; the chunk sums are scratch of the build
    const uint64_t n_chunks = (n_words + crp::SITE_CHUNK - 1) / crp::SITE_CHUNK;
    const uint64_t occ_bytes = n * n_words * 8, rank_bytes = n * (n_words + 1) * 4, chunk_bytes = std::max<uint64_t>(n * n_chunks * 4, 4);
    const uint64_t bytes = occ_bytes + rank_bytes + chunk_bytes;
    if (n != a->site_alloc_enzymes || n_words != a->site_alloc_words || !a->d_site_occ) {  // (each buffer's size depends on both)
        crp::site_free(a);
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&a->d_site_occ), occ_bytes);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&a->d_site_rank), rank_bytes);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&a->d_site_chunk), chunk_bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            crp::site_free(a);
            ctx->last_error = who + "the occurrence planes and ranks of " + std::to_string(n) + " enzymes over " + std::to_string(n_words) +
                              " plane words need " + std::to_string(bytes) + " bytes of device memory (12 per word and enzyme): " + hipGetErrorString(e);
            return e == hipErrorOutOfMemory ? CRP_ERR_NOMEM : CRP_ERR_HIP;
        }
        a->site_index_bytes = bytes;
        a->site_alloc_enzymes = n;
        a->site_alloc_words = n_words;
    }
    int rc = crp::grow(ctx, reinterpret_cast<void **>(&a->d_site_enz), &a->site_enz_cap, crp::SITE_MAX_ENZYMES, sizeof(crp::SiteEnzyme));
    for (int s = 0; s < 2 && rc == CRP_OK; ++s)
        rc = crp::grow(ctx, reinterpret_cast<void **>(&a->d_site_text[s]), &a->site_text_cap[s], std::max<uint64_t>(n_texts, 1), sizeof(uint32_t));
    if (rc != CRP_OK) return rc;
    CRP_HIP(ctx, hipMemcpyAsync(a->d_site_enz, table, sizeof(table), hipMemcpyHostToDevice, ctx->stream));
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (table is a local)
    if (n_texts) {
        rc = crp::staged_h2d(ctx, a->d_site_text[0], text_starts, n_texts * sizeof(uint32_t));
        if (rc == CRP_OK) rc = crp::staged_h2d(ctx, a->d_site_text[1], text_ends, n_texts * sizeof(uint32_t));
        if (rc != CRP_OK) return rc;
    }
    for (hipEvent_t &e : a->ev_sites)
        if (!e) CRP_HIP(ctx, hipEventCreate(&e));
    const crp::SitePlanes planes{a->d_plane[0], a->d_plane[1], a->d_plane[3], n_words};
    CRP_HIP(ctx, hipEventRecord(a->ev_sites[0], ctx->stream));
    CRP_HIP(ctx, crp::launch_site_planes(ctx->stream, planes, a->d_site_enz, (uint32_t)n, a->d_site_occ));
    CRP_HIP(ctx, hipEventRecord(a->ev_sites[1], ctx->stream));
    CRP_HIP(ctx, crp::launch_site_ranks(ctx->stream, a->d_site_occ, n_words, (uint32_t)n, a->d_site_chunk, a->d_site_rank));
    CRP_HIP(ctx, hipEventRecord(a->ev_sites[2], ctx->stream));
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    a->site_ms[0] = hipEventElapsedTime(&ms, a->ev_sites[0], a->ev_sites[1]) == hipSuccess ? ms : 0.0;
    a->site_ms[1] = hipEventElapsedTime(&ms, a->ev_sites[1], a->ev_sites[2]) == hipSuccess ? ms : 0.0;
    a->site_ms[2] = 0;
    a->n_site_enzymes = (uint32_t)n;
    a->site_m_max = m_max;
    a->site_words = n_words;
    a->n_site_texts = (uint32_t)n_texts;
    a->have_sites = true;
    return CRP_OK;
}

int crp_site_columns(crp_arena *a, int flank, uint64_t *plus, uint64_t *minus)
{
    crp::Range roctx_range("crp: restriction site columns");
    if (!a) return CRP_ERR_INVALID;
    crp_ctx *ctx = a->ctx;
    if (!a->have_hits) {
        ctx->last_error = "crp_site_columns: the arena has no hit tables (crp_scan_score)";
        return CRP_ERR_STATE;
    }
    if (!a->have_sites) {
        ctx->last_error = "crp_site_columns: the arena has no enzyme set (crp_sites_set_enzymes)";
        return CRP_ERR_STATE;
    }
    const int l = a->pend_guide_len;
    if (l < 1 || l > crp::SITE_MAX_GUIDE) {
        ctx->last_error = "crp_site_columns: the tables were scanned at guide length " + std::to_string(l) + ": a guide of 1.." +
                          std::to_string(crp::SITE_MAX_GUIDE) + " letters has a window";
        return CRP_ERR_INVALID;
    }
    if (flank < (int)a->site_m_max || flank > crp::SITE_MAX_FLANK) {
        ctx->last_error = "crp_site_columns: the amplicon's half-width is " + std::to_string(a->site_m_max) + " (the longest motif) .. " +
                          std::to_string(crp::SITE_MAX_FLANK) + ", not " + std::to_string(flank);
        return CRP_ERR_INVALID;
    }
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    a->have_site_col = false;
    for (int s = 0; s < 2; ++s) {
        const int rc = crp::grow(ctx, reinterpret_cast<void **>(&a->d_sites[s]), &a->sites_cap[s], a->n_hits[s], sizeof(uint64_t));
        if (rc != CRP_OK) return rc;
    }
    const crp::SiteTable tp{a->d_pos[0], reinterpret_cast<unsigned long long *>(a->d_sites[0]), a->n_hits[0]};
    const crp::SiteTable tm{a->d_pos[1], reinterpret_cast<unsigned long long *>(a->d_sites[1]), a->n_hits[1]};
    const crp::SiteIndex ix{a->d_site_occ, a->d_site_rank, a->d_site_enz, a->n_site_enzymes, a->site_words, a->d_site_text[0], a->d_site_text[1],
                            a->n_site_texts};
    CRP_HIP(ctx, hipEventRecord(a->ev_sites[2], ctx->stream));
    CRP_HIP(ctx, crp::launch_site_columns(ctx->stream, tp, tm, ix, l, flank));
    CRP_HIP(ctx, hipEventRecord(a->ev_sites[3], ctx->stream));
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    a->site_ms[2] = hipEventElapsedTime(&ms, a->ev_sites[2], a->ev_sites[3]) == hipSuccess ? ms : 0.0;
    a->site_flank = flank;
    a->have_site_col = true;
    uint64_t *host[2] = {plus, minus};
    for (int s = 0; s < 2; ++s)
        if (host[s] && a->n_hits[s]) {
            const int rc = crp::staged_d2h(ctx, host[s], a->d_sites[s], a->n_hits[s] * sizeof(uint64_t));
            if (rc != CRP_OK) return rc;
        }
    return CRP_OK;
}

int crp_site_stats(const crp_arena *a, double *out, int n)
{
    if (!a || (n && !out) || n < 0 || n > 7) return CRP_ERR_INVALID;
    if (!a->have_sites) return CRP_ERR_STATE;
    const bool col = a->have_site_col;
    const double v[7] = {a->site_ms[0], a->site_ms[1], col ? a->site_ms[2] : 0.0, col ? (double)(a->n_hits[0] + a->n_hits[1]) : 0.0,
                         (double)a->n_site_enzymes, col ? (double)a->site_flank : 0.0, (double)a->site_index_bytes};
    for (int k = 0; k < n; ++k) out[k] = v[k];
    return CRP_OK;
}

}  // extern "C"
