// crp_select_self.hip -- guide selection for any nuclease on the device: for every gene, the K most
// specific guide sites of a self-search handle whose cut letter lies in the gene and that pass the thresholds
// (include/cropsr_hip.h, crp_select_run_self, states the definition).  The rows are the handle's own: the candidates in
// extraction order with their guide flags, counts and hit sums, where the compares left them.
//
//   bounds   one lane per gene: the candidates ascend by (64-position word, strand, bit), so the rows whose start lies in
//            [lo - T, hi] are inside one run of whole words -- two binary searches over the position column.  The run is a
//            superset; the exact test is the item kernel's
//   items    one WAVE per work item (a gene's run, cut by the host into pieces of at most slice_rows rows): 64 candidates
//            a trip, coalesced -- position, guide flag, the counts row, the hit sum, and the code bits only under a GC or a
//            T-run limit.  The wave keeps its top K sorted across its lanes (crp_select_insert.h) under the key ~e, so the
//            most specific site is the highest key, with the tie word cut << 1 | strand
//   gather   one lane per selected entry: its position, strand, code bits, counts, hit sum and on-target sum into compact arrays
//
// With an on-target model on the handle the items kernel's model form also reads the candidate's f64
// sum: as a bound, as the ranking key (larger sum first, self_select_model_key; the tie word is unchanged) or both.  The
// other form is section 28's, bit for bit.
//
// A cut gene's partial lists are merged by crp_select.hip's merge kernel, as they are.  The CDS test is an inline look-up
// through the arena's track and bucket table (annot_lookup_kernel's scheme), paid only by the lanes that pass every other
// test.  No atomics, no LDS, no scratch; every result slot has one owner and is written with plain vector stores.
#include "crp_kernels.h"
#include "crp_select_insert.h"
#include "crp_select_self.h"

namespace crp {

static_assert(BLOCK == SELECT_WAVES * 64, "one wave of 64 lanes per work item");

namespace {

constexpr int SELF_SELECT_ANN_SHIFT = 11;  // one bucket of the track's index = 2 048 arena positions (crp_annotate.hip)

// Extraction order as one ascending word (crp_search_self.hip states the same): (64-position word, strand, bit).
__device__ __forceinline__ uint32_t self_select_key(uint32_t pos) { return ((pos & 0x7fffffc0u) << 1) | ((pos >> 31) << 6) | (pos & 63u); }

// The first candidate whose key is not below `key` (64 bits: one word past the last one does not wrap).
__device__ __forceinline__ uint32_t self_select_lower(const uint32_t *__restrict__ cand_pos, uint32_t n, uint64_t key)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)self_select_key(cand_pos[mid]) < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(BLOCK) void select_self_bounds_kernel(const uint32_t *__restrict__ cand_pos, uint32_t n_cand, uint32_t T,
                                                                   const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi,
                                                                   uint32_t n_genes, uint2 *__restrict__ run)
{
    const uint32_t g = blockIdx.x * BLOCK + threadIdx.x;
    if (g >= n_genes) return;
    // a site with start s cuts at s + 1 .. s + T - 1: the starts of a gene's rows lie in [lo - T, hi], clamped at 0
    const uint32_t l = lo[g], h = hi[g];
    const uint32_t first = l > T ? l - T : 0u;
    uint2 out = make_uint2(0, 0);
    if (l <= h) {
        out.x = self_select_lower(cand_pos, n_cand, (uint64_t)(first >> 6) << 7);
        out.y = self_select_lower(cand_pos, n_cand, ((uint64_t)(h >> 6) + 1) << 7);
    }
    run[g] = out;
}

// The key's e of an unscored handle: counts[0] saturated at 65 535 in the top 16 bits, counts[1 .. M] saturated at 4 095
// in 12 bits each below it, the most significant field first (M <= 4: 48 bits).
__device__ __forceinline__ unsigned long long self_select_pack(const uint32_t *__restrict__ row, uint32_t c0, uint32_t stride)
{
    unsigned long long e = (unsigned long long)min(c0, 65535u) << 48;
    for (uint32_t j = 1; j < stride; ++j) e |= (unsigned long long)min(row[j], 4095u) << (48u - 12u * j);  // (wave-uniform trip count)
    return e;
}

// The longest run of set bits.
__device__ __forceinline__ uint32_t self_select_run(uint32_t m)
{
    uint32_t r = 0;
    while (m) {
        m &= m >> 1;
        ++r;
    }
    return r;
}

// The flag of the track interval under arena position `cut` (annot_one's search): false where there is none.
__device__ __forceinline__ bool self_select_cds(uint32_t cut, const SelfSelectTrack &t)
{
    const uint32_t b = min(cut >> SELF_SELECT_ANN_SHIFT, t.last_bucket);
    uint32_t lo = t.bucket[b], hi = t.bucket[b + 1];
    while (lo < hi) {  // points[lo..hi) lie inside the bucket: how many of them are <= cut
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (t.points[mid] <= cut) lo = mid + 1;
        else hi = mid;
    }
    if (!lo) return false;
    const uint32_t id = t.ids[lo - 1];
    return id < t.n_flags && t.flags[id] != 0;
}

// The list key of an on-target sum s: a larger s is a higher key.  With b the bits of s, -0.0 first
// replaced by +0.0: b ^ 0x8000000000000000 for b >= 0 as a signed value, ~b otherwise.
__device__ __forceinline__ unsigned long long self_select_model_key(double s)
{
    long long b = __double_as_longlong(s);
    if (b == (long long)0x8000000000000000ull) b = 0;
    return b >= 0 ? (unsigned long long)b ^ 0x8000000000000000ull : ~(unsigned long long)b;
}

// MODEL: the form that reads the on-target sum -- as a threshold (pred.has_min), as the ranking key (pred.rank_model) or both.
template <bool MODEL>
__global__ __launch_bounds__(BLOCK) void select_self_items_kernel(SelfSelectRows rows, SelfSelectTrack track, SelfSelectPredicate pred,
                                                                  const uint32_t *__restrict__ gene_lo, const uint32_t *__restrict__ gene_hi,
                                                                  const SelectItem *__restrict__ items, uint32_t n_items, SelectPartials part,
                                                                  SelectResult res)
{
    const uint32_t item = blockIdx.x * SELECT_WAVES + (threadIdx.x >> 6);  // (uniform per wave)
    if (item >= n_items) return;
    const int lane = threadIdx.x & 63;
    const SelectItem it = items[item];
    const int k = pred.k;
    const uint32_t lo = gene_lo[it.gene], hi = gene_hi[it.gene];
    SelEntry mine{0ull, SELECT_NONE, SELECT_NONE};  // (worse than every site: a site's tie is below 2^32 - 1)
    uint32_t n_in = 0, n_pass = 0;
    // (the item's rows lie inside the candidates: crp_select.cpp cuts them from the bounds kernel's runs and checks them;
    // 64 bits: a run may end within 64 of 2^32)
    const uint64_t end = (uint64_t)it.first[0] + it.rows[0];
    for (uint64_t r0 = it.first[0]; r0 < end; r0 += 64) {
        const uint64_t row = r0 + lane;
        const bool in = row < end;
        const uint32_t p = in ? rows.pos[row] : 0u;
        const bool guide = in && rows.flag[row] != 0;
        const uint32_t strand = p >> 31, start = p & 0x7fffffffu;
        const uint32_t cut = start + (strand ? pred.T - pred.cut : pred.cut);
        const bool inside = guide && cut >= lo && cut <= hi;
        const uint32_t *crow = rows.counts + row * rows.stride;
        const uint32_t c0 = inside ? crow[0] : 0u;
        bool pass = inside && c0 <= pred.max_mm0;
        unsigned long long e;
        if (rows.sum) {  // (uniform)
            const unsigned long long sum = inside ? rows.sum[row] : 0ull;
            pass = pass && sum <= pred.max_hit_sum;
            // no overflow: a hit's value is at most 2^30 and a site has fewer than 2^32 hits, so hit_sum < 2^62, and
            // counts[0] < 2^32 makes the second term less than 2^62 as well
            e = sum + ((unsigned long long)c0 << 30);
        } else {
            e = inside ? self_select_pack(crow, c0, rows.stride) : 0ull;
        }
        if (pred.seq_limits) {  // (uniform)
            const uint32_t h = inside ? rows.hi[row] : 0u, l = inside ? rows.lo[row] : 0u;
            const uint32_t gc = (uint32_t)__popc(h & pred.region);
            pass = pass && gc >= pred.gc_min && gc <= pred.gc_max && self_select_run(~h & l & pred.region) <= pred.max_t_run;
        }
        unsigned long long key = ~e;
        if (MODEL) {
            const double s = inside ? rows.model[row] : 0.0;
            if (pred.has_min) pass = pass && s >= pred.min_sum;  // (uniform; false for a NaN)
            if (pred.rank_model) {                                // (uniform)
                pass = pass && s == s;
                key = self_select_model_key(s);
            }
        }
        if (track.flags && pass) pass = self_select_cds(cut, track);
        n_in += (uint32_t)__popcll(__ballot(inside));
        n_pass += (uint32_t)__popcll(__ballot(pass));
        sel_insert(mine, lane, k, pass, key, cut << 1 | strand, (uint32_t)row);
    }
    if (it.slot == SELECT_NONE) {
        if (lane < k) res.sel[(uint64_t)it.gene * k + lane] = mine.row;
        if (lane == 0) {
            res.n_in[it.gene] = n_in;
            res.n_pass[it.gene] = n_pass;
        }
    } else {
        if (lane < k) {
            const uint64_t at = (uint64_t)it.slot * k + lane;
            part.key[at] = mine.key;
            part.tie[at] = mine.tie;
            part.row[at] = mine.row;
        }
        if (lane == 0) {
            part.cnt[2 * (uint64_t)it.slot] = n_in;
            part.cnt[2 * (uint64_t)it.slot + 1] = n_pass;
        }
    }
}

__global__ __launch_bounds__(BLOCK) void select_self_gather_kernel(SelfSelectRows rows, const uint32_t *__restrict__ sel, uint64_t n_entries,
                                                                   SelfSelectGathered out)
{
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_entries) return;
    const uint32_t c = sel[i];
    const bool have = c != SELECT_NONE && c < rows.n;
    const uint32_t p = have ? rows.pos[c] : SELECT_NONE;
    out.pos[i] = have ? (p & 0x7fffffffu) : SELECT_NONE;
    out.strand[i] = have ? (uint8_t)(p >> 31) : (uint8_t)0xFF;
    out.hi[i] = have ? rows.hi[c] : SELECT_NONE;
    out.lo[i] = have ? rows.lo[c] : SELECT_NONE;
    for (uint32_t j = 0; j < rows.stride; ++j) out.counts[i * rows.stride + j] = have ? rows.counts[(uint64_t)c * rows.stride + j] : SELECT_NONE;
    out.sum[i] = have && rows.sum ? rows.sum[c] : ~0ull;
    out.model[i] = have && rows.model ? rows.model[c] : __longlong_as_double(0x7ff8000000000000ll);
}

}  // namespace

hipError_t launch_select_self_bounds(hipStream_t s, const uint32_t *cand_pos, uint32_t n_cand, uint32_t T, const uint32_t *lo, const uint32_t *hi,
                                     uint32_t n_genes, uint2 *run)
{
    if (!n_genes) return hipSuccess;
    hipLaunchKernelGGL(select_self_bounds_kernel, dim3((n_genes + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, cand_pos, n_cand, T, lo, hi, n_genes,
                       run);
    return hipGetLastError();
}

hipError_t launch_select_self_items(hipStream_t s, const SelfSelectRows &rows, const SelfSelectTrack &track, const SelfSelectPredicate &pred,
                                    const uint32_t *gene_lo, const uint32_t *gene_hi, const SelectItem *items, uint32_t n_items,
                                    const SelectPartials &part, const SelectResult &res, bool model)
{
    if (!n_items) return hipSuccess;
    const dim3 grid((n_items + SELECT_WAVES - 1) / SELECT_WAVES);
    if (model)
        hipLaunchKernelGGL(select_self_items_kernel<true>, grid, dim3(BLOCK), 0, s, rows, track, pred, gene_lo, gene_hi, items, n_items, part,
                           res);
    else
        hipLaunchKernelGGL(select_self_items_kernel<false>, grid, dim3(BLOCK), 0, s, rows, track, pred, gene_lo, gene_hi, items, n_items, part,
                           res);
    return hipGetLastError();
}

hipError_t launch_select_self_gather(hipStream_t s, const SelfSelectRows &rows, const uint32_t *sel, uint64_t n_entries,
                                     const SelfSelectGathered &out)
{
    if (!n_entries) return hipSuccess;
    hipLaunchKernelGGL(select_self_gather_kernel, dim3((uint32_t)((n_entries + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, rows, sel, n_entries,
                       out);
    return hipGetLastError();
}

}  // namespace crp
