// crp_select_pairs.hip -- guide pairs on the device: for every gene, the KP best pairs of passing
// rows whose cut boundaries lie dmin .. dmax apart (include/cropsr_hip.h, crp_select_run_pairs, states the definition).
// A segmented top-K over PAIRS of rows, whose key -- the smaller of two scores -- cannot be sorted in advance:
//
//   pass key  one lane per table row: the predicate of the selection (crp_select_predicate.inc -- the very text
//             select_items_kernel's row loop includes) does not depend on the gene, so it is evaluated once per row into an
//             8-byte column per strand: the score's bits where the row passes, else 0
//   bounds    select_bounds_kernel's runs, as they are
//   pairs     one WAVE per work item (a gene's a-rows, cut by the host into pieces of at most pair_slice_rows rows).
//             64 a-rows a trip: every lane loads its row's position and pass key and finds its partner runs by binary
//             search -- per partner table the rows with c_b in [c_a + dmin, c_a + dmax] inside the gene's run, contiguous
//             because the tables ascend.  The wave then takes its passing a-rows one at a time (readlane) and streams
//             the row's partner runs 64 rows a trip, coalesced, 12 bytes a partner; qualifying partners are counted
//             from a ballot and offered to the wave's top-KP list, which is crp_select.hip's structure with a wider
//             entry: sorted across the lanes, a threshold check against lane KP - 1 before any insert, one wave shift an
//             insert.  No LDS, no atomics, no scratch
//   merge     one wave per gene that was cut into several items: the same insertion over the items' partial lists
//
// The order is total, so the KP best do not depend on how the a-rows were cut.  Every result slot has one owner and is
// written with plain vector stores.
#include "crp_kernels.h"
#include "crp_select.h"

namespace crp {

namespace {

struct PairEntry {
    unsigned long long kmin, kmax, tie;  // tie = c_a << 32 | c_b
    uint32_t a, b;                       // row | strand << 31
};

// the order of the definition: higher min score, higher max score, smaller c_a, smaller c_b, smaller strand bits
__device__ __forceinline__ bool pair_better(const PairEntry &x, const PairEntry &y)
{
    if (x.kmin != y.kmin) return x.kmin > y.kmin;
    if (x.kmax != y.kmax) return x.kmax > y.kmax;
    if (x.tie != y.tie) return x.tie < y.tie;
    return (x.a >> 31) * 2u + (x.b >> 31) < (y.a >> 31) * 2u + (y.b >> 31);
}

__device__ __forceinline__ uint32_t pair_lane32(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }
__device__ __forceinline__ unsigned long long pair_lane64(unsigned long long v, int l)
{
    return (unsigned long long)pair_lane32((uint32_t)(v >> 32), l) << 32 | pair_lane32((uint32_t)v, l);
}
__device__ __forceinline__ PairEntry pair_lane(const PairEntry &e, int l)
{
    return PairEntry{pair_lane64(e.kmin, l), pair_lane64(e.kmax, l), pair_lane64(e.tie, l), pair_lane32(e.a, l), pair_lane32(e.b, l)};
}

// No entry: worse than every pair (a pair's kmin is a passing score's bits, above 0).
__device__ __forceinline__ PairEntry pair_none() { return PairEntry{0ull, 0ull, ~0ull, SELECT_NONE, SELECT_NONE}; }

// Inserts the lanes' candidates (want: this lane has one) into the wave's sorted list, best first.  All 64 lanes call
// it together.  Lanes >= k also hold (worse) entries; only lane k - 1 decides what gets in.
__device__ __forceinline__ void pair_insert(PairEntry &mine, int lane, int k, bool want, const PairEntry &cand)
{
    PairEntry thr = pair_lane(mine, k - 1);
    unsigned long long mask = __ballot(want && pair_better(cand, thr));
    while (mask) {
        const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)mask) - 1);
        mask &= mask - 1;
        const PairEntry c = pair_lane(cand, l);
        if (!pair_better(c, thr)) continue;  // (the bar has risen since the ballot)
        // the list is sorted: the lanes whose entry the candidate beats are a suffix; its first lane takes the
        // candidate, the others their neighbour's entry
        const PairEntry up{__shfl_up(mine.kmin, 1), __shfl_up(mine.kmax, 1), __shfl_up(mine.tie, 1), __shfl_up(mine.a, 1),
                           __shfl_up(mine.b, 1)};
        if (pair_better(c, mine)) mine = (lane > 0 && pair_better(c, up)) ? up : c;
        thr = pair_lane(mine, k - 1);
    }
}

// the first row in [a, b) whose position is >= key (b when there is none)
__device__ __forceinline__ uint32_t pair_lower_bound(const uint32_t *__restrict__ pos, uint32_t a, uint32_t b, long long key)
{
    while (a < b) {
        const uint32_t mid = a + ((b - a) >> 1);
        if ((long long)pos[mid] < key) a = mid + 1;
        else b = mid;
    }
    return a;
}

}  // namespace

__global__ __launch_bounds__(BLOCK) void pair_pass_key_kernel(SelectTable t, SelectPredicate pred, unsigned long long *__restrict__ key)
{
    const uint32_t row = blockIdx.x * BLOCK + threadIdx.x;
    if (row >= t.n) return;
    const bool in = true;
    const double score = t.score[row];
    const bool scored = score != -1.0;
#include "crp_select_predicate.inc"
    key[row] = pass ? (unsigned long long)__double_as_longlong(score) : 0ull;
}

__global__ __launch_bounds__(BLOCK) void pair_items_kernel(const uint32_t *__restrict__ pos_plus, const uint32_t *__restrict__ pos_minus,
                                                           const unsigned long long *__restrict__ key_plus,
                                                           const unsigned long long *__restrict__ key_minus, PairParams pp,
                                                           const PairItem *__restrict__ items, uint32_t n_items,
                                                           unsigned long long *__restrict__ evals, PairPartials part, PairResult res)
{
    const uint32_t item = blockIdx.x * SELECT_WAVES + (threadIdx.x >> 6);  // (uniform per wave)
    if (item >= n_items) return;
    const int lane = threadIdx.x & 63;
    const PairItem it = items[item];
    const int k = pp.k;
    PairEntry mine = pair_none();
    uint32_t n_pass = 0;
    unsigned long long n_pairs = 0, n_evals = 0;
    for (int s = 0; s < 2; ++s) {
        const uint32_t *pos_a = s ? pos_minus : pos_plus;
        const unsigned long long *key_a = s ? key_minus : key_plus;
        // the cut boundary c of a row (repair.py): '+' i - 3, '-' j + 6
        const uint32_t off_a = s ? 6u : (uint32_t)-3;
        // (the item's rows lie inside the table and inside the gene's runs: crp_select.cpp cuts them from the bounds
        // kernel's runs and checks those against the tables)
        const uint32_t end = it.first[s] + it.rows[s];
        for (uint32_t r0 = it.first[s]; r0 < end; r0 += 64) {
            const uint32_t row = r0 + lane;
            const bool in = row < end;
            const unsigned long long ka = in ? key_a[row] : 0ull;
            const uint32_t ca = in ? pos_a[row] + off_a : 0u;
            // this lane's partner runs: rows [p0, p1) of table tb, inside the gene's run of that table
            uint32_t p0[2], p1[2];
#pragma unroll
            for (int tb = 0; tb < 2; ++tb) {
                const bool allowed = ka != 0ull && (pp.mask >> (s * 2 + tb) & 1u);
                const uint32_t *pos_b = tb ? pos_minus : pos_plus;
                const long long back = tb ? 6 : -3;  // pos_b = c_b - back
                p0[tb] = allowed ? pair_lower_bound(pos_b, it.run[2 * tb], it.run[2 * tb + 1], (long long)ca + pp.dmin - back) : 0u;
                p1[tb] = allowed ? pair_lower_bound(pos_b, p0[tb], it.run[2 * tb + 1], (long long)ca + pp.dmax - back + 1) : 0u;
            }
            n_pass += (uint32_t)__popcll(__ballot(ka != 0ull));
            unsigned long long todo = __ballot(p1[0] > p0[0] || p1[1] > p0[1]);
            while (todo) {
                const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
                todo &= todo - 1;
                const unsigned long long uka = pair_lane64(ka, l);
                const uint32_t uca = pair_lane32(ca, l);
                const uint32_t ua = (r0 + (uint32_t)l) | (uint32_t)s << 31;
#pragma unroll
                for (int tb = 0; tb < 2; ++tb) {
                    const uint32_t *pos_b = tb ? pos_minus : pos_plus;
                    const unsigned long long *key_b = tb ? key_minus : key_plus;
                    const uint32_t off_b = tb ? 6u : (uint32_t)-3;
                    const uint32_t q0 = pair_lane32(p0[tb], l), q1 = pair_lane32(p1[tb], l);
                    n_evals += q1 - q0;
                    for (uint32_t q = q0; q < q1; q += 64) {
                        const uint32_t rb = q + lane;
                        const bool inb = rb < q1;
                        const unsigned long long kb = inb ? key_b[rb] : 0ull;
                        const uint32_t cb = inb ? pos_b[rb] + off_b : 0u;
                        // (the run's rows have dmin <= c_b - c_a <= dmax by the searches)
                        const bool ok = kb != 0ull && !(pp.frameshift && (cb - uca) % 3u == 0u);
                        const unsigned long long any = __ballot(ok);
                        if (!any) continue;  // (wave-uniform: a trip without a qualifying partner reads no bar)
                        n_pairs += (unsigned long long)__popcll(any);
                        const PairEntry cand{uka < kb ? uka : kb, uka < kb ? kb : uka, (unsigned long long)uca << 32 | cb, ua,
                                             rb | (uint32_t)tb << 31};
                        pair_insert(mine, lane, k, ok, cand);
                    }
                }
            }
        }
    }
    if (lane == 0) evals[item] = n_evals;
    if (it.slot == SELECT_NONE) {
        if (lane < k) {
            const uint64_t at = ((uint64_t)it.gene * k + lane) * 2;
            res.pairs[at] = mine.a;
            res.pairs[at + 1] = mine.b;
        }
        if (lane == 0) {
            res.n_pass[it.gene] = n_pass;
            res.n_pairs[it.gene] = n_pairs;
        }
    } else {
        if (lane < k) {
            const uint64_t at = (uint64_t)it.slot * k + lane;
            part.kmin[at] = mine.kmin;
            part.kmax[at] = mine.kmax;
            part.tie[at] = mine.tie;
            part.a[at] = mine.a;
            part.b[at] = mine.b;
        }
        if (lane == 0) {
            part.n_pass[it.slot] = n_pass;
            part.n_pairs[it.slot] = n_pairs;
        }
    }
}

__global__ __launch_bounds__(BLOCK) void pair_merge_kernel(const SelectMerge *__restrict__ genes, uint32_t n_genes, int k, PairPartials part,
                                                           PairResult res)
{
    const uint32_t m = blockIdx.x * SELECT_WAVES + (threadIdx.x >> 6);
    if (m >= n_genes) return;
    const int lane = threadIdx.x & 63;
    const SelectMerge g = genes[m];
    PairEntry mine = pair_none();
    uint32_t n_pass = 0;
    unsigned long long n_pairs = 0;
    for (uint32_t j = 0; j < g.n_slots; ++j) {
        const uint64_t slot = (uint64_t)g.slot + j;
        const uint64_t at = slot * k + lane;
        PairEntry cand = pair_none();
        if (lane < k) cand = PairEntry{part.kmin[at], part.kmax[at], part.tie[at], part.a[at], part.b[at]};
        n_pass += part.n_pass[slot];
        n_pairs += part.n_pairs[slot];
        pair_insert(mine, lane, k, cand.a != SELECT_NONE, cand);
    }
    if (lane < k) {
        const uint64_t at = ((uint64_t)g.gene * k + lane) * 2;
        res.pairs[at] = mine.a;
        res.pairs[at + 1] = mine.b;
    }
    if (lane == 0) {
        res.n_pass[g.gene] = n_pass;
        res.n_pairs[g.gene] = n_pairs;
    }
}

hipError_t launch_pair_pass_key(hipStream_t s, const SelectTable &table, const SelectPredicate &pred, unsigned long long *key)
{
    if (!table.n) return hipSuccess;
    hipLaunchKernelGGL(pair_pass_key_kernel, dim3((table.n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, table, pred, key);
    return hipGetLastError();
}

hipError_t launch_pair_items(hipStream_t s, const uint32_t *pos_plus, const uint32_t *pos_minus, const unsigned long long *key_plus,
                             const unsigned long long *key_minus, const PairParams &pp, const PairItem *items, uint32_t n_items,
                             unsigned long long *evals, const PairPartials &part, const PairResult &res)
{
    if (!n_items) return hipSuccess;
    hipLaunchKernelGGL(pair_items_kernel, dim3((n_items + SELECT_WAVES - 1) / SELECT_WAVES), dim3(BLOCK), 0, s, pos_plus, pos_minus, key_plus,
                       key_minus, pp, items, n_items, evals, part, res);
    return hipGetLastError();
}

hipError_t launch_pair_merge(hipStream_t s, const SelectMerge *genes, uint32_t n_genes, int k, const PairPartials &part,
                             const PairResult &res)
{
    if (!n_genes) return hipSuccess;
    hipLaunchKernelGGL(pair_merge_kernel, dim3((n_genes + SELECT_WAVES - 1) / SELECT_WAVES), dim3(BLOCK), 0, s, genes, n_genes, k, part, res);
    return hipGetLastError();
}

}  // namespace crp
