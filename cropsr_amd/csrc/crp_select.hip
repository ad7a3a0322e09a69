// crp_select.hip -- guide selection on the device: for every gene, the K best-scoring rows of
// the resident hit tables whose cut site lies in the gene and that pass the thresholds (include/cropsr_hip.h,
// crp_select_run, states the definition).  A segmented top-K over runs of the two tables:
//
//   bounds   one lane per gene: the tables ascend in position, so a gene's rows are one run per strand -- four binary
//            searches over the two position columns ('+': on pos - 3, the cut site)
//   select   one WAVE per work item (a gene's runs, cut by the host into pieces of at most slice_rows rows): 64 rows a
//            trip, coalesced; the wave keeps its current top K SORTED ACROSS ITS LANES -- lane r holds the r-th best
//            entry (key = the score's bits, tie = cut site << 1 | strand, the packed row).  A row that beats lane
//            K - 1's entry is inserted: its entry is broadcast, every lane compares it with its own, the lanes behind
//            the insertion point take their neighbour's entry (one wave shift).  No LDS, no atomics, no scratch;
//            after the first trips inserts are rare (~K ln(n / K) per item)
//   merge    one wave per gene that was cut into several items: the same insertion over the items' partial lists
//
// The order (higher key, then smaller tie) is total, so the K best do not depend on how the rows were cut.  Every
// result slot has one owner and is written with plain vector stores.
#include "crp_kernels.h"
#include "crp_select.h"
#include "crp_select_insert.h"

namespace crp {

static_assert(BLOCK == SELECT_WAVES * 64, "one wave of 64 lanes per work item");

__global__ __launch_bounds__(BLOCK) void select_bounds_kernel(const uint32_t *__restrict__ pos_plus, uint32_t n_plus,
                                                              const uint32_t *__restrict__ pos_minus, uint32_t n_minus,
                                                              const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi,
                                                              uint32_t n_genes, uint4 *__restrict__ bounds)
{
    const uint32_t g = blockIdx.x * BLOCK + threadIdx.x;
    if (g >= n_genes) return;
    uint32_t out[4];
    for (int q = 0; q < 4; ++q) {
        const bool minus = q >= 2;
        const uint32_t *pos = minus ? pos_minus : pos_plus;
        // q even: the first row with cut site >= lo; q odd: the first with cut site > hi ('+': cut site = pos - 3)
        const uint64_t key = (uint64_t)((q & 1) ? hi[g] : lo[g]) + (minus ? 0u : 3u) + (q & 1);
        uint32_t a = 0, b = minus ? n_minus : n_plus;
        while (a < b) {
            const uint32_t mid = a + ((b - a) >> 1);
            if (pos[mid] < key) a = mid + 1;
            else b = mid;
        }
        out[q] = a;
    }
    bounds[g] = make_uint4(out[0], out[1], out[2], out[3]);
}

// (8 waves per SIMD, said out loud: with the repair column's pointers and limits among its arguments the kernel would take
// 103 SGPRs and run at 7, which cost 5-7 % on the plain selection; held to 96 the compiler keeps 24 of them in VGPR lanes --
// 23 VGPRs, no scratch -- and the time is the one of before: profiles/EXPERIMENTS.md, "Repair outcome")
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8))) void select_items_kernel(SelectTable plus, SelectTable minus,
                                                                                                        SelectPredicate pred,
                                                             const SelectItem *__restrict__ items, uint32_t n_items,
                                                             SelectPartials part, SelectResult res)
{
    const uint32_t item = blockIdx.x * SELECT_WAVES + (threadIdx.x >> 6);  // (uniform per wave)
    if (item >= n_items) return;
    const int lane = threadIdx.x & 63;
    const SelectItem it = items[item];
    const int k = pred.k;
    SelEntry mine{0ull, SELECT_NONE, SELECT_NONE};  // (worse than every row: a row's tie is below 2^32 - 1)
    uint32_t n_in = 0, n_pass = 0;
    for (int s = 0; s < 2; ++s) {
        const SelectTable t = s ? minus : plus;
        const uint32_t back = s ? 0u : 3u;
        // (the item's rows lie inside the table: crp_select.cpp cuts them from the bounds kernel's runs and checks them)
        const uint32_t end = it.first[s] + it.rows[s];
        for (uint32_t r0 = it.first[s]; r0 < end; r0 += 64) {
            const uint32_t row = r0 + lane;
            const bool in = row < end;
            const double score = in ? t.score[row] : -1.0;
            const uint32_t cut = in ? t.pos[row] - back : 0u;
            const bool scored = in && score != -1.0;  // an unscored row has no cut site: in no gene
#include "crp_select_predicate.inc"
            n_in += (uint32_t)__popcll(__ballot(scored));
            n_pass += (uint32_t)__popcll(__ballot(pass));
            sel_insert(mine, lane, k, pass, (unsigned long long)__double_as_longlong(score), cut << 1 | (uint32_t)s,
                       row | (uint32_t)s << 31);
        }
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

__global__ __launch_bounds__(BLOCK) void select_merge_kernel(const SelectMerge *__restrict__ genes, uint32_t n_genes, int k,
                                                             SelectPartials part, SelectResult res)
{
    const uint32_t m = blockIdx.x * SELECT_WAVES + (threadIdx.x >> 6);
    if (m >= n_genes) return;
    const int lane = threadIdx.x & 63;
    const SelectMerge g = genes[m];
    SelEntry mine{0ull, SELECT_NONE, SELECT_NONE};
    uint32_t n_in = 0, n_pass = 0;
    for (uint32_t j = 0; j < g.n_slots; ++j) {
        const uint64_t slot = (uint64_t)g.slot + j;
        const bool in = lane < k;
        const uint64_t at = slot * k + lane;
        const unsigned long long key = in ? part.key[at] : 0ull;
        const uint32_t tie = in ? part.tie[at] : SELECT_NONE;
        const uint32_t row = in ? part.row[at] : SELECT_NONE;
        n_in += part.cnt[2 * slot];
        n_pass += part.cnt[2 * slot + 1];
        sel_insert(mine, lane, k, row != SELECT_NONE, key, tie, row);
    }
    if (lane < k) res.sel[(uint64_t)g.gene * k + lane] = mine.row;
    if (lane == 0) {
        res.n_in[g.gene] = n_in;
        res.n_pass[g.gene] = n_pass;
    }
}

hipError_t launch_select_bounds(hipStream_t s, const uint32_t *pos_plus, uint32_t n_plus, const uint32_t *pos_minus, uint32_t n_minus,
                                const uint32_t *lo, const uint32_t *hi, uint32_t n_genes, uint4 *bounds)
{
    if (!n_genes) return hipSuccess;
    hipLaunchKernelGGL(select_bounds_kernel, dim3((n_genes + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, pos_plus, n_plus, pos_minus, n_minus,
                       lo, hi, n_genes, bounds);
    return hipGetLastError();
}

hipError_t launch_select_items(hipStream_t s, const SelectTable &plus, const SelectTable &minus, const SelectPredicate &pred,
                               const SelectItem *items, uint32_t n_items, const SelectPartials &part, const SelectResult &res)
{
    if (!n_items) return hipSuccess;
    hipLaunchKernelGGL(select_items_kernel, dim3((n_items + SELECT_WAVES - 1) / SELECT_WAVES), dim3(BLOCK), 0, s, plus, minus, pred, items,
                       n_items, part, res);
    return hipGetLastError();
}

hipError_t launch_select_merge(hipStream_t s, const SelectMerge *genes, uint32_t n_genes, int k, const SelectPartials &part,
                               const SelectResult &res)
{
    if (!n_genes) return hipSuccess;
    hipLaunchKernelGGL(select_merge_kernel, dim3((n_genes + SELECT_WAVES - 1) / SELECT_WAVES), dim3(BLOCK), 0, s, genes, n_genes, k, part,
                       res);
    return hipGetLastError();
}

}  // namespace crp
