// crp_select_family.hip -- the guide selection with family limits, and the family values of given (gene, row) pairs
// (DESIGN.md section 23).  The kernels of crp_select.hip are held to their assembly, so the selection's row loop stands
// here once more with the family terms behind its predicate, as it does in crp_select_coding.hip:
//
//   select   select_items_kernel's wave per work item, 64 rows a trip, the same sorted list across the lanes
//            (crp_select_insert.h) and the same partial lists, which select_merge_kernel merges as they are.  The item's
//            gene is wave-uniform, and so are its family and that family's size.  A lane that has passed everything else
//            reads its row's family columns and compares integers.
//   eval     one lane per (gene, row) query, the same function.
//
// No LDS, no atomics, no scratch; every result slot has one owner and is written with plain vector stores.
#include "crp_kernels.h"
#include "crp_select_family.h"
#include "crp_select_insert.h"

namespace crp {

static_assert(BLOCK == SELECT_WAVES * 64, "one wave of 64 lanes per work item");

__global__ __launch_bounds__(BLOCK) void select_items_family_kernel(SelectTable plus, SelectTable minus, SelectPredicate pred, SelectFamily fam,
                                                                    FamilyLimits lim, const SelectItem *__restrict__ items, uint32_t n_items,
                                                                    SelectPartials part, SelectResult res)
{
    const uint32_t item = blockIdx.x * SELECT_WAVES + (threadIdx.x >> 6);  // (uniform per wave)
    if (item >= n_items) return;
    const int lane = threadIdx.x & 63;
    const SelectItem it = items[item];
    const int k = pred.k;
    // the gene's family: uniform per wave
    const uint32_t gene_family = fam.gene_family[it.gene];
    const uint32_t need = lim.min_members == SELECT_ALL_MEMBERS ? fam.gene_size[it.gene] : lim.min_members;
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
            if (pass) {  // (the predicate has seen the joined columns: the row is joined)
                const FamilyValues v = family_values(fam, s, row, gene_family);
                pass = v.outside_mm0 <= lim.max_mm0_outside && v.outside_sum <= lim.max_hit_sum_outside && v.members_hit >= need;
            }
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

__global__ __launch_bounds__(BLOCK) void family_eval_kernel(SelectFamily fam, const uint32_t *__restrict__ gene_row,
                                                            const uint32_t *__restrict__ packed_row, uint32_t n,
                                                            uint32_t *__restrict__ outside_mm0, unsigned long long *__restrict__ outside_sum,
                                                            uint32_t *__restrict__ members_hit, uint32_t *__restrict__ family_size,
                                                            unsigned long long *__restrict__ cover)
{
    const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
    if (q >= n) return;
    const uint32_t g = gene_row[q], packed = packed_row[q];
    const FamilyValues v = family_values(fam, (int)(packed >> 31), packed & 0x7FFFFFFFu, fam.gene_family[g]);
    outside_mm0[q] = v.outside_mm0;
    outside_sum[q] = v.outside_sum;
    members_hit[q] = v.members_hit;
    family_size[q] = fam.gene_size[g];
    cover[q] = v.cover;
}

hipError_t launch_select_items_family(hipStream_t s, const SelectTable &plus, const SelectTable &minus, const SelectPredicate &pred,
                                      const SelectFamily &fam, const FamilyLimits &lim, const SelectItem *items, uint32_t n_items,
                                      const SelectPartials &part, const SelectResult &res)
{
    if (!n_items) return hipSuccess;
    hipLaunchKernelGGL(select_items_family_kernel, dim3((n_items + SELECT_WAVES - 1) / SELECT_WAVES), dim3(BLOCK), 0, s, plus, minus, pred, fam, lim,
                       items, n_items, part, res);
    return hipGetLastError();
}

hipError_t launch_family_eval(hipStream_t s, const SelectFamily &fam, const uint32_t *gene_row, const uint32_t *packed_row, uint32_t n,
                              uint32_t *outside_mm0, unsigned long long *outside_sum, uint32_t *members_hit, uint32_t *family_size,
                              unsigned long long *cover)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(family_eval_kernel, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, fam, gene_row, packed_row, n, outside_mm0, outside_sum,
                       members_hit, family_size, cover);
    return hipGetLastError();
}

}  // namespace crp
