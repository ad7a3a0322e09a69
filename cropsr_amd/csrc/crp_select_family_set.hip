// crp_select_family_set.hip -- one greedy step of the family sets: for every gene family the
// candidate -- a passing row of a member gene -- that covers the most members not covered yet.
//
//   step   select_items_family_kernel's wave per work item and its row loop: 64 rows a trip, crp_select_predicate.inc
//          included as text, then the family limits.  Where that kernel keeps a sorted list of K entries across the
//          lanes, this one keeps one running best per lane -- (gain, key, tie), the item's gene is wave-uniform -- and
//          reduces the 64 of them once, at the end of the item.  The family's `covered` word is wave-uniform.
//   pick   one wave per family over the proposals of that family's items (a CSR list from the host), the same order
//          with the layout row as its last term.
//
// No LDS, no atomics, no scratch; every slot has one owner and is written by lane 0 with plain vector stores.
#include "crp_kernels.h"
#include "crp_select_family_set.h"

namespace crp {

static_assert(BLOCK == SELECT_WAVES * 64, "one wave of 64 lanes per work item");
static_assert(sizeof(FamilyProposal) == 32, "the layout of crp_family_step_best");

namespace {

// the wave's best proposal, in every lane
__device__ __forceinline__ FamilyProposal wave_best(FamilyProposal mine)
{
    for (int off = 32; off > 0; off >>= 1) {
        FamilyProposal o;
        o.key = __shfl_xor(mine.key, off);
        o.cover = __shfl_xor(mine.cover, off);
        o.gain = __shfl_xor(mine.gain, off);
        o.tie = __shfl_xor(mine.tie, off);
        o.row = __shfl_xor(mine.row, off);
        o.gene = __shfl_xor(mine.gene, off);
        if (set_better(o.gain, o.key, o.tie, o.gene, mine.gain, mine.key, mine.tie, mine.gene)) mine = o;
    }
    return mine;
}

}  // namespace

__global__ __launch_bounds__(BLOCK) void family_set_step_kernel(SelectTable plus, SelectTable minus, SelectPredicate pred, SelectFamily fam,
                                                                FamilyLimits lim, const uint32_t *__restrict__ gene_member,
                                                                const unsigned long long *__restrict__ covered,
                                                                const SelectItem *__restrict__ items, uint32_t n_items,
                                                                FamilyProposal *__restrict__ prop)
{
    const uint32_t item = blockIdx.x * SELECT_WAVES + (threadIdx.x >> 6);  // (uniform per wave)
    if (item >= n_items) return;
    const int lane = threadIdx.x & 63;
    const SelectItem it = items[item];
    // the gene's family, its own bit and what the family has covered so far: uniform per wave
    const uint32_t gene_family = fam.gene_family[it.gene];
    const uint32_t need = lim.min_members == SELECT_ALL_MEMBERS ? fam.gene_size[it.gene] : lim.min_members;
    const unsigned long long own = 1ull << (gene_member[it.gene] & 63u);
    const unsigned long long open = ~covered[gene_family];
    FamilyProposal mine{0ull, 0ull, 0u, SELECT_NONE, SELECT_NONE, it.gene};
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
                if (v.outside_mm0 <= lim.max_mm0_outside && v.outside_sum <= lim.max_hit_sum_outside && v.members_hit >= need) {
                    const unsigned long long c = v.cover | own;  // (the row cuts inside the gene: its own bit is always in)
                    const uint32_t gain = (uint32_t)__popcll(c & open);
                    const unsigned long long key = (unsigned long long)__double_as_longlong(score);
                    const uint32_t tie = cut << 1 | (uint32_t)s;
                    if (gain && set_better(gain, key, tie, 0u, mine.gain, mine.key, mine.tie, 0u)) {
                        mine.gain = gain;
                        mine.key = key;
                        mine.tie = tie;
                        mine.row = row | (uint32_t)s << 31;
                        mine.cover = c;
                    }
                }
            }
        }
    }
    mine = wave_best(mine);
    if (lane == 0) prop[item] = mine;
}

__global__ __launch_bounds__(BLOCK) void family_set_pick_kernel(const FamilyProposal *__restrict__ prop, const uint32_t *__restrict__ start,
                                                                const uint32_t *__restrict__ slots, uint32_t n_families,
                                                                FamilyProposal *__restrict__ best)
{
    const uint32_t f = blockIdx.x * SELECT_WAVES + (threadIdx.x >> 6);  // (uniform per wave)
    if (f >= n_families) return;
    const int lane = threadIdx.x & 63;
    FamilyProposal mine{0ull, 0ull, 0u, SELECT_NONE, SELECT_NONE, SELECT_NONE};
    const uint32_t end = start[f + 1];
    for (uint32_t i = start[f] + lane; i < end; i += 64) {
        const FamilyProposal p = prop[slots[i]];
        if (p.gain && set_better(p.gain, p.key, p.tie, p.gene, mine.gain, mine.key, mine.tie, mine.gene)) mine = p;
    }
    mine = wave_best(mine);
    if (lane == 0) best[f] = mine;
}

hipError_t launch_family_set_step(hipStream_t s, const SelectTable &plus, const SelectTable &minus, const SelectPredicate &pred,
                                  const SelectFamily &fam, const FamilyLimits &lim, const uint32_t *gene_member,
                                  const unsigned long long *covered, const SelectItem *items, uint32_t n_items, FamilyProposal *prop)
{
    if (!n_items) return hipSuccess;
    hipLaunchKernelGGL(family_set_step_kernel, dim3((n_items + SELECT_WAVES - 1) / SELECT_WAVES), dim3(BLOCK), 0, s, plus, minus, pred, fam, lim,
                       gene_member, covered, items, n_items, prop);
    return hipGetLastError();
}

hipError_t launch_family_set_pick(hipStream_t s, const FamilyProposal *prop, const uint32_t *start, const uint32_t *slots,
                                  uint32_t n_families, FamilyProposal *best)
{
    if (!n_families) return hipSuccess;
    hipLaunchKernelGGL(family_set_pick_kernel, dim3((n_families + SELECT_WAVES - 1) / SELECT_WAVES), dim3(BLOCK), 0, s, prop, start, slots,
                       n_families, best);
    return hipGetLastError();
}

}  // namespace crp
