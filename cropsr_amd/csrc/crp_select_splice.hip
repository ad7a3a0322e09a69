// crp_select_splice.hip -- the guide selection for base editors that destroy a splice site, and the splice outcome of given
// (gene, row) pairs.  The kernels of crp_select.hip, crp_select_pairs.hip, crp_select_coding.hip and
// crp_select_edit.hip are held to their assembly, so the selection's row loop stands here once more with the splice test
// as its predicate's last term:
//
//   select   select_items_edit_kernel's wave per work item, 64 rows a trip, the same sorted list across the lanes
//            (crp_select_insert.h) and the same partial lists, which select_merge_kernel merges as they are.  The item's
//            gene is wave-uniform, and so are the slice of its steps, L_P, the info word, the window, the editor, both sets
//            of limits and the planes' bounds.  A lane that has passed everything cheaper runs splice_outcome
//            (crp_splice.h) on its row: at most two words of each of three planes, and only where the letters make a
//            destroyed site possible one binary search over the gene's change points and a short walk forward.  With edit
//            limits set as well a row that fails the splice test may still pass by edit_outcome / edit_pass (crp_edit.h).
//   eval     one lane per (gene, row) query, the same function.
//
// No LDS, no atomics, no scratch; every result slot has one owner and is written with plain vector stores.
#include "crp_kernels.h"
#include "crp_select_insert.h"
#include "crp_select_splice.h"

namespace crp {

static_assert(BLOCK == SELECT_WAVES * 64, "one wave of 64 lanes per work item");

__global__ __launch_bounds__(BLOCK) void select_items_splice_kernel(SelectTable plus, SelectTable minus, SelectPredicate pred, SelectCoding cod,
                                                                    EditPlanes planes, SpliceTest test, const SelectItem *__restrict__ items,
                                                                    uint32_t n_items, SelectPartials part, SelectResult res)
{
    const uint32_t item = blockIdx.x * SELECT_WAVES + (threadIdx.x >> 6);  // (uniform per wave)
    if (item >= n_items) return;
    const int lane = threadIdx.x & 63;
    const SelectItem it = items[item];
    const int k = pred.k;
    // the gene's model: uniform per wave
    const uint32_t step0 = cod.first[it.gene], n_steps = cod.first[it.gene + 1] - step0;
    const uint32_t L = cod.length[it.gene], info = cod.info[it.gene];
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
            if (pass) {  // the row's match index: the cut site plus 3 on the '+' table, the cut site itself on the '-' table
                const SpliceOutcome o = splice_outcome(planes, cod.at + step0, cod.word + step0, cod.cum + step0, n_steps, L, info, cut + back, s != 0,
                                                       test.window, test.editor);
                pass = splice_pass(o, L, test.splice);
                if (!pass && test.with_stop) {  // the alternative, under its own limits
                    const EditOutcome e = edit_outcome(planes, cod.at + step0, cod.word + step0, cod.cum + step0, n_steps, L, info, cut + back, s != 0,
                                                       test.window);
                    pass = edit_pass(e, L, test.stop);
                }
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

__global__ __launch_bounds__(BLOCK) void splice_eval_kernel(const uint32_t *__restrict__ pos_plus, const uint32_t *__restrict__ pos_minus,
                                                            SelectCoding cod, EditPlanes planes, EditWindow win, uint32_t editor,
                                                            const uint32_t *__restrict__ gene_row, const uint32_t *__restrict__ packed_row, uint32_t n,
                                                            uint32_t *__restrict__ counts, uint32_t *__restrict__ off)
{
    const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
    if (q >= n) return;
    const uint32_t g = gene_row[q], packed = packed_row[q], row = packed & 0x7FFFFFFFu;
    const bool minus = packed >> 31;
    const uint32_t pos = minus ? pos_minus[row] : pos_plus[row];
    const uint32_t step0 = cod.first[g];
    const SpliceOutcome o = splice_outcome(planes, cod.at + step0, cod.word + step0, cod.cum + step0, cod.first[g + 1] - step0, cod.length[g],
                                           cod.info[g], pos, minus, win, editor);
    counts[q] = o.targets | o.donors << 8 | o.acceptors << 16;
    off[2 * (uint64_t)q] = o.donor_off;
    off[2 * (uint64_t)q + 1] = o.acceptor_off;
}

hipError_t launch_select_items_splice(hipStream_t s, const SelectTable &plus, const SelectTable &minus, const SelectPredicate &pred,
                                      const SelectCoding &coding, const EditPlanes &planes, const SpliceTest &test, const SelectItem *items,
                                      uint32_t n_items, const SelectPartials &part, const SelectResult &res)
{
    if (!n_items) return hipSuccess;
    hipLaunchKernelGGL(select_items_splice_kernel, dim3((n_items + SELECT_WAVES - 1) / SELECT_WAVES), dim3(BLOCK), 0, s, plus, minus, pred, coding,
                       planes, test, items, n_items, part, res);
    return hipGetLastError();
}

hipError_t launch_splice_eval(hipStream_t s, const uint32_t *pos_plus, const uint32_t *pos_minus, const SelectCoding &coding, const EditPlanes &planes,
                              const EditWindow &window, uint32_t editor, const uint32_t *gene_row, const uint32_t *packed_row, uint32_t n,
                              uint32_t *counts, uint32_t *off)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(splice_eval_kernel, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, pos_plus, pos_minus, coding, planes, window, editor,
                       gene_row, packed_row, n, counts, off);
    return hipGetLastError();
}

}  // namespace crp
