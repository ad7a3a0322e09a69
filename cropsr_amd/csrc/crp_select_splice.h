// crp_select_splice.h -- launch interface of crp_select_splice.hip (the guide selection with the
// splice-site test, alone or as the alternative to the stop-codon test, and the evaluation of given (gene, row) pairs),
// shared with crp_select.cpp.
#pragma once
#include "crp_select_edit.h"
#include "crp_splice.h"

namespace crp {

// what is wave-uniform about the test: the window, the editor, the splice limits, and the edit limits if stops are an
// alternative (with_stop; CBE only)
struct SpliceTest {
    EditWindow window;
    uint32_t editor;
    SpliceLimits splice;
    uint32_t with_stop;
    EditLimits stop;
};

// select_items_kernel's work and results (crp_select.h), with the splice test -- or stop-or-splice -- as the predicate's last term
hipError_t launch_select_items_splice(hipStream_t s, const SelectTable &plus, const SelectTable &minus, const SelectPredicate &pred,
                                      const SelectCoding &coding, const EditPlanes &planes, const SpliceTest &test, const SelectItem *items,
                                      uint32_t n_items, const SelectPartials &part, const SelectResult &res);
// counts[q] = targets | donors << 8 | acceptors << 16, off[2 q] = donor_off and off[2 q + 1] = acceptor_off of packed_row[q]
// (row | strand << 31; rows inside the tables) for gene gene_row[q] (inside the model): the host has checked both
hipError_t launch_splice_eval(hipStream_t s, const uint32_t *pos_plus, const uint32_t *pos_minus, const SelectCoding &coding, const EditPlanes &planes,
                              const EditWindow &window, uint32_t editor, const uint32_t *gene_row, const uint32_t *packed_row, uint32_t n,
                              uint32_t *counts, uint32_t *off);

}  // namespace crp
