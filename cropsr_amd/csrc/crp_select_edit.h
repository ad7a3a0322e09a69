// crp_select_edit.h -- launch interface of crp_select_edit.hip (the guide selection with the
// base-editing test, and the evaluation of given (gene, row) pairs), shared with crp_select.cpp.
#pragma once
#include "crp_edit.h"
#include "crp_select_coding.h"

namespace crp {

// select_items_kernel's work and results (crp_select.h), with the base-editing test as the predicate's last term
hipError_t launch_select_items_edit(hipStream_t s, const SelectTable &plus, const SelectTable &minus, const SelectPredicate &pred,
                                    const SelectCoding &coding, const EditPlanes &planes, const EditWindow &window, const EditLimits &lim,
                                    const SelectItem *items, uint32_t n_items, const SelectPartials &part, const SelectResult &res);
// counts[q] = targets | stops << 8 and stop_off[q] of packed_row[q] (row | strand << 31; rows inside the tables) for gene
// gene_row[q] (inside the model): the host has checked both
hipError_t launch_edit_eval(hipStream_t s, const uint32_t *pos_plus, const uint32_t *pos_minus, const SelectCoding &coding, const EditPlanes &planes,
                            const EditWindow &window, const uint32_t *gene_row, const uint32_t *packed_row, uint32_t n, uint32_t *counts,
                            uint32_t *stop_off);

}  // namespace crp
