// crp_select_coding.h -- launch interface of crp_select_coding.hip (the guide selection with the
// coding test, and the evaluation of given (gene, row) pairs), shared with crp_select.cpp.
#pragma once
#include "crp_coding.h"
#include "crp_select.h"

namespace crp {

// The coding model of a handle's genes in HBM (crp_coding.h has the form): info / length per gene, first with one more
// element than the genes, and the steps.
struct SelectCoding {
    const uint32_t *info, *length, *first;
    const uint32_t *at, *word, *cum;
};

// select_items_kernel's work and results (crp_select.h), with the coding test as the predicate's last term
hipError_t launch_select_items_coding(hipStream_t s, const SelectTable &plus, const SelectTable &minus, const SelectPredicate &pred,
                                      const SelectCoding &coding, const CodingLimits &lim, const SelectItem *items, uint32_t n_items,
                                      const SelectPartials &part, const SelectResult &res);
// off[q], cover[q] of the cut of packed_row[q] (row | strand << 31; rows inside the tables) for gene gene_row[q] (inside
// the model): the host has checked both
hipError_t launch_coding_eval(hipStream_t s, const uint32_t *pos_plus, const uint32_t *pos_minus, const SelectCoding &coding,
                              const uint32_t *gene_row, const uint32_t *packed_row, uint32_t n, uint32_t *off, uint32_t *cover);

}  // namespace crp
