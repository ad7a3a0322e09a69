// crp_properties.h -- launch interface of crp_properties.hip (guide sequence properties: GC, runs, poly-T and hairpin
// stem of every hit's guide window), shared with the selection (crp_select.cpp reads the column).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace crp {

constexpr int PROP_MAX_GUIDE = 50;  // the window fits one 64-bit value after a funnel shift

// One strand's table as the kernel sees it: positions in, one packed word per row out.
struct PropTable {
    const uint32_t *pos;
    uint32_t *props;  // gc | run << 8 | t_run << 16 | stem << 24
    uint64_t n;
};

// The three planes the definition reads (the `up` plane is not: case is ignored) and the words each of them has.
struct PropPlanes {
    const uint64_t *hi, *lo, *ac;
    uint64_t n_words;  // a word at or beyond this index is never read: its positions are non-bases
};

// Both tables in one launch, one lane per row; guide_len 1 .. PROP_MAX_GUIDE (the caller checks).
hipError_t launch_guide_properties(hipStream_t s, const PropTable &plus, const PropTable &minus, const PropPlanes &planes, int guide_len);

}  // namespace crp
