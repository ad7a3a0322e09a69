// crp_repair.h -- launch interface of crp_repair.hip (repair outcome of every hit's cut: microhomology and out-of-frame
// score), shared with the selection (crp_select.cpp reads the column).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace crp {

constexpr int REPAIR_MIN_FLANK = 2, REPAIR_MAX_FLANK = 32;  // 2 F letters fit one 64-bit value after a funnel shift

// One strand's table as the kernel sees it: positions in, one packed value per row out.
struct RepairTable {
    const uint32_t *pos;
    unsigned long long *out;  // mh | oof << 32
    uint64_t n;
};

// The three planes the definition reads (the `up` plane is not: case is ignored) and the words each of them has.
struct RepairPlanes {
    const uint64_t *hi, *lo, *ac;
    uint64_t n_words;  // a word at or beyond this index is never read: its positions are non-bases
};

// Both tables in one launch, one lane per row; flank REPAIR_MIN_FLANK .. REPAIR_MAX_FLANK (the caller checks).
hipError_t launch_repair_scores(hipStream_t s, const RepairTable &plus, const RepairTable &minus, const RepairPlanes &planes, int flank);

}  // namespace crp
