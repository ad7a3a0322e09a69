// crp_select_insert.h -- the wave's sorted top-K list of the guide selection: its entry and the
// insertion all 64 lanes run together.  Shared by the kernels of crp_select.hip and crp_select_coding.hip; device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace crp {

namespace {

struct SelEntry {
    unsigned long long key;
    uint32_t tie, row;
};

__device__ __forceinline__ bool sel_better(unsigned long long ka, uint32_t ta, unsigned long long kb, uint32_t tb)
{
    return ka > kb || (ka == kb && ta < tb);
}

// value of wave-uniform lane `l`
__device__ __forceinline__ uint32_t sel_lane32(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }
__device__ __forceinline__ unsigned long long sel_lane64(unsigned long long v, int l)
{
    return (unsigned long long)sel_lane32((uint32_t)(v >> 32), l) << 32 | sel_lane32((uint32_t)v, l);
}

// Inserts the lanes' candidates (want: this lane has one) into the wave's sorted list, best first.  All 64 lanes call
// it together.  Lanes >= k also hold (worse) entries; only lane k - 1 decides what gets in.
__device__ __forceinline__ void sel_insert(SelEntry &mine, int lane, int k, bool want, unsigned long long ckey, uint32_t ctie,
                                           uint32_t crow)
{
    unsigned long long thr_key = sel_lane64(mine.key, k - 1);
    uint32_t thr_tie = sel_lane32(mine.tie, k - 1);
    unsigned long long mask = __ballot(want && sel_better(ckey, ctie, thr_key, thr_tie));
    while (mask) {
        const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)mask) - 1);
        mask &= mask - 1;
        const unsigned long long bkey = sel_lane64(ckey, l);
        const uint32_t btie = sel_lane32(ctie, l), brow = sel_lane32(crow, l);
        if (!sel_better(bkey, btie, thr_key, thr_tie)) continue;  // (the bar has risen since the ballot)
        // the list is sorted: the lanes whose entry the candidate beats are a suffix; its first lane takes the
        // candidate, the others their neighbour's entry
        const unsigned long long ukey = __shfl_up(mine.key, 1);
        const uint32_t utie = __shfl_up(mine.tie, 1), urow = __shfl_up(mine.row, 1);
        if (sel_better(bkey, btie, mine.key, mine.tie)) {
            const bool shifted = lane > 0 && sel_better(bkey, btie, ukey, utie);
            mine.key = shifted ? ukey : bkey;
            mine.tie = shifted ? utie : btie;
            mine.row = shifted ? urow : brow;
        }
        thr_key = sel_lane64(mine.key, k - 1);
        thr_tie = sel_lane32(mine.tie, k - 1);
    }
}

}  // namespace

}  // namespace crp
