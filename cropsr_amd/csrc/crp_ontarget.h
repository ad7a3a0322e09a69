// crp_ontarget.h -- launch interface of crp_ontarget.hip (the on-target sum of every guide site of a self-search handle from
// a position-specific linear model), shared with its host side in crp_search_self.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace crp {

constexpr int MODEL_MAX_W = 64;                       // the window fits one 64-bit value after a funnel shift
constexpr int MODEL_SINGLE = MODEL_MAX_W * 4;         // doubles: single[w][b]
constexpr int MODEL_PAIR = (MODEL_MAX_W - 1) * 16;    // doubles: pair[w][b1][b2]
constexpr int MODEL_GC = 33;                          // doubles: gc[0 .. G], G <= 32
constexpr int MODEL_TABLE = MODEL_SINGLE + MODEL_PAIR + MODEL_GC;  // one device buffer: single, pair, gc

// The three planes the definition reads and the words each of them has (crp_repair.h's rule: a word at or beyond n_words
// is never read, its positions are non-bases).
struct ModelPlanes {
    const uint64_t *hi, *lo, *ac;
    uint64_t n_words;
};

struct ModelShape {
    int W, left, T;       // window letters, window letters before pattern position 0 of the oriented site, pattern letters
    uint32_t region;      // the guide region's pattern positions (GC is counted over them, from the handle's hi field)
    double intercept;
};

// One lane per candidate, in extraction order: out[i] = the sum of candidate i, quiet NaN where it is no guide site or its
// window holds a non-base.  table: MODEL_TABLE doubles on the device, terms not set 0.0.
hipError_t launch_self_model(hipStream_t s, const uint32_t *pos, const uint32_t *hi, const uint8_t *flag, uint32_t n, const ModelPlanes &planes,
                             const ModelShape &shape, const double *table, double *out);

}  // namespace crp
