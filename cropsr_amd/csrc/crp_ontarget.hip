// crp_ontarget.hip -- the on-target sum of every guide site of a self-search handle from a position-specific linear model
// (cropsr_amd/ontarget.py states the definition, tests/ontarget_reference.py restates it twice).  Not
// in the reference, opt-in.
//
// A model of a pattern of T letters: a window of W <= 64 letters of the oriented site, `left` of them before pattern
// position 0; an intercept, a weight per (window position, letter), a weight per (window position, adjacent pair) and a
// weight per GC count of the guide region.  Per candidate of the handle, in extraction order:
//
//   window   '+' site with forward start s: forward positions s - left .. s - left + W - 1; '-' site: forward positions
//            s + T - 1 + left down to s + T + left - W, each complemented (A=00 T=01 C=10 G=11: the low code bit flips)
//   base     a letter whose `ac` bit is set -- case is not looked at, U was packed as A; N, IUPAC letters, decoration and void
//            positions are non-bases, and so is every position outside the planes.  A window with a non-base has no sum
//   sum      ((intercept + gc[GC]) + single[0] + .. + single[W - 1]) + pair[0] + .. + pair[W - 2], in f64, one add per term
//            in that order, zero terms included (the library is built with -ffp-contract=off; the body only adds)
//
// One lane per candidate: its position and guide flag (coalesced), at most two words of each of three planes (crp_repair.hip's
// window: words outside the planes read as zero, one funnel shift), one f64 to its own slot.  A candidate that is no guide site,
// or whose window holds a non-base, gets a quiet NaN.  The tables are staged once per workgroup into LDS (2 KB single, 8 KB
// pair, 264 B gc) and read from there by letter code; the trip counts are the same for every lane.  No atomics, no scratch.
#include "crp_internal.h"
#include "crp_ontarget.h"

namespace crp {

namespace {

// bits [start, start + n) of a plane as the low n bits of one value (n <= 64); a start below 0 and words at or beyond
// n_words read as zero (repair_window's rule)
__device__ __forceinline__ unsigned long long model_window(const uint64_t *__restrict__ plane, uint64_t n_words, long long start, int n,
                                                           unsigned long long mask)
{
    const long long w = start >> 6;  // (arithmetic: negative for a start below 0)
    const int sh = (int)(start & 63);
    const unsigned long long x0 = w >= 0 && (uint64_t)w < n_words ? plane[w] : 0ull;
    unsigned long long v = x0 >> sh;
    if (sh + n > 64) {  // (sh >= 1 here: the shift below is 1 .. 63)
        const unsigned long long x1 = w + 1 >= 0 && (uint64_t)(w + 1) < n_words ? plane[w + 1] : 0ull;
        v |= x1 << (64 - sh);
    }
    return v & mask;
}

}  // namespace

__global__ __launch_bounds__(BLOCK) void self_model_kernel(const uint32_t *__restrict__ pos, const uint32_t *__restrict__ hi,
                                                           const uint8_t *__restrict__ flag, uint32_t n, ModelPlanes planes, ModelShape shape,
                                                           const double *__restrict__ table, double *__restrict__ out)
{
    __shared__ double tab[MODEL_TABLE];
    for (int i = threadIdx.x; i < MODEL_TABLE; i += BLOCK) tab[i] = table[i];
    __syncthreads();
    const uint64_t row = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (row >= n) return;
    const double *single = tab, *pair = tab + MODEL_SINGLE, *gc = tab + MODEL_SINGLE + MODEL_PAIR;
    const int W = shape.W;
    const uint32_t p = pos[row];
    const bool minus = (p >> 31) != 0;
    const long long s = (long long)(p & 0x7fffffffu);
    const long long start = minus ? s + shape.T + shape.left - W : s - shape.left;
    const unsigned long long mask = ~0ull >> (64 - W);
    const unsigned long long AC = model_window(planes.ac, planes.n_words, start, W, mask);
    unsigned long long H = model_window(planes.hi, planes.n_words, start, W, mask);
    unsigned long long L = model_window(planes.lo, planes.n_words, start, W, mask);
    if (minus) {  // window position w is forward bit W - 1 - w, complemented
        H = __brevll(H) >> (64 - W);
        L = (__brevll(L) >> (64 - W)) ^ mask;
    }
    const bool have = flag[row] != 0 && AC == mask;
    double acc = shape.intercept + gc[__popc(hi[row] & shape.region)];  // (at most 32 set bits: inside gc[0 .. 32])
#pragma clang loop unroll(disable)
    for (int w = 0; w < W; ++w) {  // (uniform)
        const uint32_t code = (uint32_t)((H >> w) & 1ull) << 1 | (uint32_t)((L >> w) & 1ull);
        acc = acc + single[w * 4 + code];
    }
#pragma clang loop unroll(disable)
    for (int w = 0; w + 1 < W; ++w) {  // (uniform)
        const uint32_t c1 = (uint32_t)((H >> w) & 1ull) << 1 | (uint32_t)((L >> w) & 1ull);
        const uint32_t c2 = (uint32_t)((H >> (w + 1)) & 1ull) << 1 | (uint32_t)((L >> (w + 1)) & 1ull);
        acc = acc + pair[w * 16 + c1 * 4 + c2];
    }
    out[row] = have ? acc : __longlong_as_double(0x7ff8000000000000ll);
}

hipError_t launch_self_model(hipStream_t s, const uint32_t *pos, const uint32_t *hi, const uint8_t *flag, uint32_t n, const ModelPlanes &planes,
                             const ModelShape &shape, const double *table, double *out)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(self_model_kernel, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, pos, hi, flag, n, planes, shape, table, out);
    return hipGetLastError();
}

}  // namespace crp
