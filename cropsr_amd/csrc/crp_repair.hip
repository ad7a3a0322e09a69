// crp_repair.hip -- what the cut of every kept hit does to the gene: the microhomology score and the out-of-frame score
// of Bae, Kweon, Kim and Kim 2014 (cropsr_amd/repair.py states the definition,
// tests/repair_reference.py restates it twice).  Not in the reference, opt-in.
//
// Per row of the resident hit tables, from the 2 F letters around its cut in the arena's bit-planes (F: the flank, 2 .. 32):
//
//   cut      the boundary c between s[c - 1] and s[c]: c = i - 3 for a '+' row (match index i), c = j + 6 for a '-' row
//            (match index j): three letters into the protospacer from the PAM on either strand
//   window   w[p] = s[c - F + p], p = 0 .. 2 F - 1; left flank p < F, right flank p >= F
//   base     a letter whose `ac` bit is set; its code is (hi, lo) -- case is not looked at, U was packed as A; N, IUPAC
//            letters, decoration and void positions are non-bases, and so is every position outside the planes
//   d        a deletion length 1 .. 2 F - 1: the left copy's letters are p in [max(0, F - d), min(F, 2 F - d)), the right
//            copy's are p + d
//   m_d(p)   w[p] and w[p + d] are bases and equal
//   n_d      over every maximal run of m_d of length k >= 2 inside that range: k + (its letters that are C or G)
//   result   mh = sum W[d] n_d, oof = the same over d that are no multiple of 3; W from microhomology_weights.def
//
// One lane per row, both tables in one launch (guide_properties_kernel's scheme); a lane reads its position (coalesced), at
// most two words of each of three planes and writes one 8-byte value to its own slot.  No atomics, no LDS.  A diagonal is
// 32-bit work: the left copy lies in p < F <= 32, so only the low half of every shifted value is looked at -- one
// v_alignbit_b32 per plane while d < 32, one shift of the high half from there on.  d, the range mask and the two weights
// are the same for every lane: scalar registers and scalar loads from the constant tables.
#include "crp_internal.h"
#include "crp_repair.h"
#include "crp_roctx.h"

namespace crp {

namespace {

// per deletion length d (index 0 unused): .x = W[d], what a letter of a microhomology adds to mh; .y = the same with the
// multiples of 3 zeroed, what it adds to oof.  One 8-byte scalar load per diagonal.
struct RepairWeights {
    uint2 w[64];
};
constexpr RepairWeights repair_weights()
{
    constexpr uint32_t W[64] = {0,
#include "microhomology_weights.def"
    };
    RepairWeights t{};
    for (int d = 0; d < 64; ++d) {
        t.w[d].x = W[d];
        t.w[d].y = d % 3 ? W[d] : 0u;
    }
    return t;
}
__constant__ RepairWeights REPAIR_W = repair_weights();

// bits [start, start + n) of a plane as the low n bits of one value (n = 2 F <= 64); a start below 0 and words at or
// beyond n_words read as zero
__device__ __forceinline__ unsigned long long repair_window(const uint64_t *__restrict__ plane, uint64_t n_words, long long start, int n,
                                                            unsigned long long mask)
{
    const long long w = start >> 6;  // (arithmetic: -1 for a start in -64 .. -1)
    const int sh = (int)(start & 63);
    const unsigned long long x0 = w >= 0 && (uint64_t)w < n_words ? plane[w] : 0ull;
    unsigned long long v = x0 >> sh;
    if (sh + n > 64) {  // (sh >= 1 here: the shift below is 1 .. 63)
        const unsigned long long x1 = w + 1 >= 0 && (uint64_t)(w + 1) < n_words ? plane[w + 1] : 0ull;
        v |= x1 << (64 - sh);
    }
    return v & mask;
}

// what diagonal d adds: the left copy's bits of the three planes (a*), the right copy's shifted down onto them (b*)
__device__ __forceinline__ uint32_t repair_diagonal(uint32_t ah, uint32_t al, uint32_t aa, uint32_t bh, uint32_t bl, uint32_t ba, uint32_t range)
{
    const uint32_t m = ~((ah ^ bh) | (al ^ bl)) & aa & ba & range;
    const uint32_t r = m & (m >> 1 | m << 1);  // the letters of runs of two and more
    return (uint32_t)__popc(r) + (uint32_t)__popc(r & ah);
}

}  // namespace

__global__ __launch_bounds__(BLOCK) void repair_scores_kernel(RepairTable plus, RepairTable minus, uint32_t blocks_plus, RepairPlanes planes,
                                                              int flank)
{
    const bool is_minus = blockIdx.x >= blocks_plus;  // (uniform per workgroup)
    const RepairTable t = is_minus ? minus : plus;
    const uint64_t row = (uint64_t)(blockIdx.x - (is_minus ? blocks_plus : 0u)) * BLOCK + threadIdx.x;
    if (row >= t.n) return;
    const uint32_t pos = t.pos[row];
    const int F = flank;
    const long long start = (long long)pos + (is_minus ? 6 : -3) - F;
    const unsigned long long mask = ~0ull >> (64 - 2 * F);
    const unsigned long long AC = repair_window(planes.ac, planes.n_words, start, 2 * F, mask);
    const unsigned long long H = repair_window(planes.hi, planes.n_words, start, 2 * F, mask) & AC;
    const unsigned long long L = repair_window(planes.lo, planes.n_words, start, 2 * F, mask) & AC;
    const uint32_t h0 = (uint32_t)H, h1 = (uint32_t)(H >> 32), l0 = (uint32_t)L, l1 = (uint32_t)(L >> 32);
    const uint32_t a0 = (uint32_t)AC, a1 = (uint32_t)(AC >> 32);

    uint32_t mh = 0, oof = 0;
    const int last = 2 * F - 1, split = last < 31 ? last : 31;
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
    for (int d = 1; d <= split; ++d) {
        // p in [max(0, F - d), min(F, 2 F - d)): uniform, scalar work
        const int lo = F - d > 0 ? F - d : 0, hi = 2 * F - d < F ? 2 * F - d : F;
        const uint32_t range = (uint32_t)((1ull << hi) - 1ull) & ~(uint32_t)((1ull << lo) - 1ull);
        const uint32_t n = repair_diagonal(h0, l0, a0, __builtin_amdgcn_alignbit(h1, h0, (uint32_t)d), __builtin_amdgcn_alignbit(l1, l0, (uint32_t)d),
                                           __builtin_amdgcn_alignbit(a1, a0, (uint32_t)d), range);
        const uint2 w = REPAIR_W.w[d];  // (n <= 64, w <= 951: 24-bit products)
        mh += __umul24(w.x, n);
        oof += __umul24(w.y, n);
    }
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
    for (int d = 32; d <= last; ++d) {  // (F >= 17: lo = 0, hi = 2 F - d)
        const uint32_t range = (uint32_t)((1ull << (2 * F - d)) - 1ull);
        const uint32_t n = repair_diagonal(h0, l0, a0, h1 >> (d - 32), l1 >> (d - 32), a1 >> (d - 32), range);
        const uint2 w = REPAIR_W.w[d];  // (n <= 64, w <= 951: 24-bit products)
        mh += __umul24(w.x, n);
        oof += __umul24(w.y, n);
    }
    t.out[row] = (unsigned long long)mh | (unsigned long long)oof << 32;
}

hipError_t launch_repair_scores(hipStream_t s, const RepairTable &plus, const RepairTable &minus, const RepairPlanes &planes, int flank)
{
    const uint32_t bp = (uint32_t)((plus.n + BLOCK - 1) / BLOCK), bm = (uint32_t)((minus.n + BLOCK - 1) / BLOCK);
    if (!(bp + bm)) return hipSuccess;
    hipLaunchKernelGGL(repair_scores_kernel, dim3(bp + bm), dim3(BLOCK), 0, s, plus, minus, bp, planes, flank);
    return hipGetLastError();
}

}  // namespace crp

extern "C" {

int crp_repair_scores(crp_arena *a, int flank, uint64_t *plus, uint64_t *minus)
{
    crp::Range roctx_range("crp: repair scores");
    if (!a) return CRP_ERR_INVALID;
    crp_ctx *ctx = a->ctx;
    if (flank < crp::REPAIR_MIN_FLANK || flank > crp::REPAIR_MAX_FLANK) {
        ctx->last_error = "crp_repair_scores: a flank of " + std::to_string(crp::REPAIR_MIN_FLANK) + ".." + std::to_string(crp::REPAIR_MAX_FLANK) +
                          " letters on either side of the cut is scored, not " + std::to_string(flank);
        return CRP_ERR_INVALID;
    }
    if (!a->have_hits) return CRP_ERR_STATE;
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    a->have_repair = false;
    for (int s = 0; s < 2; ++s) {
        const int rc = crp::grow(ctx, reinterpret_cast<void **>(&a->d_repair[s]), &a->repair_cap[s], a->n_hits[s], sizeof(uint64_t));
        if (rc != CRP_OK) return rc;
    }
    for (hipEvent_t &e : a->ev_repair)
        if (!e) CRP_HIP(ctx, hipEventCreate(&e));
    const crp::RepairTable tp{a->d_pos[0], reinterpret_cast<unsigned long long *>(a->d_repair[0]), a->n_hits[0]};
    const crp::RepairTable tm{a->d_pos[1], reinterpret_cast<unsigned long long *>(a->d_repair[1]), a->n_hits[1]};
    const crp::RepairPlanes planes{a->d_plane[0], a->d_plane[1], a->d_plane[3], a->padded_words};
    CRP_HIP(ctx, hipEventRecord(a->ev_repair[0], ctx->stream));
    CRP_HIP(ctx, crp::launch_repair_scores(ctx->stream, tp, tm, planes, flank));
    CRP_HIP(ctx, hipEventRecord(a->ev_repair[1], ctx->stream));
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    a->repair_ms = hipEventElapsedTime(&ms, a->ev_repair[0], a->ev_repair[1]) == hipSuccess ? ms : 0.0;
    a->repair_flank = flank;
    a->have_repair = true;
    uint64_t *host[2] = {plus, minus};
    for (int s = 0; s < 2; ++s)
        if (host[s] && a->n_hits[s]) {
            const int rc = crp::staged_d2h(ctx, host[s], a->d_repair[s], a->n_hits[s] * sizeof(uint64_t));
            if (rc != CRP_OK) return rc;
        }
    return CRP_OK;
}

int crp_repair_scores_stats(const crp_arena *a, double *out, int n)
{
    if (!a || (n && !out) || n < 0 || n > 3) return CRP_ERR_INVALID;
    if (!a->have_repair) return CRP_ERR_STATE;
    const double v[3] = {a->repair_ms, (double)(a->n_hits[0] + a->n_hits[1]), (double)a->repair_flank};
    for (int k = 0; k < n; ++k) out[k] = v[k];
    return CRP_OK;
}

}  // extern "C"
