// crp_coding.h -- the coding test of the guide selection: from a gene row's step function and a
// cut boundary to "inside the primary transcript's coding sequence", the coding offset and the number of transcripts
// cut, and on to pass / fail against the coding limits.  One statement, compiled for the host and the device: the
// selection kernel and the evaluation kernel (crp_select_coding.hip) and a CPU driver (tests/native/coding_driver.cpp)
// call these very functions.  No HIP header is needed to include it on the host.
//
// The step function of a gene row (crp_annotation_coding_layout builds it) is a list of change points over the cut
// boundaries c of the arena (the boundary c lies between s[c - 1] and s[c]):
//   at[k]    ascending boundaries; before at[0] nothing holds, and at[k] <= c < at[k + 1] is step k
//   word[k]  cover (bits 0..15: the coding transcripts the boundary is inside) | inside P << 16 | grow << 17, where grow
//            says that s[c] is a coding letter of the primary transcript P
//   cum[k]   cum_P(at[k]): P's coding letters with index below at[k], counted on the whole contig
// so that cum_P(c) = cum[k] + grow * (c - at[k]) inside step k.  A gene's info word is n_tx | minus << 16 | model << 17.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CRP_CODING_FN __host__ __device__ inline
#else
#define CRP_CODING_FN inline
#endif

namespace crp {

constexpr uint32_t CODING_NOT_INSIDE = 0xFFFFFFFFu;  // off of a cut that is not inside P
constexpr uint32_t CODING_INSIDE_BIT = 1u << 16, CODING_GROW_BIT = 1u << 17;      // of a step's word
constexpr uint32_t CODING_MINUS_BIT = 1u << 16, CODING_MODEL_BIT = 1u << 17;      // of a gene's info word

struct CodingLimits {
    uint32_t min_pct, max_pct, min_transcripts_pct;  // each 0..100, min_pct <= max_pct
};

struct CodingPosition {
    uint32_t off;    // CODING_NOT_INSIDE, or 1 .. L_P - 1
    uint32_t cover;  // 0 .. n_tx
};

// Where boundary c lies for a gene row with n steps at at / word / cum (n may be 0), P's length L and info word `info`.
CRP_CODING_FN CodingPosition coding_position(const uint32_t *at, const uint32_t *word, const uint32_t *cum, uint32_t n, uint32_t L, uint32_t info,
                                             uint32_t c)
{
    CodingPosition out = {CODING_NOT_INSIDE, 0u};
    if (!(info & CODING_MODEL_BIT)) return out;
    // the first step that begins after c
    uint32_t a = 0, b = n;
    while (a < b) {
        const uint32_t mid = a + ((b - a) >> 1);
        if (at[mid] <= c) a = mid + 1;
        else b = mid;
    }
    if (!a) return out;
    const uint32_t k = a - 1, w = word[k];
    out.cover = w & 0xFFFFu;
    if (w & CODING_INSIDE_BIT) {
        const uint32_t before = cum[k] + ((w & CODING_GROW_BIT) ? c - at[k] : 0u);
        out.off = (info & CODING_MINUS_BIT) ? L - before : before;
    }
    return out;
}

// The limits of the definition, in integers with 64-bit products: the gene has a model, the cut is inside P,
// min_pct L <= 100 off <= max_pct L, and 100 cover >= min_transcripts_pct n_tx.
CRP_CODING_FN bool coding_pass(const CodingPosition &p, uint32_t L, uint32_t info, const CodingLimits &lim)
{
    if (!(info & CODING_MODEL_BIT) || p.off == CODING_NOT_INSIDE) return false;
    const uint64_t off100 = 100ull * p.off;
    return (uint64_t)lim.min_pct * L <= off100 && off100 <= (uint64_t)lim.max_pct * L &&
           100ull * p.cover >= (uint64_t)lim.min_transcripts_pct * (info & 0xFFFFu);
}

}  // namespace crp
