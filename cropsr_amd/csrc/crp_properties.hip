// crp_properties.hip -- guide sequence properties of every kept hit (cropsr_amd/properties.py states
// the definition, tests/guide_properties_reference.py restates it twice).  Not in the reference, opt-in.
//
// Per row of the resident hit tables, from the l letters of its guide window in the arena's bit-planes:
//
//   window   forward text s[i - l : i] of a '+' row (match index i), s[j + 3 : j + 3 + l] of a '-' row (match index j)
//   base     a letter whose `ac` bit is set; its code is (hi, lo), A=00 T=01 C=10 G=11 -- case is not looked at, U was
//            packed as A; N, IUPAC letters, decoration and void positions are non-bases
//   gc       letters that are C or G                               popcount of hi
//   run      longest run of equal bases (a non-base ends a run)     x &= x >> 1 ladder on the "equals its neighbour" mask
//   t_run    longest run of T in the SPACER's orientation: T in a '+' window, A in a '-' window (the spacer of a '-'
//            row is the window's reverse complement)
//   stem     the longest hairpin stem: the largest s with a, b such that w[a + t] pairs with w[b - t] (A-T, C-G) for
//            t < s and at least 3 letters stay unpaired between the arms.  Equivalently: over every anti-diagonal
//            c = p + q the longest run in p of pairing (p, q) with q - p >= 4.  The window is reversed once
//            (__brevll); diagonal c is then one shift of the reversed copy against the window, and "pairs" is one
//            expression: both bases, hi equal, lo different.
//
// One lane per row, both tables in one launch (annot_lookup_kernel's scheme); a lane reads its position (coalesced), at
// most two words of each of three planes (neighbouring rows share them: served by the caches) and writes one packed
// 32-bit word to its own slot.  No atomics, no LDS.  ~12 B of table traffic per row; the stem loop's VALU work is the
// bound (2 l - 1 diagonals at most, walked from the middle outwards and left as soon as no diagonal can beat the best).
#include "crp_internal.h"
#include "crp_properties.h"
#include "crp_roctx.h"

namespace crp {

namespace {

// longest run of set bits
__device__ __forceinline__ uint32_t prop_longest_run(unsigned long long x)
{
    uint32_t n = 0;
    while (x) {
        x &= x >> 1;
        ++n;
    }
    return n;
}

// bits [start, start + l) of a plane as the low l bits of one value; words at or beyond n_words read as zero
__device__ __forceinline__ unsigned long long prop_window(const uint64_t *__restrict__ plane, uint64_t n_words, uint64_t start, int l,
                                                          unsigned long long mask)
{
    const uint64_t w = start >> 6;
    const int sh = (int)(start & 63);
    const unsigned long long x0 = w < n_words ? plane[w] : 0ull;
    unsigned long long v = x0 >> sh;
    if (sh + l > 64) {  // (sh >= 15 here: the shift below is 1 .. 49)
        const unsigned long long x1 = w + 1 < n_words ? plane[w + 1] : 0ull;
        v |= x1 << (64 - sh);
    }
    return v & mask;
}

}  // namespace

__global__ __launch_bounds__(BLOCK) void guide_properties_kernel(PropTable plus, PropTable minus, uint32_t blocks_plus, PropPlanes planes,
                                                                 int l)
{
    const bool is_minus = blockIdx.x >= blocks_plus;  // (uniform per workgroup)
    const PropTable t = is_minus ? minus : plus;
    const uint64_t row = (uint64_t)(blockIdx.x - (is_minus ? blocks_plus : 0u)) * BLOCK + threadIdx.x;
    if (row >= t.n) return;
    const uint32_t pos = t.pos[row];
    // '+': i - l (the scan keeps i - l >= 5; a position that wrapped would index beyond every plane and read as non-bases)
    const uint64_t start = is_minus ? (uint64_t)pos + 3u : (uint64_t)pos - (uint64_t)l;
    const unsigned long long mask = ~0ull >> (64 - l);
    const unsigned long long AC = prop_window(planes.ac, planes.n_words, start, l, mask);
    const unsigned long long H = prop_window(planes.hi, planes.n_words, start, l, mask) & AC;
    const unsigned long long L = prop_window(planes.lo, planes.n_words, start, l, mask) & AC;

    const uint32_t gc = (uint32_t)__popcll(H);
    // bit p: letters p and p + 1 are bases and equal
    const unsigned long long eq = AC & (AC >> 1) & ~(H ^ (H >> 1)) & ~(L ^ (L >> 1));
    const uint32_t run = AC ? prop_longest_run(eq) + 1u : 0u;
    const uint32_t t_run = prop_longest_run(AC & ~H & (is_minus ? ~L : L));

    // stem: R* bit k = letter l - 1 - k.  On diagonal c the partner of p is q = c - p, i.e. bit p + (l - 1 - c) of R*.
    const unsigned long long RAC = __brevll(AC) >> (64 - l), RH = __brevll(H) >> (64 - l), RL = __brevll(L) >> (64 - l);
    uint32_t stem = 0;
    for (int d = 0; d < l; ++d) {
        // c = l - 1 - d holds (c >> 1) - 1 pairs with q - p >= 4, c = l - 1 + d holds d fewer of them than (c >> 1) - 1:
        // neither bound rises with d
        const int c_lo = l - 1 - d, c_hi = l - 1 + d;
        const int room_lo = (c_lo >> 1) - 1, room_hi = (c_hi >> 1) - 1 - d;
        if (room_lo <= (int)stem && room_hi <= (int)stem) break;
        if (room_lo > (int)stem) {
            const unsigned long long gap = ~0ull >> (64 - room_lo);  // p <= (c - 4) / 2
            const unsigned long long m = ~(H ^ (RH >> d)) & (L ^ (RL >> d)) & AC & (RAC >> d) & gap;
            stem = max(stem, prop_longest_run(m));
        }
        if (d && room_hi > (int)stem) {
            // (p runs from d: the bits below are empty in the shifted copy)
            const unsigned long long gap = ~0ull >> (64 - ((c_hi >> 1) - 1));
            const unsigned long long m = ~(H ^ (RH << d)) & (L ^ (RL << d)) & AC & (RAC << d) & gap;
            stem = max(stem, prop_longest_run(m));
        }
    }
    t.props[row] = gc | run << 8 | t_run << 16 | stem << 24;
}

hipError_t launch_guide_properties(hipStream_t s, const PropTable &plus, const PropTable &minus, const PropPlanes &planes, int guide_len)
{
    const uint32_t bp = (uint32_t)((plus.n + BLOCK - 1) / BLOCK), bm = (uint32_t)((minus.n + BLOCK - 1) / BLOCK);
    if (!(bp + bm)) return hipSuccess;
    hipLaunchKernelGGL(guide_properties_kernel, dim3(bp + bm), dim3(BLOCK), 0, s, plus, minus, bp, planes, guide_len);
    return hipGetLastError();
}

}  // namespace crp

extern "C" {

int crp_guide_properties(crp_arena *a, uint32_t *props_plus, uint32_t *props_minus)
{
    crp::Range roctx_range("crp: guide properties");
    if (!a) return CRP_ERR_INVALID;
    if (!a->have_hits) return CRP_ERR_STATE;
    crp_ctx *ctx = a->ctx;
    const int l = a->pend_guide_len;
    if (l < 1 || l > crp::PROP_MAX_GUIDE) {
        ctx->last_error = "crp_guide_properties: the tables were scanned at guide length " + std::to_string(l) + ": a guide of 1.." +
                          std::to_string(crp::PROP_MAX_GUIDE) + " letters has properties";
        return CRP_ERR_INVALID;
    }
    CRP_HIP(ctx, hipSetDevice(ctx->device));
    a->have_props = false;
    for (int s = 0; s < 2; ++s) {
        const int rc = crp::grow(ctx, reinterpret_cast<void **>(&a->d_props[s]), &a->props_cap[s], a->n_hits[s], sizeof(uint32_t));
        if (rc != CRP_OK) return rc;
    }
    for (hipEvent_t &e : a->ev_props)
        if (!e) CRP_HIP(ctx, hipEventCreate(&e));
    const crp::PropTable plus{a->d_pos[0], a->d_props[0], a->n_hits[0]};
    const crp::PropTable minus{a->d_pos[1], a->d_props[1], a->n_hits[1]};
    const crp::PropPlanes planes{a->d_plane[0], a->d_plane[1], a->d_plane[3], a->padded_words};
    crp::prof_begin(ctx, CRP_K_PROPERTIES);
    CRP_HIP(ctx, hipEventRecord(a->ev_props[0], ctx->stream));
    CRP_HIP(ctx, crp::launch_guide_properties(ctx->stream, plus, minus, planes, l));
    CRP_HIP(ctx, hipEventRecord(a->ev_props[1], ctx->stream));
    crp::prof_end(ctx, CRP_K_PROPERTIES);
    CRP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    crp::prof_collect(ctx, CRP_K_PROPERTIES);
    float ms = 0.f;
    a->props_ms = hipEventElapsedTime(&ms, a->ev_props[0], a->ev_props[1]) == hipSuccess ? ms : 0.0;
    a->have_props = true;
    uint32_t *host[2] = {props_plus, props_minus};
    for (int s = 0; s < 2; ++s)
        if (host[s] && a->n_hits[s]) {
            const int rc = crp::staged_d2h(ctx, host[s], a->d_props[s], a->n_hits[s] * sizeof(uint32_t));
            if (rc != CRP_OK) return rc;
        }
    return CRP_OK;
}

int crp_guide_properties_stats(const crp_arena *a, double *out, int n)
{
    if (!a || (n && !out) || n < 0 || n > 3) return CRP_ERR_INVALID;
    if (!a->have_props) return CRP_ERR_STATE;
    const double v[3] = {a->props_ms, (double)(a->n_hits[0] + a->n_hits[1]), (double)a->pend_guide_len};
    for (int k = 0; k < n; ++k) out[k] = v[k];
    return CRP_OK;
}

}  // extern "C"
