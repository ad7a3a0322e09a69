// crp_sites.h -- launch interface of crp_sites.hip (restriction sites: occurrence planes of an enzyme set over the arena,
// their rank index and the per-hit cloning / assay masks), shared with the selection (crp_select.cpp
// reads the column).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace crp {

constexpr int SITE_MAX_ENZYMES = 32;
constexpr int SITE_MIN_MOTIF = 4, SITE_MAX_MOTIF = 16;  // the halo of a plane word is its successor alone
constexpr int SITE_MAX_GUIDE = 50;
constexpr int SITE_MAX_FLANK = 100000;
constexpr int SITE_RANK_WORDS = 4;                            // plane words per lane of the rank kernels
constexpr uint32_t SITE_CHUNK = 256 * SITE_RANK_WORDS;        // plane words per workgroup of the rank kernels

// One enzyme as the kernels read it (a table in device memory, read with wave-uniform indices): letter k of the motif is
// the nibble fwd >> 4 k, letter k of its reverse complement the nibble rev >> 4 k; a nibble is the set of bases the letter
// stands for, bit 0 A, bit 1 C, bit 2 G, bit 3 T.
struct SiteEnzyme {
    unsigned long long fwd, rev;
    uint32_t len;
    uint32_t palindrome;  // rev == fwd: one pass
};

// The three planes the definition reads and the words each of them -- and every occurrence plane -- has.
struct SitePlanes {
    const uint64_t *hi, *lo, *ac;
    uint64_t n_words;  // a word at or beyond this index is never read: its positions are non-bases
};

// occ: n_enzymes planes of n_words words; rank: n_enzymes rows of n_words + 1 values (the last is the enzyme's total)
struct SiteIndex {
    const unsigned long long *occ;
    const uint32_t *rank;
    const SiteEnzyme *enzymes;
    uint32_t n_enzymes;
    uint64_t n_words;
    const uint32_t *text_start, *text_end;  // ascending; text k is [text_start[k], text_end[k])
    uint32_t n_texts;
};

// One strand's table as the column kernel sees it: positions in, in_guide | assay << 32 per row out.
struct SiteTable {
    const uint32_t *pos;
    unsigned long long *out;
    uint64_t n;
};

hipError_t launch_site_planes(hipStream_t s, const SitePlanes &planes, const SiteEnzyme *enzymes, uint32_t n_enzymes, unsigned long long *occ);
// chunk_sum: n_enzymes * n_chunks values of scratch, n_chunks = ceil(n_words / SITE_CHUNK)
hipError_t launch_site_ranks(hipStream_t s, const unsigned long long *occ, uint64_t n_words, uint32_t n_enzymes, uint32_t *chunk_sum,
                             uint32_t *rank);
// Both tables in one launch, one lane per row; guide_len 1 .. SITE_MAX_GUIDE, flank from the set's longest motif to SITE_MAX_FLANK (the caller checks).
hipError_t launch_site_columns(hipStream_t s, const SiteTable &plus, const SiteTable &minus, const SiteIndex &index, int guide_len, int flank);

}  // namespace crp
