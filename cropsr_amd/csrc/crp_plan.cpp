// crp_plan.cpp -- how ONE genome is spread over the devices of a node: crp_plan_shares of the C ABI, and what crp_node_load
// (crp_node.cpp) cuts by.  The reference's contig loop (CROPSR.py:409) carries no state from one contig to the next, and
// everything it looks at around a match lies within 58 characters of it: any cut with a halo of CRP_HALO = 128 characters
// gives the same hits.  The rule (the same as cropsr_amd/parallel.py split_evenly, which the process-per-GPU path uses;
// tests/test_node.py holds the two against each other): the contigs, in their order, as CONTIGUOUS runs of equal size --
// device r gets the characters [r, r + 1) * total / world of the concatenation; a contig that straddles a boundary is cut
// there unless one side would be shorter than min_piece, in which case it stays whole on the side that holds most of it.
// At most world - 1 cuts; only a device's FIRST piece can begin inside a contig and only its LAST can end inside one -- so
// the rows a device owns are ONE run of each of its tables, which is what crp_node_gather sends.
// Below that, what the node handle and the pipelined scan (crp_stream.cpp) both cut by: a piece's uploaded text, the packing of
// a run of pieces into arenas, an arena's ownership needles and piece map, and the reading of their lower bounds.
#include "crp_plan.h"

#include <algorithm>
#include <cstring>

#include "cropsr_hip.h"

namespace crp {

Piece make_piece(uint64_t contig, uint64_t start, uint64_t end, uint64_t group, uint64_t contig_len, uint64_t halo)
{
    const uint64_t text_lo = start > halo ? start - halo : 0;
    return Piece{contig, start, end, group, text_lo, std::min(contig_len, end + halo) - text_lo};
}

void plan_shares(const uint64_t *lens, uint64_t n, int world, uint64_t min_piece, uint64_t halo, std::vector<Piece> &out)
{
    out.clear();
    int64_t total = 0;
    for (uint64_t k = 0; k < n; ++k) total += (int64_t)lens[k];
    std::vector<int64_t> bounds((size_t)world);
    for (int r = 0; r < world; ++r)
        bounds[(size_t)r] = (int64_t)(((unsigned __int128)(r + 1) * (unsigned __int128)total) / (unsigned)world);
    const int64_t minp = (int64_t)min_piece;
    int r = 0;
    int64_t acc = 0;
    for (uint64_t k = 0; k < n; ++k) {
        const int64_t len = (int64_t)lens[k];
        int64_t start = 0;
        auto put = [&](int64_t end) { out.push_back(make_piece(k, (uint64_t)start, (uint64_t)end, (uint64_t)r, lens[k], halo)); };
        for (;;) {
            const int64_t rest = len - start, room = bounds[(size_t)r] - acc;
            if (r == world - 1 || rest <= room) {
                put(len);
                acc += rest;
                break;
            }
            if (room >= minp && rest - room >= minp) {  // cut at the boundary
                put(start + room);
                acc += room;
                start += room;
                r += 1;
            } else if (2 * room >= rest) {  // a sliver would be left over: the rest of the contig stays here
                put(len);
                acc += rest;
                break;
            } else {  // a sliver would be cut off: the next device takes the contig from here
                r += 1;
            }
        }
        while (r < world - 1 && acc >= bounds[(size_t)r]) r += 1;
    }
}

static inline uint64_t words_for(uint64_t len) { return (len + 63) / 64 + 1; }  // = crp_arena_words_for (crp_api.cpp; no HIP here)

uint64_t slice_words_min(uint64_t halo) { return words_for(2 * halo + 64) + 2; }

void pack_pieces(const Piece *run, size_t n_run, const uint64_t *lens, uint64_t limit_words, uint64_t halo, std::vector<Piece> &out)
{
    uint64_t arena = 0, used = 1;  // (word 0 of an arena is its leading separator)
    bool any = false;              // the current arena holds a piece
    for (size_t i = 0; i < n_run; ++i) {
        const uint64_t k = run[i].contig, last = run[i].end;
        uint64_t start = run[i].start;
        for (;;) {
            Piece p = make_piece(k, start, last, 0, lens[k], halo);
            uint64_t need = words_for(p.text_len);
            bool cut = false;
            if (used + need > limit_words) {
                if (any) {  // the run goes on in a new arena
                    arena += 1;
                    used = 1;
                    any = false;
                }
                if (used + need > limit_words) {  // not even an empty arena holds it: cut to what one takes
                    const uint64_t chars = (limit_words - used - 1) * 64;
                    const uint64_t own = (chars - owned_begin(p, 0) - halo) & ~(uint64_t)63;
                    p = make_piece(k, start, start + own, 0, lens[k], halo);
                    need = words_for(p.text_len);
                    cut = true;
                }
            }
            p.group = arena;
            out.push_back(p);
            used += need;
            any = true;
            if (cut) {  // a piece that ends inside its contig closes its arena: one run per table
                arena += 1;
                used = 1;
                any = false;
            }
            if (p.end == last) break;
            start = p.end;
        }
    }
}

void plan_slices(const uint64_t *lens, uint64_t n, uint64_t limit_words, uint64_t halo, std::vector<Piece> &out)
{
    std::vector<Piece> whole((size_t)n);
    for (uint64_t k = 0; k < n; ++k) whole[(size_t)k] = make_piece(k, 0, lens[k], 0, lens[k], halo);
    out.clear();
    pack_pieces(whole.data(), whole.size(), lens, limit_words, halo, out);
}

void plan_slices(const uint64_t *lens, uint64_t n, uint64_t limit_words, uint64_t halo, std::vector<std::array<uint64_t, 4>> &out)
{
    std::vector<Piece> pieces;
    plan_slices(lens, n, limit_words, halo, pieces);
    out.clear();
    for (const Piece &p : pieces) out.push_back({p.contig, p.start, p.end, p.group});
}

uint64_t owned_begin(const Piece &p, uint64_t arena_off) { return arena_off + (p.start - p.text_lo); }

void piece_cuts(const Piece *pieces, size_t np, const uint64_t *arena_off, uint32_t *needles, uint32_t *map)
{
    for (size_t j = 0; j < np; ++j) {
        const Piece &p = pieces[j];
        const uint64_t begin = owned_begin(p, arena_off[j]);
        if (needles) {
            needles[2 * j] = (uint32_t)begin;
            needles[2 * j + 1] = (uint32_t)(begin + (p.end - p.start));
        }
        map[j] = (uint32_t)begin;
        map[np + j] = (uint32_t)(begin - p.start);  // (mod 2^32)
    }
}

bool owned_run(const uint32_t *b, size_t np, uint64_t *first, uint64_t *last, uint32_t *counts)
{
    for (size_t j = 0; j < np; ++j) {
        if (b[2 * j + 1] < b[2 * j] || (j + 1 < np && b[2 * j + 2] != b[2 * j + 1])) return false;
        counts[j] = b[2 * j + 1] - b[2 * j];
    }
    *first = np ? b[0] : 0;
    *last = np ? b[2 * np - 1] : 0;
    return true;
}

}  // namespace crp

extern "C" int crp_plan_shares(const uint64_t *lens, uint64_t n, int world, uint64_t min_piece, uint64_t *pieces, uint64_t cap,
                               uint64_t *n_pieces)
{
    if ((n && !lens) || world < 1 || !n_pieces || (cap && !pieces)) return CRP_ERR_INVALID;
    for (uint64_t k = 0; k < n; ++k)
        if (lens[k] >> 62) return CRP_ERR_INVALID;
    std::vector<crp::Piece> out;
    try {
        crp::plan_shares(lens, n, world, min_piece ? min_piece : 4096, CRP_HALO, out);
    } catch (...) {
        return CRP_ERR_NOMEM;
    }
    *n_pieces = out.size();
    if (out.size() > cap) return CRP_ERR_CAPACITY;
    for (size_t q = 0; q < out.size(); ++q) {
        const uint64_t row[4] = {out[q].contig, out[q].start, out[q].end, out[q].group};
        std::memcpy(pieces + 4 * q, row, sizeof row);
    }
    return CRP_OK;
}
