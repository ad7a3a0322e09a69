// crp_plan.h -- the cut of a genome into pieces with halos: over the devices of a node, into the arenas of a device, into the
// slices of the pipelined scan -- and what the ownership cuts of an arena's tables are made from and read by (crp_plan.cpp;
// no HIP in either file: the sanitizer tests build them with g++).
#pragma once
#include <array>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace crp {

// The piece [start, end) of contig string `contig`, and the characters uploaded for it: [text_lo, text_lo + text_len) of the
// contig, the piece with up to `halo` characters of context either side.  A hit belongs to the piece its match index falls
// in.  `group` is the device (plan_shares) or the arena / slice (pack_pieces, plan_slices).
struct Piece {
    uint64_t contig, start, end, group, text_lo, text_len;
};
Piece make_piece(uint64_t contig, uint64_t start, uint64_t end, uint64_t group, uint64_t contig_len, uint64_t halo);

// the contigs dealt to `world` devices as contiguous equal shares, in contig order; throws std::bad_alloc only
void plan_shares(const uint64_t *lens, uint64_t n, int world, uint64_t min_piece, uint64_t halo, std::vector<Piece> &out);

// One ordered run of pieces (it may begin and end inside a contig, as a device's share does) packed into ARENAS of at most
// limit_words arena words each (crp_arena_words_for per text, + 1 per arena), appended to `out` with group = the arena: an
// arena is filled with whole pieces; a piece that would not fit goes on in the next arena, and one that no arena can hold is
// cut to what an arena takes (the rest follows with halos like every other piece).  Only an arena's FIRST piece can begin
// inside a contig and only its LAST can end inside one, so the owned rows of an arena's tables are one run.  limit_words must
// hold a piece of 64 owned characters between two halos (slice_words_min).  Throws std::bad_alloc only.
uint64_t slice_words_min(uint64_t halo);
void pack_pieces(const Piece *run, size_t n_run, const uint64_t *lens, uint64_t limit_words, uint64_t halo, std::vector<Piece> &out);
// whole contigs, in order, as the slices of crp_scan_stream: pack_pieces of the run {k, 0, lens[k]}; the second form gives
// {contig, start, end, slice} alone
void plan_slices(const uint64_t *lens, uint64_t n, uint64_t limit_words, uint64_t halo, std::vector<Piece> &out);
void plan_slices(const uint64_t *lens, uint64_t n, uint64_t limit_words, uint64_t halo, std::vector<std::array<uint64_t, 4>> &out);

// arena position of a piece's first owned character, its text lying at arena_off (arena_off = 0: the length of its left halo)
uint64_t owned_begin(const Piece &p, uint64_t arena_off);

// The ownership cuts of ONE arena holding pieces[0, np), piece j's text at arena_off[j]: needles {begin, end} of every
// piece's owned arena positions (what launch_lower_bound searches for in both tables), and the piece map {begin[np], sub[np]}
// that turns an arena position a of an owned row into the position inside its contig, (uint32_t)(a - sub[j]) (sub is mod 2^32).
// needles may be null (the gather's root wants the maps alone).
void piece_cuts(const Piece *pieces, size_t np, const uint64_t *arena_off, uint32_t *needles, uint32_t *map);

// The lower bounds of an arena's 2 np needles in one table: are the owned rows ONE run?  Then [*first, *last) is that run and
// counts[j] the rows piece j owns.  false: a piece's end lies before its begin, or the next piece's begin is not its end.
bool owned_run(const uint32_t *bounds, size_t np, uint64_t *first, uint64_t *last, uint32_t *counts);

}  // namespace crp
