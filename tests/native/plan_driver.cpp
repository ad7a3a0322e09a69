// Sanitizer + fuzz driver for the node's cut (crp_plan.cpp): random contig-length lists over 1..17 devices through
// crp_plan_shares under ASan + UBSan; every plan must cover each contig once and in order, give the devices non-decreasing
// contiguous runs, cut at most world - 1 times, and let only a device's first piece begin -- and only its last piece end --
// inside a contig (what crp_node_gather's "one run of owned rows per table" rests on).  Also the capacity protocol.
// Then what crp_node_load and crp_scan_stream both cut by: plan_slices, pack_pieces on every device's share (against a
// restatement of the loop crp_node_load used to carry), piece_cuts and owned_run.
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "cropsr_hip.h"
#include "crp_plan.h"

#define REQUIRE(c)                                                       \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::printf("FAILED %s (line %d, trial %d)\n", #c, __LINE__, trial); \
            return 1;                                                    \
        }                                                                \
    } while (0)

// crp_node_load's former loop, restated: one device's share into arenas of at most `limit` words
static void node_loop(const crp::Piece *share, size_t n_share, const uint64_t *lens, uint64_t limit, uint64_t halo, std::vector<crp::Piece> &out)
{
    uint64_t n_slots = 0, words = 0;
    for (size_t i = 0; i < n_share; ++i) {
        uint64_t start = share[i].start;
        const uint64_t end = share[i].end, len = lens[share[i].contig];
        for (;;) {
            crp::Piece p{share[i].contig, start, end, 0, start > halo ? start - halo : 0, 0};
            p.text_len = std::min(len, p.end + halo) - p.text_lo;
            uint64_t need = (p.text_len + 63) / 64 + 1;
            if (!n_slots || words + need > limit) {  // the share goes on in a new arena
                n_slots += 1;
                words = 1;
                if (words + need > limit) {  // a piece that would not fit an empty one is cut to what one holds
                    const uint64_t chars = (limit - words - 1) * 64;
                    const uint64_t own = (chars - (p.start - p.text_lo) - halo) & ~(uint64_t)63;
                    p.end = p.start + own;
                    p.text_len = std::min(len, p.end + halo) - p.text_lo;
                    need = (p.text_len + 63) / 64 + 1;
                }
            }
            p.group = n_slots - 1;
            words += need;
            if (p.end != end) words = limit;  // a piece that ends inside its contig closes its arena
            out.push_back(p);
            if (p.end == end) break;
            start = p.end;
        }
    }
}

int main()
{
    std::mt19937_64 rng(20251004);
    for (int trial = 0; trial < 20000; ++trial) {
        const int world = 1 + (int)(rng() % 17);
        const uint64_t n = rng() % 40;
        std::vector<uint64_t> lens(n);
        const int kind = (int)(rng() % 4);
        for (auto &l : lens)
            l = kind == 0 ? rng() % 50000 : kind == 1 ? (rng() % 8 == 0 ? 1000000 + rng() % 8000000 : rng() % 30000)
                : kind == 2 ? rng() % 5000000 : (uint64_t)1 << (rng() % 34);
        const uint64_t minp = (uint64_t[]){0, 1, 64, 4096, 100000}[rng() % 5];
        uint64_t need = 0;
        REQUIRE(crp_plan_shares(lens.data(), n, world, minp, nullptr, 0, &need) == (need ? CRP_ERR_CAPACITY : CRP_OK));
        REQUIRE(need >= n && need <= n + (uint64_t)world - (n ? 1 : 0) + (n ? 0 : 0));
        std::vector<uint64_t> p(4 * need + 4);
        uint64_t got = 0;
        if (need > 1) REQUIRE(crp_plan_shares(lens.data(), n, world, minp, p.data(), need - 1, &got) == CRP_ERR_CAPACITY && got == need);
        REQUIRE(crp_plan_shares(lens.data(), n, world, minp, p.data(), need, &got) == CRP_OK && got == need);
        uint64_t q = 0, prev_dev = 0;
        for (uint64_t k = 0; k < n; ++k) {
            uint64_t at = 0;
            bool first = true;
            while (q < got && p[4 * q] == k) {
                const uint64_t s = p[4 * q + 1], e = p[4 * q + 2], d = p[4 * q + 3];
                REQUIRE(s == at && e >= s && e <= lens[k] && (e > s || lens[k] == 0) && d < (uint64_t)world && d >= prev_dev);
                if (!first) REQUIRE(d > prev_dev);               // a cut moves on to a later device
                if (s > 0) REQUIRE(q == 0 || p[4 * (q - 1) + 3] != d);  // begins inside a contig: first piece of its device
                if (e < lens[k]) REQUIRE(q + 1 == got || p[4 * (q + 1) + 3] != d);  // ends inside one: last piece of its device
                at = e;
                prev_dev = d;
                first = false;
                ++q;
            }
            REQUIRE(!first && at == lens[k]);
        }
        REQUIRE(q == got);
    }
    // plan_slices (crp_scan_stream's cut; the node handle packs a device's share into arenas by the same rule): every contig
    // covered once and in order, slices in order, no slice over its word limit, and only a slice's FIRST piece begins -- only
    // its LAST ends -- inside a contig
    for (int trial = 0; trial < 20000; ++trial) {
        const uint64_t halo = 128;
        const uint64_t n = rng() % 30;
        std::vector<uint64_t> lens(n);
        const int kind = (int)(rng() % 3);
        for (auto &l : lens) l = kind == 0 ? rng() % 3000 : kind == 1 ? rng() % 200000 : (rng() % 6 == 0 ? 500000 + rng() % 3000000 : rng() % 20000);
        const uint64_t lo = crp::slice_words_min(halo);
        const uint64_t limit = rng() % 4 == 0 ? lo + rng() % 8 : lo + rng() % 20000;
        std::vector<std::array<uint64_t, 4>> out;
        crp::plan_slices(lens.data(), n, limit, halo, out);
        size_t q = 0;
        uint64_t prev_slice = 0, used = 1;
        for (uint64_t k = 0; k < n; ++k) {
            uint64_t at = 0;
            bool first = true;
            while (q < out.size() && out[q][0] == k) {
                const uint64_t s = out[q][1], e = out[q][2], sl = out[q][3];
                REQUIRE(s == at && e >= s && e <= lens[k] && (e > s || lens[k] == 0) && sl >= prev_slice && sl <= prev_slice + 1);
                if (sl != prev_slice) used = 1;
                const uint64_t text_lo = s > halo ? s - halo : 0, text_end = std::min(lens[k], e + halo);
                used += (text_end - text_lo + 63) / 64 + 1;
                REQUIRE(used <= limit);
                if (s > 0) REQUIRE(q == 0 || out[q - 1][3] != sl);                  // begins inside a contig: first piece of its slice
                if (e < lens[k]) REQUIRE(q + 1 == out.size() || out[q + 1][3] != sl);  // ends inside one: last piece of its slice
                at = e;
                prev_slice = sl;
                first = false;
                ++q;
            }
            REQUIRE(!first && at == lens[k]);
        }
        REQUIRE(q == out.size());
    }
    // pack_pieces on every device's share of a random plan_shares result (what crp_node_load does), and piece_cuts on every
    // arena that comes out.  Lengths: the kinds of the first loop (kind 3 reaches 2^33 characters), and a kind whose contigs
    // reach 2^32 - 1, the longest the tables' 32-bit positions take, so that the piece map's sub[] wraps.  Kinds 3 and 4 lift
    // the limit by total / (64 * 4096) words: a trial then makes a few thousand cuts, not a hundred million.
    for (int trial = 0; trial < 3000; ++trial) {
        const uint64_t halo = 128;
        const int world = 1 + (int)(rng() % 17);
        const int kind = (int)(rng() % 5);
        const uint64_t n = kind == 4 ? rng() % 4 : rng() % 40;
        std::vector<uint64_t> lens(n);
        uint64_t total = 0, longest = 0;
        for (auto &l : lens) {
            l = kind == 0 ? rng() % 50000 : kind == 1 ? (rng() % 8 == 0 ? 1000000 + rng() % 8000000 : rng() % 30000)
                : kind == 2 ? rng() % 5000000 : kind == 3 ? (uint64_t)1 << (rng() % 34) : 0xFFFFFFFFull - (rng() % 3 ? rng() % 1000 : 0);
            total += l;
            longest = std::max(longest, l);
        }
        const uint64_t minp = (uint64_t[]){1, 64, 4096, 100000}[rng() % 4];
        const uint64_t lo = crp::slice_words_min(halo) + (kind >= 3 ? total / (64 * 4096) : 0);
        const uint64_t limit = rng() % 4 == 0 ? lo + rng() % 8 : lo + rng() % 20000;
        std::vector<crp::Piece> shares, out, ref;
        std::vector<uint64_t> off;
        std::vector<uint32_t> needles, map, map_only;
        crp::plan_shares(lens.data(), n, world, minp, halo, shares);
        for (size_t q = 0; q < shares.size();) {
            size_t n_run = 1;
            while (q + n_run < shares.size() && shares[q + n_run].group == shares[q].group) ++n_run;
            out.clear();
            ref.clear();
            crp::pack_pieces(&shares[q], n_run, lens.data(), limit, halo, out);
            node_loop(&shares[q], n_run, lens.data(), limit, halo, ref);
            REQUIRE(out.size() == ref.size());
            size_t at = 0;
            uint64_t used = 1, prev_arena = 0;
            for (size_t i = 0; i < n_run; ++i) {  // the share covered once and in order
                const crp::Piece &sh = shares[q + i];
                uint64_t pos = sh.start;
                bool first = true;
                while (at < out.size() && out[at].contig == sh.contig && (first || pos < sh.end)) {
                    const crp::Piece &p = out[at], &r = ref[at];
                    REQUIRE(p.contig == r.contig && p.start == r.start && p.end == r.end && p.group == r.group && p.text_lo == r.text_lo && p.text_len == r.text_len);
                    REQUIRE(p.start == pos && p.end >= p.start && p.end <= sh.end && (p.end > p.start || sh.end == sh.start));
                    REQUIRE(p.group >= prev_arena && p.group <= prev_arena + 1 && (at > 0 || p.group == 0));
                    if (p.group != prev_arena) used = 1;
                    const uint64_t text_lo = p.start > halo ? p.start - halo : 0, text_end = std::min(lens[p.contig], p.end + halo);
                    REQUIRE(p.text_lo == text_lo && p.text_len == text_end - text_lo);
                    used += (p.text_len + 63) / 64 + 1;
                    REQUIRE(used <= limit);
                    if (p.start > 0) REQUIRE(at == 0 || out[at - 1].group != p.group);                      // begins inside a contig: first piece of its arena
                    if (p.end < lens[p.contig]) REQUIRE(at + 1 == out.size() || out[at + 1].group != p.group);  // ends inside one: last piece of its arena
                    pos = p.end;
                    prev_arena = p.group;
                    first = false;
                    ++at;
                }
                REQUIRE(!first && pos == sh.end);
            }
            REQUIRE(at == out.size());
            q += n_run;
            if (longest > 0xFFFFFFFFull) continue;  // (no such contig is loaded: positions are 32-bit)
            // piece_cuts, arena by arena, the texts at ascending arena offsets that do not overlap
            for (size_t a0 = 0, a1; a0 < out.size(); a0 = a1) {
                for (a1 = a0 + 1; a1 < out.size() && out[a1].group == out[a0].group;) ++a1;
                const size_t np = a1 - a0;
                off.resize(np);
                uint64_t cur = 64;
                for (size_t j = 0; j < np; ++j) {
                    off[j] = cur;
                    cur += out[a0 + j].text_len + 1 + rng() % 200;
                }
                needles.assign(2 * np, 0);
                map.assign(2 * np, 0);
                map_only.assign(2 * np, 0);
                crp::piece_cuts(&out[a0], np, off.data(), needles.data(), map.data());
                crp::piece_cuts(&out[a0], np, off.data(), nullptr, map_only.data());
                REQUIRE(map == map_only);
                for (size_t j = 0; j < np; ++j) REQUIRE(map[j] == needles[2 * j]);
                for (int pick = 0; pick < (np == 1 ? 1 : 10); ++pick) {  // the first piece, the last, and some between
                    const size_t j = pick == 0 ? 0 : pick == 1 ? np - 1 : rng() % np;
                    const crp::Piece &p = out[a0 + j];
                    if (p.end == p.start) {  // (an empty contig owns nothing)
                        REQUIRE(needles[2 * j] == needles[2 * j + 1]);
                        continue;
                    }
                    const uint64_t cs[3] = {p.start, p.end - 1, p.start + rng() % (p.end - p.start)};
                    for (uint64_t c : cs) {
                        const uint64_t a = off[j] + (c - p.text_lo);
                        for (size_t i = 0; i < np; ++i) REQUIRE((needles[2 * i] <= a && a < needles[2 * i + 1]) == (i == j));
                        REQUIRE((uint32_t)((uint32_t)a - map[np + j]) == c);
                    }
                }
            }
        }
    }
    // owned_run: bounds made from per-piece counts are one run, with that first, last and those counts; one entry nudged
    // -- an end before its begin, or a gap before the next piece's begin -- and they are not
    int refused_end = 0, refused_gap = 0;
    for (int trial = 0; trial < 20000; ++trial) {
        const size_t np = 1 + rng() % 40;
        std::vector<uint32_t> want(np), b(2 * np), got(np, 77);
        uint32_t cum = 1 + (uint32_t)(rng() % 1000);
        for (size_t j = 0; j < np; ++j) {
            want[j] = rng() % 3 == 0 ? 0 : (uint32_t)(rng() % 50);
            b[2 * j] = cum;
            b[2 * j + 1] = cum += want[j];
        }
        uint64_t first = 0, last = 0;
        REQUIRE(crp::owned_run(b.data(), np, &first, &last, got.data()) && first == b[0] && last == cum && got == want);
        const size_t j = rng() % np;
        if (want[j] == 0) refused_end += 1;  // the end falls before the begin
        else if (j + 1 < np) refused_gap += 1;  // the end still at or after the begin, the next begin no longer at the end
        else continue;
        b[2 * j + 1] -= 1;
        REQUIRE(!crp::owned_run(b.data(), np, &first, &last, got.data()));
    }
    int trial = -1;
    REQUIRE(refused_end > 1000 && refused_gap > 1000);
    uint64_t x = 0, one = (uint64_t)1 << 63;
    REQUIRE(crp_plan_shares(&one, 1, 2, 0, nullptr, 0, &x) == CRP_ERR_INVALID);
    REQUIRE(crp_plan_shares(nullptr, 0, 3, 0, nullptr, 0, &x) == CRP_OK && x == 0);
    std::printf("OK\n");
    return 0;
}
