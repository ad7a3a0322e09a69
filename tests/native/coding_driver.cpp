// Sanitizer driver for the coding position, compiled with crp_annotation.cpp under ASan + UBSan.
//   1. crp_coding.h -- the one function the selection kernel, the evaluation kernel and this program call -- over hand-made
//      step functions against a brute-force count over per-letter membership, with L_P and off near 2^32, where 100 off
//      needs its 64 bits (the brute force multiplies in 128), on both strands and with limits hit with equality.
//   2. the GFF model builder and crp_annotation_coding_layout over the files named on the command line (the tests' zoo),
//      over every prefix of each (truncated lines) and over copies with bytes overwritten (garbage): the capacity protocol,
//      and the invariants of the step function the device code relies on.
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <random>
#include <string>
#include <vector>

#include "cropsr_hip.h"
#include "crp_coding.h"

#define REQUIRE(c)                                                                  \
    do {                                                                            \
        if (!(c)) {                                                                 \
            std::printf("FAILED %s (line %d, case %s)\n", #c, __LINE__, what.c_str()); \
            return 1;                                                               \
        }                                                                           \
    } while (0)

namespace {

struct Hand {
    std::vector<uint32_t> at, word, cum;
    std::vector<std::vector<std::pair<int, int>>> tx;  // letters [a, b] of the text 0..99; tx[0] is P
    uint64_t before, L;                                // P's letters before the text, and L_P
};

constexpr uint32_t I = crp::CODING_INSIDE_BIT, G = crp::CODING_GROW_BIT;

// P = [10, 19] [30, 30] [40, 41], a second transcript = [10, 14] [40, 60]; `before` letters of P lie before the text
Hand hand(uint64_t before, uint64_t L)
{
    Hand h;
    const uint32_t b = (uint32_t)before;
    h.at = {10, 11, 15, 20, 30, 31, 40, 41, 42, 61};
    h.word = {G, 2 | I | G, 1 | I | G, 0, G, 0, G, 2 | I | G, 1, 0};
    h.cum = {b, b + 1, b + 5, b + 10, b + 10, b + 11, b + 11, b + 12, b + 13, b + 13};
    h.tx = {{{10, 19}, {30, 30}, {40, 41}}, {{10, 14}, {40, 60}}};
    h.before = before;
    h.L = L;
    return h;
}

int check_hand(const Hand &h, bool minus, const crp::CodingLimits &lim, uint64_t *n_pass, const std::string &what)
{
    std::vector<std::vector<char>> letter(h.tx.size(), std::vector<char>(102, 0));
    for (size_t t = 0; t < h.tx.size(); ++t)
        for (auto ab : h.tx[t])
            for (int p = ab.first; p <= ab.second; ++p) letter[t][p] = 1;
    const uint32_t info = (uint32_t)h.tx.size() | (minus ? crp::CODING_MINUS_BIT : 0u) | crp::CODING_MODEL_BIT;
    for (uint32_t c = 0; c <= 100; ++c) {
        uint32_t cover = 0;
        for (size_t t = 0; t < h.tx.size(); ++t) cover += c >= 1 && letter[t][c - 1] && letter[t][c];
        const bool inside = c >= 1 && letter[0][c - 1] && letter[0][c];
        uint64_t before = h.before;
        for (uint32_t p = 0; p < c; ++p) before += letter[0][p];
        const uint64_t off = minus ? h.L - before : before;
        const crp::CodingPosition got = crp::coding_position(h.at.data(), h.word.data(), h.cum.data(), (uint32_t)h.at.size(), (uint32_t)h.L, info, c);
        REQUIRE(got.cover == cover);
        REQUIRE(got.off == (inside ? (uint32_t)off : crp::CODING_NOT_INSIDE));
        if (inside) REQUIRE(off >= 1 && off <= h.L - 1);
        const unsigned __int128 off100 = (unsigned __int128)100 * off;
        const bool want = inside && (unsigned __int128)lim.min_pct * h.L <= off100 && off100 <= (unsigned __int128)lim.max_pct * h.L &&
                          100u * cover >= lim.min_transcripts_pct * (uint32_t)h.tx.size();
        REQUIRE(crp::coding_pass(got, (uint32_t)h.L, info, lim) == want);
        *n_pass += want;
        // a gene without a model, and a row without steps
        REQUIRE(crp::coding_position(h.at.data(), h.word.data(), h.cum.data(), (uint32_t)h.at.size(), (uint32_t)h.L, info & 0xFFFFu, c).off == crp::CODING_NOT_INSIDE);
        REQUIRE(!crp::coding_pass(crp::coding_position(nullptr, nullptr, nullptr, 0, (uint32_t)h.L, info, c), (uint32_t)h.L, info, lim));
    }
    return 0;
}

int hand_made()
{
    std::string what = "hand-made";
    const uint64_t top = 0xFFFFFFFFull;
    uint64_t n_pass = 0, n_equal = 0, unused = 0;
    for (int minus = 0; minus < 2; ++minus) {
        // off near 2^32 on the '+' strand (letters before the text) and on the '-' strand (letters after it)
        for (uint64_t before : {uint64_t(0), uint64_t(1000), top - 13 - 700, top - 13})
            for (const crp::CodingLimits &lim : {crp::CodingLimits{0, 100, 0}, crp::CodingLimits{5, 65, 0}, crp::CodingLimits{0, 0, 0},
                                                 crp::CodingLimits{99, 100, 0}, crp::CodingLimits{0, 100, 100}, crp::CodingLimits{0, 100, 51},
                                                 crp::CodingLimits{0, 1, 50}})
                if (check_hand(hand(before, top), minus != 0, lim, &n_pass, what)) return 1;
        // equality: L_P a multiple of 100 and a cut with 100 off = 50 L_P exactly, which no other percentage pair keeps
        const uint64_t L = 4294967200ull, half = L / 2;
        const Hand h = hand(minus ? L - half - 2 : half - 2, L);  // the boundary 12 has two of the text's letters before it
        if (check_hand(h, minus != 0, crp::CodingLimits{50, 50, 0}, &n_equal, what)) return 1;
        if (check_hand(h, minus != 0, crp::CodingLimits{51, 100, 0}, &unused, what)) return 1;
    }
    REQUIRE(n_pass > 0);
    REQUIRE(n_equal == 2);  // one boundary per strand
    // 32-bit products would have got these wrong: 100 off wraps
    const Hand h = hand(top - 13 - 700, top);
    const uint32_t info = 2u | crp::CODING_MODEL_BIT;
    const crp::CodingPosition p = crp::coding_position(h.at.data(), h.word.data(), h.cum.data(), (uint32_t)h.at.size(), (uint32_t)h.L, info, 12);
    REQUIRE(p.off == (uint32_t)(top - 13 - 700 + 2));
    REQUIRE(crp::coding_pass(p, (uint32_t)h.L, info, crp::CodingLimits{99, 100, 0}));
    REQUIRE(!crp::coding_pass(p, (uint32_t)h.L, info, crp::CodingLimits{0, 98, 0}));
    return 0;
}

// One annotation through the model and the layout: the capacity protocol and the step function's invariants.
int drive(const std::string &text, const std::string &what)
{
    crp_annotation *an = nullptr;
    REQUIRE(crp_annotation_build(reinterpret_cast<const uint8_t *>(text.data()), text.size(), nullptr, 0, &an) == CRP_OK);
    uint64_t n_seq = 0, n_genes = 0;
    REQUIRE(crp_annotation_stats(an, &n_seq, nullptr, nullptr, &n_genes, nullptr) == CRP_OK);
    std::vector<uint8_t> strand(n_genes + 1);
    std::vector<uint32_t> n_tx(n_genes + 1), len(n_genes + 1);
    REQUIRE(crp_annotation_gene_coding(an, strand.data(), n_tx.data(), len.data()) == CRP_OK);
    for (uint64_t g = 0; g < n_genes; ++g) {
        REQUIRE(strand[g] == '+' || strand[g] == '-' || strand[g] == '.');
        REQUIRE((n_tx[g] == 0) == (len[g] == 0));
        if (strand[g] == '.') REQUIRE(n_tx[g] == 0);
    }
    for (int dec = 0; dec < 2; ++dec) {
        // every seqid whole, then a piece of it that starts 37 letters in
        std::vector<uint64_t> entries;
        uint64_t base = 64;
        for (uint64_t k = 0; k <= n_seq; ++k)  // (one seqid too many: it names nothing)
            for (int piece = 0; piece < 2; ++piece) {
                const uint64_t first = piece ? 37 : 0, length = piece ? 150 : 400;
                entries.insert(entries.end(), {k, first, length, base});
                base += 512;
            }
        const uint64_t n_entries = entries.size() / 4;
        uint64_t rows = 0, steps = 0, rows2 = 0, steps2 = 0, plain = 0;
        const int rc = crp_annotation_coding_layout(an, entries.data(), n_entries, dec, nullptr, nullptr, nullptr, 0, &rows, nullptr, nullptr, nullptr, 0, &steps);
        REQUIRE(rc == (rows || steps ? CRP_ERR_CAPACITY : CRP_OK));
        REQUIRE(crp_annotation_gene_layout(an, entries.data(), n_entries, dec, nullptr, nullptr, nullptr, 0, &plain) == (plain ? CRP_ERR_CAPACITY : CRP_OK));
        REQUIRE(rows == plain);
        std::vector<uint32_t> info(rows + 1), length(rows + 1), at(steps + 1), word(steps + 1), cum(steps + 1), lo(rows + 1), hi(rows + 1);
        std::vector<uint64_t> first(rows + 2), gene(rows + 1);
        if (steps) {  // too small for the steps alone: nothing is written past the capacity
            at[steps - 1] = word[steps - 1] = cum[steps - 1] = 0xABCDEF01u;
            REQUIRE(crp_annotation_coding_layout(an, entries.data(), n_entries, dec, info.data(), length.data(), first.data(), rows, &rows2, at.data(),
                                                 word.data(), cum.data(), steps - 1, &steps2) == CRP_ERR_CAPACITY);
            REQUIRE(rows2 == rows && steps2 == steps && at[steps - 1] == 0xABCDEF01u && word[steps - 1] == 0xABCDEF01u && cum[steps - 1] == 0xABCDEF01u);
        }
        REQUIRE(crp_annotation_coding_layout(an, entries.data(), n_entries, dec, info.data(), length.data(), first.data(), rows, &rows2, at.data(),
                                             word.data(), cum.data(), steps, &steps2) == CRP_OK);
        REQUIRE(rows2 == rows && steps2 == steps);
        REQUIRE(crp_annotation_gene_layout(an, entries.data(), n_entries, dec, lo.data(), hi.data(), gene.data(), rows, &plain) == CRP_OK);
        first[rows] = steps;
        for (uint64_t r = 0; r < rows; ++r) {
            const uint64_t g = gene[r];
            REQUIRE(g < n_genes && first[r] <= first[r + 1] && first[r + 1] <= steps);
            const bool model = n_tx[g] != 0;
            REQUIRE(info[r] == (model ? n_tx[g] | (strand[g] == '-' ? crp::CODING_MINUS_BIT : 0u) | crp::CODING_MODEL_BIT : 0u));
            REQUIRE(length[r] == len[g]);
            if (!model) REQUIRE(first[r] == first[r + 1]);
            // which text the row lies in
            uint64_t e = 0;
            while (!(entries[4 * e + 3] <= lo[r] && lo[r] < entries[4 * e + 3] + entries[4 * e + 2])) e += 1;
            const uint64_t text_lo = entries[4 * e + 3], text_end = text_lo + entries[4 * e + 2];
            uint32_t last = 0;
            for (uint64_t k = first[r]; k < first[r + 1]; ++k) {
                REQUIRE(at[k] >= text_lo && at[k] <= text_end);  // clipped to the text
                if (k > first[r]) REQUIRE(at[k] > at[k - 1] && cum[k] >= cum[k - 1] && cum[k] - cum[k - 1] <= at[k] - at[k - 1]);
                REQUIRE(word[k] != last && (word[k] & 0xFFFFu) <= n_tx[g] && cum[k] <= len[g]);
                if (word[k] & crp::CODING_INSIDE_BIT) REQUIRE((word[k] & 0xFFFFu) >= 1 && (word[k] & crp::CODING_GROW_BIT));
                last = word[k];
            }
            REQUIRE(last == 0);  // every row ends with nothing holding
            const uint32_t n = (uint32_t)(first[r + 1] - first[r]);
            for (uint64_t c = text_lo > 3 ? text_lo - 3 : 0; c <= text_end + 3; ++c) {
                const crp::CodingPosition p = crp::coding_position(at.data() + first[r], word.data() + first[r], cum.data() + first[r], n, length[r], info[r], (uint32_t)c);
                REQUIRE(p.cover <= n_tx[g]);
                if (p.off != crp::CODING_NOT_INSIDE) REQUIRE(p.off >= 1 && p.off <= length[r] - 1 && c > text_lo && c < text_end);
            }
        }
    }
    REQUIRE(crp_annotation_destroy(an) == CRP_OK);
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (hand_made()) return 1;
    std::mt19937 rng(20);
    for (int f = 1; f < argc; ++f) {
        std::ifstream in(argv[f], std::ios::binary);
        const std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        const std::string what = argv[f];
        if (text.empty()) {
            std::printf("FAILED: %s is empty or missing\n", argv[f]);
            return 1;
        }
        for (size_t n = 0; n <= text.size(); ++n)  // truncated: every prefix
            if (drive(text.substr(0, n), what + " prefix")) return 1;
        for (int trial = 0; trial < 60; ++trial) {  // garbage: bytes overwritten, tabs and separators among them
            std::string t = text;
            const int n = 1 + (int)(rng() % 6);
            for (int j = 0; j < n; ++j) t[rng() % t.size()] = "\t\n;=,+-.09x \0"[rng() % 13];
            if (drive(t, what + " garbage")) return 1;
        }
    }
    // a gene with more than 65 535 coding transcripts: the layout refuses it, the per-gene view still counts them
    {
        const std::string what = "65 536 transcripts";
        std::string t = "s\tx\tgene\t1\t300\t.\t+\t.\tID=g\n";
        for (int k = 0; k < 65536; ++k) {
            const std::string id = "t" + std::to_string(k);
            t += "s\tx\tmRNA\t1\t300\t.\t+\t.\tID=" + id + ";Parent=g\ns\tx\tCDS\t10\t20\t.\t+\t.\tParent=" + id + "\n";
        }
        crp_annotation *an = nullptr;
        REQUIRE(crp_annotation_build(reinterpret_cast<const uint8_t *>(t.data()), t.size(), nullptr, 0, &an) == CRP_OK);
        uint32_t n_tx = 0;
        REQUIRE(crp_annotation_gene_coding(an, nullptr, &n_tx, nullptr) == CRP_OK && n_tx == 65536);
        const uint64_t entry[4] = {0, 0, 400, 64};
        uint64_t rows = 0, steps = 0;
        REQUIRE(crp_annotation_coding_layout(an, entry, 1, 0, nullptr, nullptr, nullptr, 0, &rows, nullptr, nullptr, nullptr, 0, &steps) == CRP_ERR_UNSUPPORTED);
        crp_annotation_destroy(an);
    }
    std::printf("OK\n");
    return 0;
}
