// Sanitizer driver for the base-editing test, compiled stand-alone under ASan + UBSan.
// crp_edit.h -- the one function the selection kernel, the evaluation kernel and this program call -- over hand-made
// planes and step functions against a brute-force loop over letters: every row position of a 256-letter text and beyond
// it on both row strands and both gene strands, every window of the tests, spans that straddle two plane words, begin at
// bit 0, lie in word 0 and in the last word, reach below position 0 and past the planes (the planes are allocated to
// the word, so a read outside them is ASan's to find), L_P near 2^32, zero steps, one step, and the limits with
// products that need their 64 bits.
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "crp_edit.h"

#define REQUIRE(c)                                                                  \
    do {                                                                            \
        if (!(c)) {                                                                 \
            std::printf("FAILED %s (line %d, case %s)\n", #c, __LINE__, what.c_str()); \
            return 1;                                                               \
        }                                                                           \
    } while (0)

namespace {

constexpr uint32_t I = crp::CODING_INSIDE_BIT, G = crp::CODING_GROW_BIT;
constexpr int N = 256;  // letters of the text: four plane words

struct Text {
    std::string s;                     // N letters
    std::vector<uint64_t> hi, lo, ac;  // exactly n_words words each
    uint64_t n_words;
};

int code_of(char ch)
{
    switch (ch) {
    case 'A': case 'a': case 'U': case 'u': return 0;
    case 'T': case 't': return 1;
    case 'C': case 'c': return 2;
    case 'G': case 'g': return 3;
    }
    return -1;
}

// the planes of s; the hi / lo bits of a non-base are garbage, which the function must mask; words at and beyond n_words
// do not exist
Text text_of(const std::string &s, uint64_t n_words, std::mt19937 &rng)
{
    Text t;
    t.s = s;
    t.n_words = n_words;
    t.hi.assign(n_words, 0);
    t.lo.assign(n_words, 0);
    t.ac.assign(n_words, 0);
    for (int x = 0; x < N && (uint64_t)(x >> 6) < n_words; ++x) {
        const int c = code_of(s[x]);
        const uint64_t bit = 1ull << (x & 63);
        if (c >= 0) t.ac[x >> 6] |= bit;
        const int v = c >= 0 ? c : (int)(rng() & 3);
        if (v & 2) t.hi[x >> 6] |= bit;
        if (v & 1) t.lo[x >> 6] |= bit;
    }
    return t;
}

struct Model {
    std::vector<uint32_t> at, word, cum;
    uint64_t L;
};

// exons [a, b] (ascending, apart) as the layout writes them: a (grow), a + 1 (inside), b + 1 (nothing); `before` letters
// of P lie before the text and `after` behind it
Model model_of(const std::vector<std::pair<int, int>> &exons, uint64_t before, uint64_t after)
{
    Model m;
    uint64_t c = before;
    for (auto ab : exons) {
        m.at.push_back((uint32_t)ab.first);
        m.word.push_back(G);
        m.cum.push_back((uint32_t)c);
        if (ab.second > ab.first) {
            m.at.push_back((uint32_t)ab.first + 1);
            m.word.push_back(1u | I | G);
            m.cum.push_back((uint32_t)c + 1);
        }
        c += (uint64_t)(ab.second - ab.first + 1);
        m.at.push_back((uint32_t)ab.second + 1);
        m.word.push_back(0);
        m.cum.push_back((uint32_t)c);
    }
    m.L = c + after;
    return m;
}

// the letter at x: 'A', 'C', 'G', 'T' or 0 for a non-base (outside the words that exist too)
char base_at(const Text &t, long long x)
{
    if (x < 0 || x >= N || (uint64_t)(x >> 6) >= t.n_words) return 0;
    const int c = code_of(t.s[(size_t)x]);
    return c < 0 ? 0 : "ATCG"[c];
}

// the coding index of letter x in the gene's orientation, -1 where x is no coding letter of P (the steps, letter by letter)
long long index_at(const Model &m, bool minus_gene, long long x)
{
    if (x < 0) return -1;
    long long k = -1;
    for (size_t j = 0; j < m.at.size(); ++j)
        if ((long long)m.at[j] <= x) k = (long long)j;
    if (k < 0 || !(m.word[(size_t)k] & G)) return -1;
    const long long c = (long long)m.cum[(size_t)k] + (x - (long long)m.at[(size_t)k]);
    return minus_gene ? (long long)m.L - 1 - c : c;
}

bool is_stop(const char *c) { return c[0] == 'T' && ((c[1] == 'A' && (c[2] == 'A' || c[2] == 'G')) || (c[1] == 'G' && c[2] == 'A')); }

char complement(char b) { return b == 'A' ? 'T' : b == 'T' ? 'A' : b == 'C' ? 'G' : 'C'; }

// index_at for x = -PAD .. N + 2 PAD - 1, once per (model, gene strand)
constexpr int PAD = 30;
std::vector<long long> indices(const Model &m, bool minus_gene)
{
    std::vector<long long> idx;
    for (long long x = -PAD; x < N + 2 * PAD; ++x) idx.push_back(index_at(m, minus_gene, x));
    return idx;
}

crp::EditOutcome brute(const Text &t, const Model &m, const std::vector<long long> &idx, bool minus_gene, uint32_t pos, bool minus_row, crp::EditWindow w)
{
    crp::EditOutcome out = {0, 0, crp::EDIT_NO_STOP};
    std::vector<long long> targets;
    for (uint32_t p = w.lo; p <= w.hi; ++p) {
        const long long x = minus_row ? (long long)pos + 23 - p : (long long)pos - 21 + p;
        if (base_at(t, x) == (minus_row ? 'G' : 'C')) targets.push_back(x);
    }
    out.targets = (uint32_t)targets.size();
    auto is_target = [&](long long x) {
        for (long long y : targets)
            if (y == x) return true;
        return false;
    };
    long long best = -1;
    for (long long x = -PAD + 2; x < N + 2 * PAD - 2; ++x) {  // the first letter of a codon, in the gene's orientation
        const long long i = idx[(size_t)(x + PAD)];
        if (i < 0 || i % 3 || i + 2 >= (long long)m.L) continue;
        char before[3], after[3];
        bool whole = true;
        for (int j = 0; j < 3; ++j) {
            const long long y = minus_gene ? x - j : x + j;
            const char b = base_at(t, y);
            if (idx[(size_t)(y + PAD)] != i + j || !b) {
                whole = false;
                break;
            }
            const char e = is_target(y) ? (minus_row ? 'A' : 'T') : b;
            before[j] = minus_gene ? complement(b) : b;
            after[j] = minus_gene ? complement(e) : e;
        }
        if (!whole || is_stop(before) || !is_stop(after)) continue;
        out.stops += 1;
        if (best < 0 || i < best) best = i;
    }
    if (best >= 0) out.stop_off = (uint32_t)best;
    return out;
}

int compare(const Text &t, const Model &m, const std::string &what, uint64_t *n_stops, uint64_t *n_pass)
{
    const crp::EditPlanes planes = {t.hi.data(), t.lo.data(), t.ac.data(), t.n_words};
    const crp::EditWindow windows[] = {{4, 8}, {1, 20}, {1, 1}, {20, 20}, {13, 17}};
    const crp::EditLimits limits[] = {{0, 100, 20}, {5, 65, 20}, {0, 100, 0}, {0, 100, 1}, {50, 50, 20}, {99, 100, 3}};
    for (const crp::EditWindow &w : windows)
        for (int strands = 0; strands < 4; ++strands) {
            const bool minus_gene = strands & 1, minus_row = strands & 2;
            const uint32_t info = 1u | (minus_gene ? crp::CODING_MINUS_BIT : 0u) | crp::CODING_MODEL_BIT;
            const std::vector<long long> idx = indices(m, minus_gene);
            for (uint32_t pos = 0; pos < (uint32_t)N + 40; ++pos) {
                const crp::EditOutcome want = brute(t, m, idx, minus_gene, pos, minus_row, w);
                const crp::EditOutcome got = crp::edit_outcome(planes, m.at.data(), m.word.data(), m.cum.data(), (uint32_t)m.at.size(), (uint32_t)m.L,
                                                               info, pos, minus_row, w);
                REQUIRE(got.targets == want.targets);
                REQUIRE(got.stops == want.stops);
                REQUIRE(got.stop_off == want.stop_off);
                REQUIRE(got.targets <= w.hi - w.lo + 1 && (got.stops == 0) == (got.stop_off == crp::EDIT_NO_STOP));
                if (got.stops) REQUIRE(got.stop_off % 3 == 0 && (uint64_t)got.stop_off + 2 < m.L);
                *n_stops += got.stops;
                for (const crp::EditLimits &lim : limits) {
                    const unsigned __int128 off100 = (unsigned __int128)100 * want.stop_off;
                    const bool pass = want.stop_off != crp::EDIT_NO_STOP && (unsigned __int128)lim.min_pct * m.L <= off100 &&
                                      off100 <= (unsigned __int128)lim.max_pct * m.L && want.targets <= lim.max_targets;
                    REQUIRE(crp::edit_pass(got, (uint32_t)m.L, lim) == pass);
                    *n_pass += pass;
                }
                // a gene without a model, and a row without steps: the targets alone
                const crp::EditOutcome bare = crp::edit_outcome(planes, m.at.data(), m.word.data(), m.cum.data(), (uint32_t)m.at.size(), (uint32_t)m.L,
                                                                info & 0x1FFFFu, pos, minus_row, w);
                const crp::EditOutcome none = crp::edit_outcome(planes, nullptr, nullptr, nullptr, 0, (uint32_t)m.L, info, pos, minus_row, w);
                REQUIRE(bare.targets == want.targets && bare.stops == 0 && bare.stop_off == crp::EDIT_NO_STOP);
                REQUIRE(none.targets == want.targets && none.stops == 0 && none.stop_off == crp::EDIT_NO_STOP);
            }
        }
    return 0;
}

std::string random_text(std::mt19937 &rng, const char *alphabet, int n_alpha)
{
    std::string s(N, 'A');
    for (int x = 0; x < N; ++x) s[x] = alphabet[rng() % n_alpha];
    return s;
}

}  // namespace

int main()
{
    std::mt19937 rng(21);
    uint64_t n_stops = 0, n_pass = 0;
    const uint64_t top = 0xFFFFFFFFull;
    // letters rich in what the editor turns into stops, so that every case of the closed form occurs many times
    std::string rich(N, 'A');
    const char *pieces[] = {"CAA", "CAG", "CGA", "TGG", "TTG", "CTG", "TCG", "CCA", "TAG", "CCC", "GGG", "CNA", "cag", "tgg", "AUA"};
    for (int x = 0; x + 3 <= N; x += 3) {
        const char *p = pieces[rng() % 15];
        rich[x] = p[0], rich[x + 1] = p[1], rich[x + 2] = p[2];
    }
    const std::vector<std::vector<std::pair<int, int>>> exon_sets = {
        {{0, 255}},                                               // one exon over the whole text: spans at bit 0 and in the last word
        {{3, 62}, {64, 64}, {66, 130}, {140, 141}, {190, 255}},   // edges at the words' seams, one- and two-letter exons
        {{10, 20}, {22, 24}, {26, 27}, {29, 33}, {35, 35}, {37, 39}, {41, 60}, {62, 70}},  // many steps inside one span
        {{100, 102}},                                             // one codon
        {},                                                       // zero steps
    };
    int n = 0;
    for (const auto &exons : exon_sets)
        for (int frame = 0; frame < 3; ++frame)
            for (int kind = 0; kind < 3; ++kind) {
                const std::string what = "exon set " + std::to_string(n++ / 9) + " frame " + std::to_string(frame) + " kind " + std::to_string(kind);
                const std::string s = kind == 0 ? rich : kind == 1 ? random_text(rng, "ACGT", 4) : random_text(rng, "ACGTNacgtu-", 11);
                uint64_t letters = 0;
                for (auto ab : exons) letters += (uint64_t)(ab.second - ab.first + 1);
                // P's letters before and behind the text: small, and such that L_P and the offsets lie near 2^32
                for (uint64_t before : {uint64_t(frame), top - letters - 7 - (uint64_t)frame}) {
                    const Model m = model_of(exons, before, top - before - letters >= 7 ? 7 : 0);
                    for (uint64_t n_words : {uint64_t(4), uint64_t(3), uint64_t(1), uint64_t(0)})
                        if (n_words == 4 || kind == 0)
                            if (compare(text_of(s, n_words, rng), m, what, &n_stops, &n_pass)) return 1;
                }
            }
    // one step that never ends (crp_select_set_coding accepts any ascending model): grow from letter 5 on
    {
        const std::string what = "one step";
        Model m;
        m.at = {5};
        m.word = {G};
        m.cum = {9};
        m.L = 9 + 400;
        if (compare(text_of(rich, 4, rng), m, what, &n_stops, &n_pass)) return 1;
    }
    const std::string what = "totals";
    REQUIRE(n_stops > 1000 && n_pass > 1000);
    // 32-bit products would have got this wrong: 100 stop_off wraps
    const crp::EditOutcome o = {1, 1, 4294967100u};
    REQUIRE(crp::edit_pass(o, (uint32_t)top, crp::EditLimits{99, 100, 20}) && !crp::edit_pass(o, (uint32_t)top, crp::EditLimits{0, 98, 20}));
    std::printf("OK\n");
    return 0;
}
