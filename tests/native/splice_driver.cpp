// Sanitizer driver for the splice-site test, compiled stand-alone under ASan + UBSan.
// crp_splice.h -- the one function the selection kernel, the evaluation kernel and this program call -- over hand-made
// planes and step functions against a brute-force loop over letters: every row position of a 256-letter text and beyond
// it on both row strands and both gene strands with both editors, every window of the tests, spans that straddle two plane
// words, begin at bit 0, lie in word 0 and in the last word, reach below position 0 and past the planes (the planes are
// allocated to the word, so a read outside them is ASan's to find), garbage code bits under non-bases, introns of 1, 2, 3
// and 4 letters whose boundaries pass through every bit of the span as the row moves, L_P near 2^32, zero steps, one
// endless step, and the limits with products that need their 64 bits.
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "crp_splice.h"

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

// letter by letter over the steps: whether x is a coding letter of P, and cum_P at boundary x
struct At {
    bool coding;
    uint64_t cum;
};
At step_at(const Model &m, long long x)
{
    if (m.at.empty()) return {false, 0};
    long long k = -1;
    for (size_t j = 0; j < m.at.size(); ++j)
        if ((long long)m.at[j] <= x) k = (long long)j;
    if (k < 0) return {false, m.cum[0]};
    const bool grow = (m.word[(size_t)k] & G) != 0;
    return {grow, (uint64_t)m.cum[(size_t)k] + (grow ? (uint64_t)(x - (long long)m.at[(size_t)k]) : 0)};
}

constexpr int PAD = 40;

crp::SpliceOutcome brute(const Text &t, const Model &m, const std::vector<At> &st, bool minus_gene, uint32_t pos, bool minus_row, crp::EditWindow w,
                         uint32_t editor)
{
    crp::SpliceOutcome out = {0, 0, 0, crp::SPLICE_NO_SITE, crp::SPLICE_NO_SITE};
    const char from = editor == crp::SPLICE_ABE ? (minus_row ? 'T' : 'A') : (minus_row ? 'G' : 'C');
    std::vector<long long> targets;
    for (uint32_t p = w.lo; p <= w.hi; ++p) {
        const long long x = minus_row ? (long long)pos + 23 - p : (long long)pos - 21 + p;
        if (base_at(t, x) == from) targets.push_back(x);
    }
    out.targets = (uint32_t)targets.size();
    if (m.at.empty()) return out;
    auto is_target = [&](long long x) {
        for (long long y : targets)
            if (y == x) return true;
        return false;
    };
    auto at = [&](long long x) { return st[(size_t)(x + PAD)]; };
    long long best[2] = {-1, -1};  // donor, acceptor: cum_P at the intron of the site nearest the 5' end
    for (long long x = -PAD + 3; x < N + 2 * PAD - 3; ++x) {  // a boundary
        for (int ending = 0; ending < 2; ++ending) {
            long long a;  // the site's lower letter
            if (!ending) {
                if (!(at(x - 1).coding && !at(x).coding && at(x).cum < m.L)) continue;
                a = x;
            } else {
                if (!(!at(x - 1).coding && at(x).coding && at(x).cum > 0)) continue;
                a = x - 2;
            }
            const char b0 = base_at(t, a), b1 = base_at(t, a + 1);
            if (!b0 || !b1 || at(a).coding || at(a + 1).coding) continue;
            const char want0 = !ending ? (minus_gene ? 'C' : 'G') : 'A', want1 = !ending ? 'T' : (minus_gene ? 'C' : 'G');
            if (b0 != want0 || b1 != want1) continue;
            if (!is_target(a) && !is_target(a + 1)) continue;
            const int kind = (ending != 0) != minus_gene ? 1 : 0;  // '+' gene: start = donor; '-' gene: start = acceptor
            (kind ? out.acceptors : out.donors) += 1;
            const long long c = (long long)at(x).cum;
            if (best[kind] < 0 || (minus_gene ? c > best[kind] : c < best[kind])) best[kind] = c;
        }
    }
    if (best[0] >= 0) out.donor_off = (uint32_t)(minus_gene ? (long long)m.L - best[0] : best[0]);
    if (best[1] >= 0) out.acceptor_off = (uint32_t)(minus_gene ? (long long)m.L - best[1] : best[1]);
    return out;
}

struct Totals {
    uint64_t donors[2] = {0, 0}, acceptors[2] = {0, 0}, pass = 0, both = 0;
};

int compare(const Text &t, const Model &m, const std::string &what, Totals *tot)
{
    const crp::EditPlanes planes = {t.hi.data(), t.lo.data(), t.ac.data(), t.n_words};
    const crp::EditWindow windows[] = {{4, 8}, {1, 20}, {1, 1}, {20, 20}, {13, 17}};
    const crp::SpliceLimits limits[] = {{0, 100, 20, 3}, {5, 65, 20, 3}, {0, 100, 0, 3}, {0, 100, 1, 1}, {50, 50, 20, 2}, {99, 100, 3, 3}, {0, 100, 20, 1},
                                        {0, 100, 20, 2}};
    std::vector<At> st;
    for (long long x = -PAD; x < N + 2 * PAD; ++x) st.push_back(step_at(m, x));
    for (const crp::EditWindow &w : windows)
        for (int strands = 0; strands < 8; ++strands) {
            const bool minus_gene = strands & 1, minus_row = strands & 2;
            const uint32_t editor = strands & 4 ? crp::SPLICE_ABE : crp::SPLICE_CBE;
            const uint32_t info = 1u | (minus_gene ? crp::CODING_MINUS_BIT : 0u) | crp::CODING_MODEL_BIT;
            for (uint32_t pos = 0; pos < (uint32_t)N + 40; ++pos) {
                const crp::SpliceOutcome want = brute(t, m, st, minus_gene, pos, minus_row, w, editor);
                const crp::SpliceOutcome got = crp::splice_outcome(planes, m.at.data(), m.word.data(), m.cum.data(), (uint32_t)m.at.size(), (uint32_t)m.L,
                                                                   info, pos, minus_row, w, editor);
                REQUIRE(got.targets == want.targets);
                REQUIRE(got.donors == want.donors);
                REQUIRE(got.acceptors == want.acceptors);
                REQUIRE(got.donor_off == want.donor_off);
                REQUIRE(got.acceptor_off == want.acceptor_off);
                REQUIRE(got.targets <= w.hi - w.lo + 1);
                REQUIRE((got.donors == 0) == (got.donor_off == crp::SPLICE_NO_SITE) && (got.acceptors == 0) == (got.acceptor_off == crp::SPLICE_NO_SITE));
                if (got.donors) REQUIRE(got.donor_off >= 1 && (uint64_t)got.donor_off < m.L);
                if (got.acceptors) REQUIRE(got.acceptor_off >= 1 && (uint64_t)got.acceptor_off < m.L);
                tot->donors[editor] += got.donors;
                tot->acceptors[editor] += got.acceptors;
                tot->both += got.donors && got.acceptors;
                for (const crp::SpliceLimits &lim : limits) {
                    bool pass = false;
                    for (int kind = 0; kind < 2; ++kind) {
                        const uint32_t off = kind ? want.acceptor_off : want.donor_off;
                        const unsigned __int128 off100 = (unsigned __int128)100 * off;
                        pass = pass || ((lim.kinds >> kind & 1u) && off != crp::SPLICE_NO_SITE && (unsigned __int128)lim.min_pct * m.L <= off100 &&
                                        off100 <= (unsigned __int128)lim.max_pct * m.L);
                    }
                    pass = pass && want.targets <= lim.max_targets;
                    REQUIRE(crp::splice_pass(got, (uint32_t)m.L, lim) == pass);
                    tot->pass += pass;
                }
                // a gene without a model, and a row without steps: the targets alone
                const crp::SpliceOutcome bare = crp::splice_outcome(planes, m.at.data(), m.word.data(), m.cum.data(), (uint32_t)m.at.size(),
                                                                    (uint32_t)m.L, info & 0x1FFFFu, pos, minus_row, w, editor);
                const crp::SpliceOutcome none = crp::splice_outcome(planes, nullptr, nullptr, nullptr, 0, (uint32_t)m.L, info, pos, minus_row, w, editor);
                REQUIRE(bare.targets == want.targets && !bare.donors && !bare.acceptors && bare.donor_off == crp::SPLICE_NO_SITE &&
                        bare.acceptor_off == crp::SPLICE_NO_SITE);
                REQUIRE(none.targets == want.targets && !none.donors && !none.acceptors && none.donor_off == crp::SPLICE_NO_SITE &&
                        none.acceptor_off == crp::SPLICE_NO_SITE);
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

// site letters at the exons' edges, so that destroyed sites of every kind occur by the hundred: behind an exon GT, CT, or
// something else; before one AG, AC, or something else (a later exon's letters overwrite an earlier one's in short introns)
void plant(std::string &s, const std::vector<std::pair<int, int>> &exons, std::mt19937 &rng)
{
    const char *starts[] = {"GT", "CT", "GT", "CT", "GC", "gt", "NT", "cT"}, *ends[] = {"AG", "AC", "AG", "AC", "AT", "ag", "AN", "Uc"};
    for (auto ab : exons) {
        if (ab.second + 2 < N) {
            const char *p = starts[rng() % 8];
            s[ab.second + 1] = p[0], s[ab.second + 2] = p[1];
        }
        if (ab.first >= 2 && rng() % 4) {
            const char *p = ends[rng() % 8];
            s[ab.first - 2] = p[0], s[ab.first - 1] = p[1];
        }
    }
}

}  // namespace

int main()
{
    std::mt19937 rng(22);
    Totals tot;
    const uint64_t top = 0xFFFFFFFFull;
    const std::vector<std::vector<std::pair<int, int>>> exon_sets = {
        {{0, 255}},                                               // one exon over the whole text: no intron
        {{3, 61}, {64, 64}, {67, 125}, {128, 141}, {190, 253}},   // sites at the words' seams, a one-letter exon
        {{10, 20}, {22, 24}, {27, 28}, {32, 33}, {38, 38}, {41, 60}, {63, 70}, {75, 80}},  // introns of 1, 2, 3 and 4 letters, many steps in one span
        {{2, 100}, {110, 253}},                                   // sites next to position 0 and to the text's end
        {{100, 102}},                                             // one exon in the middle: the boundaries before P's first and behind its last
        {},                                                       // zero steps
    };
    int n = 0;
    for (const auto &exons : exon_sets)
        for (int kind = 0; kind < 3; ++kind) {
            const int frame = n % 2;  // (one or no letter more of P before the text, in turn)
            const std::string what = "exon set " + std::to_string(n++ / 3) + " frame " + std::to_string(frame) + " kind " + std::to_string(kind);
            std::string s = kind == 0 ? random_text(rng, "ACGT", 4) : kind == 1 ? random_text(rng, "AACCGGTTNacgtu-", 15) : random_text(rng, "AT", 2);
            plant(s, exons, rng);
            uint64_t letters = 0;
            for (auto ab : exons) letters += (uint64_t)(ab.second - ab.first + 1);
            // P's letters before and behind the text: none (the text's first exon is P's first, its last P's last), a few,
            // and such that L_P and the offsets lie near 2^32
            for (uint64_t before : {uint64_t(0), uint64_t(5 + frame), top - letters - 7 - (uint64_t)frame}) {
                const Model m = model_of(exons, before, before == 0 ? 0 : top - before - letters >= 7 ? 7 : 0);
                for (uint64_t n_words : {uint64_t(4), uint64_t(3), uint64_t(1), uint64_t(0)})
                    if (n_words == 4 || kind == 0)
                        if (compare(text_of(s, n_words, rng), m, what, &tot)) return 1;
            }
        }
    // one step that never ends (crp_select_set_coding accepts any ascending model): grow from letter 5 on, after an intron
    // (cum > 0) and as P's first letter (cum = 0)
    for (uint32_t c : {9u, 0u}) {
        const std::string what = "one step";
        Model m;
        m.at = {5};
        m.word = {G};
        m.cum = {c};
        m.L = c + 400;
        std::string s = random_text(rng, "ACGT", 4);
        s[3] = 'A', s[4] = 'G';
        if (compare(text_of(s, 4, rng), m, what, &tot)) return 1;
    }
    const std::string what = "totals";
    std::printf("donors %llu / %llu acceptors %llu / %llu (CBE / ABE), both in one row %llu, passes %llu\n", (unsigned long long)tot.donors[0],
                (unsigned long long)tot.donors[1], (unsigned long long)tot.acceptors[0], (unsigned long long)tot.acceptors[1], (unsigned long long)tot.both,
                (unsigned long long)tot.pass);
    REQUIRE(tot.donors[0] > 500 && tot.donors[1] > 500 && tot.acceptors[0] > 500 && tot.acceptors[1] > 500 && tot.both > 20 && tot.pass > 1000);
    // 32-bit products would have got this wrong: 100 off wraps
    const crp::SpliceOutcome o = {1, 1, 0, 4294967100u, crp::SPLICE_NO_SITE};
    REQUIRE(crp::splice_pass(o, (uint32_t)top, crp::SpliceLimits{99, 100, 20, 3}) && !crp::splice_pass(o, (uint32_t)top, crp::SpliceLimits{0, 98, 20, 3}) &&
            !crp::splice_pass(o, (uint32_t)top, crp::SpliceLimits{99, 100, 20, 2}));
    std::printf("OK\n");
    return 0;
}
