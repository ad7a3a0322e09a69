// Sanitizer + fuzz driver for the native VCF reader (crp_variants.cpp): seeded well-formed VCF files, the same files with
// mutated bytes, and byte soups go through crp_variants_create / _add_bytes (in random chunks) / _finish / _track with
// random entry lists.  Checked: a file gives the same statistics, error and track however it is chunked; a track is two
// ascending arrays of one length below 2^31 whose k-th start never lies above the k-th end + 1 (what e >= s - 1 leaves of
// the pairs once each array is sorted on its own); the capacity protocol; calls out of order.  Built and run by
// tests/test_variants_native.py with -fsanitize=address,undefined.
#include "cropsr_hip.h"

#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

namespace {

std::mt19937_64 rng(20261);

uint64_t below(uint64_t n) { return n ? rng() % n : 0; }

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);         \
            return 1;                                                      \
        }                                                                  \
    } while (0)

std::string bases(size_t n, bool lower)
{
    static const char up[] = "ACGTN", lo[] = "acgtn";
    std::string s;
    for (size_t k = 0; k < n; ++k) s += (lower && below(4) == 0 ? lo : up)[below(5)];
    return s;
}

std::string gt(int n_alt)
{
    std::string s;
    const int ploidy = 1 + (int)below(3);
    for (int k = 0; k < ploidy; ++k) {
        if (k) s += below(2) ? '/' : '|';
        s += below(6) == 0 ? std::string(".") : std::to_string(below((uint64_t)n_alt + 1));
    }
    return s;
}

std::string well_formed(int n_records, int n_samples)
{
    static const char *chroms[] = {"c0", "c1", "chr2", "scaffold_three", "nowhere"};
    std::string text = "##fileformat=VCFv4.2\n##contig=<ID=c0>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO";
    if (n_samples) text += "\tFORMAT";
    for (int s = 0; s < n_samples; ++s) text += "\tS" + std::to_string(s);
    text += below(2) ? "\n" : "\r\n";
    for (int r = 0; r < n_records; ++r) {
        const std::string ref = bases(1 + below(below(8) ? 3 : 40), true);
        const int n_alt = 1 + (int)below(3);
        std::string alt;
        for (int k = 0; k < n_alt; ++k) {
            if (k) alt += ',';
            switch (below(10)) {
            case 0: alt += "*"; break;
            case 1: alt += "."; break;
            case 2: alt += "<DEL>"; break;
            case 3: alt += "N[c1:77["; break;
            case 4: alt += ref + bases(1 + below(5), false); break;
            case 5: alt += ref.substr(0, 1); break;
            default: alt += bases(1 + below(4), true);
            }
        }
        text += std::string(chroms[below(5)]) + "\t" + std::to_string(1 + below(below(20) ? 20000 : 3000000000ull)) + "\t.\t" + ref + "\t" + alt +
                "\t50\t" + (below(4) ? "PASS" : below(2) ? "." : "q10") + "\t.";
        if (n_samples) {
            text += below(5) ? "\tGT:DP" : "\tDP:GT";
            const bool gt_first = text[text.size() - 5] == 'G';
            for (int s = 0; s < n_samples; ++s) text += "\t" + (gt_first ? gt(n_alt) + ":7" : "7:" + gt(n_alt));
        }
        text += below(8) ? "\n" : "\r\n";
    }
    if (below(3) == 0 && !text.empty()) text.pop_back();  // no final line end
    return text;
}

struct Result {
    int rc_add = CRP_OK, rc_finish = CRP_OK;
    std::string error;
    uint64_t stats[8] = {};
    std::vector<uint32_t> starts, ends1;
    int rc_track = CRP_OK;
};

int feed(const std::string &text, const std::vector<const char *> &samples, int pass_only, uint64_t chunk, const std::vector<uint64_t> &entries,
         int dec, Result *out)
{
    crp_variants *v = nullptr;
    CHECK(crp_variants_create(samples.empty() ? nullptr : samples.data(), samples.size(), pass_only, &v) == CRP_OK && v);
    uint64_t n_out = 0;
    CHECK(crp_variants_track(v, entries.data(), entries.size() / 4, dec, nullptr, nullptr, 0, &n_out) == CRP_ERR_STATE);  // before finish
    size_t at = 0;
    while (at < text.size() && out->rc_add == CRP_OK) {
        const size_t n = chunk ? std::min<size_t>(text.size() - at, 1 + below(chunk)) : text.size() - at;
        // (the bytes handed over are an exact-size copy: a read past the chunk is a sanitizer error)
        std::vector<uint8_t> piece(text.begin() + (long)at, text.begin() + (long)(at + n));
        out->rc_add = crp_variants_add_bytes(v, piece.data(), piece.size());
        at += n;
    }
    out->rc_finish = crp_variants_finish(v);
    out->error = crp_variants_error(v);
    CHECK(crp_variants_stats(v, out->stats, 8) == CRP_OK);
    CHECK(crp_variants_stats(v, out->stats, 9) == CRP_ERR_INVALID);
    if (out->rc_add != CRP_OK || out->rc_finish != CRP_OK) {
        CHECK(out->error.rfind("line ", 0) == 0);
        CHECK(crp_variants_add_bytes(v, reinterpret_cast<const uint8_t *>("x"), 1) == CRP_ERR_INVALID);  // the handle stays refused
        CHECK(crp_variants_track(v, entries.data(), entries.size() / 4, dec, nullptr, nullptr, 0, &n_out) == CRP_ERR_STATE);
    } else {
        CHECK(out->error.empty());
        CHECK(crp_variants_add_bytes(v, reinterpret_cast<const uint8_t *>("x"), 1) == CRP_ERR_STATE);  // after finish
        for (uint64_t k = 0; k < out->stats[7]; ++k) {
            const uint8_t *name = nullptr;
            uint64_t len = 0;
            CHECK(crp_variants_chrom(v, k, &name, &len) == CRP_OK && name && len);
        }
        const uint8_t *name = nullptr;
        uint64_t len = 0;
        CHECK(crp_variants_chrom(v, out->stats[7], &name, &len) == CRP_ERR_INVALID);
        out->rc_track = crp_variants_track(v, entries.data(), entries.size() / 4, dec, nullptr, nullptr, 0, &n_out);
        if (out->rc_track == CRP_ERR_CAPACITY || out->rc_track == CRP_OK) {
            if (n_out > 1) {  // a capacity one short: refused, nothing written past it
                std::vector<uint32_t> s(n_out - 1), e(n_out - 1);
                uint64_t again = 0;
                CHECK(crp_variants_track(v, entries.data(), entries.size() / 4, dec, s.data(), e.data(), n_out - 1, &again) == CRP_ERR_CAPACITY && again == n_out);
            }
            out->starts.assign(n_out, 0);
            out->ends1.assign(n_out, 0);
            uint64_t again = 0;
            std::vector<uint32_t> none(1);
            out->rc_track = crp_variants_track(v, entries.data(), entries.size() / 4, dec, n_out ? out->starts.data() : none.data(),
                                               n_out ? out->ends1.data() : none.data(), n_out ? n_out : 1, &again);
            CHECK(out->rc_track == CRP_OK && again == n_out);
            for (uint64_t k = 0; k < n_out; ++k) {
                CHECK(out->starts[k] < 0x80000000u && out->ends1[k] < 0x80000000u);
                CHECK(!k || (out->starts[k] >= out->starts[k - 1] && out->ends1[k] >= out->ends1[k - 1]));
                CHECK(out->starts[k] <= out->ends1[k]);
            }
        } else {
            CHECK(out->rc_track == CRP_ERR_INVALID);
        }
    }
    CHECK(crp_variants_destroy(v) == CRP_OK);
    return 0;
}

std::vector<uint64_t> random_entries(bool valid)
{
    std::vector<uint64_t> e;
    uint64_t base = 64;
    const int n = (int)below(6);
    for (int k = 0; k < n; ++k) {
        const uint64_t len = below(10) ? below(30000) : 0, first = below(3) ? 0 : below(25000);
        e.insert(e.end(), {below(7) ? below(5) : ~0ull, first, len, base});
        base += ((len + 63) / 64 + 1) * 64;
    }
    if (!valid && n >= 2) e[7] = e[3];  // two texts at one offset
    return e;
}

}  // namespace

int main()
{
    CHECK(crp_variants_create(nullptr, 0, 0, nullptr) == CRP_ERR_INVALID);
    CHECK(crp_variants_add_bytes(nullptr, nullptr, 0) == CRP_ERR_INVALID && crp_variants_finish(nullptr) == CRP_ERR_INVALID);
    CHECK(crp_variants_destroy(nullptr) == CRP_OK && std::strlen(crp_variants_error(nullptr)) == 0);
    int n_ok = 0, n_bad = 0;
    uint64_t n_track = 0;
    for (int trial = 0; trial < 600; ++trial) {
        const int n_samples = (int)below(4);
        std::string text = trial % 10 == 9 ? std::string() : well_formed((int)below(60), n_samples);
        if (trial % 3 == 1)  // mutated bytes: tabs, line ends, letters, digits and anything else land anywhere
            for (int m = 0, n = 1 + (int)below(6); m < n && !text.empty(); ++m) {
                static const char pool[] = "\t\n\r,:/|.<>[]*#ACGTNacgtnXx0123456789- \0";
                text[below(text.size())] = below(4) ? pool[below(sizeof pool - 1)] : (char)below(256);
            }
        if (trial % 10 == 9)
            for (int k = 0, n = (int)below(400); k < n; ++k) text += (char)below(256);
        std::vector<const char *> samples;
        if (n_samples && below(2)) samples.push_back("S0");
        if (n_samples > 1 && below(2)) samples.push_back("S1");
        if (below(20) == 0) samples.push_back("S9");  // unknown: an error at the #CHROM line
        const int pass_only = (int)below(2), dec = (int)below(3);
        const std::vector<uint64_t> entries = random_entries(below(10) != 0);
        Result whole, pieces, bytes;
        if (feed(text, samples, pass_only, 0, entries, dec, &whole)) return 1;
        if (feed(text, samples, pass_only, 1 + below(70), entries, dec, &pieces)) return 1;
        if (feed(text, samples, pass_only, 1, entries, dec, &bytes)) return 1;
        for (const Result *r : {&pieces, &bytes}) {
            CHECK((r->rc_add != CRP_OK || r->rc_finish != CRP_OK) == (whole.rc_add != CRP_OK || whole.rc_finish != CRP_OK));
            CHECK(r->error == whole.error && r->rc_track == whole.rc_track);
            CHECK(r->starts == whole.starts && r->ends1 == whole.ends1);
            if (whole.error.empty()) CHECK(std::memcmp(r->stats, whole.stats, sizeof whole.stats) == 0);
        }
        (whole.error.empty() ? n_ok : n_bad) += 1;
        n_track += whole.starts.size();
    }
    CHECK(n_ok > 150 && n_bad > 100 && n_track > 500);
    std::printf("%d files read, %d refused, %llu track values\nOK\n", n_ok, n_bad, (unsigned long long)n_track);
    return 0;
}
