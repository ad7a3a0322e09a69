// crp_variants.cpp -- host side of the variant-aware guides (include/cropsr_hip.h states the
// definition, cropsr_amd/variants.py restates it, tests/variant_reference.py holds a pure-Python reader of the same
// rules): text VCF bytes, in chunks, -> per CHROM the closed intervals [s, e] of its kept ALT alleles, and per arena the
// track the device counts on (crp_variants.hip).  No GPU needed.
//
//   allele    REF and ALT lose their common prefix (letters compared without case), then what is left loses its common
//             suffix: REF', ALT', p = POS + the prefix' length.  [s, e] = [p, p + len(REF') - 1]; an insertion is the
//             empty interval [p, p - 1]; REF' and ALT' both empty: dropped.  e >= s - 1 always.
//   track     per text of the arena the intervals of its CHROM, in string indices (coordinate + dec - 1), clipped to
//             [first, first + length - 1] and kept when e' >= s' - 1; arena position = index - first + offset; equal
//             (s', e') pairs count once; starts = every s', ends1 = every e' + 1, each sorted ascending on its own.
//
// A line is checked as a whole before any filter looks at it: a malformed line is an error wherever it stands.
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <string_view>
#include <unordered_map>
#include <utility>
#include <vector>

#include "cropsr_hip.h"

struct crp_variants {
    std::vector<std::string> samples;
    bool pass_only = false;
    // reader state
    std::string carry;  // the bytes of a line whose end has not arrived
    uint64_t line_no = 0;
    bool finished = false, failed = false, have_header = false;
    std::string error;
    std::vector<size_t> sample_col;  // column of every named sample (after #CHROM)
    // what was read
    struct Chrom {
        std::string name;
        std::vector<std::pair<uint64_t, uint64_t>> iv;  // (s, e + 1) in 1-based coordinates: e + 1 >= s
    };
    std::vector<Chrom> chroms;  // in order of first appearance among the kept alleles
    std::unordered_map<std::string, uint32_t> chrom_index;
    uint64_t stats[8] = {};
    std::vector<char> carried;  // scratch: which ALT alleles the named samples carry
};

namespace {

enum { ST_LINES, ST_RECORDS, ST_FILTERED, ST_KEPT, ST_SKIPPED, ST_NOT_CARRIED, ST_EMPTY, ST_CHROMS };

int bad(crp_variants *v, const std::string &what)
{
    v->failed = true;
    v->error = "line " + std::to_string(v->line_no) + ": " + what;
    return CRP_ERR_INVALID;
}

bool is_base(char c)
{
    switch (c) {
    case 'A': case 'C': case 'G': case 'T': case 'N': case 'a': case 'c': case 'g': case 't': case 'n': return true;
    default: return false;
    }
}

bool all_bases(std::string_view s)
{
    if (s.empty()) return false;
    for (char c : s)
        if (!is_base(c)) return false;
    return true;
}

char upper(char c) { return c >= 'a' && c <= 'z' ? (char)(c - 32) : c; }

void split(std::string_view s, char sep, std::vector<std::string_view> *out)
{
    out->clear();
    size_t at = 0;
    for (;;) {
        const size_t k = s.find(sep, at);
        if (k == std::string_view::npos) {
            out->push_back(s.substr(at));
            return;
        }
        out->push_back(s.substr(at, k - at));
        at = k + 1;
    }
}

// 0: a sequence allele, 1: one the reader skips (`.`, `*`, symbolic, breakend), -1: malformed
int alt_kind(std::string_view a)
{
    if (a == "." || a == "*") return 1;
    if (a.find('[') != std::string_view::npos || a.find(']') != std::string_view::npos) return 1;
    if (a.size() >= 2 && a.front() == '<' && a.back() == '>') return 1;
    return all_bases(a) ? 0 : -1;
}

int header_line(crp_variants *v, std::string_view line)
{
    std::vector<std::string_view> col;
    split(line, '\t', &col);
    v->have_header = true;
    v->sample_col.clear();
    for (const std::string &name : v->samples) {
        size_t at = 0;
        for (size_t c = 9; c < col.size() && !at; ++c)
            if (col[c] == name) at = c;
        if (!at) return bad(v, "the #CHROM line names no sample " + name);
        v->sample_col.push_back(at);
    }
    return CRP_OK;
}

int data_line(crp_variants *v, std::string_view line)
{
    std::vector<std::string_view> col, alts, fmt, parts;
    split(line, '\t', &col);
    if (col.size() < 5) return bad(v, "fewer than 5 tab-separated columns");
    if (col[0].empty()) return bad(v, "an empty CHROM");
    const std::string_view pos_text = col[1];
    if (pos_text.empty() || pos_text.size() > 15) return bad(v, "POS is not a number of 1 to 15 digits");
    uint64_t pos = 0;
    for (char c : pos_text) {
        if (c < '0' || c > '9') return bad(v, "POS is not a plain digit string");
        pos = pos * 10 + (uint64_t)(c - '0');
    }
    if (pos < 1) return bad(v, "POS is below 1");
    const std::string_view ref = col[3];
    if (!all_bases(ref)) return bad(v, "REF is not made of the letters ACGTN");
    split(col[4], ',', &alts);
    std::vector<int> kind(alts.size());
    for (size_t k = 0; k < alts.size(); ++k) {
        kind[k] = alt_kind(alts[k]);
        if (kind[k] < 0) return bad(v, "ALT allele " + std::to_string(k + 1) + " is neither letters of ACGTN nor `.`, `*`, <...> or a breakend");
    }
    if (v->pass_only && col.size() < 7) return bad(v, "no FILTER column");
    const bool by_sample = !v->samples.empty();
    v->carried.assign(alts.size(), by_sample ? 0 : 1);
    if (by_sample) {
        if (!v->have_header) return bad(v, "a record before the #CHROM line that names the samples");
        if (col.size() < 10) return bad(v, "no FORMAT and sample columns");
        split(col[8], ':', &fmt);
        size_t gt = fmt.size();
        for (size_t k = 0; k < fmt.size() && gt == fmt.size(); ++k)
            if (fmt[k] == "GT") gt = k;
        for (size_t c : v->sample_col) {
            if (c >= col.size()) return bad(v, "fewer sample columns than the #CHROM line names");
            if (gt == fmt.size()) continue;  // (a record without genotypes: no sample carries anything)
            split(col[c], ':', &parts);
            if (gt >= parts.size()) continue;
            const std::string_view g = parts[gt];
            size_t at = 0;
            while (at <= g.size()) {
                size_t end = at;
                while (end < g.size() && g[end] != '/' && g[end] != '|') ++end;
                const std::string_view tok = g.substr(at, end - at);
                if (tok != "." && !tok.empty()) {
                    if (tok.size() > 6) return bad(v, "a GT allele index that is no small number");
                    uint64_t k = 0;
                    for (char ch : tok) {
                        if (ch < '0' || ch > '9') return bad(v, "a GT allele that is neither a number nor `.`");
                        k = k * 10 + (uint64_t)(ch - '0');
                    }
                    if (k > alts.size()) return bad(v, "a GT allele index beyond the ALT list");
                    if (k) v->carried[k - 1] = 1;
                } else if (tok.empty()) {
                    return bad(v, "an empty GT allele");
                }
                at = end + 1;
            }
        }
    }
    // the line is well-formed: count and filter
    v->stats[ST_RECORDS] += 1;
    if (v->pass_only && col[6] != "PASS" && col[6] != ".") {
        v->stats[ST_FILTERED] += 1;
        return CRP_OK;
    }
    for (size_t k = 0; k < alts.size(); ++k) {
        if (kind[k] == 1) {
            v->stats[ST_SKIPPED] += 1;
            continue;
        }
        if (!v->carried[k]) {
            v->stats[ST_NOT_CARRIED] += 1;
            continue;
        }
        const std::string_view alt = alts[k];
        size_t pre = 0;
        while (pre < ref.size() && pre < alt.size() && upper(ref[pre]) == upper(alt[pre])) ++pre;
        size_t suf = 0;
        while (suf < ref.size() - pre && suf < alt.size() - pre && upper(ref[ref.size() - 1 - suf]) == upper(alt[alt.size() - 1 - suf])) ++suf;
        const size_t ref_left = ref.size() - pre - suf, alt_left = alt.size() - pre - suf;
        if (!ref_left && !alt_left) {
            v->stats[ST_EMPTY] += 1;
            continue;
        }
        auto it = v->chrom_index.find(std::string(col[0]));
        if (it == v->chrom_index.end()) {
            it = v->chrom_index.emplace(std::string(col[0]), (uint32_t)v->chroms.size()).first;
            v->chroms.push_back(crp_variants::Chrom{std::string(col[0]), {}});
        }
        const uint64_t s = pos + pre;
        v->chroms[it->second].iv.emplace_back(s, s + ref_left);
        v->stats[ST_KEPT] += 1;
    }
    return CRP_OK;
}

int one_line(crp_variants *v, std::string_view line)
{
    v->line_no += 1;
    v->stats[ST_LINES] += 1;
    if (!line.empty() && line.back() == '\r') line.remove_suffix(1);
    if (line.empty()) return CRP_OK;
    if (line[0] == '#') {
        if (line.substr(0, 7) == "#CHROM\t" || line == "#CHROM") return header_line(v, line);
        return CRP_OK;
    }
    return data_line(v, line);
}

}  // namespace

extern "C" {

int crp_variants_create(const char *const *samples, uint64_t n_samples, int pass_only, crp_variants **out)
{
    if (!out || (n_samples && !samples)) return CRP_ERR_INVALID;
    *out = nullptr;
    for (uint64_t k = 0; k < n_samples; ++k)
        if (!samples[k] || !samples[k][0]) return CRP_ERR_INVALID;
    crp_variants *v = new (std::nothrow) crp_variants();
    if (!v) return CRP_ERR_NOMEM;
    for (uint64_t k = 0; k < n_samples; ++k) v->samples.emplace_back(samples[k]);
    v->pass_only = pass_only != 0;
    *out = v;
    return CRP_OK;
}

int crp_variants_add_bytes(crp_variants *v, const uint8_t *bytes, uint64_t n)
{
    if (!v || (n && !bytes)) return CRP_ERR_INVALID;
    if (v->failed) return CRP_ERR_INVALID;
    if (v->finished) return CRP_ERR_STATE;
    const char *p = reinterpret_cast<const char *>(bytes), *end = p + n;
    while (p < end) {
        const char *nl = static_cast<const char *>(std::memchr(p, '\n', (size_t)(end - p)));
        if (!nl) {
            v->carry.append(p, (size_t)(end - p));
            break;
        }
        int rc;
        if (v->carry.empty()) {
            rc = one_line(v, std::string_view(p, (size_t)(nl - p)));
        } else {
            v->carry.append(p, (size_t)(nl - p));
            rc = one_line(v, v->carry);
            v->carry.clear();
        }
        if (rc != CRP_OK) return rc;
        p = nl + 1;
    }
    return CRP_OK;
}

int crp_variants_finish(crp_variants *v)
{
    if (!v) return CRP_ERR_INVALID;
    if (v->failed) return CRP_ERR_INVALID;
    if (v->finished) return CRP_OK;
    if (!v->carry.empty()) {  // a last line without its line end
        const int rc = one_line(v, v->carry);
        v->carry.clear();
        if (rc != CRP_OK) return rc;
    }
    for (crp_variants::Chrom &c : v->chroms) {
        std::sort(c.iv.begin(), c.iv.end());
        c.iv.erase(std::unique(c.iv.begin(), c.iv.end()), c.iv.end());
    }
    v->stats[ST_CHROMS] = v->chroms.size();
    v->finished = true;
    return CRP_OK;
}

int crp_variants_destroy(crp_variants *v)
{
    delete v;
    return CRP_OK;
}

const char *crp_variants_error(const crp_variants *v) { return v ? v->error.c_str() : ""; }

int crp_variants_stats(const crp_variants *v, uint64_t *out, int n)
{
    if (!v || (n && !out) || n < 0 || n > 8) return CRP_ERR_INVALID;
    for (int k = 0; k < n; ++k) out[k] = v->stats[k];
    return CRP_OK;
}

int crp_variants_chrom(const crp_variants *v, uint64_t k, const uint8_t **name, uint64_t *name_len)
{
    if (!v || !name || !name_len) return CRP_ERR_INVALID;
    if (!v->finished) return CRP_ERR_STATE;
    if (k >= v->chroms.size()) return CRP_ERR_INVALID;
    *name = reinterpret_cast<const uint8_t *>(v->chroms[k].name.data());
    *name_len = v->chroms[k].name.size();
    return CRP_OK;
}

int crp_variants_track(const crp_variants *v, const uint64_t *entries, uint64_t n_entries, int dec, uint32_t *starts, uint32_t *ends1,
                       uint64_t cap, uint64_t *n_out)
{
    if (!v || (n_entries && !entries) || !n_out || (cap && (!starts || !ends1)) || dec < 0 || dec > 1 << 20) return CRP_ERR_INVALID;
    if (!v->finished) return CRP_ERR_STATE;
    std::vector<std::pair<uint32_t, uint32_t>> pairs;  // (s', e' + 1) in arena positions
    uint64_t prev_base = 0, prev_end = 0;
    for (uint64_t k = 0; k < n_entries; ++k) {
        const uint64_t chrom = entries[4 * k], first = entries[4 * k + 1], len = entries[4 * k + 2], base = entries[4 * k + 3];
        // texts lie in the arena in ascending order and do not overlap (crp_annotation_track's rule)
        if (base + len > 0x7fffffffull || first > 1ull << 62 || (k && (base < prev_end || base <= prev_base))) return CRP_ERR_INVALID;
        prev_base = base;
        prev_end = base + len;
        if (chrom >= v->chroms.size() || !len) continue;
        // string index of coordinate c: c + dec - 1; the text holds the indices [first, first + len)
        const uint64_t shift = (uint64_t)dec;  // index + 1 = c + dec
        for (const std::pair<uint64_t, uint64_t> &iv : v->chroms[chrom].iv) {
            // in "index + 1" units, so that nothing goes below zero: s1 = s + dec, the end e1 = (e + 1) + dec - 1 + 1
            const uint64_t s1 = iv.first + shift, e1x = iv.second + shift;  // e1x = index of e, plus 2 = exclusive end, plus 1
            if (s1 > first + len + 1) break;  // (sorted by s: nothing further reaches the text)
            const uint64_t cs = std::max(s1, first + 1);          // s' + 1
            const uint64_t ce = std::min(e1x, first + len + 1);   // e' + 2
            if (ce < cs) continue;                                // e' + 1 < s': outside the text
            // arena position = index - first + base
            pairs.emplace_back((uint32_t)(cs - 1 - first + base), (uint32_t)(ce - 1 - first + base));
        }
    }
    std::sort(pairs.begin(), pairs.end());
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
    const uint64_t n = pairs.size();
    *n_out = n;
    if (n > cap) return CRP_ERR_CAPACITY;
    for (uint64_t k = 0; k < n; ++k) {
        starts[k] = pairs[k].first;  // (sorted by s' first: ascending as they stand)
        ends1[k] = pairs[k].second;
    }
    std::sort(ends1, ends1 + n);
    return CRP_OK;
}

}  // extern "C"
