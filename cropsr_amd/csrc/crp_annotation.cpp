// crp_annotation.cpp -- host side of the opt-in annotation join: GFF3 (+ Phytozome
// annotation_info) bytes -> label-set strings and, per seqid, the elementary-interval track the device look-up
// (crp_annotate.hip) works on.  No GPU needed.
//
// The reference reads the GFF into a DataFrame (CROPSR.py:77-95, called at :375), never uses it, and writes '' into
// `features` (:466, :468); `-p` is only echoed (:364).  The join is therefore this engine's own definition
// (cropsr_amd/annotate.py; oracle/annotate_oracle.py restates it as a loop over every GFF line per CSV row):
//
//   rows    lines that do not start with '#', with >= 9 tab-separated fields, type (field 3) `gene` or `CDS`, start /
//           end (fields 4, 5) made of digits only; seqid = field 1; in file order
//   label   "<type>:<ident>", ident = the ID attribute, else Name, else Parent, else "." (attributes = field 9 split at
//           ';', each part stripped, key = text before the first '=', first occurrence of a key wins); for a gene
//           whose Name (else ID) is a locusName of the annotation_info file: + "|" + Best-hit-arabi-name and
//           + "|" + arabi-defline (empty fields left out)
//   set     for a 1-based coordinate x of a seqid: the labels of the rows with start <= x <= end, file order, each
//           label once, joined with ';'
//
// The same pass keeps, for the coding position of a cut (cropsr_amd/coding.py has the definition),
// the gene rows' strand, the `mRNA` / `transcript` rows and every row's ID and Parent: build_coding links them once the file
// is read into every gene's coding transcripts, and crp_annotation_coding_layout lays those out beside the gene rows.  The
// rows above do not see any of it: an mRNA row adds no label, no interval, no seqid and no count.
//
// The interval ends cut a seqid's axis into elementary intervals with a constant set: one sweep over the sorted
// points builds one string per DISTINCT set (interned over the whole file) and the id of every interval.
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "cropsr_hip.h"

struct crp_annotation {
    struct Seq {
        std::string name;
        std::vector<int64_t> points;  // ascending 1-based coordinates; interval k = [points[k], points[k+1])
        std::vector<uint32_t> ids;    // its label set (CRP_NO_FEATURE: none)
    };
    std::vector<Seq> seqs;  // in order of first appearance in the GFF
    std::string blob;       // the distinct label-set strings, back to back
    std::vector<uint64_t> off{0};
    std::vector<uint8_t> cds_flag;  // per label-set string: 1 when the set holds a CDS label
    uint64_t n_gene = 0, n_cds = 0;
    // the gene rows, in file order (guide selection, cropsr_amd/select.py): 1-based closed range, index into seqs, and
    // the label "gene:<ident>" without the annotation_info suffix
    struct Gene {
        int64_t start, end;
        uint32_t seq;
    };
    std::vector<Gene> genes;
    std::vector<std::vector<uint32_t>> genes_of;  // per seqid: its genes (indices into `genes`), file order
    std::string gene_blob;
    std::vector<uint64_t> gene_off{0};
    // the coding model of every gene (cropsr_amd/coding.py states the definition): its coding
    // transcripts in file order, each the merged closed ranges of its CDS rows in GFF coordinates
    struct Transcript {
        uint64_t seg_first, seg_n, len;
    };
    struct Coding {
        uint8_t strand = 0;  // 1: '+', 2: '-', 0: anything else
        bool model = false;
        uint32_t n_tx = 0;  // (without a model: 0, and so is len)
        uint64_t len = 0;   // L_P
        uint64_t tx_first = 0, primary = 0;  // txs[tx_first .. tx_first + n_tx); the primary one among them
    };
    std::vector<Coding> coding;  // per gene
    std::vector<Transcript> txs;
    std::vector<std::pair<int64_t, int64_t>> segs;
};

namespace {

using sv = std::string_view;

bool is_space(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f'; }

sv strip(sv s)
{
    while (!s.empty() && is_space(s.front())) s.remove_prefix(1);
    while (!s.empty() && is_space(s.back())) s.remove_suffix(1);
    return s;
}

// fields of one line (no newline inside)
void split_tabs(sv line, std::vector<sv> &out)
{
    out.clear();
    size_t a = 0;
    for (;;) {
        const size_t b = line.find('\t', a);
        if (b == sv::npos) {
            out.push_back(line.substr(a));
            return;
        }
        out.push_back(line.substr(a, b - a));
        a = b + 1;
    }
}

bool digits(sv s, int64_t *v)
{
    if (s.empty() || s.size() > 18) return false;
    int64_t x = 0;
    for (char c : s) {
        if (c < '0' || c > '9') return false;
        x = x * 10 + (c - '0');
    }
    *v = x;
    return true;
}

struct Info {
    std::string best_hit, defline;
};

// Phytozome annotation_info: tab-separated, columns by name from a '#...' header line that has a locusName column,
// else the usual positions; the first line of a locus wins
void parse_info(sv data, std::unordered_map<std::string, Info> &info)
{
    std::vector<std::string> names = {"pacId", "locusName", "transcriptName", "peptideName", "Pfam", "Panther", "KOG",
                                      "KEGG/ec", "KO", "GO", "Best-hit-arabi-name", "arabi-symbol", "arabi-defline"};
    std::vector<sv> cols;
    size_t p = 0;
    while (p < data.size()) {
        size_t q = data.find('\n', p);
        if (q == sv::npos) q = data.size();
        const sv line = data.substr(p, q - p);
        p = q + 1;
        split_tabs(line, cols);
        if (!line.empty() && line[0] == '#') {
            std::vector<std::string> head;
            bool has = false;
            for (sv c : cols) {
                while (!c.empty() && c[0] == '#') c.remove_prefix(1);
                head.emplace_back(c);
                has = has || c == "locusName";
            }
            if (has) names.swap(head);
            continue;
        }
        if (cols.size() < 2) continue;
        // (a repeated column name: the last one counts, like dict(zip(names, cols)))
        sv locus, best, defline;
        const size_t n = std::min(names.size(), cols.size());
        for (size_t k = 0; k < n; ++k) {
            if (names[k] == "locusName") locus = cols[k];
            else if (names[k] == "Best-hit-arabi-name") best = cols[k];
            else if (names[k] == "arabi-defline") defline = cols[k];
        }
        if (locus.empty()) continue;
        info.try_emplace(std::string(locus), Info{std::string(best), std::string(defline)});
    }
}

struct Feature {
    int64_t start, end;
    uint32_t label;  // index into the label table (equal strings share one)
};

// What the coding model keeps of a row until the whole file is read (children may come before their parents).  `seq`
// numbers the seqids of these rows alone: an mRNA row must not add a seqid to the annotation's own list.
struct ModelRow {
    uint32_t seq;
    uint64_t line;  // rows in file order
    sv id, parent;
    int64_t start, end;
};

// the values of a Parent attribute: a comma-separated list; empty values name nothing
template <class F>
void each_parent(sv list, F &&f)
{
    size_t a = 0;
    for (;;) {
        const size_t b = list.find(',', a);
        const sv v = list.substr(a, b == sv::npos ? sv::npos : b - a);
        if (!v.empty()) f(v);
        if (b == sv::npos) return;
        a = b + 1;
    }
}

std::string model_key(uint32_t seq, sv id)
{
    std::string k = std::to_string(seq);
    k.push_back('\t');
    k.append(id);
    return k;
}

// Links the rows and builds every gene's coding transcripts (cropsr_amd/coding.py has the definition).
void build_coding(crp_annotation *an, const std::vector<ModelRow> &genes, const std::vector<uint8_t> &strands, const std::vector<ModelRow> &txs,
                  const std::vector<ModelRow> &cds)
{
    using Ranges = std::vector<std::pair<int64_t, int64_t>>;
    std::unordered_map<std::string, uint32_t> gene_by, tx_by;  // the first row of an ID owns the children
    for (uint32_t g = 0; g < genes.size(); ++g)
        if (!genes[g].id.empty()) gene_by.try_emplace(model_key(genes[g].seq, genes[g].id), g);
    for (uint32_t t = 0; t < txs.size(); ++t)
        if (!txs[t].id.empty()) tx_by.try_emplace(model_key(txs[t].seq, txs[t].id), t);
    std::vector<Ranges> tx_ranges(txs.size()), own_ranges(genes.size());
    std::vector<std::vector<uint32_t>> txs_of(genes.size());
    for (uint32_t t = 0; t < txs.size(); ++t)
        each_parent(txs[t].parent, [&](sv v) {
            const auto g = gene_by.find(model_key(txs[t].seq, v));
            if (g == gene_by.end()) return;
            std::vector<uint32_t> &list = txs_of[g->second];
            if (list.empty() || list.back() != t) list.push_back(t);  // (rows come in order: a value named twice is the last one)
        });
    for (const ModelRow &c : cds) {
        if (c.start > c.end) continue;
        each_parent(c.parent, [&](sv v) {
            const std::string key = model_key(c.seq, v);
            const auto t = tx_by.find(key);
            if (t != tx_by.end()) tx_ranges[t->second].emplace_back(c.start, c.end);
            const auto g = gene_by.find(key);
            if (g != gene_by.end()) own_ranges[g->second].emplace_back(c.start, c.end);
        });
    }
    an->coding.assign(genes.size(), crp_annotation::Coding());
    std::vector<std::pair<uint64_t, Ranges *>> cand;  // (line, ranges): the gene's transcripts in file order
    for (uint32_t g = 0; g < genes.size(); ++g) {
        crp_annotation::Coding &c = an->coding[g];
        c.strand = strands[g];
        if (!c.strand || genes[g].id.empty()) continue;
        cand.clear();
        cand.emplace_back(genes[g].line, &own_ranges[g]);  // the implicit transcript stands at the gene row
        for (uint32_t t : txs_of[g]) cand.emplace_back(txs[t].line, &tx_ranges[t]);  // (a row that owns no children has no ranges)
        std::sort(cand.begin(), cand.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
        const uint64_t tx_first = an->txs.size(), seg_first = an->segs.size();
        uint64_t best = 0, primary = 0;
        for (const auto &one : cand) {
            Ranges r = *one.second;  // (a transcript may serve several genes: a copy)
            if (r.empty()) continue;
            std::sort(r.begin(), r.end());
            crp_annotation::Transcript tx{an->segs.size(), 0, 0};
            for (const auto &ab : r) {
                if (tx.seg_n && ab.first <= an->segs.back().second + 1) an->segs.back().second = std::max(an->segs.back().second, ab.second);
                else an->segs.push_back(ab), tx.seg_n += 1;
            }
            // (merged segments are disjoint ranges of coordinates below 10^18, so the sum cannot wrap; it is capped all the same)
            for (uint64_t k = 0; k < tx.seg_n; ++k)
                tx.len = std::min<uint64_t>(tx.len + (uint64_t)(an->segs[tx.seg_first + k].second - an->segs[tx.seg_first + k].first) + 1, 1ull << 40);
            if (tx.len > best) best = tx.len, primary = an->txs.size() - tx_first;  // (a tie: the earlier row stays)
            an->txs.push_back(tx);
        }
        const uint64_t n_tx = an->txs.size() - tx_first;
        if (!n_tx || best > 0xFFFFFFFFull) {  // no coding transcript, or a length no contig can hold: no model
            an->txs.resize(tx_first);
            an->segs.resize(seg_first);
            continue;
        }
        c.model = true;
        c.n_tx = (uint32_t)std::min<uint64_t>(n_tx, 0xFFFFFFFFull);
        c.len = best;
        c.tx_first = tx_first;
        c.primary = primary;
    }
}

}  // namespace

extern "C" {

int crp_annotation_build(const uint8_t *gff, uint64_t gff_len, const uint8_t *info_text, uint64_t info_len,
                         crp_annotation **out)
{
    if (!out || (gff_len && !gff) || (info_len && !info_text)) return CRP_ERR_INVALID;
    *out = nullptr;
    crp_annotation *an = new (std::nothrow) crp_annotation();
    if (!an) return CRP_ERR_NOMEM;
    try {
        std::unordered_map<std::string, Info> info;
        const bool have_info = info_text != nullptr;
        if (have_info) parse_info(sv(reinterpret_cast<const char *>(info_text), info_len), info);
        const sv data(reinterpret_cast<const char *>(gff), gff_len);
        std::unordered_map<std::string, uint32_t> seq_of, label_of;
        std::vector<std::string> labels;
        std::vector<std::vector<Feature>> feats;  // per seqid, file order
        std::vector<sv> cols;
        std::string label;
        // (sized for a typical GFF -- a gene / CDS row every ~250 bytes -- so the tables do not rehash on the way)
        label_of.reserve(gff_len / 256 + 16);
        labels.reserve(gff_len / 256 + 16);
        std::unordered_map<std::string, uint32_t> model_seq_of;
        std::vector<ModelRow> model_genes, model_txs, model_cds;
        std::vector<uint8_t> model_strands;
        uint32_t model_seq = 0;
        sv model_seq_name;
        bool have_model_seq = false;
        uint64_t n_rows = 0;
        uint32_t last_seq = 0;  // consecutive rows usually share their seqid
        bool have_last = false;
        size_t p = 0;
        while (p < data.size()) {
            size_t q = data.find('\n', p);
            if (q == sv::npos) q = data.size();
            const sv line = data.substr(p, q - p);
            p = q + 1;
            if (line.empty() || line[0] == '#') continue;
            split_tabs(line, cols);
            if (cols.size() < 9) continue;
            const bool gene = cols[2] == "gene";
            const bool transcript = cols[2] == "mRNA" || cols[2] == "transcript";  // (read by the coding model alone)
            if (!gene && !transcript && cols[2] != "CDS") continue;
            int64_t start, end;
            if (!digits(cols[3], &start) || !digits(cols[4], &end)) continue;  // unreadable coordinates join nothing
            sv id, name, parent;
            bool has_id = false, has_name = false, has_parent = false;
            {
                const sv attrs = cols[8];
                size_t a = 0;
                for (;;) {
                    size_t b = attrs.find(';', a);
                    const sv part = strip(attrs.substr(a, b == sv::npos ? sv::npos : b - a));
                    const size_t eq = part.find('=');
                    const sv key = part.substr(0, eq), val = eq == sv::npos ? sv() : part.substr(eq + 1);
                    if (key == "ID" && !has_id) id = val, has_id = true;
                    else if (key == "Name" && !has_name) name = val, has_name = true;
                    else if (key == "Parent" && !has_parent) parent = val, has_parent = true;
                    if (b == sv::npos) break;
                    a = b + 1;
                }
            }
            {
                if (!have_model_seq || model_seq_name != cols[0]) {
                    model_seq = model_seq_of.emplace(std::string(cols[0]), (uint32_t)model_seq_of.size()).first->second;
                    model_seq_name = cols[0];
                    have_model_seq = true;
                }
                const ModelRow row{model_seq, n_rows++, id, parent, start, end};
                if (gene) {
                    model_genes.push_back(row);
                    model_strands.push_back(cols[6] == "+" ? 1 : cols[6] == "-" ? 2 : 0);
                } else {
                    (transcript ? model_txs : model_cds).push_back(row);
                }
            }
            if (transcript) continue;  // labels, intervals and counts are the gene and CDS rows' alone
            const sv ident = !id.empty() ? id : !name.empty() ? name : !parent.empty() ? parent : sv(".");
            label.assign(gene ? "gene:" : "CDS:");
            label.append(ident);
            const size_t plain_len = label.size();  // (the gene's own label ends here: what follows names it further)
            if (have_info && gene) {
                auto hit = info.find(std::string(name));
                if (hit == info.end()) hit = info.find(std::string(id));
                if (hit != info.end()) {
                    if (!hit->second.best_hit.empty()) label.append("|").append(hit->second.best_hit);
                    if (!hit->second.defline.empty()) label.append("|").append(hit->second.defline);
                }
            }
            if (!have_last || an->seqs[last_seq].name != cols[0]) {
                auto s = seq_of.find(std::string(cols[0]));
                if (s == seq_of.end()) {
                    s = seq_of.emplace(std::string(cols[0]), (uint32_t)an->seqs.size()).first;
                    an->seqs.emplace_back();
                    an->seqs.back().name.assign(cols[0]);
                    feats.emplace_back();
                    an->genes_of.emplace_back();
                }
                last_seq = s->second;
                have_last = true;
            }
            auto l = label_of.find(label);
            if (l == label_of.end()) {
                l = label_of.emplace(label, (uint32_t)labels.size()).first;
                labels.push_back(label);
            }
            feats[last_seq].push_back(Feature{start, end, l->second});
            (gene ? an->n_gene : an->n_cds) += 1;
            if (gene) {
                an->genes_of[last_seq].push_back((uint32_t)an->genes.size());
                an->genes.push_back(crp_annotation::Gene{start, end, last_seq});
                an->gene_blob.append(label, 0, plain_len);
                an->gene_off.push_back(an->gene_blob.size());
            }
        }
        build_coding(an, model_genes, model_strands, model_txs, model_cds);
        // the sweep, seqid by seqid
        std::unordered_map<std::string, uint32_t> string_of;
        string_of.reserve(2 * labels.size() + 16);
        an->off.reserve(2 * labels.size() + 16);
        std::vector<uint32_t> by_start, active, set;
        std::string text;
        for (size_t k = 0; k < an->seqs.size(); ++k) {
            const std::vector<Feature> &f = feats[k];
            crp_annotation::Seq &seq = an->seqs[k];
            seq.points.reserve(2 * f.size());
            for (const Feature &t : f) {
                seq.points.push_back(t.start);
                seq.points.push_back(t.end + 1);
            }
            std::sort(seq.points.begin(), seq.points.end());
            seq.points.erase(std::unique(seq.points.begin(), seq.points.end()), seq.points.end());
            by_start.resize(f.size());
            for (uint32_t i = 0; i < f.size(); ++i) by_start[i] = i;
            std::stable_sort(by_start.begin(), by_start.end(), [&](uint32_t a, uint32_t b) { return f[a].start < f[b].start; });
            seq.ids.assign(seq.points.size(), CRP_NO_FEATURE);
            active.clear();
            size_t nxt = 0;
            for (size_t i = 0; i < seq.points.size(); ++i) {
                const int64_t x = seq.points[i];
                while (nxt < by_start.size() && f[by_start[nxt]].start <= x) active.push_back(by_start[nxt++]);
                active.erase(std::remove_if(active.begin(), active.end(), [&](uint32_t a) { return f[a].end < x; }), active.end());
                if (active.empty()) continue;
                std::sort(active.begin(), active.end());  // feature index = file order
                set.clear();
                for (uint32_t a : active)
                    if (std::find(set.begin(), set.end(), f[a].label) == set.end()) set.push_back(f[a].label);
                text.clear();
                bool has_cds = false;
                for (size_t j = 0; j < set.size(); ++j) {
                    if (j) text.push_back(';');
                    text.append(labels[set[j]]);
                    has_cds = has_cds || labels[set[j]].compare(0, 4, "CDS:") == 0;
                }
                auto it = string_of.find(text);
                if (it == string_of.end()) {
                    it = string_of.emplace(text, (uint32_t)(an->off.size() - 1)).first;
                    an->blob.append(text);
                    an->off.push_back(an->blob.size());
                    an->cds_flag.push_back(has_cds ? 1 : 0);
                }
                seq.ids[i] = it->second;
            }
        }
    } catch (const std::bad_alloc &) {
        delete an;
        return CRP_ERR_NOMEM;
    }
    *out = an;
    return CRP_OK;
}

int crp_annotation_destroy(crp_annotation *an)
{
    delete an;
    return CRP_OK;
}

int crp_annotation_stats(const crp_annotation *an, uint64_t *n_seqids, uint64_t *n_strings, uint64_t *blob_bytes,
                         uint64_t *n_genes, uint64_t *n_cds)
{
    if (!an) return CRP_ERR_INVALID;
    if (n_seqids) *n_seqids = an->seqs.size();
    if (n_strings) *n_strings = an->off.size() - 1;
    if (blob_bytes) *blob_bytes = an->blob.size();
    if (n_genes) *n_genes = an->n_gene;
    if (n_cds) *n_cds = an->n_cds;
    return CRP_OK;
}

int crp_annotation_strings(const crp_annotation *an, uint8_t *blob, uint64_t *offsets)
{
    if (!an) return CRP_ERR_INVALID;
    if (blob && !an->blob.empty()) std::memcpy(blob, an->blob.data(), an->blob.size());
    if (offsets) std::memcpy(offsets, an->off.data(), an->off.size() * sizeof(uint64_t));
    return CRP_OK;
}

int crp_annotation_seqid(const crp_annotation *an, uint64_t k, const uint8_t **name, uint64_t *name_len,
                         const int64_t **points, const uint32_t **ids, uint64_t *n_points)
{
    if (!an || k >= an->seqs.size()) return CRP_ERR_INVALID;
    const crp_annotation::Seq &s = an->seqs[k];
    if (name) *name = reinterpret_cast<const uint8_t *>(s.name.data());
    if (name_len) *name_len = s.name.size();
    if (points) *points = s.points.data();
    if (ids) *ids = s.ids.data();
    if (n_points) *n_points = s.points.size();
    return CRP_OK;
}

int crp_annotation_track(const crp_annotation *an, const uint64_t *entries, uint64_t n_entries, int dec, uint32_t *points,
                         uint32_t *ids, uint64_t cap, uint64_t *n_out)
{
    if (!an || (n_entries && !entries) || !n_out || (cap && (!points || !ids))) return CRP_ERR_INVALID;
    uint64_t n = 0, prev_base = 0, prev_end = 0;
    for (uint64_t e = 0; e < n_entries; ++e) {
        const uint64_t seq = entries[4 * e], lo = entries[4 * e + 1], len = entries[4 * e + 2], base = entries[4 * e + 3];
        // texts lie in the arena in ascending order and do not overlap: the track comes out strictly ascending
        if (base + len > 0x7fffffffull || (e && (base < prev_end || base <= prev_base))) return CRP_ERR_INVALID;
        prev_base = base;
        prev_end = base + len;
        uint32_t first = CRP_NO_FEATURE;
        size_t k = 0;
        const crp_annotation::Seq *s = seq < an->seqs.size() ? &an->seqs[seq] : nullptr;
        // index of the 1-based genome coordinate p inside the text: p + dec - 1 - lo
        const int64_t shift = (int64_t)dec - 1 - (int64_t)lo;
        if (s) {
            // the points at or before the text's first character: the last of them says what holds there
            k = (size_t)(std::upper_bound(s->points.begin(), s->points.end(), -shift) - s->points.begin());
            if (k) first = s->ids[k - 1];
        }
        if (n < cap) {
            points[n] = (uint32_t)base;
            ids[n] = first;
        }
        n += 1;
        if (s)
            for (; k < s->points.size() && s->points[k] + shift < (int64_t)len; ++k) {
                if (n < cap) {
                    points[n] = (uint32_t)(base + (uint64_t)(s->points[k] + shift));
                    ids[n] = s->ids[k];
                }
                n += 1;
            }
    }
    *n_out = n;
    return n <= cap ? CRP_OK : CRP_ERR_CAPACITY;
}

int crp_annotation_genes(const crp_annotation *an, uint64_t *seqid, int64_t *start, int64_t *end, uint8_t *label_blob,
                         uint64_t *label_off, uint64_t *label_bytes)
{
    if (!an) return CRP_ERR_INVALID;
    for (size_t g = 0; g < an->genes.size(); ++g) {
        if (seqid) seqid[g] = an->genes[g].seq;
        if (start) start[g] = an->genes[g].start;
        if (end) end[g] = an->genes[g].end;
    }
    if (label_blob && !an->gene_blob.empty()) std::memcpy(label_blob, an->gene_blob.data(), an->gene_blob.size());
    if (label_off) std::memcpy(label_off, an->gene_off.data(), an->gene_off.size() * sizeof(uint64_t));
    if (label_bytes) *label_bytes = an->gene_blob.size();
    return CRP_OK;
}

int crp_annotation_gene_layout(const crp_annotation *an, const uint64_t *entries, uint64_t n_entries, int dec, uint32_t *lo,
                               uint32_t *hi, uint64_t *gene, uint64_t cap, uint64_t *n_out)
{
    if (!an || (n_entries && !entries) || !n_out || (cap && (!lo || !hi || !gene))) return CRP_ERR_INVALID;
    uint64_t n = 0, prev_base = 0, prev_end = 0;
    for (uint64_t e = 0; e < n_entries; ++e) {
        const uint64_t seq = entries[4 * e], first = entries[4 * e + 1], len = entries[4 * e + 2], base = entries[4 * e + 3];
        if (base + len > 0x7fffffffull || (e && (base < prev_end || base <= prev_base))) return CRP_ERR_INVALID;  // as the track
        prev_base = base;
        prev_end = base + len;
        if (seq >= an->seqs.size() || !len) continue;
        // index of the 1-based genome coordinate p inside the text: p + dec - 1 - first (crp_annotation_track)
        const int64_t shift = (int64_t)dec - 1 - (int64_t)first;
        for (uint32_t g : an->genes_of[seq]) {
            const crp_annotation::Gene &t = an->genes[g];
            if (t.start > t.end) continue;
            const int64_t a = std::max<int64_t>(t.start + shift, 0), b = std::min<int64_t>(t.end + shift, (int64_t)len - 1);
            if (a > b) continue;  // the text holds none of it
            if (n < cap) {
                lo[n] = (uint32_t)(base + (uint64_t)a);
                hi[n] = (uint32_t)(base + (uint64_t)b);
                gene[n] = g;
            }
            n += 1;
        }
    }
    *n_out = n;
    return n <= cap ? CRP_OK : CRP_ERR_CAPACITY;
}

int crp_annotation_gene_coding(const crp_annotation *an, uint8_t *strand, uint32_t *n_tx, uint32_t *length)
{
    if (!an) return CRP_ERR_INVALID;
    for (size_t g = 0; g < an->coding.size(); ++g) {
        const crp_annotation::Coding &c = an->coding[g];
        if (strand) strand[g] = c.strand == 1 ? '+' : c.strand == 2 ? '-' : '.';
        if (n_tx) n_tx[g] = c.n_tx;
        if (length) length[g] = (uint32_t)c.len;
    }
    return CRP_OK;
}

int crp_annotation_coding_layout(const crp_annotation *an, const uint64_t *entries, uint64_t n_entries, int dec, uint32_t *info,
                                 uint32_t *length, uint64_t *first, uint64_t cap_rows, uint64_t *n_rows, uint32_t *at, uint32_t *word,
                                 uint32_t *cum, uint64_t cap_steps, uint64_t *n_steps)
{
    if (!an || (n_entries && !entries) || !n_rows || !n_steps || (cap_rows && (!info || !length || !first)) ||
        (cap_steps && (!at || !word || !cum)))
        return CRP_ERR_INVALID;
    struct Event {
        int64_t at;
        int32_t cover, inside, grow;
    };
    std::vector<Event> ev;
    uint64_t n = 0, m = 0, prev_base = 0, prev_end = 0;
    try {
        for (uint64_t e = 0; e < n_entries; ++e) {
            const uint64_t seq = entries[4 * e], start = entries[4 * e + 1], len = entries[4 * e + 2], base = entries[4 * e + 3];
            if (base + len > 0x7fffffffull || (e && (base < prev_end || base <= prev_base))) return CRP_ERR_INVALID;  // as the track
            prev_base = base;
            prev_end = base + len;
            if (seq >= an->seqs.size() || !len) continue;
            const int64_t shift = (int64_t)dec - 1 - (int64_t)start;  // (crp_annotation_gene_layout's mapping, and its rows)
            for (uint32_t g : an->genes_of[seq]) {
                const crp_annotation::Gene &t = an->genes[g];
                if (t.start > t.end) continue;
                if (std::max<int64_t>(t.start + shift, 0) > std::min<int64_t>(t.end + shift, (int64_t)len - 1)) continue;
                const crp_annotation::Coding &c = an->coding[g];
                if (c.n_tx > 0xFFFFu) return CRP_ERR_UNSUPPORTED;  // (the cover field of a step has 16 bits)
                if (n < cap_rows) {
                    info[n] = c.model ? c.n_tx | (c.strand == 2 ? 1u << 16 : 0u) | 1u << 17 : 0u;
                    length[n] = (uint32_t)c.len;
                    first[n] = m;
                }
                n += 1;
                if (!c.model) continue;
                // every merged segment, clipped to the text, as letters [a, b] of the text: the cut boundaries inside it are
                // a + 1 .. b, and s[c] is one of its letters for c = a .. b
                ev.clear();
                for (uint64_t x = 0; x < c.n_tx; ++x) {
                    const crp_annotation::Transcript &tx = an->txs[c.tx_first + x];
                    const bool primary = x == c.primary;
                    for (uint64_t k = 0; k < tx.seg_n; ++k) {
                        const int64_t a = std::max<int64_t>(an->segs[tx.seg_first + k].first + shift, 0);
                        const int64_t b = std::min<int64_t>(an->segs[tx.seg_first + k].second + shift, (int64_t)len - 1);
                        if (a > b) continue;
                        if (primary) ev.push_back(Event{a, 0, 0, 1});
                        ev.push_back(Event{a + 1, 1, primary ? 1 : 0, 0});
                        ev.push_back(Event{b + 1, -1, primary ? -1 : 0, primary ? -1 : 0});
                    }
                }
                std::sort(ev.begin(), ev.end(), [](const Event &p, const Event &q) { return p.at < q.at; });
                const crp_annotation::Transcript &P = an->txs[c.tx_first + c.primary];
                // P's coding letters below the text's first letter, on the whole contig: where the running count starts
                uint64_t before = 0;
                for (uint64_t k = 0; k < P.seg_n; ++k) {
                    const int64_t a = an->segs[P.seg_first + k].first + shift, b = an->segs[P.seg_first + k].second + shift;
                    if (a < 0) before += (uint64_t)(std::min<int64_t>(0, b + 1) - a);
                }
                int32_t cover = 0, inside = 0, grow = 0;
                int64_t at_x = 0;  // `before` counts the letters below text index at_x
                uint32_t last = 0;  // the word of the step before: before the first one nothing holds
                for (size_t i = 0; i < ev.size();) {
                    const int64_t x = ev[i].at;
                    if (grow) before += (uint64_t)(x - at_x);  // (inside the text P's letters are the clipped segments': grow says it all)
                    at_x = x;
                    for (; i < ev.size() && ev[i].at == x; ++i) cover += ev[i].cover, inside += ev[i].inside, grow += ev[i].grow;
                    const uint32_t w = (uint32_t)cover | (inside ? 1u << 16 : 0u) | (grow ? 1u << 17 : 0u);
                    if (w == last) continue;
                    last = w;
                    if (m < cap_steps) {
                        at[m] = (uint32_t)(base + (uint64_t)x);
                        word[m] = w;
                        cum[m] = (uint32_t)before;
                    }
                    m += 1;
                }
            }
        }
    } catch (const std::bad_alloc &) {
        return CRP_ERR_NOMEM;
    }
    *n_rows = n;
    *n_steps = m;
    return n <= cap_rows && m <= cap_steps ? CRP_OK : CRP_ERR_CAPACITY;
}

int crp_annotation_cds_flags(const crp_annotation *an, uint8_t *flags)
{
    if (!an || (!flags && !an->cds_flag.empty())) return CRP_ERR_INVALID;
    if (!an->cds_flag.empty()) std::memcpy(flags, an->cds_flag.data(), an->cds_flag.size());
    return CRP_OK;
}

}  // extern "C"
