// crp_select_predicate.inc -- whether a table row PASSES, "in the gene" apart: the one statement of the selection's
// predicate on the device.  Included, as it stands, in the row loop of select_items_kernel (crp_select.hip), in
// pair_pass_key_kernel (crp_select_pairs.hip) and in the row loop of select_items_coding_kernel (crp_select_coding.hip), which
// goes on to clear `pass` where the coding test fails: `pass` must stay a plain, non-const bool.  A text fragment and not a function: as a __forceinline__ function the
// compiler built another select_items_kernel (601 instead of 630 instructions, other SGPR traffic), which could not be
// shown to keep the plain selection's time inside the earlier build's run-to-run spread; included as text the kernel's
// assembly is the earlier build's, instruction for instruction (DESIGN.md section 19).
//
// Reads, from the including scope: t (SelectTable), pred (SelectPredicate), row (uint32_t), in (bool: the lane holds a
// row), score (double: the row's score, -1.0 without a row) and scored (bool: in && score != -1.0 -- an unscored row has
// no cut site and passes nowhere).  Declares: bool pass.
            bool pass = scored && score >= pred.min_score;
            if (pred.stride) {
                const uint32_t c0 = in ? t.counts[(uint64_t)row * pred.stride] : SELECT_NONE;
                const unsigned long long sum = in ? t.sum[row] : ~0ull;
                pass = pass && c0 != SELECT_NONE && c0 <= pred.max_mm0 && sum <= pred.max_hit_sum;
            }
            if (pred.flags) {
                const uint32_t id = in ? t.feat[row] : SELECT_NONE;
                pass = pass && id < pred.n_flags && pred.flags[id] != 0;
            }
            if (t.props) {  // (the packed word of crp_guide_properties: gc | run << 8 | t_run << 16 | stem << 24)
                const uint32_t pr = in ? t.props[row] : 0u;
                const uint32_t gc = pr & 255u;
                pass = pass && gc >= pred.gc_min && gc <= pred.gc_max && (pr >> 8 & 255u) <= pred.max_run && (pr >> 16 & 255u) <= pred.max_t_run &&
                       pr >> 24 <= pred.max_stem;
            }
            if (t.repair) {  // (the value of crp_repair_scores: mh | oof << 32, both below 2^20)
                const unsigned long long rp = in ? t.repair[row] : 0ull;
                const uint32_t mh = (uint32_t)rp, oof = (uint32_t)(rp >> 32);
                pass = pass && mh >= pred.min_mh && 100u * oof >= pred.min_oof_pct * mh && (mh != 0u || pred.min_oof_pct == 0u);
            }
            if (t.variants) {  // (the packed word of crp_variant_counts: site | guide << 8 | seed << 16 | pam << 24, each saturated at 255)
                const uint32_t vr = in ? t.variants[row] : 0u;
                pass = pass && (vr & 255u) <= pred.max_var_site && (vr >> 8 & 255u) <= pred.max_var_guide && (vr >> 16 & 255u) <= pred.max_var_seed &&
                       vr >> 24 <= pred.max_var_pam;
            }
            if (t.sites) {  // (the value of crp_site_columns: in_guide | assay << 32, one bit per enzyme)
                const unsigned long long st = in ? t.sites[row] : 0ull;
                pass = pass && !((uint32_t)st & pred.forbid_sites) && (!pred.need_assay || ((uint32_t)(st >> 32) & pred.need_assay));
            }
