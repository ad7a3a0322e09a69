// crp_select_pairs_distinct.hip -- distinct pair selection on the device: for every gene, at most
// KP qualifying pairs taken greedily in the pairs' order (section 19: higher min score, higher max score, smaller c_a,
// smaller c_b, smaller strand bits), where a pair is taken only if neither of its two rows is a row of a pair taken
// before it (include/cropsr_hip.h, crp_select_run_pairs_distinct, states the definition).  The greedy is sequential in
// its picks and parallel over genes and over the rows of one round:
//
//   pass key  pair_pass_key_kernel, as it is: the predicate once per row, 8 bytes a row (the score's bits, else 0)
//   bounds    select_bounds_kernel's runs and crp_select_run_pairs' cut into PairItems, as they are
//   items     one WAVE per work item.  Round t walks the item's a-rows 64 a trip and streams each a-row's partner runs
//             as pair_items_kernel does (binary-searched runs, 12 bytes a partner, coalesced).  The picks live one per
//             lane -- lane u holds pick u's packed a and b -- and are read wave-uniformly.  Every lane keeps one running
//             best; a six-step butterfly reduces the 64 of them at the end of the round.  Round 0 streams every partner,
//             because it counts n_pairs.  From round 1 on only the maximum is wanted: the wave keeps `bar`, the highest
//             kmin any lane holds, and an a-row that is taken, or whose own key lies BELOW bar, is skipped with its whole
//             run (no pair of it can win; equal keys are walked, ties decide on kmax and the boundaries); a trip of
//             partners is tested against the picks only when a ballot says one of them beats a lane's best.
//             A whole gene (slot == SELECT_NONE, nearly every gene) runs all its rounds in one launch.  A piece of a cut
//             gene runs one round a launch: the picks so far come from the gene's pairs array, the best candidate goes to
//             the piece's proposal slot
//   pick      one wave per cut gene over its pieces' proposals, the same order: the winner is appended to pairs
//
// No LDS memory, no atomics, no scratch; every slot has one owner and is written with plain vector stores.
#include "crp_kernels.h"
#include "crp_select_pairs_distinct.h"

namespace crp {

static_assert(BLOCK == SELECT_WAVES * 64, "one wave of 64 lanes per work item");
static_assert(sizeof(PairProposal) == 32, "one proposal slot");

namespace {

// The entry, the order and the lane reads of crp_select_pairs.hip, restated: that file keeps its text (and its assembly).
struct PairEntry {
    unsigned long long kmin, kmax, tie;  // tie = c_a << 32 | c_b
    uint32_t a, b;                       // row | strand << 31
};

// the order of the definition: higher min score, higher max score, smaller c_a, smaller c_b, smaller strand bits
__device__ __forceinline__ bool pair_better(const PairEntry &x, const PairEntry &y)
{
    if (x.kmin != y.kmin) return x.kmin > y.kmin;
    if (x.kmax != y.kmax) return x.kmax > y.kmax;
    if (x.tie != y.tie) return x.tie < y.tie;
    return (x.a >> 31) * 2u + (x.b >> 31) < (y.a >> 31) * 2u + (y.b >> 31);
}

__device__ __forceinline__ uint32_t pair_lane32(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }
__device__ __forceinline__ unsigned long long pair_lane64(unsigned long long v, int l)
{
    return (unsigned long long)pair_lane32((uint32_t)(v >> 32), l) << 32 | pair_lane32((uint32_t)v, l);
}

// No entry: worse than every pair (a pair's kmin is a passing score's bits, above 0).
__device__ __forceinline__ PairEntry pair_none() { return PairEntry{0ull, 0ull, ~0ull, SELECT_NONE, SELECT_NONE}; }

// the wave's best entry, in every lane (a SELECT_NONE: none).  The order is total over real pairs, so both lanes of an
// exchange keep the same one
__device__ __forceinline__ PairEntry pair_wave_best(PairEntry mine)
{
    for (int off = 32; off > 0; off >>= 1) {
        const PairEntry o{__shfl_xor(mine.kmin, off), __shfl_xor(mine.kmax, off), __shfl_xor(mine.tie, off), __shfl_xor(mine.a, off),
                          __shfl_xor(mine.b, off)};
        if (pair_better(o, mine)) mine = o;
    }
    return mine;
}

// the largest of the lanes' values, wave-uniform
__device__ __forceinline__ unsigned long long pair_wave_max(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return pair_lane64(v, 0);
}

// the first row in [a, b) whose position is >= key (b when there is none)
__device__ __forceinline__ uint32_t pair_lower_bound(const uint32_t *__restrict__ pos, uint32_t a, uint32_t b, long long key)
{
    while (a < b) {
        const uint32_t mid = a + ((b - a) >> 1);
        if ((long long)pos[mid] < key) a = mid + 1;
        else b = mid;
    }
    return a;
}

}  // namespace

__global__ __launch_bounds__(BLOCK) void pair_distinct_items_kernel(const uint32_t *__restrict__ pos_plus, const uint32_t *__restrict__ pos_minus,
                                                                    const unsigned long long *__restrict__ key_plus,
                                                                    const unsigned long long *__restrict__ key_minus, PairParams pp, uint32_t round,
                                                                    const PairItem *__restrict__ items, uint32_t n_items,
                                                                    unsigned long long *__restrict__ evals, PairDistinctRounds rounds,
                                                                    PairDistinctResult res)
{
    const uint32_t item = blockIdx.x * SELECT_WAVES + (threadIdx.x >> 6);  // (uniform per wave)
    if (item >= n_items) return;
    const int lane = threadIdx.x & 63;
    const PairItem it = items[item];
    const int k = pp.k;
    const bool piece = it.slot != SELECT_NONE;
    // a piece runs round `round` alone -- and nothing once its gene has ended (a round without a pick); a whole gene runs 0 .. k
    if (piece && round && res.n_distinct[it.gene] != round) return;
    const int t0 = piece ? (int)round : 0, t1 = piece ? (int)round + 1 : k;
    // the picks so far, one per lane: both rows of pick u in lane u
    uint32_t pick_a = SELECT_NONE, pick_b = SELECT_NONE;
    if (piece && lane < t0) {
        const uint64_t at = ((uint64_t)it.gene * k + lane) * 2;
        pick_a = res.pairs[at];
        pick_b = res.pairs[at + 1];
    }
    uint32_t n_pass = 0;
    unsigned long long n_pairs = 0, n_evals = 0;
    int t = t0;
    PairEntry best = pair_none();
    for (; t < t1; ++t) {
        PairEntry mine = pair_none();
        unsigned long long bar = 0ull;  // (uniform per wave) the highest kmin a lane holds: below it nothing can win
        for (int s = 0; s < 2; ++s) {
            const uint32_t *pos_a = s ? pos_minus : pos_plus;
            const unsigned long long *key_a = s ? key_minus : key_plus;
            // the cut boundary c of a row (repair.py): '+' i - 3, '-' j + 6
            const uint32_t off_a = s ? 6u : (uint32_t)-3;
            // (the item's rows lie inside the table and inside the gene's runs: crp_select.cpp cuts them from the bounds
            // kernel's runs and checks those against the tables)
            const uint32_t end = it.first[s] + it.rows[s];
            for (uint32_t r0 = it.first[s]; r0 < end; r0 += 64) {
                const uint32_t row = r0 + lane;
                const bool in = row < end;
                const unsigned long long ka = in ? key_a[row] : 0ull;
                const uint32_t ca = in ? pos_a[row] + off_a : 0u;
                if (t == 0) n_pass += (uint32_t)__popcll(__ballot(ka != 0ull));
                // an a-row that is a row of a pick is out with its whole run, and from round 1 on so is one whose own key lies
                // below the bar: every pair of it has kmin <= ka.  Round 0 walks every passing a-row: it counts n_pairs
                const uint32_t pa = row | (uint32_t)s << 31;
                bool walk = ka != 0ull && (t == 0 || ka >= bar);
                for (int u = 0; u < t; ++u) walk = walk && pa != pair_lane32(pick_a, u) && pa != pair_lane32(pick_b, u);
                // this lane's partner runs: rows [p0, p1) of table tb, inside the gene's run of that table
                uint32_t p0[2], p1[2];
#pragma unroll
                for (int tb = 0; tb < 2; ++tb) {
                    const bool allowed = walk && (pp.mask >> (s * 2 + tb) & 1u);
                    const uint32_t *pos_b = tb ? pos_minus : pos_plus;
                    const long long back = tb ? 6 : -3;  // pos_b = c_b - back
                    p0[tb] = allowed ? pair_lower_bound(pos_b, it.run[2 * tb], it.run[2 * tb + 1], (long long)ca + pp.dmin - back) : 0u;
                    p1[tb] = allowed ? pair_lower_bound(pos_b, p0[tb], it.run[2 * tb + 1], (long long)ca + pp.dmax - back + 1) : 0u;
                }
                unsigned long long todo = __ballot(p1[0] > p0[0] || p1[1] > p0[1]);
                while (todo) {
                    const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
                    todo &= todo - 1;
                    const unsigned long long uka = pair_lane64(ka, l);
                    if (t && uka < bar) continue;  // (wave-uniform: the bar has risen since the ballot)
                    const uint32_t uca = pair_lane32(ca, l);
                    const uint32_t ua = (r0 + (uint32_t)l) | (uint32_t)s << 31;
#pragma unroll
                    for (int tb = 0; tb < 2; ++tb) {
                        const uint32_t *pos_b = tb ? pos_minus : pos_plus;
                        const unsigned long long *key_b = tb ? key_minus : key_plus;
                        const uint32_t off_b = tb ? 6u : (uint32_t)-3;
                        const uint32_t q0 = pair_lane32(p0[tb], l), q1 = pair_lane32(p1[tb], l);
                        n_evals += q1 - q0;
                        for (uint32_t q = q0; q < q1; q += 64) {
                            const uint32_t rb = q + lane;
                            const bool inb = rb < q1;
                            const unsigned long long kb = inb ? key_b[rb] : 0ull;
                            const uint32_t cb = inb ? pos_b[rb] + off_b : 0u;
                            // (the run's rows have dmin <= c_b - c_a <= dmax by the searches)
                            const bool ok = kb != 0ull && !(pp.frameshift && (cb - uca) % 3u == 0u);
                            if (t == 0) n_pairs += (unsigned long long)__popcll(__ballot(ok));
                            const PairEntry cand{uka < kb ? uka : kb, uka < kb ? kb : uka, (unsigned long long)uca << 32 | cb, ua,
                                                 rb | (uint32_t)tb << 31};
                            bool want = ok && cand.kmin >= bar && pair_better(cand, mine);
                            if (!__ballot(want)) continue;  // (wave-uniform: a trip that beats no lane's best reads no pick)
                            for (int u = 0; u < t; ++u) want = want && cand.b != pair_lane32(pick_a, u) && cand.b != pair_lane32(pick_b, u);
                            if (want) mine = cand;
                            if (__ballot(want)) bar = pair_wave_max(mine.kmin);
                        }
                    }
                }
            }
        }
        best = pair_wave_best(mine);
        if (piece || best.a == SELECT_NONE) break;  // (a round without a candidate ends the gene)
        if (lane == t) {
            pick_a = best.a;
            pick_b = best.b;
        }
    }
    // (a piece's slot in evals is its own from launch to launch: later rounds add to round 0's count)
    if (lane == 0) evals[item] = (piece && round ? evals[item] : 0ull) + n_evals;
    if (piece) {
        if (lane == 0) {
            rounds.prop[it.slot] = PairProposal{best.kmin, best.kmax, best.tie, best.a, best.b};
            if (round == 0) {
                rounds.slot_pass[it.slot] = n_pass;
                rounds.slot_pairs[it.slot] = n_pairs;
            }
        }
    } else {
        // (t: the pairs taken; lanes t .. k - 1 still hold SELECT_NONE)
        if (lane < k) {
            const uint64_t at = ((uint64_t)it.gene * k + lane) * 2;
            res.pairs[at] = pick_a;
            res.pairs[at + 1] = pick_b;
        }
        if (lane == 0) {
            res.n_pass[it.gene] = n_pass;
            res.n_pairs[it.gene] = n_pairs;
            res.n_distinct[it.gene] = (uint32_t)t;
        }
    }
}

__global__ __launch_bounds__(BLOCK) void pair_distinct_pick_kernel(const SelectMerge *__restrict__ genes, uint32_t n_genes, uint32_t first_gene,
                                                                   int k, uint32_t round, PairDistinctRounds rounds, PairDistinctResult res)
{
    const uint32_t m = blockIdx.x * SELECT_WAVES + (threadIdx.x >> 6);  // (uniform per wave)
    if (m >= n_genes) return;
    const int lane = threadIdx.x & 63;
    const SelectMerge g = genes[m];
    if (round && res.n_distinct[g.gene] != round) {  // the gene has ended
        if (lane == 0) rounds.picked[first_gene + m] = 0u;
        return;
    }
    PairEntry mine = pair_none();
    uint32_t n_pass = 0;
    unsigned long long n_pairs = 0;
    for (uint32_t j = lane; j < g.n_slots; j += 64) {
        const uint64_t slot = (uint64_t)g.slot + j;
        const PairProposal p = rounds.prop[slot];
        const PairEntry cand{p.kmin, p.kmax, p.tie, p.a, p.b};
        if (p.a != SELECT_NONE && pair_better(cand, mine)) mine = cand;
        if (round == 0) {
            n_pass += rounds.slot_pass[slot];
            n_pairs += rounds.slot_pairs[slot];
        }
    }
    mine = pair_wave_best(mine);
    const bool found = mine.a != SELECT_NONE;
    if (round == 0) {
        for (int off = 32; off > 0; off >>= 1) {
            n_pass += __shfl_xor(n_pass, off);
            n_pairs += __shfl_xor(n_pairs, off);
        }
        if (lane < k) {
            const uint64_t at = ((uint64_t)g.gene * k + lane) * 2;
            res.pairs[at] = (lane == 0 && found) ? mine.a : SELECT_NONE;
            res.pairs[at + 1] = (lane == 0 && found) ? mine.b : SELECT_NONE;
        }
    }
    if (lane == 0) {
        if (round == 0) {
            res.n_pass[g.gene] = n_pass;
            res.n_pairs[g.gene] = n_pairs;
        }
        if (found && round) {
            const uint64_t at = ((uint64_t)g.gene * k + round) * 2;
            res.pairs[at] = mine.a;
            res.pairs[at + 1] = mine.b;
        }
        if (found || round == 0) res.n_distinct[g.gene] = round + (found ? 1u : 0u);
        rounds.picked[first_gene + m] = found ? 1u : 0u;
    }
}

hipError_t launch_pair_distinct_items(hipStream_t s, const uint32_t *pos_plus, const uint32_t *pos_minus, const unsigned long long *key_plus,
                                      const unsigned long long *key_minus, const PairParams &pp, uint32_t round, const PairItem *items,
                                      uint32_t n_items, unsigned long long *evals, const PairDistinctRounds &rounds,
                                      const PairDistinctResult &res)
{
    if (!n_items) return hipSuccess;
    hipLaunchKernelGGL(pair_distinct_items_kernel, dim3((n_items + SELECT_WAVES - 1) / SELECT_WAVES), dim3(BLOCK), 0, s, pos_plus, pos_minus,
                       key_plus, key_minus, pp, round, items, n_items, evals, rounds, res);
    return hipGetLastError();
}

hipError_t launch_pair_distinct_pick(hipStream_t s, const SelectMerge *genes, uint32_t n_genes, uint32_t first_gene, int k, uint32_t round,
                                     const PairDistinctRounds &rounds, const PairDistinctResult &res)
{
    if (!n_genes) return hipSuccess;
    hipLaunchKernelGGL(pair_distinct_pick_kernel, dim3((n_genes + SELECT_WAVES - 1) / SELECT_WAVES), dim3(BLOCK), 0, s, genes, n_genes, first_gene, k,
                       round, rounds, res);
    return hipGetLastError();
}

}  // namespace crp
