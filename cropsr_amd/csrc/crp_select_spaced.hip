// crp_select_spaced.hip -- spaced selection on the device: for every gene, at most K passing
// rows taken greedily in the selection's order -- higher score bits, then smaller cut site, then '+' before '-' -- where
// a row is taken only if its cut site lies at least D letters from the cut site of every row taken before it
// (include/cropsr_hip.h, crp_select_run_spaced, states the definition).  The greedy is sequential in its picks and
// parallel over genes and over the rows of one round:
//
//   pass key  pair_pass_key_kernel, as it is: the predicate once per row, 8 bytes a row (the score's bits, else 0)
//   items     one WAVE per work item of the selection's planner.  Round t walks the item's rows 64 a trip, 12 bytes a
//             row.  A row is a candidate when its key is not 0, it comes AFTER pick t - 1 in the order (which also
//             keeps a taken row from being taken again at D = 0) and its cut site clears every pick: the picks live
//             one per lane -- lane u holds pick u's cut site and packed row -- and are read wave-uniformly.  Every lane
//             keeps one running best; a six-step butterfly reduces the 64 of them at the end of the round.
//             A whole gene (slot == SELECT_NONE, nearly every gene) runs all its rounds in one launch, and for its
//             first 128 trips every lane remembers in two 64-bit words which of its rows are out for good: such a row
//             is never loaded again, and one that is still in is tested against the LATEST pick alone -- it cleared
//             the earlier ones in their rounds.  A piece of a cut gene runs one round a launch and remembers
//             nothing: the picks so far come from the gene's array of K cut sites, the best candidate goes to the
//             piece's proposal slot
//   pick      one wave per cut gene over its pieces' proposals, the same order: the winner is appended to the gene's
//             cut sites and to sel
//
// Distances are unsigned absolute differences of two cut sites below 2^31; nothing adds D to a cut site or takes it
// off one.  No LDS memory, no atomics, no scratch; every slot has one owner and is written with plain vector stores.
#include "crp_kernels.h"
#include "crp_select_spaced.h"

namespace crp {

static_assert(BLOCK == SELECT_WAVES * 64, "one wave of 64 lanes per work item");
static_assert(sizeof(SpacedProposal) == 16, "one proposal slot");

constexpr uint32_t SPACED_TRIPS = 128;  // trips of a whole gene whose rows keep an "out for good" bit: two 64-bit words a lane

namespace {

// the order of the definition: higher key, then smaller tie (cut site << 1 | strand)
__device__ __forceinline__ bool spaced_better(unsigned long long ka, uint32_t ta, unsigned long long kb, uint32_t tb)
{
    return ka > kb || (ka == kb && ta < tb);
}

// the wave's best proposal, in every lane (key 0: none)
__device__ __forceinline__ SpacedProposal spaced_wave_best(SpacedProposal mine)
{
    for (int off = 32; off > 0; off >>= 1) {
        SpacedProposal o;
        o.key = __shfl_xor(mine.key, off);
        o.tie = __shfl_xor(mine.tie, off);
        o.row = __shfl_xor(mine.row, off);
        if (spaced_better(o.key, o.tie, mine.key, mine.tie)) mine = o;
    }
    return mine;
}

__device__ __forceinline__ uint32_t spaced_lane32(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }

}  // namespace

__global__ __launch_bounds__(BLOCK) void spaced_items_kernel(const uint32_t *__restrict__ pos_plus, const uint32_t *__restrict__ pos_minus,
                                                             const unsigned long long *__restrict__ key_plus,
                                                             const unsigned long long *__restrict__ key_minus, int k, uint32_t min_distance,
                                                             uint32_t round, const SelectItem *__restrict__ items, uint32_t n_items,
                                                             SpacedRounds rounds, SpacedResult res)
{
    const uint32_t item = blockIdx.x * SELECT_WAVES + (threadIdx.x >> 6);  // (uniform per wave)
    if (item >= n_items) return;
    const int lane = threadIdx.x & 63;
    const SelectItem it = items[item];
    const bool piece = it.slot != SELECT_NONE;
    // a piece runs round `round` alone -- and nothing once its gene has ended (a round without a pick); a whole gene runs 0 .. k
    if (piece && round && res.n_spaced[it.gene] != round) return;
    const int t0 = piece ? (int)round : 0, t1 = piece ? (int)round + 1 : k;
    // the picks so far, one per lane, and the latest of them
    uint32_t pick_cut = 0u, pick_row = SELECT_NONE;
    SpacedProposal last{~0ull, 0u, SELECT_NONE};  // (before every row)
    if (piece && t0) {
        if (lane < t0) pick_cut = rounds.cuts[(uint64_t)it.gene * k + lane];
        last = rounds.last[it.gene];
    }
    uint32_t n_pass = 0;
    // a whole gene remembers which of its rows are out for good, one bit per trip and lane for its first SPACED_TRIPS trips
    // (8 192 rows): a row without a pass key, a row before the latest pick, a row within D - 1 of a pick.  A remembered row
    // that is still in has cleared every earlier pick in that pick's round, so a round tests it against the latest pick alone
    unsigned long long out0 = 0ull, out1 = 0ull;
    int t = t0;
    SpacedProposal best{0ull, SELECT_NONE, SELECT_NONE};
    for (; t < t1; ++t) {
        SpacedProposal mine{0ull, SELECT_NONE, SELECT_NONE};
        const uint32_t last_cut = last.tie >> 1;
        uint32_t trip = 0;  // (uniform per wave: the trip's number in the item)
        for (int s = 0; s < 2; ++s) {
            const uint32_t *pos = s ? pos_minus : pos_plus;
            const unsigned long long *keys = s ? key_minus : key_plus;
            const uint32_t back = s ? 0u : 3u;
            // (the item's rows lie inside the table: crp_select.cpp cuts them from the bounds kernel's runs and checks them)
            const uint32_t end = it.first[s] + it.rows[s];
            for (uint32_t r0 = it.first[s]; r0 < end; r0 += 64, ++trip) {
                const bool remembered = !piece && trip < SPACED_TRIPS;  // (uniform per wave)
                const unsigned long long bit = 1ull << (trip & 63u);
                const bool out = remembered && ((trip < 64u ? out0 : out1) & bit) != 0ull;
                if (remembered && !__ballot(!out)) continue;  // (wave-uniform: nothing of this trip is left)
                const uint32_t row = r0 + lane;
                const bool in = row < end;
                const unsigned long long key = in ? keys[row] : 0ull;
                const uint32_t cut = in ? pos[row] - back : 0u;
                const uint32_t tie = cut << 1 | (uint32_t)s;
                if (t == 0) n_pass += (uint32_t)__popcll(__ballot(key != 0ull));
                // passing and after the latest pick (which also keeps a taken row from being taken again at D = 0)
                bool alive = !out && key != 0ull && spaced_better(last.key, last.tie, key, tie);
                if (remembered) {
                    if (t) {
                        const uint32_t d = cut > last_cut ? cut - last_cut : last_cut - cut;
                        alive = alive && d >= min_distance;
                    }
                    if (!alive) {
                        if (trip < 64u) out0 |= bit;
                        else out1 |= bit;
                    }
                    if (alive && spaced_better(key, tie, mine.key, mine.tie)) mine = SpacedProposal{key, tie, row | (uint32_t)s << 31};
                    continue;
                }
                // nothing remembered (a piece; a whole gene's rows past SPACED_TRIPS trips): every pick, for the rows worth a
                // look -- those better than what the lane holds
                alive = alive && spaced_better(key, tie, mine.key, mine.tie);
                if (!__ballot(alive)) continue;  // (wave-uniform)
                for (int u = 0; u < t; ++u) {
                    const uint32_t p = spaced_lane32(pick_cut, u);
                    const uint32_t d = cut > p ? cut - p : p - cut;
                    alive = alive && d >= min_distance;
                }
                if (alive) mine = SpacedProposal{key, tie, row | (uint32_t)s << 31};
            }
        }
        best = spaced_wave_best(mine);
        if (piece || best.key == 0ull) break;  // (a round without a candidate ends the gene)
        if (lane == t) {
            pick_cut = best.tie >> 1;
            pick_row = best.row;
        }
        last = best;
    }
    if (piece) {
        if (lane == 0) {
            rounds.prop[it.slot] = best;
            if (round == 0) rounds.slot_pass[it.slot] = n_pass;
        }
    } else {
        // (t: the rows taken; lanes t .. k - 1 still hold SELECT_NONE)
        if (lane < k) res.sel[(uint64_t)it.gene * k + lane] = pick_row;
        if (lane == 0) {
            res.n_pass[it.gene] = n_pass;
            res.n_spaced[it.gene] = (uint32_t)t;
        }
    }
}

__global__ __launch_bounds__(BLOCK) void spaced_pick_kernel(const SelectMerge *__restrict__ genes, uint32_t n_genes, uint32_t first_gene, int k,
                                                            uint32_t round, SpacedRounds rounds, SpacedResult res)
{
    const uint32_t m = blockIdx.x * SELECT_WAVES + (threadIdx.x >> 6);  // (uniform per wave)
    if (m >= n_genes) return;
    const int lane = threadIdx.x & 63;
    const SelectMerge g = genes[m];
    if (round && res.n_spaced[g.gene] != round) {  // the gene has ended
        if (lane == 0) rounds.picked[first_gene + m] = 0u;
        return;
    }
    SpacedProposal mine{0ull, SELECT_NONE, SELECT_NONE};
    uint32_t n_pass = 0;
    for (uint32_t j = lane; j < g.n_slots; j += 64) {
        const uint64_t slot = (uint64_t)g.slot + j;
        const SpacedProposal p = rounds.prop[slot];
        if (spaced_better(p.key, p.tie, mine.key, mine.tie)) mine = p;
        if (round == 0) n_pass += rounds.slot_pass[slot];
    }
    mine = spaced_wave_best(mine);
    const bool found = mine.key != 0ull;
    if (round == 0) {
        for (int off = 32; off > 0; off >>= 1) n_pass += __shfl_xor(n_pass, off);
        if (lane < k) res.sel[(uint64_t)g.gene * k + lane] = (lane == 0 && found) ? mine.row : SELECT_NONE;
    }
    if (lane == 0) {
        if (round == 0) res.n_pass[g.gene] = n_pass;
        if (found) {
            rounds.cuts[(uint64_t)g.gene * k + round] = mine.tie >> 1;
            rounds.last[g.gene] = mine;
            if (round) res.sel[(uint64_t)g.gene * k + round] = mine.row;
        }
        if (found || round == 0) res.n_spaced[g.gene] = round + (found ? 1u : 0u);
        rounds.picked[first_gene + m] = found ? 1u : 0u;
    }
}

hipError_t launch_spaced_items(hipStream_t s, const uint32_t *pos_plus, const uint32_t *pos_minus, const unsigned long long *key_plus,
                               const unsigned long long *key_minus, int k, uint32_t min_distance, uint32_t round, const SelectItem *items,
                               uint32_t n_items, const SpacedRounds &rounds, const SpacedResult &res)
{
    if (!n_items) return hipSuccess;
    hipLaunchKernelGGL(spaced_items_kernel, dim3((n_items + SELECT_WAVES - 1) / SELECT_WAVES), dim3(BLOCK), 0, s, pos_plus, pos_minus, key_plus,
                       key_minus, k, min_distance, round, items, n_items, rounds, res);
    return hipGetLastError();
}

hipError_t launch_spaced_pick(hipStream_t s, const SelectMerge *genes, uint32_t n_genes, uint32_t first_gene, int k, uint32_t round,
                              const SpacedRounds &rounds, const SpacedResult &res)
{
    if (!n_genes) return hipSuccess;
    hipLaunchKernelGGL(spaced_pick_kernel, dim3((n_genes + SELECT_WAVES - 1) / SELECT_WAVES), dim3(BLOCK), 0, s, genes, n_genes, first_gene, k,
                       round, rounds, res);
    return hipGetLastError();
}

}  // namespace crp
