"""Contig-local positions past 2^31 through the piece path: crp_plan.cpp (pack_pieces, piece_cuts, owned_run), crp_gather.hip
(lower_bound_kernel, pos_rebase_kernel -- also in place --, pos16_buckets_kernel, pos16_pack_kernel, pos16_expand_kernel, the
Rebaser) and their callers, the pipelined scan (crp_scan_stream, Engine.scan_stream) and the node handle (crp_node_*).

The genome (long_contig_cases.py) is [S, b"", T]: S one contig string of 2^31 + 2^20 characters, filler that gives no row but
for eight islands of random letters on the boundaries of the plans -- the start, the first default slice cut, arena position
2^30 on a root and on a non-root device, the world-2 share cut, the cut that ends a full arena, contig position 2^31, the
end.  A piece that begins beyond its arena position has a `sub` that is negative modulo 2^32; here that constant, the needles,
begin[], bstart[] and b << 16 carry their high bits, tens of thousands of pos16 buckets and dozens of slices in a row are
empty, and rows lie in the last words of a full arena next to the halo cut.  Expected rows: the oracle's, composed island by
island (the CPU tests hold that composition against the oracle's scan of a whole contig at a small scale); T's straight
from the oracle.  Positions are compared as int64; the tables must carry them as uint32.

Out of scope here:
  * pos16 on a NON-ROOT device whose arena is full -- it would need 2^32 characters of host text;
  * the per-rank gather of crp_comm.cpp -- the same kernels with an empty piece map.
"""
import ctypes
import gc

import numpy as np
import pytest

import long_contig_cases as lc
from test_node import _owned_rows, _wire_bytes, bits

GUIDE_LENGTHS = (7, 20, 23)


# ------------------------------------------------------------------ CPU: the composition rule, the layout, the expectation
@pytest.mark.parametrize("merged", [True, False], ids=["B4-B5-one-island", "B4-B5-apart"])
def test_composition_equals_oracle_at_small_scale(oracle, merged):
    """The builder at 2^-10 of the full scale (S of 2^21 + 2^16 characters, every limit scaled): the rows composed island by
    island == oracle.scan_score of the whole contig, positions and the bits of both value columns, for l = 7, 20, 23 -- with
    the arena limit scaled exactly (B4 and B5 384 characters apart: one island over both) and with B4 4 480 below B5."""
    lay = lc.Layout(lc.small_scale(merged))
    assert any(len(names) == 2 for _, _, names, _ in lay.islands) == merged
    s = lay.build_contig()
    assert s.size == lay.L and s[0] == ord("'") and s[-3:].tobytes() == b"')]"
    for l in GUIDE_LENGTHS:
        want, got = oracle.scan_score(s, l), lay.expected(oracle, l)
        for key in lc.KEYS:
            assert got[key].shape == want[key].shape, (l, key)
            if key.startswith("pos_"):
                assert got[key].dtype == np.int64 and (got[key] == want[key].astype(np.int64)).all(), (l, key)
            else:
                assert (bits(got[key]) == bits(want[key])).all(), (l, key)
        assert want["pos_plus"].size > 1000 and want["pos_minus"].size > 1000
    filler = np.full(200_000, lc.FILLER, dtype=np.uint8)
    assert all(oracle.scan_score(filler, l)[key].size == 0 for l in GUIDE_LENGTHS for key in ("pos_plus", "pos_minus"))


def test_layout_at_full_scale():
    """Lengths only (nothing of 2 GB is allocated): every island straddles the boundary it is named for; B2 and B6 lie at
    arena position 2^30 of device 0 and device 1; B4's island ends next to the last text word of a FULL arena; the piece
    behind B4 and device 1's piece begin beyond their arena position (sub wraps); the default plan has 33 slices or more, 25
    or more of them without an island."""
    from cropsr_amd import _native as nat
    lay = lc.Layout(lc.full_scale())
    L, B = lay.L, lay.boundaries
    assert L == (1 << 31) + (1 << 20) and lc.HALO == nat.HALO and lay.lengths == [L, 0, lc.T_LETTERS + 4]
    assert len(lay.islands) == 8 and [names for _, _, names, _ in lay.islands] == [("B%d" % k,) for k in range(8)]
    for (lo, hi, _, text), nxt in zip(lay.islands, lay.islands[1:]):
        assert nxt[0] - hi >= lc.MIN_GAP and text.size == hi - lo == lc.ISLAND
    for name, b in B.items():
        lo, hi, _, _ = lay.island_of(name)
        if name == "B0":
            assert (lo, hi) == (1, 1 + lc.ISLAND)
        elif name == "B7":
            assert (lo, hi) == (L - 3 - lc.ISLAND, L - 3)
        else:
            assert lo == b - 1500 and hi == b + 1500 and 0 < lo < b < hi < L
    assert B["B5"] == 1 << 31 and B["B0"] < B["B1"] < B["B2"] < B["B3"] < B["B4"] < B["B5"] < B["B6"] < B["B7"]
    # the share cut, and arena position 2^30 either side of it
    assert [(c, d) for c, s, e, d in lay.shares] == [(0, 0), (0, 1), (1, 1), (2, 1)] and lay.shares[0][2] == lay.shares[1][1] == B["B3"]
    assert [p[4] for p in lay.node2] == [0, 0, 0, 0]  # one arena per device
    assert abs(lay.arena_position(B["B2"], 0) - (1 << 30)) <= 1500 and B["B2"] < B["B3"]
    assert abs(lay.arena_position(B["B6"], B["B3"]) - (1 << 30)) <= 1500 and B["B3"] < B["B6"] < L
    assert abs(B["B6"] - ((1 << 31) + (1 << 19))) < 40_000
    # Node([0]) and whole-arena slices: S is cut where an empty arena of the largest size ends its piece
    assert lay.arenas == [(0, 0, B["B4"], 0), (0, B["B4"], L, 1), (1, 0, 0, 1), (2, 0, lay.lengths[2], 1)]
    words = 1 + (B["B4"] + lc.HALO + 63) // 64 + 1  # the leading separator and the piece's text
    assert lay.scale.arena_words - 1 <= words <= lay.scale.arena_words  # a full arena
    last_text_char = lay.arena_position(B["B4"] + lc.HALO, 0)
    assert last_text_char > (1 << 31) - 140_000
    assert abs(lay.arena_position(lay.island_of("B4")[1], 0) - last_text_char) <= 1500 + lc.HALO
    # sub = begin - start (mod 2^32) wraps where a piece begins beyond its arena position
    for start in (B["B4"], B["B3"]):
        begin = lay.arena_position(start, start)
        assert begin == lc.ARENA_OFF + lc.HALO < start
    # the default slices
    assert lay.scale.slice_words == (1 << 20) + 2 and lay.slices[0][:3] == (0, 0, B["B1"])
    n_slices = lay.slices[-1][3] + 1
    owns_island = set()
    for c, s, e, k in lay.slices:
        if c == 0 and any(lo < e and s < hi for lo, hi, _, _ in lay.islands):
            owns_island.add(k)
        if c == 0 and s:
            assert lay.arena_position(s, s) < s
    assert n_slices >= 33 and n_slices - len(owns_island) >= 25
    free_runs = "".join(" " if k in owns_island else "x" for k in range(n_slices)).split()
    assert max(len(run) for run in free_runs) >= 12, free_runs  # hit-free slices in a row


def test_expected_rows_are_not_vacuous(oracle):
    """On each side of every boundary the expected tables hold 100 rows or more per strand (nothing lies before B0 or behind
    B7).  INSIDE its island, each side of a boundary holds 60 or more per strand: 1 500 random letters of ALPHA carry
    1 500 x (5/21)^2 = 85 PAMs per strand on average, and 60 is that less 2.7 standard deviations of a Poisson count --
    a 3 000-letter island cannot promise 100 per half.  Some rows score -1 (no complete 30-window, or l != 20), most at l = 20
    do not."""
    lay = lc.Layout(lc.full_scale())
    for l in GUIDE_LENGTHS:
        rows = lay.expected(oracle, l)
        for strand in ("plus", "minus"):
            pos, score = rows["pos_" + strand], rows["score_" + strand]
            assert pos.dtype == np.int64 and (np.diff(pos) > 0).all() and pos[0] < 100 and pos[-1] > lay.L - 100
            assert int((pos >= 1 << 31).sum()) > 300
            for name, b in lay.boundaries.items():
                lo, hi, _, _ = lay.island_of(name)
                left, right = int((pos < b).sum()), int((pos >= b).sum())
                print(l, strand, name, "rows left", left, "right", right, "inside the island", int(((pos >= lo - 64) & (pos < b)).sum()),
                      int(((pos >= b) & (pos < hi + 64)).sum()))
                if name != "B0":
                    assert left >= 100 and int(((pos >= lo - 64) & (pos < b)).sum()) >= 60, (l, strand, name)
                if name != "B7":
                    assert right >= 100 and int(((pos >= b) & (pos < hi + 64)).sum()) >= 60, (l, strand, name)
            if l == 20:
                assert int((score != -1).sum()) > 0.9 * score.size
            else:
                assert (score == -1).all()
    both = lay.expected(oracle, 20)
    assert int((both["score_plus"] == -1).sum() + (both["score_minus"] == -1).sum()) > 0


# ------------------------------------------------------------------ GPU
class _Big:
    def __init__(self, oracle):
        self.lay = lc.Layout(lc.full_scale())
        self.S = self.lay.build_contig()
        self.contigs = [self.S, b"", self.lay.T]
        self.oracle = oracle

    def want(self, l):
        return self.lay.expected_genome(self.oracle, l)

    def totals(self, l):
        w = self.want(l)
        return sum(c["pos_plus"].size for c in w), sum(c["pos_minus"].size for c in w)

    def check(self, hits, l, ctx, pre=False):
        """Per contig: counts, positions (as int64; carried as uint32) and the bits of the value column."""
        total = 0
        for k, want in enumerate(self.want(l)):
            got = hits.contig(k)
            for strand in ("plus", "minus"):
                g, w = got["pos_" + strand], want["pos_" + strand]
                assert g.dtype == np.uint32, (ctx, k, strand, g.dtype)
                assert g.shape == w.shape, (ctx, k, strand, g.shape, w.shape)
                bad = np.flatnonzero(g.astype(np.int64) != w)
                assert bad.size == 0, (ctx, k, strand, "first wrong row", int(bad[0]), int(g[bad[0]]), int(w[bad[0]]), "of", bad.size)
                col = "pre_" if pre else "score_"
                assert (bits(got["score_" + strand]) == bits(want[col + strand])).all(), (ctx, k, strand, col)
                total += w.size
        assert hits.n_plus + hits.n_minus == total, ctx
        return total


@pytest.fixture(scope="module")
def big(oracle):
    b = _Big(oracle)
    yield b
    b.S = b.contigs = None
    gc.collect()


def _plan_rows(node):
    return [(p["contig"], p["start"], p["end"], p["device"], p["arena"]) for p in node.plan()]


@pytest.mark.gpu
@pytest.mark.parametrize("l,pre", [(20, False), (20, True), (7, False)])
def test_scan_stream_whole_arena_slices(big, l, pre):
    """slice_chars = 2^31: a slice is a whole arena of crp_arena_max_words() -- two slices, S cut at B4.  Slice 0's rows reach
    the last words of a full arena; slice 1 begins beyond its arena position and ends past contig position 2^31."""
    from cropsr_amd import Engine
    with Engine(0) as eng:
        hits = eng.scan_stream(big.contigs, l, want_pre=pre, slice_chars=1 << 31, density=1e-5)
        assert hits.stream_stats["slices"] == 2 == big.lay.arenas[-1][3] + 1, hits.stream_stats
        big.check(hits, l, ("whole-arena slices", l, pre), pre=pre)


@pytest.mark.gpu
def test_scan_stream_default_slices_fresh_and_pinned_tables(big):
    """The default 64 Mi-character slices: as many as the restated plan has, on four lanes, most of them hit-free -- into
    fresh pageable tables and into pinned ones (Engine.empty_tables)."""
    from cropsr_amd import Engine
    n_slices = big.lay.slices[-1][3] + 1
    n_plus, n_minus = big.totals(20)
    with Engine(0) as eng:
        hits = eng.scan_stream(big.contigs, 20, density=1e-5)
        assert hits.stream_stats["slices"] == n_slices >= 33 and hits.stream_stats["lanes"] == 4, hits.stream_stats
        assert hits.stream_stats["tables_pinned"] == 0
        big.check(hits, 20, "default slices, fresh tables")
        del hits
        out = eng.empty_tables(n_plus + 10, n_minus + 10)
        hits = eng.scan_stream(big.contigs, 20, out=out)
        assert hits.stream_stats["slices"] == n_slices and hits.stream_stats["lanes"] == 4 and hits.stream_stats["tables_pinned"] == 1
        assert hits.pos_plus.ctypes.data == out[0].ctypes.data
        big.check(hits, 20, "default slices, pinned tables")


@pytest.mark.gpu
def test_scan_stream_default_slices_capacity_protocol(big):
    """The C ABI with a '+' table one row short: CRP_ERR_CAPACITY, nothing written beyond the capacity, the exact totals (as
    64-bit counts) to come back with; the '-' tables, which are large enough, are complete.  The wrapper with a density that is
    too small comes back once by itself, with tables of exactly the rows needed."""
    from cropsr_amd import Engine, _native as nat
    n_plus, n_minus = big.totals(20)
    want = big.want(20)
    with Engine(0) as eng:
        L = nat.lib()
        bufs = [np.frombuffer(c, dtype=np.uint8) if isinstance(c, bytes) else c for c in big.contigs]
        ptrs = (ctypes.c_void_p * 3)(*[b.ctypes.data if b.size else None for b in bufs])
        lens = np.array([b.size for b in bufs], dtype=np.uint64)
        cap = n_plus - 1
        pos = [np.full(cap + 64, 0xDEADBEEF, dtype=np.uint32), np.full(n_minus + 64, 0xDEADBEEF, dtype=np.uint32)]
        val = [np.full(cap + 64, -7.0), np.full(n_minus + 64, -7.0)]
        per = np.zeros((3, 2), dtype=np.uint64)
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        st = L.crp_scan_stream(eng._ctx, ptrs, lens.ctypes.data_as(nat.u64p), 3, 20, 0, 0, pos[0].ctypes.data_as(nat.u32p),
                               val[0].ctypes.data_as(nat.f64p), cap, pos[1].ctypes.data_as(nat.u32p), val[1].ctypes.data_as(nat.f64p),
                               n_minus, per.ctypes.data_as(nat.u64p), ctypes.byref(a), ctypes.byref(b), None)
        assert st == nat.CRP_ERR_CAPACITY and "rows are needed" in L.crp_last_error(eng._ctx).decode()
        assert (a.value, b.value) == (n_plus, n_minus)
        assert (pos[0][cap:] == 0xDEADBEEF).all() and (val[0][cap:] == -7.0).all()
        assert (pos[1][n_minus:] == 0xDEADBEEF).all() and (val[1][n_minus:] == -7.0).all()
        assert per.tolist() == [[w["pos_plus"].size, w["pos_minus"].size] for w in want]
        assert (pos[1][:n_minus].astype(np.int64) == np.concatenate([w["pos_minus"] for w in want])).all()
        assert (bits(val[1][:n_minus]) == bits(np.concatenate([w["score_minus"] for w in want]))).all()
        # the wrapper: 1 024 rows per strand to begin with
        hits = eng.scan_stream(big.contigs, 20, density=1e-9)
        big.check(hits, 20, "retry")
        assert hits.pos_plus.base is not None and hits.pos_plus.base.size == n_plus > 1024 and hits.pos_minus.base.size == n_minus > 1024


@pytest.mark.gpu
def test_node_one_device_two_arenas(big):
    """Node([0]): S is cut at B4 into two arenas of the one device -- the plan is the restated packing; the root's own rows
    go through pos_rebase_kernel with a wrapped `sub`, gathered on the device and over the host link; count_scored."""
    from cropsr_amd import node as nd
    want = big.want(20)
    scored = sum(int((w["score_plus"] != -1).sum() + (w["score_minus"] != -1).sum()) for w in want)
    with nd.Node([0]) as node:
        node.load(big.contigs)
        assert node.n_arenas(0) == 2
        assert _plan_rows(node) == [(c, s, e, 0, a) for c, s, e, a in big.lay.arenas]
        for kw in ({}, {"to_host": True}):
            hits = node.scan(20, **kw)
            big.check(hits, 20, ("Node([0])", kw))
            assert node.count_scored() == scored > 0, kw
            del hits


def _wire_bytes_plain(pieces, lengths, rows, root, pos16):
    """test_node._wire_bytes states a gather with both optional columns (16 B of off-target counts and a 4 B label-set id
    per row); a gather without them carries 20 B less per row of a peer."""
    return _wire_bytes(pieces, lengths, rows, root, pos16) - 20 * sum(sum(n) for dev, n in rows.items() if dev != root)


@pytest.mark.gpu
def test_node_two_devices_every_exchange(big):
    """Node([0, 0]): the share cut B3 lies inside S, so each device's arena crosses arena position 2^30 (at B2 and at B6) and
    device 1 begins beyond its arena position.  With either root the OTHER device's rows cross through pos16 buckets (more
    than 16 384 of them, all but a few empty), pack, expand and -- raw -- the in-place rebase; bytes_to_root under pos16 is
    what test_node._wire_bytes states for these pieces."""
    from cropsr_amd import node as nd
    lay = big.lay
    want = big.want(20)
    rows = _owned_rows(lay.shares, [(w["pos_plus"], w["pos_minus"]) for w in want])
    assert all(min(n) > 500 for n in rows.values()) and sorted(rows) == [0, 1]
    with nd.Node([0, 0]) as node:
        node.load(big.contigs)
        assert [node.n_arenas(k) for k in (0, 1)] == [1, 1]
        assert _plan_rows(node) == lay.node2 and [p[:4] for p in lay.node2] == lay.shares
        for kw in ({}, {"pos16": False}, {"to_host": True}, {"root": 1}, {"root": 1, "pos16": False}, {"pre": True}):
            hits = node.scan(20, **kw)
            big.check(hits, 20, ("Node([0, 0])", kw), pre=kw.get("pre", False))
            st = node.gather_stats()
            if kw.get("to_host"):
                assert st["bytes_to_root"] == 0 and st["transport"].startswith("none: every device"), st
            else:
                assert st["transport"] == "device-to-device copies", st
                pos16 = kw.get("pos16", True)
                assert st["bytes_to_root"] == _wire_bytes_plain(lay.shares, lay.lengths, rows, kw.get("root", 0), pos16), (kw, st)
            del hits


@pytest.mark.gpu
def test_engine_genome_refuses_the_contig(big, oracle):
    """with Engine.genome a contig must fit one arena -- S is refused before anything is uploaded, and the
    engine goes on serving: a classic arena scan of T equals the oracle."""
    from cropsr_amd import CropsrHipError, Engine
    with Engine(0) as eng:
        before = len(eng._arenas)
        with pytest.raises((CropsrHipError, ValueError)):
            eng.genome([big.S])
        assert len(eng._arenas) == before  # (no arena was made: nothing went up)
        arena = eng.arena([big.lay.T])
        one = arena.scan_score(20)
        want = oracle.scan_score(big.lay.T, 20)
        for key in lc.KEYS:
            assert (bits(one.contig(0)[key]) == bits(want[key])).all(), key
        assert want["pos_plus"].size > 1000
        arena.close()
