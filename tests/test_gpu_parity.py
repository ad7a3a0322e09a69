"""Parity tests proper: the HIP path, called through the C ABI (ctypes), against
the CPU oracle on the same seeded inputs, against the golden fixtures made by the
real reference, and -- at BASELINE.json's full size -- through size-independent
properties.  Integer/index columns and float columns are all compared BIT-EXACT
(tolerance 0 ulp) in the pinned `libm` environment; the only non-zero tolerances
are against fixtures from other environments (<= 2 ulp numpy-AVX512 exp,
<= 15 ulp the reference's committed sample output) and are written at the assert.
"""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from conftest import (GOLDEN, LENGTH_CASES, PROBES, VERBOSE_CASES, golden_fasta_path, normalize_verbose,
                      read_golden_csv, run_cli)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def _engine():
    from cropsr_amd import Engine
    eng = Engine(0)  # raises if libcropsr_hip.so or the GPU is missing: no fallback
    yield eng
    # no single-launch scan of this module may have run out of its look-back allowance (the fallback
    # would have hidden it: results stay right)
    assert eng.query()["chain_timeouts"] == 0
    eng.close()


@pytest.fixture(params=["single_pass-large", "single_pass-small", "two_pass-large", "two_pass-small"])
def engine(_engine, request):
    """Every parity test runs in both scan modes -- the default single launch (offsets from the chained scan inside the
    emit kernel) and the count / tile-scan / emit sequence -- and with each of the two tile geometries forced
    (CRP_OPT_TILE_GEOMETRY; by default crp_arena_seal picks one by the arena's size, and these inputs are all small)."""
    mode, geometry = request.param.split("-")
    _engine.configure(two_pass=mode == "two_pass", geometry=geometry)
    yield _engine
    _engine.configure(two_pass=False, geometry="auto")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def assert_hits_equal(got, want, ctx=""):
    for key, w in want.items():
        g = got[key]
        assert g.shape == w.shape, (ctx, key, g.shape, w.shape)
        assert (bits(g) == bits(w)).all(), (ctx, key)


def check_contigs(engine, oracle, contigs, l=20, pack="device"):
    arena = engine.arena(contigs, pack=pack)
    hits = arena.scan_score(l, want_pre=True)
    total = 0
    for k, c in enumerate(contigs):
        want = oracle.scan_score(c, l)
        assert_hits_equal(hits.contig(k), want, ctx=(k, l, pack))
        total += want["pos_plus"].size + want["pos_minus"].size
    assert hits.n_plus + hits.n_minus == total
    arena.close()
    return total


# ------------------------------------------------------------------- seam 2
def test_rs1_vectors_golden(engine, oracle):
    g = np.load(os.path.join(GOLDEN, "rs1_vectors.npz"))
    pre, score = engine.score_30mers(g["seqs"])
    opre, oscore = oracle.score30(g["seqs"])
    assert (bits(pre) == bits(opre)).all()
    assert (bits(score) == bits(oscore)).all()
    assert (bits(score) == bits(g["libm"])).all()  # the real reference, libm environment
    assert np.abs(score.view(np.int64) - g["avx512"].view(np.int64)).max() <= 2  # ulp, numpy AVX-512 exp


def test_rs1_score_dropin_batch_positions(engine):
    """Engine.rs1_score reproduces the reference's batch-position-dependent BLAS
    orders: golden vectors from the real rs1_score on batches of 1..11 rows."""
    z = np.load(os.path.join(GOLDEN, "rs1_batches.npz"))
    seqs = z["seqs"]
    for key in z.files:
        if key == "seqs":
            continue
        n = int(key[1:])
        m = (len(seqs) // n) * n
        got = np.concatenate([engine.rs1_score(seqs[k:k + n]) for k in range(0, m, n)])
        assert (bits(got) == bits(z[key])).all(), key


@pytest.mark.parametrize("order", [0, 1, 2])
def test_score_orders_vs_oracle(engine, oracle, order):
    rng = np.random.default_rng(order)
    rows = rng.choice(np.frombuffer(b"ATCGATCGATCGN'", dtype=np.uint8), size=(5000, 30))
    pre, score = engine.score_30mers(rows, order)
    opre, oscore = oracle.score30_order(rows, order)
    assert (bits(pre) == bits(opre)).all() and (bits(score) == bits(oscore)).all()


def test_score_30mers_ragged_and_empty(engine):
    pre, score = engine.score_30mers(np.empty((0, 30), dtype=np.uint8))
    assert pre.size == 0 and score.size == 0
    with pytest.raises(ValueError):
        engine.score_30mers(np.zeros((4, 29), dtype=np.uint8))


# ------------------------------------------------------------------- seam 1
@pytest.mark.parametrize("name", PROBES + ["sample"])
def test_cli_csv_bytes_equal_reference(name, manifest, tmp_path, monkeypatch):
    """python -m cropsr_amd on the GPU == every byte of the real reference's CSV
    (seeded ids) and every stdout line."""
    from cropsr_amd.cli import EngineBackend
    be = EngineBackend(0)
    got, stdout = run_cli(tmp_path, monkeypatch, golden_fasta_path(name, tmp_path), be, manifest["seed"])
    be.close()
    want = read_golden_csv(name)
    assert hashlib.md5(got).hexdigest() == manifest["cases"][name]["md5_libm"]
    assert got == want
    assert stdout == manifest["cases"][name]["stdout"]


def test_score_finalize_host_csv_bytes(manifest, tmp_path, monkeypatch, oracle):
    """--score-finalize=host on the GPU path: `pre` from the HIP kernel (bit-exact), 1/(1+np.exp(.)) by this
    host's numpy -> the md5 of the CSV the UNMODIFIED reference prints on a host with the same np.exp:
    md5_avx512 where numpy's AVX-512 exp is dispatched, md5_libm elsewhere (VERDICT r01 missing #3)."""
    x = np.random.default_rng(5).uniform(-9.3, 17.3, 200000)
    flavour = "libm" if (np.exp(x).view(np.uint64) == oracle.exp(x).view(np.uint64)).all() else "avx512"
    got, _ = run_cli(tmp_path, monkeypatch, golden_fasta_path("sample", tmp_path), None, manifest["seed"],
                     extra=("--score-finalize", "host"))
    assert hashlib.md5(got).hexdigest() == manifest["cases"]["sample"]["md5_" + flavour], flavour
    for name in ("tiny", "multi"):  # chunk-tail rows are re-scored from `pre` too
        d = tmp_path / name
        d.mkdir()
        got, _ = run_cli(d, monkeypatch, golden_fasta_path(name, tmp_path), None, manifest["seed"],
                         extra=("--score-finalize", "host"))
        if flavour == "libm":
            assert got == read_golden_csv(name)
        else:
            assert len(got) > 0 and got.count(b"\r\n") == read_golden_csv(name).count(b"\r\n")


@pytest.mark.parametrize("name,guide_len", LENGTH_CASES)
def test_cli_csv_bytes_equal_reference_other_guide_lengths(name, guide_len, manifest, tmp_path, monkeypatch):
    """The same with -l 17 ... 25 (generic-length kernels): bytes of the real reference's CSV."""
    from cropsr_amd.cli import EngineBackend
    be = EngineBackend(0)
    got, stdout = run_cli(tmp_path, monkeypatch, golden_fasta_path(name, tmp_path), be, manifest["seed"],
                          extra=("-l", str(guide_len)))
    be.close()
    case = manifest["cases"]["%s.l%d" % (name, guide_len)]
    assert got == read_golden_csv(name, guide_len)
    assert hashlib.md5(got).hexdigest() == case["md5_libm"] and stdout == case["stdout"]


@pytest.mark.parametrize("name", VERBOSE_CASES)
def test_cli_verbose_output_equals_reference(name, manifest, tmp_path, monkeypatch):
    """-v on the GPU path: the reference's banner, progress lines and pre-filter site counts."""
    from cropsr_amd.cli import EngineBackend
    be = EngineBackend(0)
    got, stdout = run_cli(tmp_path, monkeypatch, golden_fasta_path(name, tmp_path), be, manifest["seed"], extra=("-v",))
    be.close()
    assert got == read_golden_csv(name)
    assert normalize_verbose(stdout) == normalize_verbose(manifest["cases"][name + ".verbose"]["stdout"])


def test_sample_vs_committed_reference_output(engine, sample_fasta_text):
    """The reference's own sample_data/output.csv: positions/strings exact, score <= 15 ulp."""
    import gzip
    from cropsr_amd import fasta, rows
    table = fasta.contig_table(sample_fasta_text)
    (name, s), = table.items()
    arena = engine.arena([s])
    block = rows.ContigRows(name, s, arena.scan_score(20).contig(0), 20)
    arena.close()
    with gzip.open(os.path.join(GOLDEN, "sample_output_committed.csv.gz"), "rt", newline="") as f:
        committed = f.read().split("\r\n")[1:-1]
    assert block.n == len(committed) == 17314
    worst = 0
    for k, line in enumerate(committed):
        f = line.split(",")
        # id, cas9, sequence, long, "('Chr01'", ",", start, end, cutsite, strand, score, features, status
        assert f[2] == block.short[k] and f[3] == block.long[k]
        assert int(f[6]) == block.start[k] and int(f[7]) == block.end[k]
        worst = max(worst, abs(int(np.float64(f[10]).view(np.int64)) - int(np.float64(block.score[k]).view(np.int64))))
    assert worst <= 15  # ulp


ALPHABETS = {
    "acgt": b"ACGT",
    "softmask": b"ACGTACGTACGTacgtN",
    "exotic": b"ACGTacgtNUZuzRYKM')],-",
    "gc_rich": b"GGCC",
}


@pytest.mark.parametrize("alpha", sorted(ALPHABETS))
@pytest.mark.parametrize("pack", ["device", "host"])
def test_random_contigs_vs_oracle(engine, oracle, alpha, pack):
    rng = np.random.default_rng(sum(ALPHABETS[alpha]))
    a = np.frombuffer(ALPHABETS[alpha], dtype=np.uint8)
    lens = [0, 1, 2, 3, 22, 29, 30, 31, 63, 64, 65, 127, 128, 129, 1000, 16383, 16384, 16385, 16447,
            32768, 65535, 65536, 65537, 70001, 131073]
    contigs = [rng.choice(a, n).tobytes() for n in lens]
    assert check_contigs(engine, oracle, contigs, 20, pack) > 500


def test_decorated_contig_edges_vs_oracle(engine, oracle):
    """Contig strings as the reference builds them: quote/paren decoration at both ends,
    PAMs hard against the ends, truncated '-' windows (score -1)."""
    rng = np.random.default_rng(2)
    contigs = []
    for k in range(40):
        n = int(rng.integers(20, 200))
        body = rng.choice(np.frombuffer(b"ACGGCC", dtype=np.uint8), n).tobytes()
        contigs.append(b"'" + body + (b"')," if k % 2 else b"')]"))
    contigs.append(b"'" + b"G" * 300 + b"'),")
    contigs.append(b"'" + b"C" * 300 + b"')]")
    check_contigs(engine, oracle, contigs)
    # at least one truncated window must have been exercised
    arena = engine.arena(contigs)
    h = arena.scan_score(20)
    assert (h.score_minus == -1.0).any() and not (h.score_plus == -1.0).any()
    arena.close()


def test_every_position_a_hit_multi_round(engine, oracle):
    """poly-G / poly-C: every position is a hit, so one tile overflows the LDS hit
    list several times (the multi-round path of the emit kernel)."""
    contigs = [b"G" * 40000, b"C" * 40000, b"GC" * 20000, (b"G" * 100 + b"C" * 100) * 300]
    n = check_contigs(engine, oracle, contigs)
    assert n > 100000


@pytest.mark.parametrize("l", [0, 1, 2, 7, 8, 9, 19, 21, 30, 35, 36, 50])
def test_guide_lengths_vs_oracle(engine, oracle, l):
    """-l != 20: the keep-filter moves and long_sequence is l+10 characters, so rows
    are unscored (-1, CROPSR.py:466-468) -- except, for l > 20, a window that the end
    of the string cuts to exactly 30 characters, which the reference does score."""
    rng = np.random.default_rng(l)
    a = np.frombuffer(b"ACGTacgtNGGCC", dtype=np.uint8)
    contigs = [rng.choice(a, n).tobytes() for n in (5, 40, 64, 100, 129, 5000)]
    contigs += [b"'" + rng.choice(a, 77).tobytes() + b"'),"]
    # contigs whose last CC sits exactly 28 before the end: cut-to-30 windows for l > 20
    contigs += [rng.choice(a, 60).tobytes() + b"ACCA" + rng.choice(a, 25).tobytes() for _ in range(8)]
    contigs += [rng.choice(a, 60).tobytes() + b"AGG" + tail for tail in (b"", b"A", b"AC", b"ACG")]
    check_contigs(engine, oracle, contigs, l)
    arena = engine.arena(contigs)
    h = arena.scan_score(l)
    if l < 20:
        assert (h.score_plus == -1.0).all() and (h.score_minus == -1.0).all()
    if l == 21:
        assert (h.score_minus != -1.0).any()
    arena.close()


def test_unsupported_and_misordered_calls(engine):
    from cropsr_amd import CropsrHipError
    from cropsr_amd import _native as nat
    arena = engine.arena([b"ACGTGGCCACGT" * 10])
    for l in (51, -1, -3):  # (0 is the bare PAM filter the host uses for -l <= 0; cli.device_guide_length)
        with pytest.raises(CropsrHipError) as e:
            arena.scan_score(l)
        assert e.value.status == -7  # CRP_ERR_UNSUPPORTED
    with pytest.raises(CropsrHipError) as e:
        arena.fetch(1, 1)  # nothing scanned yet (a refused scan leaves no tables)
    assert e.value.status == -5  # CRP_ERR_STATE
    arena.close()
    L = nat.lib()
    h = ctypes.c_void_p()
    assert L.crp_arena_create(engine._ctx, 4, ctypes.byref(h)) == 0
    buf = (ctypes.c_uint8 * 1000)()
    assert L.crp_arena_add_contig_ascii(h, buf, 1000, None) == -6  # CRP_ERR_CAPACITY
    assert L.crp_scan_score(h, 20, 0, None, None) == -5            # not sealed
    assert L.crp_arena_destroy(h) == 0
    with pytest.raises(CropsrHipError):
        engine.score_30mers(np.zeros((2, 30), dtype=np.uint8), order=3)


def test_deterministic_and_repeatable(engine):
    rng = np.random.default_rng(12)
    contigs = [rng.choice(np.frombuffer(b"ACGTacgtN", dtype=np.uint8), 300000).tobytes() for _ in range(3)]
    arena = engine.arena(contigs)
    a = arena.scan_score(20, want_pre=True)
    b = arena.scan_score(20, want_pre=True)
    for name in ("pos_plus", "pre_plus", "score_plus", "pos_minus", "pre_minus", "score_minus"):
        assert (bits(getattr(a, name)) == bits(getattr(b, name))).all()
    arena.close()


def test_fetch_into_reused_arrays(engine, oracle):
    """Arena.fetch(out=...) fills the arrays of a previous fetch again (a caller that keeps its host buffers does not pay
    the first touch of fresh pages): same values, same storage where it is large enough, fresh arrays where it is not."""
    rng = np.random.default_rng(8)
    a = np.frombuffer(b"ACGTacgtNGGCC", dtype=np.uint8)
    big, small = rng.choice(a, 60000).tobytes(), rng.choice(a, 9000).tobytes()
    ar_big, ar_small = engine.arena([big]), engine.arena([small])
    nb, ns = ar_big.scan_score_device(20, want_pre=True), ar_small.scan_score_device(20, want_pre=True)
    first = ar_big.fetch(*nb, want_pre=True)
    keep = [c.copy() for c in first]
    again = ar_small.fetch(*ns, want_pre=True, out=first)          # smaller tables: views of the same storage
    assert all(np.shares_memory(x, y) for x, y in zip(again, first))
    want = oracle.scan_score(small, 20)
    off = int(ar_small.offsets[0])
    assert (again[0] - off == want["pos_plus"]).all() and (bits(again[2]) == bits(want["score_plus"])).all()
    assert (again[3] - off == want["pos_minus"]).all() and (bits(again[4]) == bits(want["pre_minus"])).all()
    back = ar_big.fetch(*nb, want_pre=True, out=again)              # larger tables than the views: fresh arrays
    assert all((bits(x) == bits(y)).all() for x, y in zip(back, keep))
    no_pre = ar_big.fetch(*nb, out=back)
    assert no_pre[1] is None and no_pre[4] is None and np.shares_memory(no_pre[0], back[0])
    ar_big.close()
    ar_small.close()


def test_single_pass_equals_two_pass(engine):
    """crp_scan_score's one-kernel mode (chained scan across workgroups) and the
    count / scan / emit sequence must produce identical tables; poly-G forces the
    'tables too small, repeat with exact sizes' path of the one-kernel mode."""
    rng = np.random.default_rng(77)
    contigs = [rng.choice(np.frombuffer(b"ACGTacgtNGGCC", dtype=np.uint8), n).tobytes()
               for n in (1, 70000, 16384 * 3, 500000, 123)]
    contigs.append(b"G" * 200000)
    results = []
    for two_pass in (False, True, False):
        engine.configure(two_pass=two_pass)
        arena = engine.arena(contigs)
        results.append(arena.scan_score(20, want_pre=True))
        again = arena.scan_score(20, want_pre=True)  # second scan: sizes now known
        for name in ("pos_plus", "pre_plus", "score_plus", "pos_minus", "pre_minus", "score_minus"):
            assert (bits(getattr(results[-1], name)) == bits(getattr(again, name))).all()
        arena.close()
    engine.configure(two_pass=False)  # the default
    for name in ("pos_plus", "pre_plus", "score_plus", "pos_minus", "pre_minus", "score_minus"):
        assert (bits(getattr(results[0], name)) == bits(getattr(results[1], name))).all(), name
        assert (bits(getattr(results[0], name)) == bits(getattr(results[2], name))).all(), name
    assert results[0].n_plus > 200000


def test_medium_genome_vs_oracle(engine, oracle):
    """A 6 Mb multi-contig arena with soft-masked runs and N runs, compared hit by
    hit (positions, pre, score) with the oracle."""
    rng = np.random.default_rng(33)
    contigs = []
    for n in (3000000, 2000000, 700000, 250000, 50000, 999):
        a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)]
        # soft-mask runs and N runs
        for _ in range(n // 20000 + 1):
            st = int(rng.integers(0, n))
            ln = int(rng.geometric(1 / 2000.0))
            a[st:st + ln] |= 0x20
        for _ in range(n // 200000 + 1):
            st = int(rng.integers(0, n))
            a[st:st + int(rng.integers(100, 5000))] = ord("N")
        contigs.append(b"'" + a.tobytes() + b"'),")
    n = check_contigs(engine, oracle, contigs)
    assert n > 500000


def test_big_chunk_csv_md5(manifest, tmp_path, monkeypatch):
    """> 1 000 000 hits on one contig: the reference's broken final chunk and
    backwards ids, compared by md5 with a real reference run (fixture: checksum)."""
    from cropsr_amd.cli import EngineBackend
    r = np.random.default_rng(12345)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[r.integers(0, 4, 9000000)].tobytes().decode()
    fa = tmp_path / "big.fa"
    with open(fa, "w") as f:
        f.write(">chrBig\n")
        f.write("\n".join(seq[i:i + 80] for i in range(0, len(seq), 80)))
        f.write("\n")
    be = EngineBackend(0)
    got, _ = run_cli(tmp_path, monkeypatch, str(fa), be, manifest["seed"])
    be.close()
    assert got.count(b"\r\n") - 1 == manifest["cases"]["big9m"]["rows"] == 1124618
    assert hashlib.md5(got).hexdigest() == manifest["cases"]["big9m"]["md5_libm"]


# --------------------------------------------- BASELINE-size property tests
def _complement_reverse(a):
    lut = np.arange(256, dtype=np.uint8)
    for x, y in (b"AT", b"TA", b"CG", b"GC"):
        lut[x] = y
    return lut[a][::-1]


def test_full_size_properties(engine):
    """The bench workload's size (>= 1 Gb, BASELINE.json north_star) through
    properties that need no oracle pass:
      * counts equal a vectorised numpy count of the same predicate,
      * positions are strictly ascending per strand,
      * reverse-complement symmetry: the '+' hits of S are the '-' hits of rc(S)
        at mirrored positions WITH BIT-IDENTICAL scores (and vice versa).
    """
    total = int(float(os.environ.get("CROPSR_TEST_BIG_BASES", "1.13e9")))
    rng = np.random.default_rng(5)
    n_contigs = 16
    per = total // n_contigs
    G, C = ord("G"), ord("C")
    fw, rc = [], []
    want_plus = want_minus = 0
    for k in range(n_contigs):
        a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, per, dtype=np.uint8)]
        fw.append(a)
        rc.append(np.ascontiguousarray(_complement_reverse(a)))
        gg = (a[1:-1] == G) & (a[2:] == G)          # i in [0, n-3]
        want_plus += int(gg[25:].sum())               # keep i - 20 >= 5
        cc = (a[:-2] == C) & (a[1:-1] == C)          # j in [0, n-3]
        want_minus += int(cc[2:per - 12].sum())       # keep j >= 2 and j + 23 <= n + 10
    af = engine.arena(fw)
    ar = engine.arena(rc)
    hf = af.scan_score(20, want_pre=False)
    hr = ar.scan_score(20, want_pre=False)
    assert hf.n_plus == want_plus and hf.n_minus == want_minus
    assert (np.diff(hf.pos_plus.astype(np.int64)) > 0).all()
    assert (np.diff(hf.pos_minus.astype(np.int64)) > 0).all()
    for k in range(n_contigs):
        f, r = hf.contig(k), hr.contig(k)
        # '+' hit at i in S  <->  '-' hit at n-3-i in rc(S); compare where both windows are interior
        i = f["pos_plus"].astype(np.int64)
        keep = (i >= 25) & (i + 5 <= per) & (per - 3 - i >= 2) & (per - 3 - i + 28 <= per)
        j = (per - 3 - i[keep])[::-1]
        rj = r["pos_minus"].astype(np.int64)
        sel = (rj >= 2) & (rj + 28 <= per) & (per - 3 - rj >= 25) & (per - 3 - rj + 5 <= per)
        assert (rj[sel] == j).all()
        assert (bits(r["score_minus"][sel]) == bits(f["score_plus"][keep][::-1])).all()
        # unscored rows exist only where the string end cuts the window
        assert not (f["score_plus"][i + 5 <= per] == -1.0).any()
    af.close()
    ar.close()


@pytest.mark.parametrize("config", ["ecoli", "tair10", "sorghum", "switchgrass"])
def test_baseline_config_workloads_sampled_against_oracle(_engine, oracle, config):
    """The four genome configurations of BASELINE.json as seeded stand-ins (bench_workload.py: same
    size, contig structure, GC, soft-mask and N content), decorated as the reference decorates
    them, scanned whole on the GPU (as many arenas as needed) and then checked against the oracle:
    the whole genome for E. coli, and for the larger ones the first and last 200 kb of the big
    contigs, every small contig and 40 random 100 kb windows (interior hits only: a window is
    re-scanned by the oracle as if it were a contig, so hits within 64 positions of its cut ends
    are left out).  Positions and scores bit-exact; per-strand counts of the whole genome equal a
    numpy count of the PAM predicate."""
    import bench_workload as bw
    scale = float(os.environ.get("CROPSR_TEST_CONFIG_SCALE", "1.0"))
    wl = {"ecoli": bw.ecoli_like, "tair10": bw.tair10_like, "sorghum": bw.sorghum_like,
          "switchgrass": lambda: bw.switchgrass_like(scale=scale)}[config]()
    _engine.configure(two_pass=False)
    strings = [wl.contig_string(k) for k in range(len(wl.specs))]
    genome = _engine.genome(strings)
    hits = genome.scan_score(20, want_pre=False)
    G, C = ord("G"), ord("C")
    n_plus = n_minus = 0
    rng = np.random.default_rng(17)
    big = [k for k, s in enumerate(strings) if s.size > 2_000_000]
    windows = [(k, 0, s.size) for k, s in enumerate(strings) if s.size <= 300_000][:60]
    if config == "ecoli":
        windows = [(0, 0, strings[0].size)]
    else:
        for k in big:
            windows += [(k, 0, 200_000), (k, strings[k].size - 200_000, strings[k].size)]
        for _ in range(40):
            k = big[int(rng.integers(0, len(big)))]
            a = int(rng.integers(0, strings[k].size - 100_000))
            windows.append((k, a, a + 100_000))
    per_contig = {}
    for k, s in enumerate(strings):
        # the reference's predicate on the decorated string (upper-case G / C only, CROPSR.py:98-104,419,430)
        gg = (s[1:-1] == G) & (s[2:] == G)
        cc = (s[:-2] == C) & (s[1:-1] == C)
        i = np.nonzero(gg)[0]
        j = np.nonzero(cc)[0]
        n_plus += int((i - 20 >= 5).sum())
        n_minus += int(((j >= 2) & (j + 23 <= s.size + 10) & (j + 2 < s.size)).sum())
    assert (hits.n_plus, hits.n_minus) == (n_plus, n_minus)
    checked = 0
    for k, a, b in windows:
        if k not in per_contig:
            per_contig[k] = hits.contig(k)
        got = per_contig[k]
        s = strings[k]
        want = oracle.scan_score(s[a:b].tobytes(), 20)
        lo = a if a == 0 else a + 64
        hi = b if b == s.size else b - 64
        for strand in ("plus", "minus"):
            gp = got["pos_" + strand].astype(np.int64)
            gsel = (gp >= lo) & (gp < hi)
            wp = want["pos_" + strand].astype(np.int64) + a
            wsel = (wp >= lo) & (wp < hi)
            assert (gp[gsel] == wp[wsel]).all(), (config, k, a, strand)
            assert (bits(got["score_" + strand][gsel]) == bits(want["score_" + strand][wsel])).all(), (config, k, a, strand)
            checked += int(gsel.sum())
    assert checked > {"ecoli": 400_000, "tair10": 300_000, "sorghum": 400_000, "switchgrass": 400_000 * scale}[config]
    genome.close()


def _table_digest(h):
    d = hashlib.sha256()
    for key in ("pos_plus", "score_plus", "pos_minus", "score_minus"):
        d.update(np.ascontiguousarray(h[key]).tobytes())
    return d.hexdigest()


@pytest.mark.slow
@pytest.mark.parametrize("config,geometry", [("tair10", "auto"), ("tair10", "small"), ("sorghum", "auto"), ("switchgrass", "auto")])
def test_baseline_config_workloads_whole_genome_digest(_engine, oracle, config, geometry):
    """Configs 3, 4 and 5 of BASELINE.json WHOLE: the oracle is streamed over every
    contig on the host's cores (it is the checker; ctypes releases the GIL) while the contigs are uploaded,
    and the SHA-256 of (positions, scores) per strand of every contig must equal the digest of the GPU's
    tables for that contig -- every one of the 7.7 M / 33 M / 52 M hits, bit for bit
    (CROPSR.py:413-434, :458-461)."""
    from concurrent.futures import ThreadPoolExecutor
    import bench_workload as bw
    wl = {"tair10": bw.tair10_like, "sorghum": bw.sorghum_like, "switchgrass": bw.switchgrass_like}[config]()
    _engine.configure(two_pass=False, geometry=geometry)  # (auto: LARGE for all three; SMALL forced once)
    threads = max(2, min(16, len(os.sched_getaffinity(0))))
    builder = _engine.arena_builder([s.length + 4 for s in wl.specs])
    want = []
    with ThreadPoolExecutor(threads) as pool:
        for k in range(len(wl.specs)):
            s = wl.contig_string(k)
            builder.add(s)
            want.append(pool.submit(lambda t=s: _table_digest(oracle.scan_score(t, 20))))
            del s
            while sum(not f.done() for f in want) > threads + 2:  # bound the strings kept alive
                [f for f in want if not f.done()][0].result()
        arena = builder.seal()
        _engine.configure(geometry="auto")
        tiles = arena.tiles()
        assert tiles["geometry"] == (geometry if geometry != "auto" else "large")
        hits = arena.scan_score(20, want_pre=False)
        want = [f.result() for f in want]
    got = [_table_digest(hits.contig(k)) for k in range(len(wl.specs))]
    n_hits = hits.n_plus + hits.n_minus
    arena.close()
    bad = [k for k in range(len(want)) if want[k] != got[k]]
    assert not bad, (config, "contigs whose tables differ from the oracle's", bad[:10])
    assert n_hits > {"tair10": 7_000_000, "sorghum": 25_000_000, "switchgrass": 50_000_000}[config]
    print("whole-genome digest %s (%s tiles x %d): %d contigs, %d hits, sha256 of digests %s"
          % (config, tiles["geometry"], tiles["n_tiles"], len(want), n_hits, hashlib.sha256("".join(got).encode()).hexdigest()))


def test_many_small_contigs_between_large_ones(engine, oracle):
    """crp_arena_add_contigs_ascii: thousands of small contigs (empty ones, lengths around the 64-word group and the
    16-byte alignment of the batch buffer) share copies and pack launches, large ones (>= 8 MiB) stream through the
    single-contig path in between; the order, the arena offsets and every hit table are what one contig at a time gives
    -- checked against the oracle contig by contig, through Engine.arena and through the buffering ArenaBuilder."""
    rng = np.random.default_rng(4242)
    a = np.frombuffer(b"ACGTacgtNGGCC", dtype=np.uint8)
    sizes = [0, 1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 70000] + rng.integers(0, 9000, 2500).tolist()
    contigs = [rng.choice(a, int(n)).tobytes() for n in sizes]
    big = np.frombuffer(b"'", dtype=np.uint8).tolist() + rng.choice(a, (9 << 20) + 123).tolist()
    big = bytes(big) + b"'),"
    contigs = contigs[:700] + [big] + contigs[700:1500] + [big[: 8 << 20]] + contigs[1500:]
    want_big = oracle.scan_score(big, 20)
    for how in ("arena", "builder"):
        if how == "arena":
            arena = engine.arena(contigs)
        else:
            b = engine.arena_builder([len(c) for c in contigs])
            for c in contigs:
                b.add(c)
            arena = b.seal()
        assert arena.stats()["n_contigs"] == len(contigs)
        assert (np.diff(arena.offsets.astype(np.int64)) > 0).all() and (arena.offsets % 64 == 0).all()
        hits = arena.scan_score(20, want_pre=True)
        for k in list(range(0, len(contigs), 37)) + [700, 1501]:
            want = want_big if k == 700 else oracle.scan_score(contigs[k], 20)
            assert_hits_equal(hits.contig(k), want, ctx=(how, k))
        total = sum(oracle.scan(c, 20)[0].size + oracle.scan(c, 20)[1].size for c in contigs)
        assert hits.n_plus + hits.n_minus == total
        arena.close()


def test_empty_and_degenerate_arenas(engine, oracle):
    """No contig at all, only empty contigs, contigs shorter than any window, a contig of
    characters that are no bases: the oracle's (mostly empty) tables, no error, in both scan modes."""
    for contigs in ([], [b""], [b"", b"", b""], [b"A"], [b"GG"], [b"CC"], [b"'),"], [b"N" * 5000],
                    [b"", b"ACGTTGCA" * 3, b""]):
        arena = engine.arena(contigs)
        hits = arena.scan_score(20, want_pre=True)
        want = [oracle.scan_score(c, 20) for c in contigs]
        assert hits.n_plus == sum(w["pos_plus"].size for w in want)
        assert hits.n_minus == sum(w["pos_minus"].size for w in want)
        for k, w in enumerate(want):
            assert_hits_equal(hits.contig(k), w, ctx=(contigs, k))
        assert arena.stats()["n_contigs"] == len(contigs)
        arena.close()


def test_largest_arena(_engine, oracle):
    """One contig that fills the largest arena the library accepts (just under 2^31 characters:
    positions are 32-bit, the chained-scan descriptors carry 31-bit counts).  The contig is one
    4 KiB block repeated, so every interior repeat must carry the first repeat's hits shifted by
    a multiple of the period, with bit-identical scores; the two ends are compared with the
    oracle; one character more is refused."""
    from cropsr_amd import _native as nat
    from cropsr_amd import CropsrHipError
    _engine.configure(two_pass=False)
    max_chars = int(nat.lib().crp_arena_max_words()) * 64 - 192  # room for the separators around the contig
    period = 4096
    rng = np.random.default_rng(2)
    block = rng.choice(np.frombuffer(b"ACGTACGTACGTacgtN", dtype=np.uint8), period)
    n_rep = max_chars // period
    text = np.tile(block, n_rep)
    assert text.size > 2**31 - 300000
    arena = _engine.arena([text])
    hits = arena.scan_score(20, want_pre=False)
    del text
    ref = oracle.scan_score(np.tile(block, 4).tobytes(), 20)  # repeats 1 and 2 of these 4 are "interior"
    for strand in ("plus", "minus"):
        pos = hits.contig(0)["pos_" + strand].astype(np.int64)
        sc = hits.contig(0)["score_" + strand]
        rp = ref["pos_" + strand].astype(np.int64)
        interior = (rp >= period) & (rp < 2 * period)
        want_pos, want_sc = rp[interior] - period, ref["score_" + strand][interior]
        per = want_pos.size
        assert per > 100
        for k in (1, 2, n_rep // 2, n_rep - 3, n_rep - 2):  # repeat k of the big contig
            a, b = np.searchsorted(pos, [k * period, (k + 1) * period])
            assert b - a == per and (pos[a:b] - k * period == want_pos).all(), (strand, k)
            assert (bits(sc[a:b]) == bits(want_sc)).all(), (strand, k)
        first = rp < period  # the contig's own left end
        a = np.searchsorted(pos, period)
        assert (pos[:a] == rp[first]).all() and (bits(sc[:a]) == bits(ref["score_" + strand][first])).all()
        assert abs(pos.size - per * n_rep) <= 2 * per and (np.diff(pos) > 0).all() and pos[-1] < 2**31
    arena.close()
    with pytest.raises((CropsrHipError, ValueError)):
        _engine.arena([np.zeros(max_chars + 4096, dtype=np.uint8)])


def test_several_arenas_and_contexts_interleaved(engine, oracle):
    """Arenas of one context scanned alternately (each owns its descriptor buffers and tables), a
    second context on the same device in between, different guide lengths on one arena: no scan
    disturbs another's result."""
    from cropsr_amd import Engine
    rng = np.random.default_rng(91)
    a = np.frombuffer(b"ACGTacgtNGGCC", dtype=np.uint8)
    sets = [[rng.choice(a, n).tobytes() for n in ns] for ns in ((70000, 300), (150000,), (9, 40000, 40000))]
    arenas = [engine.arena(cs) for cs in sets]
    other = Engine(0)
    other_arena = other.arena(sets[1])
    want = {(i, l): [oracle.scan_score(c, l) for c in cs] for i, cs in enumerate(sets) for l in (20, 23)}
    for l in (20, 23, 20):
        got = [ar.scan_score_device(l, want_pre=True) for ar in arenas]   # all launched before any table is read
        o = other_arena.scan_score(l, want_pre=True)
        for i, (ar, (n_plus, n_minus)) in enumerate(zip(arenas, got)):
            from cropsr_amd.engine import Hits
            hits = Hits(ar.offsets, ar.lengths, l, ar.fetch(n_plus, n_minus, want_pre=True))
            for k in range(len(sets[i])):
                assert_hits_equal(hits.contig(k), want[(i, l)][k], ctx=(i, l, k))
        assert_hits_equal(o.contig(0), want[(1, l)][0], ctx=("other", l))
    other_arena.close()
    other.close()
    for ar in arenas:
        ar.close()


def test_genome_spread_over_several_arenas(engine, oracle):
    """Inputs beyond one arena (2^31 characters) are split contig by contig; forced here
    with a tiny per-arena limit.  Results must not depend on the split."""
    rng = np.random.default_rng(55)
    a = np.frombuffer(b"ACGTacgtNGGCC", dtype=np.uint8)
    contigs = [rng.choice(a, n).tobytes() for n in (3000, 10, 0, 7000, 6400, 64, 129, 5000)]
    one = engine.genome(contigs)
    many = engine.genome(contigs, max_words=120)  # 120 words = 7680 characters per arena
    assert len(one.arenas) == 1 and len(many.arenas) >= 4
    h1, hm = one.scan_score(20, want_pre=True), many.scan_score(20, want_pre=True)
    assert (h1.n_plus, h1.n_minus) == (hm.n_plus, hm.n_minus)
    for k, c in enumerate(contigs):
        want = oracle.scan_score(c, 20)
        assert_hits_equal(h1.contig(k), want, ctx=("one", k))
        assert_hits_equal(hm.contig(k), want, ctx=("many", k))
    with pytest.raises(ValueError):
        engine.genome([b"A" * 10000], max_words=100)
    one.close()
    many.close()


# ------------------------------------------------------- multi-GPU plumbing
def test_cut_contig_on_gpu_equals_whole(engine, oracle):
    """parallel.cut_contigs: the pieces of one long contig (what several ranks would each scan,
    halo included) through the GPU engine and stitched == the contig scanned whole == the oracle."""
    from cropsr_amd import parallel
    rng = np.random.default_rng(64)
    c = b"'" + rng.choice(np.frombuffer(b"ACGTacgtNGGCC", dtype=np.uint8), 700000).tobytes() + b"')]"
    pieces = parallel.cut_contigs([len(c)], 8)
    assert len(pieces) == 8
    views = [parallel.piece_view(c, s, e) for _, s, e in pieces]
    arena = engine.arena([v for v, _ in views])
    hits = arena.scan_score(20, want_pre=True)
    got = parallel.stitch_pieces([(s, e, shift, hits.contig(q)) for q, ((_, s, e), (_, shift)) in enumerate(zip(pieces, views))])
    arena.close()
    assert_hits_equal(got, oracle.scan_score(c, 20), ctx="stitched")


def test_device_tables_and_scored_count(engine, oracle):
    """crp_hits_device hands out the addresses of the tables in HBM (for a device-side consumer) and
    crp_count_scored counts, on the GPU, the rows that carry a real score."""
    rng = np.random.default_rng(8)
    c = b"'" + rng.choice(np.frombuffer(b"ACGTacgtNGG", dtype=np.uint8), 200000).tobytes() + b"')]"
    arena = engine.arena([c])
    n_plus, n_minus = arena.scan_score_device(20)
    ptrs = arena.device_tables()
    assert len(ptrs) == 4 and all(p for p in ptrs)
    want = oracle.scan_score(c, 20)
    assert arena.count_scored() == int((want["score_plus"] != -1).sum() + (want["score_minus"] != -1).sum())
    arena.close()


def _rccl_world1(out_path, port):
    """One rank, the real transport: RCCL through the C ABI (crp_comm_init, crp_gather_hits,
    crp_comm_allreduce_f64, crp_offtarget_reduce)."""
    import sys
    from conftest import ROOT
    sys.path.insert(0, ROOT)
    from cropsr_amd import Engine, rendezvous
    group = rendezvous.Group(0, 1)
    eng = Engine(0)
    eng.comm_init(group)
    ok = eng.query()["comm_world"] == 1
    arena = eng.arena([b"ACGGTCCAGGTTCCAAGG" * 500, b"'" + b"GGACCTTGGCCAATTGGCCA" * 300 + b"')]"])
    n_plus, n_minus = arena.scan_score_device(20)
    eng.offtarget_reset()
    arena.offtarget_add(20)
    eng.offtarget_reduce()
    eng.offtarget_solve()
    ot = arena.offtarget_counts(n_plus, n_minus)
    # the annotation join's ids travel as one more column (CRP_GATHER_FEATURES); without a look-up the flag is a
    # state error every rank agrees on, and the communicator stays usable
    try:
        eng.gather_hits(arena, 0, features=True)
        ok = False
    except Exception as e:
        ok = ok and getattr(e, "status", 0) == -5
    arena.annotate_set_track(np.array([int(arena.offsets[0]), int(arena.offsets[0]) + 700, int(arena.offsets[1])], np.uint32),
                             np.array([7, 0xFFFFFFFF, 9], np.uint32))
    feat = arena.annotate_lookup(n_plus, n_minus)
    for _ in range(2):
        counts = eng.gather_hits(arena, 0, offtarget=True, features=True)
        got = eng.gathered_fetch(0, counts, offtarget=True, features=True)
    ok = ok and (got["feat_plus"] == feat[0]).all() and (got["feat_minus"] == feat[1]).all()
    ok = ok and set(np.unique(feat[0]).tolist()) == {7, 9, 0xFFFFFFFF}
    cols = arena.fetch(n_plus, n_minus)
    ok = ok and counts.tolist() == [[n_plus, n_minus]]
    ok = ok and (got["pos_plus"] == cols[0]).all() and (got["pos_minus"] == cols[3]).all()
    ok = ok and (got["score_plus"].view(np.uint64) == cols[2].view(np.uint64)).all()
    ok = ok and (got["ot_plus"] == ot[0]).all() and (got["ot_minus"] == ot[1]).all()
    ok = ok and eng.comm_allreduce([1.5, 2.0], "sum") == [1.5, 2.0] and eng.comm_allreduce([3.0], "max") == [3.0]
    eng.comm_barrier()
    ok = ok and eng.gather_hits(None, 0).tolist() == [[0, 0]]  # a rank with nothing to contribute
    arena.close()
    # bench.py's strong-scaling block on the REAL transport (fences and sums on RCCL, crp_gather_hits + crp_gathered_fetch),
    # as far as one GPU allows: a "world" of one rank that owns the whole plan -- stitched tables against the N = 1 scan
    import argparse
    import bench
    from cropsr_amd import _native as nat
    args = argparse.Namespace(workload="switchgrass", scale=0.01, steps=2, warmup=1, preheat_ms=0.0, strong_steps=0,
                              no_strong_check=False, fasta=None, no_node_block=True)

    def fence():
        nat.check(nat.lib().crp_synchronize(eng._ctx), "crp_synchronize", eng._ctx)
        eng.comm_barrier()
    st = bench.strong_scaling_block(args, eng, group, True, fence, eng.comm_allreduce)
    ok = ok and st["digest_ok"] is True and st["gatherv_transport"].startswith("RCCL") and st["kept_hits"] == st["n1"]["kept_hits"]
    ok = ok and st["ms_gatherv"] > 0 and len(st["per_rank"]) == 1 and st["bytes_to_root"] == 0
    eng.close()
    with open(out_path, "w") as f:
        f.write("ok" if ok else "bad")


def test_gather_runs_on_rccl_in_library(tmp_path):
    """The N > 1 code path on the real transport, as far as one GPU allows: a communicator of one
    rank, in a child process (librccl.so is dlopen()ed by the library on the first crp_comm_* call)."""
    import multiprocessing as mp
    out = str(tmp_path / "r.txt")
    p = mp.get_context("spawn").Process(target=_rccl_world1, args=(out, 29533))
    p.start()
    p.join(600)
    assert p.exitcode == 0
    assert open(out).read() == "ok"


@pytest.mark.parametrize("extra", [(), ("--offtarget",)])
def test_cli_multi_process_on_gpu(manifest, tmp_path, extra):
    """`python -m torch.distributed.run --nproc-per-node 2 -m cropsr_amd ...`: two processes, contigs
    cut into 100-character pieces and dealt to them, HIP tables gathered to rank 0, which writes the
    reference's bytes.  One GPU here, so both ranks use device 0 and the exchange runs over the control
    sockets (CROPSR_GATHER=host; RCCL cannot put two ranks on one GPU); on a multi-GPU node the same
    command without that variable moves the tables over RCCL.  With --offtarget the two ranks' site
    histograms are summed and the output equals the one-process run."""
    import subprocess
    import sys
    from conftest import ROOT
    out_csv = tmp_path / "out.csv"
    env = dict(os.environ, CROPSR_GATHER="host", CROPSR_DIST_MAX_PIECE="100", PYTHONPATH=ROOT)
    common = ["-f", os.path.join(GOLDEN, "probe_mixed.fa"), "-g", os.path.join(GOLDEN, "sample_head.gff"), "--cas9",
              "--seed", str(manifest["seed"]), "--device", "0"] + list(extra)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29541", "-m", "cropsr_amd", "-o", str(out_csv)] + common
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path), env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    assert manifest["cases"]["mixed"]["stdout"] in p.stdout
    if not extra:
        assert out_csv.read_bytes() == read_golden_csv("mixed")
    else:
        one = tmp_path / "one.csv"
        q = subprocess.run([sys.executable, "-m", "cropsr_amd", "-o", str(one)] + common, capture_output=True, text=True,
                           timeout=600, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT))
        assert q.returncode == 0, q.stderr[-2000:]
        assert out_csv.read_bytes() == one.read_bytes()


def test_no_pytorch_in_the_product_process():
    """north_star: "no PyTorch" -- importing the package, opening the GPU and scanning pulls in no torch."""
    import subprocess
    import sys
    from conftest import ROOT
    code = ("import sys; sys.path.insert(0, %r); import cropsr_amd, cropsr_amd.cli, cropsr_amd.parallel, cropsr_amd.rendezvous;"
            "e = cropsr_amd.Engine(0); a = e.arena([b'ACGGTCCAGGTTCCAAGG' * 50]); a.scan_score(20); e.close();"
            "assert 'torch' not in sys.modules; print('clean')") % ROOT
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "clean" in p.stdout, p.stderr[-2000:]


def test_bench_line_contract():
    """bench.py prints ONE JSON line with the contract's keys (tiny workload)."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--scale", "0.01", "--steps", "2", "--warmup", "1",
                        "--cpu-sample-bases", "20000", "--full"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["vs_baseline"] is None and d["value"] > 0
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert "traffic_source" in r and d["config"]["chain_timeouts"] == 0 and d["config"]["launches_per_step"] == 1
    a = d["annotate"]  # the opt-in annotation join over the same resident tables (synthetic GFF)
    assert a["roofline"]["frac"] > 0 and a["hits_with_a_feature"] > 0 and a["gff"]["gene_rows"] > 0 and a["kernel_ms"] > 0
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 1 and c["value"] > 0 and "sample" in c
    assert c["all_cores"]["cores"] >= 1 and c["all_cores"]["value"] > 0
    assert "workload" in d["config"] and "model" not in d["config"]
    o = d["offtarget"]
    assert o["value"] > 0 and o["roofline"]["bound"] == "hbm" and o["sites_total"] > 0 and "error" not in o


def test_bench_plain_run_dumps_the_last_steps_tables(_engine, tmp_path):
    """A plain bench run (no --full) prints the headline line without the side blocks, and --dump-outputs writes the
    tables of its last timed step: bit for bit the tables of the same seeded genome scanned here through the same arena
    builder."""
    import argparse
    import json
    import subprocess
    import sys
    import bench
    from conftest import ROOT
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--scale", "0.01", "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"] == "gRNAs scored/sec" and d["unit"] == "gRNAs/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0 and d["roofline"]["kernel_ms"] > 0
    for key in ("cpu_baseline", "offtarget", "annotate", "pcie_inclusive"):
        assert key not in d, key
    assert "three_launch" not in d["roofline"]
    got = {f.stem: np.load(f) for f in out.glob("*.npy")}
    assert set(got) == {"counts", "pos_plus", "score_plus", "pos_minus", "score_minus"}
    assert all(a.dtype == np.float64 for a in got.values()) and sum(a.nbytes for a in got.values()) <= 64 << 20
    wl = bench.make_workload(argparse.Namespace(fasta=None, workload="switchgrass", scale=0.01), 0)
    _engine.configure(two_pass=False, geometry="auto")
    builder = _engine.arena_builder([wl.string_length(k) for k in range(len(wl.specs))])
    for k in range(len(wl.specs)):
        builder.add(wl.contig_string(k))
    arena = builder.seal()
    n_plus, n_minus = arena.scan_score_device(20, want_pre=False)
    cols = arena.fetch(n_plus, n_minus)
    assert got["counts"].tolist() == [n_plus, n_minus, arena.count_scored()] and d["config"]["kept_hits_total"] == n_plus + n_minus
    arena.close()
    assert max(n_plus, n_minus) <= bench.DUMP_ROWS  # (small enough to be dumped whole)
    assert (got["pos_plus"] == cols[0]).all() and (got["pos_minus"] == cols[3]).all()
    assert (got["score_plus"].view(np.uint64) == cols[2].view(np.uint64)).all()
    assert (got["score_minus"].view(np.uint64) == cols[5].view(np.uint64)).all()


@pytest.mark.parametrize("launcher", ["none", "torch.distributed.run"])
def test_bench_starts_its_own_ranks(launcher):
    """`python bench.py --gpus 2` with NO launcher in the environment (what the driver's N > 1 command looks
    like if it has the N = 1 command's shape): the parent starts two fresh ranks itself (cropsr_amd/launch.py),
    rank 0 prints the ONE line, the status is 0.  One GPU here, so --share-gpu0 puts both ranks on device 0 with the
    host transport for fences and the final gatherv.  Second case: the contract's own N > 1 command
    (`python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port P bench.py --gpus 2
    ...`): the launcher's environment is used as it is, nothing is spawned."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "CROPSR_LAUNCHED")}
    head = [sys.executable] if launcher == "none" else \
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29547"]
    p = subprocess.run(head + [os.path.join(ROOT, "bench.py"), "--gpus", "2", "--share-gpu0", "--scale", "0.02",
                               "--steps", "3", "--warmup", "1", "--offtarget-steps", "0", "--full"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["gatherv_ok"] is True and d["value"] > 0 and d["scaling"] == "weak"
    assert d["value_with_final_gatherv"] > 0 and d["value_with_final_gatherv"] < d["value"]
    ranks = d["per_rank"]
    assert [r["rank"] for r in ranks] == [0, 1] and all(r["kernel_ms"] > 0 and r["kept_hits"] > 0 for r in ranks)
    assert sum(r["kept_hits"] for r in ranks) == d["config"]["kept_hits_total"]
    # the strong-scaling block: ONE genome cut over the two ranks, scanned, gathered, stitched on rank 0
    # and compared, contig by contig, with rank 0's own N = 1 scan of the whole genome
    st = d["strong"]
    assert st["scaling"] == "strong" and st["genomes"] == 1 and st["digest_ok"] is True, st
    assert st["ms_scan_max_rank"] > 0 and st["ms_gatherv"] > 0 and st["value"] > 0 and st["value"] < st["value_scan_only"]
    assert st["contigs_cut"] >= 1 and [r["rank"] for r in st["per_rank"]] == [0, 1]
    assert st["kept_hits"] == st["n1"]["kept_hits"] and 0 < st["efficiency_vs_n1"] <= st["efficiency_vs_n1_scan_only"]
    assert abs(st["per_rank"][0]["bases"] - st["per_rank"][1]["bases"]) < 0.02 * st["per_rank"][0]["bases"]
    assert all(r["tiles"] > 0 and r["kernel_ms"] > 0 for r in st["per_rank"])
    # rank 0's closing block: a child process drives the same devices through the single-process node handle -- same genome,
    # digest-checked against its own N = 1 scan
    nb = d["single_process_node"]
    assert nb["digest_ok"] is True and nb["kept_hits"] == st["kept_hits"] and nb["gatherv_transport"] == "device-to-device copies", nb
    assert 0 < nb["bytes_to_root"] < nb["gatherv_raw_u32_positions"]["bytes_to_root"] and nb["devices"] == [0, 0]


def test_bench_four_ranks_on_the_one_gpu():
    """The first real multi-GPU run will start N HIP contexts, N arenas and N rendezvous clients with real skew; rehearsed
    here with FOUR self-launched ranks on the one GPU -- the GPU pool ends a job that keeps more than six processes on a
    card, the test runner itself holds the GPU, and one slot is left free (VERDICT r03 asked for eight; six ranks ran
    standalone, profiles/r04/; world 8 runs on the CPU in tests/test_distributed.py, and `--gpus 8` is the driver's to
    start).  One line, four per-rank entries, the host-transport gatherv and the strong-scaling block's digest check green,
    status 0."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "CROPSR_LAUNCHED")}
    # (--no-node-block: rank 0's closing block is one more process on the card -- four ranks, the child and this test runner
    # would be the six the pool allows; the two-rank test above runs it)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--share-gpu0", "--scale", "0.05",
                        "--steps", "3", "--warmup", "1", "--offtarget-steps", "0", "--no-node-block", "--full"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 4 and d["gatherv_ok"] is True and d["value"] > 0
    assert [r["rank"] for r in d["per_rank"]] == list(range(4))
    assert all(r["kernel_ms"] > 0 and r["kept_hits"] > 0 and r["rendezvous_s"] >= 0 and r["device_hbm_in_use_GiB"] > 0 for r in d["per_rank"])
    st = d["strong"]
    assert st["digest_ok"] is True and len(st["per_rank"]) == 4 and st["kept_hits"] == st["n1"]["kept_hits"], st
    shares = [r["bases"] for r in st["per_rank"]]
    assert max(shares) - min(shares) <= 6 * 4096 * 2
    assert "single_process_node" not in d
    print("four ranks on one GPU: rendezvous %.2f-%.2f s, device HBM in use %.2f GiB; strong: scan %.3f ms + gatherv %.1f ms"
          % (min(r["rendezvous_s"] for r in d["per_rank"]), max(r["rendezvous_s"] for r in d["per_rank"]),
             max(r["device_hbm_in_use_GiB"] for r in d["per_rank"]), st["ms_scan_max_rank"], st["ms_gatherv"]))


@pytest.mark.slow
def test_cli_four_ranks_tair10_like_offtarget_equals_one_process(tmp_path):
    """`python -m cropsr_amd --gpus 4 --offtarget` (no launcher) on the TAIR10-like FASTA, every chromosome cut into 5 Mb pieces
    (halos, stitching, owned ranges for the site histogram, histograms summed over the ranks), all four ranks on the one GPU
    over the host transport (four: the pool's limit of six processes per card, less the test runner, less one): the CSV has
    the md5 of the one-process run (1.1 GB, 7.7 M rows)."""
    import hashlib
    import subprocess
    import sys
    import time
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_workload as bw
    from e2e_cli import write_fasta
    fa, gff = str(tmp_path / "tair10_like.fa"), str(tmp_path / "empty.gff")
    write_fasta(bw.tair10_like(), fa)
    with open(gff, "w") as f:
        f.write("##gff-version 3\n")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "CROPSR_LAUNCHED")}
    env["PYTHONPATH"] = ROOT
    common = ["-f", fa, "-g", gff, "--cas9", "--seed", "1", "--each-contig-once", "--offtarget", "--device", "0"]

    def md5(path):
        h = hashlib.md5()
        with open(path, "rb") as f:
            for chunk in iter(lambda: f.read(1 << 24), b""):
                h.update(chunk)
        return h.hexdigest(), os.path.getsize(path)
    out = str(tmp_path / "out.csv")
    t0 = time.time()
    p = subprocess.run([sys.executable, "-m", "cropsr_amd", "-o", out] + common, capture_output=True, text=True, timeout=900,
                       cwd=str(tmp_path), env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    t_one = time.time() - t0
    want = md5(out)
    os.remove(out)
    t0 = time.time()
    q = subprocess.run([sys.executable, "-m", "cropsr_amd", "--gpus", "4", "-o", out] + common, capture_output=True, text=True,
                       timeout=900, cwd=str(tmp_path), env=dict(env, CROPSR_GATHER="host", CROPSR_DIST_MAX_PIECE="5000000"))
    assert q.returncode == 0, q.stderr[-2000:]
    t_four = time.time() - t0
    got = md5(out)
    os.remove(out)
    assert got == want and want[1] > 1_000_000_000
    print("TAIR10-like --offtarget: one process %.1f s, four ranks on one GPU (5 Mb pieces, host transport) %.1f s, md5 %s"
          % (t_one, t_four, want[0]))


def test_bench_prints_its_line_when_the_exchange_never_returns():
    """A final gatherv that hangs (here: rank 1 never reaches it, test hook CROPSR_BENCH_TEST_STALL) must not cost the
    run its scan measurement: after --collective-timeout rank 0 prints the ONE line with the timed steps' numbers and
    `gatherv_ok: false`, takes every rank down and the status is non-zero."""
    import json
    import subprocess
    import sys
    import time
    from conftest import ROOT
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "CROPSR_LAUNCHED")}
    env["CROPSR_BENCH_TEST_STALL"] = "1:gatherv"
    t0 = time.time()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--share-gpu0", "--scale", "0.02",
                        "--steps", "3", "--warmup", "1", "--offtarget-steps", "0", "--collective-timeout", "5", "--full"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert p.returncode != 0 and time.time() - t0 < 600
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, (p.stdout[-2000:], p.stderr[-2000:])
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["gatherv_ok"] is False and "did not return" in d["gatherv"]["error"]
    assert d["value"] > 0 and d["roofline"]["kernel_ms"] > 0 and len(d["per_rank"]) == 2
    assert "value_with_final_gatherv" not in d


def test_bench_goes_on_when_the_rccl_bootstrap_never_returns():
    """ncclCommInitRank has no time-out: a bootstrap that hangs (here: rank 1 never calls it, test hook
    CROPSR_TEST_COMM_INIT_STALL, so rank 0 waits for a peer that does not come) must not take the measurement with it.
    After CROPSR_COMM_INIT_TIMEOUT_S every rank agrees on the error, the bench goes on over the host transport, says so in
    the line (`rccl_error`) and leaves with status 0 through os._exit (a thread is still inside RCCL)."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "CROPSR_LAUNCHED")}
    env.update(CROPSR_BENCH_FORCE_RCCL="1", CROPSR_TEST_HOOKS="1", CROPSR_TEST_COMM_INIT_STALL="1", CROPSR_COMM_INIT_TIMEOUT_S="5")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--share-gpu0", "--scale", "0.02",
                        "--steps", "3", "--warmup", "1", "--offtarget-steps", "0", "--full"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, (p.stdout[-2000:], p.stderr[-2000:])
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and "did not return" in d["rccl_error"] and d["gatherv_ok"] is True and d["value"] > 0
    assert "host-socket" in d["config"]["parallelism"]


def test_cli_starts_its_own_ranks(manifest, tmp_path):
    """`python -m cropsr_amd --gpus 2 ...` without a launcher writes the reference's bytes (both ranks on the one GPU
    here, host transport)."""
    import subprocess
    import sys
    from conftest import ROOT
    out_csv = tmp_path / "out.csv"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "CROPSR_LAUNCHED")}
    env.update(CROPSR_GATHER="host", CROPSR_DIST_MAX_PIECE="100", PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "cropsr_amd", "--gpus", "2", "--device", "0", "-o", str(out_csv),
                        "-f", os.path.join(GOLDEN, "probe_mixed.fa"), "-g", os.path.join(GOLDEN, "sample_head.gff"), "--cas9",
                        "--seed", str(manifest["seed"])], capture_output=True, text=True, timeout=600, cwd=str(tmp_path), env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    assert manifest["cases"]["mixed"]["stdout"] in p.stdout
    assert out_csv.read_bytes() == read_golden_csv("mixed")


def _gather_failure_world1(out_path, mode):
    import sys
    from conftest import ROOT
    sys.path.insert(0, ROOT)
    os.environ["CRP_TEST_GATHER_FAIL"] = str(mode)
    from cropsr_amd import Engine, rendezvous
    from cropsr_amd import _native as nat
    eng = Engine(0)
    eng.comm_init(rendezvous.Group(0, 1))
    arena = eng.arena([b"ACGGTCCAGGTTCCAAGG" * 500])
    arena.scan_score_device(20)
    status, text = 0, ""
    try:
        eng.gather_hits(arena, 0)
    except nat.CropsrHipError as e:
        status, text = e.status, str(e)
    # the failure was agreed on BEFORE the exchange: the communicator is still usable
    after = eng.comm_allreduce([2.0], "sum")
    arena.close()
    eng.close()
    with open(out_path, "w") as f:
        f.write("%d|%s|%r" % (status, text, after))


@pytest.mark.parametrize("mode,want", [(1, -4), (2, -5)])
def test_gather_failure_is_agreed_on_before_the_exchange(tmp_path, mode, want):
    """a root that cannot size its receive buffers (mode 1, injected) or a rank whose arena
    has no tables (mode 2) must not return alone from crp_gather_hits and leave its peers in ncclSend/Recv.  The
    status now travels with the counts (all-gather) and every rank returns from the same call; with one rank the
    visible part is: the call fails with the rank's OWN status after both agreement rounds ran on RCCL, and the
    communicator still works.  (N > 1 on real GPUs is the driver's to run.)"""
    import multiprocessing as mp
    out = str(tmp_path / "r.txt")
    p = mp.get_context("spawn").Process(target=_gather_failure_world1, args=(out, mode))
    p.start()
    p.join(600)
    assert p.exitcode == 0
    status, text, after = open(out).read().split("|")
    assert int(status) == want, text
    assert after == "[2.0]"


def test_randomised_arenas_vs_oracle(engine, oracle):
    """Seeded fuzz: arenas with random contig counts, lengths clustered around word (64) and
    tile (16384) boundaries, random alphabets / decoration / guide lengths / packers."""
    from conftest import fuzz_settings
    trials, seed, tick = fuzz_settings(60, 20261003)
    rng = np.random.default_rng(seed)
    alphabets = [b"ACGT", b"ACGTacgtN", b"GGCC", b"ACGTUZuzN')],", b"GGGGGGCCCCCCAT"]
    # contig lengths around word (64), wave (128 words), half-tile and tile (1 024 words = 65 536 positions) borders
    anchors = [0, 1, 30, 63, 64, 65, 8191, 8192, 8193, 16383, 16384, 16385, 2 * 16384 - 1, 2 * 16384, 2 * 16384 + 1, 3 * 16384 + 7,
               4 * 16384 - 1, 4 * 16384, 4 * 16384 + 65, 8 * 16384 - 1, 8 * 16384, 8 * 16384 + 1]
    total_hits = 0
    for trial in range(trials):
        tick("arenas", trial)
        contigs = []
        for _ in range(int(rng.integers(1, 9))):
            n = max(0, int(anchors[rng.integers(len(anchors))] + rng.integers(-40, 41)))
            if rng.random() < 0.3:
                n = int(rng.integers(0, 4000))
            body = rng.choice(np.frombuffer(alphabets[rng.integers(len(alphabets))], dtype=np.uint8), n).tobytes()
            deco = rng.integers(3)
            contigs.append(body if deco == 0 else b"'" + body + (b"')," if deco == 1 else b"')]"))
        l = 20 if rng.random() < 0.7 else int(rng.integers(1, 51))
        total_hits += check_contigs(engine, oracle, contigs, l, "device" if trial % 2 else "host")
    assert total_hits > 50000


def test_results_do_not_depend_on_where_a_contig_lies_in_the_arena(engine, oracle):
    """Shift invariance: one 300 kb contig (soft-masked stretches, N runs, PAM-rich stretches) behind filler contigs of
    0 ... 140 words, so that its words fall on every kind of lane / wave (128 words) / tile (1 024 words) border in turn.
    Its tables must be bit-identical wherever it lies, and equal to the oracle's."""
    rng = np.random.default_rng(77)
    a = np.frombuffer(b"ACGT", dtype=np.uint8)
    body = rng.choice(a, 300_000)
    body[40_000:48_000] |= 0x20           # a soft-masked run
    body[90_000:90_700] = ord("N")
    body[131_000:131_400] = ord("G")       # every position a '+' hit
    body[131_400:131_800] = ord("C")
    body[65_536 - 40:65_536 + 40] = np.frombuffer(b"GGCC" * 20, dtype=np.uint8)  # hits across a tile border (at shift 0)
    main = b"'" + body.tobytes() + b"'),"
    want = oracle.scan_score(main, 20)
    shifts = [0, 1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 64 * 127 - 3, 64 * 128, 64 * 140 + 17, 65_536 - 7, 65_536 + 64]
    for sh in shifts:
        filler = rng.choice(a, sh).tobytes()
        arena = engine.arena([filler, main] if sh else [main])
        got = arena.scan_score(20, want_pre=True).contig(1 if sh else 0)
        assert_hits_equal(got, want, ctx=("shift", sh))
        arena.close()


def test_chain_timeout_falls_back_to_three_launches(oracle, monkeypatch):
    """The safety net of the single-launch mode: a tile that never publishes its counts (test hook
    CRP_TEST_MUTE_TILE) makes every later look-back run out of its TIME allowance; the scan must come
    back with the RIGHT tables all the same (repeated with count / scan / emit) and say so -- in
    crp_last_error and in crp_query's counter.  The fallback is per scan: the next scan tries the
    single launch again, and only three failures in a row latch the three-launch mode
    (crp_configure(CRP_OPT_TWO_PASS, 0) clears the latch)."""
    from cropsr_amd import Engine
    from cropsr_amd import _native as nat
    monkeypatch.setenv("CRP_TEST_MUTE_TILE", "3")
    eng = Engine(0)
    monkeypatch.delenv("CRP_TEST_MUTE_TILE")
    eng.configure(chain_timeout_us=2000)  # 2 ms instead of the default 20: the test times out four times
    rng = np.random.default_rng(101)
    contigs = [rng.choice(np.frombuffer(b"ACGTacgtN", dtype=np.uint8), n).tobytes() for n in (400000, 1234, 250000)]
    arena = eng.arena(contigs)
    assert arena.stats()["n_words"] > 5 * 1024  # more tiles than the muted one
    assert eng.query()["chain_timeouts"] == 0
    got = arena.scan_score(20, want_pre=True)
    for k, c in enumerate(contigs):
        assert_hits_equal(got.contig(k), oracle.scan_score(c, 20), ctx=("fallback", k))
    assert b"timed out" in nat.lib().crp_last_error(eng._ctx)
    assert eng.query() == dict(chain_timeouts=1, two_pass_active=0, comm_world=0, comm_rank=0)
    eng.profile(2)
    eng.profile_read(reset=True)
    again = arena.scan_score(20, want_pre=True)  # tries the single launch again, times out again
    prof = eng.profile_read(reset=True)
    assert prof["count"]["launches"] == 1 and prof["tile_scan"]["launches"] == 1
    assert (bits(again.score_plus) == bits(got.score_plus)).all()
    assert eng.query()["chain_timeouts"] == 2 and eng.query()["two_pass_active"] == 0
    arena.scan_score(20)
    assert eng.query()["chain_timeouts"] == 3 and eng.query()["two_pass_active"] == 1  # latched
    arena.scan_score(20)
    assert eng.query()["chain_timeouts"] == 3  # three launches from the start now
    eng.configure(two_pass=False)
    assert eng.query()["two_pass_active"] == 0
    arena.close()
    eng.close()
