"""The PAM scorer's table indices and tail gates, evaluated with the 32-bit semantics of the instructions the kernel
issues for them (CPU only).

Each chain-prefix table is read at the index the emitted expression computes from the one-hot masks: AND, OR and
shifts on 32-bit words, and __umul24 = v_mul_u32_u24, the low 32 bits of the product of the operands' low 24 bits.
For every one of the 2^k gate patterns of every chain the expression is evaluated with numpy uint32 arithmetic on masks
that set exactly that pattern's gate bits, and the entry it reads must be the chain's start value plus the pattern's
weights added one by one in chain order (one rounding per addition).  The gated FMAs left after the tables must each
place their mask bit in the high word's exponent field (bits 20..30) with a weight scaled exactly for that bit."""
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cropsr_amd", "csrc")


def generated():
    import sys
    sys.path.insert(0, CSRC)
    try:
        import gen_score_terms as g
    finally:
        sys.path.pop(0)
    text, _, _ = g.generate(os.path.join(CSRC, "doench_weights.def"))
    return text


def weights():
    w = {}
    for line in open(os.path.join(CSRC, "doench_weights.def")):
        t = line.split("#", 1)[0].split()
        if t and t[0] == "FIRST":
            w["%s%02d" % (t[1], int(t[2]))] = float(t[3])
        elif t and t[0] == "SECOND":
            w["%s%s%02d" % (t[1], t[2], int(t[3]))] = float(t[4])
    return w


def umul24(a, b):
    """v_mul_u32_u24: low 32 bits of the product of the low 24 bits of both operands"""
    a = np.asarray(a, dtype=np.uint32).astype(np.uint64) & np.uint64(0xFFFFFF)
    b = np.uint64(int(b) & 0xFFFFFF)
    return ((a * b) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def evaluate(expr, masks):
    """the emitted C expression on uint32 arrays: literals become np.uint32, so every operation wraps at 32 bits"""
    py = re.sub(r"0x([0-9a-f]+)u", lambda m: "U(0x%s)" % m.group(1), expr).replace("__umul24(", "umul24(")
    assert re.fullmatch(r"[\smnATCG()&|<>0-9a-fxU,]*(umul24)?[\smnATCG()&|<>0-9a-fxU,]*", py), py
    out = eval(py, {"__builtins__": {}}, dict(masks, U=np.uint32, umul24=umul24))
    assert out.dtype == np.uint32
    return out


def pam_body(text):
    body = text[text.index("#define CRP_SCORE_BODY_PAM_TABLES"):]
    return body[:body.index("/* end */")]


def test_table_indices_read_sequential_sums():
    text = generated()
    data = [float.fromhex(x) for x in re.search(r"#define CRP_SCORE_TAB_DATA \{ \\\n(.*?)\n    \}", text, re.S).group(1)
            .replace("\\", "").replace(",", " ").split()]
    init = {m.group(1): float.fromhex(m.group(2)) for m in re.finditer(r"#define CRP_PAM_INIT_(\w\w) (\S+)", text)}
    w = weights()
    body = pam_body(text)
    # the kernel's second-base masks are the one-hot masks moved down one position
    assert "const uint32_t nA = (mA) >> 1, nT = (mT) >> 1, nC = (mC) >> 1, nG = (mG) >> 1;" in body
    chains = list(re.finditer(r"(\w\w) = crp_tab_at\(score_tab, (\d+), (.*?)\); /\* (\d+) terms: (.*?) \*/", body))
    assert [m.group(1) for m in chains] == ["fA", "fT", "fC", "fG", "sA", "sT", "sC", "sG"]
    looked_up, end = 0, 0
    for m in chains:
        chain, base, expr, k, names = m.group(1), int(m.group(2)), m.group(3), int(m.group(4)), m.group(5).split()
        assert len(names) == k and base == end  # the tables sit back to back, in chain order
        end = base + 8 * (1 << k)
        patterns = np.arange(1 << k, dtype=np.uint32)
        masks = {"%s%s" % (c, b): np.zeros(1 << k, dtype=np.uint32) for c in "mn" for b in "ATCG"}
        for i, name in enumerate(names):
            on = ((patterns >> np.uint32(i)) & np.uint32(1)).astype(bool)
            if chain[0] == "f":
                assert name[0] == chain[1]
                p = int(name[1:]) - 1
                masks["m" + chain[1]][on] |= np.uint32(1 << p)
            else:
                # pair b1 b2 at p: b1 at position p (mB1 bit p) and b2 at p + 1 (nB2 bit p)
                assert name[1] == chain[1]
                p = int(name[2:]) - 1
                masks["m" + name[0]][on] |= np.uint32(1 << p)
                masks["n" + chain[1]][on] |= np.uint32(1 << p)
        off = evaluate(expr, masks).astype(np.int64)
        assert (off % 8 == 0).all() and (off >= 0).all() and (off < 8 * (1 << k)).all(), chain
        assert len(set(off.tolist())) == 1 << k, chain
        for pattern in range(1 << k):
            v = init[chain]
            for i in range(k):
                if (pattern >> i) & 1:
                    v = v + w[names[i]]
            assert data[(base + int(off[pattern])) // 8] == v, (chain, pattern)
        looked_up += k
    assert end == 8 * len(data) and looked_up >= 40


def test_tail_gates_read_exponent_bits_with_exact_weights():
    text = generated()
    w = weights()
    body = pam_body(text)
    seen = 0
    for m in re.finditer(r"CRP_TERM(2?)\((\w\w), (\w+), (?:(\w+), )?\s*(\d+), (\S+)\) /\* (\w+) ", body):
        two, chain, copy1, copy2, bit, lit, name = m.groups()
        bit = int(bit)
        p = int(re.sub(r"^[ATCG]+", "", name)) - 1
        if lit.startswith("CRP_WS("):
            continue  # a term on a shifted copy: the generic scorer's weight table, checked with that scorer
        assert 20 <= bit <= 30 and bit == p, name  # unshifted mask: position p is high-word bit p
        if two:
            assert copy1 == "m" + name[0] and copy2 == "n" + name[1] and chain == "s" + name[1]
        else:
            assert copy1 == "m" + name[0] and chain == "f" + name[0]
        # gate = 2^(E - 1023) with E = 1 << (bit - 20): the weight times the gate is the reference weight, exactly
        gate = math.ldexp(1.0, (1 << (bit - 20)) - 1023)
        assert float.fromhex(lit) * gate == w[name], name
        seen += 1
    assert seen == 13
