#!/usr/bin/env python3
"""Static instruction budget of the emit kernel, read from the gfx950 ISA the compiler makes of it (no GPU needed).

Compiles cropsr_amd/csrc/crp_kernels.hip for gfx950 with the library's flags (-S --cuda-device-only), takes one
instantiation of emit_kernel (by default the one bench.py times: the LARGE geometry, single launch, l = 20, no
pre-sigmoid column, no seed words), splits it into basic blocks and prints

  row loop   the innermost loop that holds the f64 scorer: one trip through all its blocks
  set-up     every block laid out before the round loop (loads, masks, block scan, descriptors, table staging)
  rounds     the round loop outside the row loop (hit-list build, per-round and per-wave hand-over work)
  void terms the part of the set-up that only a wave with a void bit in reach runs (the void tests of the hit masks),
             and whether the branch around it is a scalar one

  vmem loads the vector-memory loads outside the set-up, by region (rounds, row loop, behind the round loop), and those of
             them that are the successor prefetch: indexed buffer loads whose result nothing reads
  head loads whether the loads at the head of a tile's serial chain leave together: the `s_waitcnt vmcnt` between the
             descriptor loads of the look-back's first look, and the scorer-table loads issued before the first wait

as VALU / f64 / SALU instruction counts, plus the compiler's resource usage: VGPRs, SGPR spills, scratch, LDS and
occupancy.  These are static counts: how often each block runs depends on the genome.

  python tools/emit_isa_budget.py [--json] [--kernel large|small] [--lfix 20|0] [--pre] [--seeds] [--three-launch]
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cropsr_amd", "csrc")
GEOMETRY = {"large": "512ELi1024ELi2ELi5016ELi53760E", "small": "512ELi512ELi1ELi3072ELi53760E"}


def hipcc():
    for c in (os.environ.get("HIPCC"), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc"),
              shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    raise SystemExit("hipcc not found (set HIPCC or ROCM_PATH)")


def makefile_flags():
    """CXXFLAGS of the library build (cropsr_amd/csrc/Makefile), so the ISA is the one that ships"""
    with open(os.path.join(CSRC, "Makefile")) as f:
        for line in f:
            m = re.match(r"CXXFLAGS \?= (.*)", line)
            if m:
                return m.group(1).split()
    raise SystemExit("CXXFLAGS not found in the Makefile")


def compile_asm(workdir, extra=()):
    """(assembly text, compiler remarks) of crp_kernels.hip for gfx950; generated tables go to workdir"""
    sys.path.insert(0, CSRC)
    try:
        import gen_score_terms as g
    finally:
        sys.path.pop(0)
    text, (w1, w2), _ = g.generate(os.path.join(CSRC, "doench_weights.def"))
    with open(os.path.join(workdir, "score_terms.inc"), "w") as f:
        f.write(text)
    with open(os.path.join(workdir, "dense_weights.inc"), "w") as f:
        f.write("__device__ const double CRP_W1[120] = {%s};\n" % ", ".join(v.hex() for v in w1))
        f.write("__device__ const double CRP_W2[464] = {%s};\n" % ", ".join(v.hex() for v in w2))
    with open(os.path.join(workdir, "exp_table.inc"), "w") as f:
        for t, h in g.exp2_table():
            f.write("0x%016xULL, 0x%016xULL,\n" % (t, h))
    out = os.path.join(workdir, "crp_kernels.s")
    # the sources are copied next to the tables, so that their quoted includes find these and nothing in the tree
    for name in os.listdir(CSRC):
        if name.endswith((".h", ".hip")):
            shutil.copy(os.path.join(CSRC, name), os.path.join(workdir, name))
    cmd = [hipcc()] + makefile_flags() + list(extra) + [
        "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only",
        "-Rpass-analysis=kernel-resource-usage", os.path.join(workdir, "crp_kernels.hip"), "-o", out]
    r = subprocess.run(cmd, cwd=workdir, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit("hipcc failed:\n" + r.stderr[-4000:])
    with open(out) as f:
        return f.read(), r.stderr


def kernel_name(geo="large", chained=True, lfix=20, pre=False, seeds=False):
    b = lambda v: "Lb1E" if v else "Lb0E"
    return ("_ZN3crp11emit_kernelINS_7TileGeoILi%sEE%sLi%dE%s%sEEvNS_6PlanesEmiPK15HIP_vector_typeIjLj2EEPmS8_NS_9HitTablesEjjj"
            % (GEOMETRY[geo], b(chained), lfix, b(pre), b(seeds)))


def resources(remarks, name):
    """the compiler's -Rpass-analysis=kernel-resource-usage lines of one kernel"""
    res, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark: (?:\s*)Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        m = re.search(r"remark:\s+([^:]+): (\S+)", line)
        if m and cur == name:
            res[m.group(1).strip()] = m.group(2)
    if not res:
        raise SystemExit("no resource usage for " + name)
    return res


def blocks_of(asm, name):
    """[(label, innermost loop header or None, loop depth, [instructions])] in layout order"""
    lines = asm.splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
    blocks = [["entry", None, 0, []]]
    for i in range(start + 1, len(lines)):
        l = lines[i]
        if l.startswith(".Lfunc_end"):
            break
        m = re.match(r"^\.LBB(\w+):(.*)", l)
        if m:
            label = "BB" + m.group(1)
            hm = re.search(r"Header=(BB\w+) Depth=(\d+)", m.group(2))
            nm = re.search(r"Loop Header: Depth=(\d+)", lines[i + 1]) if i + 1 < len(lines) else None
            if nm:
                blocks.append([label, label, int(nm.group(1)), []])
            else:
                blocks.append([label, hm.group(1) if hm else None, int(hm.group(2)) if hm else 0, []])
            continue
        s = l.split(";")[0].strip()
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        blocks[-1][3].append(s)
    return blocks


def counts(instrs):
    ops = [i.split()[0] for i in instrs]
    return {
        "valu": sum(o.startswith("v_") for o in ops),
        "f64": sum(o.startswith("v_") and "f64" in o for o in ops),
        "salu": sum(o.startswith("s_") and not o.startswith(("s_waitcnt", "s_nop", "s_cbranch", "s_branch")) for o in ops),
        "writelane": sum(o.startswith("v_writelane") for o in ops),
        "readlane": sum(o.startswith("v_readlane") for o in ops),
    }


def void_region(asm, name):
    """The set-up's conditional region with the void terms of the hit masks: the basic blocks (labelled or fall-through)
    ahead of the first loop that shift the void mask in from the left neighbour -- wave_shr:1, which nothing else in
    the kernel uses.  `uniform`: every such block is entered past a scalar conditional branch (s_cbranch_scc / vcc on a
    wave-uniform condition), not under an exec mask."""
    lines = asm.splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
    subs = [[]]  # instructions of each basic block, in layout order
    for l in lines[start + 1:]:
        if l.startswith(".Lfunc_end") or "Loop Header" in l:
            break
        if l.startswith((".LBB", "; %bb.")):
            subs.append([])
            continue
        s = l.split(";")[0].strip()
        if s and not s.startswith(".") and not s.endswith(":"):
            subs[-1].append(s)
    region, uniform = [], True
    for k, ins in enumerate(subs):
        if any("wave_shr:1" in i for i in ins):
            region += ins
            last = subs[k - 1][-1] if k and subs[k - 1] else ""
            uniform = uniform and last.startswith(("s_cbranch_scc", "s_cbranch_vcc"))
    return dict(counts(region), uniform=bool(region) and uniform)


def vmem_loads(instrs):
    """the vector-memory loads among `instrs`; `prefetch`: the indexed buffer loads (idxen), which only the successor prefetch
    of the single-launch kernel issues -- every other buffer access of the kernel addresses by offset"""
    loads = [i for i in instrs if i.split()[0].startswith(("buffer_load", "global_load", "flat_load", "scratch_load"))]
    return {"count": len(loads), "prefetch": sum(i.split()[-1] == "idxen" for i in loads), "instructions": loads}


def registers(operand):
    """the VGPR numbers an operand names: v7 -> {7}, v[4:5] -> {4, 5}"""
    m = re.fullmatch(r"v(\d+)", operand)
    if m:
        return {int(m.group(1))}
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", operand)
    return set(range(int(m.group(1)), int(m.group(2)) + 1)) if m else set()


def prefetch_dst_written(prefetch_ins, row_loop_ins):
    """Row-loop instructions that write the register a prefetch loads into.  The load returns long after it was issued, and
    the compiler does not know: the register must be one that nothing writes while the load is in flight.  (First operand =
    destination of every VALU, LDS-read and load instruction; stores and LDS writes have none.)"""
    dst = set()
    for i in prefetch_ins:
        dst |= registers(i.split()[1].rstrip(","))
    hits = []
    for i in row_loop_ins:
        op = i.split()
        if len(op) > 1 and not op[0].startswith(("buffer_store", "global_store", "flat_store", "ds_write", "s_", "v_cmp")) \
                and registers(op[1].rstrip(",")) & dst:
            hits.append(i)
    return hits


def is_vmcnt_wait(instr):
    return instr.startswith("s_waitcnt") and "vmcnt" in instr


def is_descriptor_load(instr):
    """an 8-byte load past this XCD's L2: what the single-launch kernel's look-back reads tile descriptors with"""
    return instr.startswith("global_load_dwordx2") and instr.split()[-1] == "sc1"


def first_window(round_blocks):
    """The look-back's first look: the descriptor loads of the round loop that are laid out ahead of the look-back's own
    loop (whose header follows them; the spin on one descriptor and the loop's re-load lie inside it).  `round_blocks`:
    the round loop's (label, is a loop header, instructions) in layout order.  Returns (loads, `s_waitcnt vmcnt` between
    the first and the last of them) -- 0 waits: all of the window's requests are out before any answer is waited for --,
    or (0, None) where the kernel has no look-back."""
    ins, seen = [], False
    for label, is_header, block in round_blocks:
        if seen and is_header:
            break
        for i in block:
            seen = seen or is_descriptor_load(i)
            if seen:
                ins.append(i)
    at = [k for k, i in enumerate(ins) if is_descriptor_load(i)]
    if not at:
        return 0, None
    return len(at), sum(is_vmcnt_wait(i) for i in ins[at[0]:at[-1]])


def staging_loads_before_first_wait(all_ins):
    """The scorer tables' way into LDS: 16-byte loads from CRP_TABS.  Counts the `global_load_dwordx4` from the instruction
    that takes the table's address to the first `s_waitcnt vmcnt` behind a load: a thread's requests in flight together."""
    start = next((k for k, i in enumerate(all_ins) if "CRP_TABS" in i), None)
    if start is None:
        return None
    n = 0
    for i in all_ins[start:]:
        if i.startswith("global_load_dwordx4"):
            n += 1
        elif n and is_vmcnt_wait(i):
            break
    return n


def add(a, b):
    return {k: a.get(k, 0) + b[k] for k in b}


def budget(asm, remarks, name):
    blocks = blocks_of(asm, name)
    parent = {}  # loop header -> enclosing loop header: a header's own annotation names it ("Parent Loop BBx")
    for l in asm.splitlines():
        m = re.match(r"^\.LBB(\w+):.*Parent Loop (BB\w+)", l)
        if m:
            parent["BB" + m.group(1)] = m.group(2)

    def loops_of(header):
        chain = []
        while header:
            chain.append(header)
            header = parent.get(header)
        return chain

    scorer = max(blocks, key=lambda b: (counts(b[3])["f64"], b[2]))  # (the first row's copy sits one loop out)
    row_loop = scorer[1]
    if row_loop is None:
        raise SystemExit("the scorer is not inside a loop")
    outer = loops_of(row_loop)[-1]
    row, setup, rounds = {}, {}, {}
    round_blocks = []
    region_ins = {"rounds": [], "row_loop": [], "tail": []}  # (tail: laid out behind the round loop's header, outside the loop)
    seen_outer = False
    zero = counts([])
    for label, header, _, ins in blocks:
        c = counts(ins)
        in_loops = loops_of(header) if header else []
        if label == outer:
            seen_outer = True
        if row_loop in in_loops:
            row = add(row or zero, c)
            region_ins["row_loop"] += ins
        elif outer in in_loops:
            rounds = add(rounds or zero, c)
            region_ins["rounds"] += ins
            round_blocks.append((label, label == header, ins))
        elif not seen_outer:
            setup = add(setup or zero, c)
        else:
            region_ins["tail"] += ins
    res = resources(remarks, name)
    all_ins = [i for b in blocks for i in b[3]]
    return {
        "kernel": name,
        "row_loop": row,
        "row_block": counts(scorer[3]),
        "setup": setup,
        "setup_void": void_region(asm, name),
        "rounds": rounds,
        "whole": counts(all_ins),
        "vmem_loads": {region: vmem_loads(ins) for region, ins in region_ins.items()},
        "prefetch": {"dst_written_in_row_loop": prefetch_dst_written(
            [i for ins in region_ins.values() for i in vmem_loads(ins)["instructions"] if i.split()[-1] == "idxen"], region_ins["row_loop"])},
        "lookback": dict(zip(("first_window_loads", "first_window_waits_between_loads"), first_window(round_blocks))),
        "staging": {"loads_before_first_wait": staging_loads_before_first_wait(all_ins)},
        "vgprs": int(res["VGPRs"]),
        "sgprs": int(res["TotalSGPRs"]),
        "sgpr_spills": int(res["SGPRs Spill"]),
        "vgpr_spills": int(res["VGPRs Spill"]),
        "scratch": int(res["ScratchSize [bytes/lane]"]),
        "lds": int(res["LDS Size [bytes/block]"]),
        "occupancy": int(res["Occupancy [waves/SIMD]"]),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernel", choices=sorted(GEOMETRY), default="large")
    ap.add_argument("--lfix", type=int, choices=(20, 0), default=20)
    ap.add_argument("--pre", action="store_true")
    ap.add_argument("--seeds", action="store_true")
    ap.add_argument("--three-launch", action="store_true")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        asm, remarks = compile_asm(d)
    b = budget(asm, remarks, kernel_name(a.kernel, not a.three_launch, a.lfix, a.pre, a.seeds))
    if a.json:
        print(json.dumps(b, indent=1))
        return
    print(b["kernel"])
    for part in ("row_loop", "row_block", "setup", "rounds", "whole"):
        c = b[part]
        print("  %-10s VALU %4d  f64 %3d  SALU %4d  writelane %3d  readlane %3d"
              % (part, c["valu"], c["f64"], c["salu"], c["writelane"], c["readlane"]))
    v = b["setup_void"]
    print("  void terms VALU %4d of the set-up's, behind a %s branch" % (v["valu"], "scalar" if v["uniform"] else "NON-UNIFORM"))
    for region, v in b["vmem_loads"].items():
        print("  vmem loads in %-8s %d, of which prefetch %d" % (region, v["count"], v["prefetch"]))
    print("  look-back: %s vmcnt waits between the first window's %d descriptor loads; staging: %s table loads before the first wait"
          % (b["lookback"]["first_window_waits_between_loads"], b["lookback"]["first_window_loads"], b["staging"]["loads_before_first_wait"]))
    print("  VGPRs %d  SGPRs %d  SGPR spills %d  VGPR spills %d  scratch %d B  LDS %d B  occupancy %d waves/SIMD"
          % (b["vgprs"], b["sgprs"], b["sgpr_spills"], b["vgpr_spills"], b["scratch"], b["lds"], b["occupancy"]))


if __name__ == "__main__":
    main()
