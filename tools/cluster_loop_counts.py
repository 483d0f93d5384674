#!/usr/bin/env python3
"""Static instruction counts of the dedicated cluster kernel (csrc/sse_cluster.hip.h), from the compiler's assembly.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -S --cuda-device-only sweep_cluster.hip -o sweep_cluster.s
    python tools/cluster_loop_counts.py sweep_cluster.s [mangled-symbol-substring] >> profiles/rNN_cluster_static_counts.txt

Parts are found by shape, not by label (labels move with every change):
  * build loop: the longest backward-branch span without a barrier that holds both a compare-and-store (ds_cmpst_b32: the
    rewrite of the two legs' entries behind a union) and global loads (the prefetch of the next tile);
  * a row's union block, fast path: inside the build loop, from the "needs a union" compare in front of the last row's
    compare-and-stores (followed by a wave-uniform any-lane test up to r12, by the exec-masked branch over the block since r15)
    to the second of them, without the serial routine (the span between the exec-masked branch that skips it and that
    branch's target);
  * initialisation loops: every innermost loop in front of the kernel's first barrier, in program order (state and touch words,
    bond entries, chunk counts, per-wave tables, parent table);
  * loops between the scan and the apply pass (range joins, flatten, coins): every outermost barrier-free loop behind the build
    loop and in front of the first apply loop, in program order, named by what it holds: a returning compare-and-swap
    (ds_cmpst_rtn: the range joins), a returning add (ds_add_rtn: the root list's append), Philox rounds (the coin draws), LDS
    reads and writes only (flip bits, state tail), writes only (zeroing);
  * apply loops: the innermost loops behind the build loop that hold global loads, global stores and LDS reads and no Philox:
    the deferred one stores bytes (global_store_byte), the in-place one dwords.  Where the deferred loop is unrolled over the slots
    of its prefetch queue, the row says how many tiles one iteration holds.
Counts are of the text of a span, rarely taken paths included.  A static figure; executed counts come from the SQ_INSTS_*
counters.  The last line is the kernel's register / spill / scratch record from the same file."""
import re
import sys

CLASSES = ["valu", "salu", "lds", "vmem", "smem", "branch", "wait", "other"]
DETAIL = ["s_and_saveexec", "s_or_b64", "s_and_b64", "s_mov_b64", "s_cbranch", "v_cndmask", "v_and_b32", "v_lshl_add", "v_lshlrev", "ds_read", "ds_write",
          "ds_cmpst"]


def classify(op):
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith(("s_load", "s_buffer_load")):
        return "smem"
    if op.startswith(("s_barrier", "s_nop", "s_endpgm", "s_sleep", "s_setprio")):
        return "other"
    return "salu"


def parse(lines, sym):
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*" + re.escape(sym) + r"\w*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
    label_at, insts = {}, []
    for l in lines[start:end]:
        t = l.split(";")[0].strip()
        m = re.match(r"^(\.LBB\w+):", t)
        if m:
            label_at[m.group(1)] = len(insts)
            continue
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        parts = t.split(None, 1)
        insts.append((parts[0], parts[1].strip() if len(parts) > 1 else ""))
    return lines[start].split(":")[0], label_at, insts


def row(what, ops, note=""):
    c = {k: 0 for k in CLASSES}
    for op in ops:
        c[classify(op)] += 1
    d = " ".join(f"{k}={sum(1 for op in ops if op.startswith(k))}" for k in DETAIL if any(op.startswith(k) for op in ops))
    print(f"  {what:<34}{len(ops):>6}" + "".join(f"{c[k]:>8}" for k in CLASSES) + f"   {d}{note}")


def main():
    path = sys.argv[1]
    sym = sys.argv[2] if len(sys.argv) > 2 else "cluster_kernelILi4ELb0ELi0E"
    text = open(path).read().splitlines()
    name, label_at, insts = parse(text, sym)
    ops = [op for op, _ in insts]
    spans = sorted({(label_at[a], i + 1) for i, (op, a) in enumerate(insts) if op.startswith(("s_cbranch", "s_branch")) and a in label_at and label_at[a] <= i})
    has = lambda s, pre: any(o.startswith(pre) for o in ops[s[0]:s[1]])
    innermost = lambda s: not any(t != s and s[0] <= t[0] and t[1] <= s[1] for t in spans)
    philox = lambda s: sum(1 for o in ops[s[0]:s[1]] if o.startswith("v_mad_u64_u32")) >= 8
    build = max((s for s in spans if has(s, "ds_cmpst") and has(s, "global_load") and not has(s, "s_barrier")), key=lambda s: s[1] - s[0])
    print(f"# {name}")
    print(f"  {'part':<34}{'instr':>6}" + "".join(f"{k:>8}" for k in CLASSES))
    row("build loop (one tile)", ops[build[0]:build[1]])
    # the last row's union block: back from its two compare-and-stores to the wave-uniform test in front of it
    cas = [i for i in range(build[0], build[1]) if ops[i].startswith("ds_cmpst")]
    b = cas[-1] + 1
    old = [i for i in range(build[0], cas[-2]) if ops[i] == "s_cmp_lg_u64" and insts[i][1].startswith("vcc") and ops[i - 1].startswith("v_cmp_ne_u32")]
    if old:  # up to r12: a wave-uniform "any lane" test (v_cmp, s_cmp_lg_u64 vcc) in front of the exec-masked block
        a = max(old) - 1
    else:  # since r15 the block is entered on its exec mask alone: v_cmp, s_and_saveexec, s_cbranch_execz to just behind the block
        a = max(i for i in range(build[0], cas[-2]) if ops[i] == "s_cbranch_execz" and label_at.get(insts[i][1]) == b and ops[i - 1].startswith("s_and_saveexec")) - 2
    inner = [s for s in spans if a <= s[0] and s[1] <= b]
    skip, serial = (b, b), (b, b)
    if inner:
        lo, hi = min(s[0] for s in inner), max(s[1] for s in inner)
        cand = [i for i in range(a, lo) if ops[i] == "s_cbranch_execz" and label_at.get(insts[i][1], -1) >= hi]
        if cand:
            serial = (cand[-1] + 1, label_at[insts[cand[-1]][1]])
            # since r16 the lanes beyond the fast path are parked: around the serial routine (now the branch of the lanes that find
            # the queue full) lies the exec-masked park branch, itself inside the block's own branch
            skip = (cand[1] + 1, label_at[insts[cand[1]][1]]) if len(cand) > 2 else serial
    fast = ops[a:skip[0]] + ops[skip[1]:b]
    if skip == serial:
        row("union block of a row, fast path", fast, f"   (serial routine left out: {skip[1] - skip[0]} instructions)")
    else:
        row("union block of a row, fast path", fast, f"   (park branch left out: {skip[1] - skip[0]} instructions)")
        row("  its park branch", ops[skip[0]:serial[0]] + ops[serial[1]:skip[1]], f"   (serial routine for a full queue left out: {serial[1] - serial[0]} instructions)")
        # the drain of a full queue: in front of the first row's union block, the shortest loop of the tile that walks the parent
        # table AND links (16-bit reads and writes: the serial routine's retry loop around its walk; the scan's own loops, two
        # cuts on one variable, read lanes instead), without a compare-and-store or a global access
        drains = [s for s in spans if build[0] <= s[0] and s[1] <= cas[0] and has(s, "ds_read_u16") and has(s, "ds_write_b16")
                  and not has(s, "ds_cmpst") and not has(s, "global_")]
        if drains:
            s = min(drains, key=lambda s: s[1] - s[0])
            row("drain of a full queue, its loop", ops[s[0]:s[1]])
    first_barrier = ops.index("s_barrier")
    init = [s for s in spans if s[1] <= first_barrier and innermost(s)]
    for k, s in enumerate(init):
        row(f"initialisation loop {k}", ops[s[0]:s[1]])
    row("initialisation, all loops", [o for s in init for o in ops[s[0]:s[1]]])
    # between the scan and the apply pass: outermost barrier-free loops, in program order
    is_apply = lambda s: innermost(s) and has(s, "global_load") and has(s, "global_store") and has(s, "ds_read") and not philox(s)
    first_apply = min((s[0] for s in spans if s[0] >= build[1] and is_apply(s)), default=len(ops))
    post = [s for s in spans if build[1] <= s[0] and s[1] <= first_apply and not has(s, "s_barrier") and not has(s, "global_load")]
    post = [s for s in post if not any(t != s and t[0] <= s[0] and s[1] <= t[1] for t in post)]
    for s in post:
        traits = [n for n, pre in (("joins", "ds_cmpst_rtn"), ("root list", "ds_add_rtn")) if has(s, pre)] + (["coins"] if philox(s) else [])
        if not traits:
            traits = ["LDS reads and writes"] if has(s, "ds_read") else ["writes only"]
        row("post-scan loop: " + " + ".join(traits), ops[s[0]:s[1]])
    row("post-scan loops, all", [o for s in post for o in ops[s[0]:s[1]]])
    print(f"  barriers in the kernel: {ops.count('s_barrier')}, instructions in the kernel: {len(ops)}")
    for s in spans:
        if s[0] >= build[1] and innermost(s) and has(s, "global_load") and has(s, "global_store") and has(s, "ds_read") and not philox(s):
            if has(s, "global_store_byte"):  # a tile is K byte stores: the loop may be unrolled over the slots of its prefetch queue
                k = int(re.search(r"cluster_kernelILi(\d+)E", name).group(1))
                tiles = max(1, sum(1 for o in ops[s[0]:s[1]] if o.startswith("global_store_byte")) // k)
                row("apply loop, deferred (one tile)" if tiles == 1 else f"apply loop, deferred ({tiles} tiles)", ops[s[0]:s[1]])
            else:
                row("apply loop, in place (one tile)", ops[s[0]:s[1]])
    # the kernel's metadata record: the keys between the "  - .agpr_count:" lines around its .name
    at = next(i for i, l in enumerate(text) if l.strip().startswith(".name:") and l.split()[-1] == name)
    lo = max(i for i in range(at) if text[i].startswith("  - ."))
    hi = next((i for i in range(at, len(text)) if text[i].startswith("  - .")), len(text))
    rec = {}
    for l in text[lo:hi]:
        m = re.match(r"^  [- ] \.(vgpr_count|agpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s*(\d+)", l)
        if m:
            rec[m.group(1)] = int(m.group(2))
    print(f"  registers: VGPR {rec.get('vgpr_count')}  AGPR {rec.get('agpr_count', 0)}  SGPR {rec.get('sgpr_count')}  vector spills {rec.get('vgpr_spill_count')}  "
          f"scalar spills {rec.get('sgpr_spill_count')}  scratch {rec.get('private_segment_fixed_size')} B")


if __name__ == "__main__":
    main()
