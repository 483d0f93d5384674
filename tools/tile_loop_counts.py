#!/usr/bin/env python3
"""Static instruction counts of the trimmed diagonal kernel's tile loop, from the compiler's assembly.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -S --cuda-device-only sweep_fast.hip -o sweep_fast.s
    python tools/tile_loop_counts.py sweep_fast.s [mangled-symbol-substring] >> profiles/rNN_diag_static_counts.txt

The tile loop is found by shape, not by name: the shortest backward-branch span of the kernel that holds the whole Philox
(at least 36 v_mad_u64_u32); a round of the fixed point is the backward-branch span inside it that holds the v_mbcnt prefix
counts.  Counts are of the text between the loop's label and its back edge, rarely taken paths included: what a wave executes
per tile is a subset of the body plus (rounds - 1) times the round.  A static figure; executed counts come from the SQ_INSTS_*
counters."""
import re
import sys


def kernel_text(lines, sym):
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*" + re.escape(sym) + r"\w*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
    return lines[start:end]


def classify(op):
    if op.startswith(("v_readlane", "v_writelane")):
        return "lane_rw"
    if op.startswith("v_readfirstlane"):
        return "readfirstlane"
    if op.startswith("v_"):
        return "valu"
    if op.startswith(("s_waitcnt", "s_cbranch", "s_branch", "s_barrier", "s_nop", "s_setprio", "s_endpgm", "s_sleep")):
        return "wait_branch"
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        return "smem"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    return "other"


def counts(body):
    c = {}
    for op in body:
        k = classify(op)
        c[k] = c.get(k, 0) + 1
    for name in ("v_mad_u64_u32", "v_bitop3", "s_add_u32", "v_cndmask", "v_cvt_f64", "v_mul_f64", "v_cmp", "ds_read", "ds_write"):
        c[name] = sum(1 for op in body if op.startswith(name))
    return c


def main():
    path = sys.argv[1]
    sym = sys.argv[2] if len(sys.argv) > 2 else "sweep_fast_kernelILi4ELi0E"
    lines = kernel_text(open(path).read().splitlines(), sym)
    label_at, insts = {}, []  # label -> index of the next instruction; instructions as (opcode, operands)
    for l in lines:
        t = l.split(";")[0].strip()
        m = re.match(r"^(\.LBB\w+):", t)
        if m:
            label_at[m.group(1)] = len(insts)
            continue
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        parts = t.split(None, 1)
        insts.append((parts[0], parts[1] if len(parts) > 1 else ""))
    spans = []
    for i, (op, args) in enumerate(insts):
        if op.startswith(("s_cbranch", "s_branch")) and args.strip() in label_at and label_at[args.strip()] <= i:
            spans.append((label_at[args.strip()], i + 1))
    ops = [op for op, _ in insts]
    philox = [s for s in spans if sum(1 for o in ops[s[0]:s[1]] if o.startswith("v_mad_u64_u32")) >= 36]
    tile = min(philox, key=lambda s: s[1] - s[0])
    rounds = [s for s in spans if tile[0] <= s[0] and s[1] <= tile[1] and s != tile and any(o.startswith("v_mbcnt") for o in ops[s[0]:s[1]])]
    rnd = min(rounds, key=lambda s: s[1] - s[0])
    name = lines[0].split(":")[0]
    print(f"# {name}")
    keys = ["valu", "lane_rw", "readfirstlane", "salu", "smem", "wait_branch", "lds", "vmem", "v_mad_u64_u32", "v_bitop3", "s_add_u32", "v_cndmask",
            "v_cvt_f64", "v_mul_f64", "v_cmp", "ds_read", "ds_write"]
    print(f"  {'part':<28}" + "".join(f"{k:>14}" for k in keys))
    for what, s in (("tile loop body", tile), ("one fixed-point round", rnd)):
        c = counts(ops[s[0]:s[1]])
        print(f"  {what:<28}" + "".join(f"{c.get(k, 0):>14}" for k in keys) + f"   ({s[1] - s[0]} instructions)")


if __name__ == "__main__":
    main()
