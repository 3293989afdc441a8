#!/usr/bin/env python3
"""Compare two gfx950 assembly listings of one source, function by function.

  hipcc <the flags of ops/build.py> --cuda-device-only -S csrc/kernels/X.hip -o X.s
  python tools/isa_compare.py PARENT.s NEW.s

One row per function: `identical` (the same instruction text once labels are normalised), `blocks
reordered` (the same multiset of instruction lines, branches aside, and every basic block with a
v_mfma has the parent's opcode sequence and s_waitcnt immediates), or `differs` with what does.
Resource changes are appended to the row; VGPR / AGPR / scratch / spill / LDS / occupancy changes and
added or dropped functions make the exit status 1. SGPR figures are reported only.
"""
import collections
import re
import sys

HARD = ("vgpr_count", "agpr_count", "private_segment_fixed_size", "vgpr_spill_count", "group_segment_fixed_size", "occupancy")
SOFT = ("sgpr_count", "sgpr_spill_count")


def parse(path):
    text = open(path).read()
    funcs = {}
    for m in re.finditer(r"^(\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:(.*?; Occupancy: (\d+))", text, re.M | re.S):
        blocks = [[]]   # basic blocks: lists of instruction lines, labels -> L, comments dropped
        for raw in m.group(2).split("\n"):
            line = raw.split(";")[0].strip()
            if re.match(r"\.LBB\d+_\d+:", line) or raw.startswith("; %bb."):
                blocks.append([])
            elif line and not line.startswith("."):
                blocks[-1].append(re.sub(r"\.LBB\d+_\d+", "L", " ".join(line.split())))
        funcs[m.group(1)] = {"blocks": [b for b in blocks if b], "occupancy": m.group(4)}
    for entry in text[text.index("amdhsa.kernels:"):].split("\n  - ")[1:]:
        kv = dict(re.findall(r"^\s*\.(\w+):\s+(\S+)\s*$", entry, re.M))
        if "name" in kv:   # (the version list that follows the kernels has none)
            funcs[kv["name"]].update(kv)
    return funcs


def is_branch(line):
    return line.startswith(("s_cbranch", "s_branch"))


def mfma_schedule(blocks):
    """per basic block with a v_mfma: its opcodes, an s_waitcnt with its operands"""
    out = []
    for b in blocks:
        if any(l.startswith("v_mfma") for l in b):
            out.append(tuple(l if l.startswith("s_waitcnt") else l.split()[0] for l in b if not is_branch(l)))
    return sorted(out)


def main(parent_path, new_path):
    old, new = parse(parent_path), parse(new_path)
    bad = sorted(set(old) ^ set(new))
    for name in bad:
        print(f"{name}\t{'dropped' if name in old else 'added'}")
    tally = collections.Counter()
    for name in sorted(set(old) & set(new)):
        o, n = old[name], new[name]
        lines = [collections.Counter(l for b in f["blocks"] for l in b if not is_branch(l)) for f in (o, n)]
        if o["blocks"] == n["blocks"]:
            status = "identical"
        elif lines[0] == lines[1] and mfma_schedule(o["blocks"]) == mfma_schedule(n["blocks"]):
            status = "blocks reordered"
        else:
            delta = sum(((lines[0] - lines[1]) + (lines[1] - lines[0])).values())
            ops = [collections.Counter(l.split()[0] for l in c.elements()) for c in lines]
            moved = " ".join(f"{k}{ops[1][k] - ops[0][k]:+d}" for k in sorted(set(ops[0]) | set(ops[1])) if ops[0][k] != ops[1][k])
            sched = [collections.Counter(mfma_schedule(f["blocks"])) for f in (o, n)]
            status = (f"differs ({delta} lines; opcode counts: {moved or 'equal'}; "
                      f"{sum((sched[0] - sched[1]).values())} of {sum(sched[0].values())} mfma blocks differ)")
        res = [f"{k} {o[k]}->{n[k]}" for k in HARD + SOFT if o[k] != n[k]]
        if any(o[k] != n[k] for k in HARD):
            bad.append(name)
        tally[status.split(" (")[0]] += 1
        print("\t".join([name, status] + res))
    print(f"# {len(old)} parent functions, {len(new)} new; " + ", ".join(f"{v} {k}" for k, v in sorted(tally.items())) +
          f"; {len(bad)} with added / dropped names or changed hard resources")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
