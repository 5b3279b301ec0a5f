#!/usr/bin/env python3
"""Issue slots of ONE Newton iteration of the Ant row solver, counted on compiled code (no GPU).

    tools/isa_one.sh 0 16 false 0 > /tmp/k.s  &&  python tools/newton_slots.py /tmp/k.s [--markdown]

`ant_solve_rows_core` (csrc/ant_newton_rows.h) brackets its `while` loop with two assembler comments, `; newton loop begin` and
`; newton loop end`.  Everything the compiler emits between them is the loop: its head (the two exit tests), the gradient and
Hessian, the elimination, the vote, the line search, the update.  This tool classifies the instructions between the marks and
splits them by the path a wave takes:

  * a *slot chain* is a run of wave-uniform guards `cx.any(ncon > k)` around the code of contact slot k (each_contact): a run of
    forward wave-uniform branches (`s_cbranch_vccz` / `vccnz` / `scc0` / `scc1`) with no label between them, at least four of which jump to the same join label.  The stretch behind the
    k-th guard of a chain is slot k's; from the fifth guard on (slots 4 and up, in pairs and fours) to the join label it is "5+";
  * the line search is the innermost loop of the region ("Child Loop" of the compiler's comments) and the blocks it returns
    through: it runs only in an iteration whose active set changes, behind the first `ls_fast_iters` iterations of a solve;
  * everything else is executed by every iteration ("common").

A path with n contact slots executes common + slots 0 .. n-1.  The counts are static: an exec-mask region counts whether or not the
branch around it is taken.
"""
import argparse
import collections
import re
import sys

BEGIN, END = "; newton loop begin", "; newton loop end"
INST = re.compile(r"^((?:v|s|ds|global|buffer|flat|scratch)_\w+)\s*(.*)$")

# float arithmetic: what a Newton iteration is for
FLOAT_PREFIXES = ("v_fma_f32", "v_fmac_f32", "v_mul_f32", "v_add_f32", "v_sub_f32", "v_subrev_f32", "v_pk_fma_f32", "v_pk_mul_f32",
                  "v_pk_add_f32", "v_rcp_f32", "v_sqrt_f32", "v_rsq_f32", "v_max_f32", "v_min_f32", "v_div_", "v_mad_f32", "v_fma_mix")

# a wave-uniform guard ends in one of these (which one depends on how the compiler holds the vote)
GUARD_BRANCHES = ("s_cbranch_vccz", "s_cbranch_vccnz", "s_cbranch_scc0", "s_cbranch_scc1")

CLASSES = ["float arithmetic", "v_cndmask", "v_cmp", "v_mov", "v_accvgpr", "lane read/write", "other VALU", "SALU", "s_nop",
           "s_and_saveexec + branch", "s_waitcnt", "memory"]


def classify(mn):
    if mn.startswith(FLOAT_PREFIXES):
        return "float arithmetic"
    if mn.startswith("v_cndmask"):
        return "v_cndmask"
    if mn.startswith("v_cmp"):
        return "v_cmp"
    if mn.startswith("v_mov"):
        return "v_mov"
    if mn.startswith("v_accvgpr"):
        return "v_accvgpr"
    if mn.startswith(("v_readlane", "v_readfirstlane", "v_writelane")):
        return "lane read/write"
    if mn.startswith("v_"):
        return "other VALU"
    if mn == "s_nop":
        return "s_nop"
    if mn == "s_waitcnt":
        return "s_waitcnt"
    if mn.startswith(("s_and_saveexec", "s_or_saveexec", "s_cbranch", "s_branch")):
        return "s_and_saveexec + branch"
    if mn.startswith("s_"):
        return "SALU"
    return "memory"


def loop_lines(path):
    """the lines of the .s between the two marks (exactly one pair: the metric instantiation inlines one solve)"""
    lines = open(path).read().split("\n")
    b = [i for i, l in enumerate(lines) if l.strip() == BEGIN]
    e = [i for i, l in enumerate(lines) if l.strip() == END]
    if len(b) != 1 or len(e) != 1 or b[0] >= e[0]:
        raise SystemExit(f"{path}: expected one '{BEGIN}' in front of one '{END}', found {len(b)} / {len(e)}")
    return lines[b[0] + 1:e[0]]


def parse(lines):
    """[(mnemonic without _e32/_e64, operands, label in front or None)] and the index of each label"""
    insts, labels, pending = [], {}, None
    for raw in lines:
        m = re.match(r"^(\.LBB\d+_\d+):", raw)
        if m:
            pending = m.group(1)
            labels[pending] = len(insts)
            continue
        m = INST.match(raw.split(";")[0].strip())
        if m:
            insts.append((re.sub(r"_e(32|64)$", "", m.group(1)), m.group(2).strip(), pending))
            pending = None
    return insts, labels


def chains(insts, labels):
    """slot chains: [(indices of the guards' branches, index of the join label)]"""
    runs, cur = [], []
    for i, (mn, ops, lab) in enumerate(insts):
        if lab is not None:
            if cur:
                runs.append(cur)
            cur = []
        if mn in GUARD_BRANCHES and labels.get(ops, -1) > i:
            cur.append(i)
    if cur:
        runs.append(cur)
    out = []
    for run in runs:
        tg = collections.Counter(insts[i][1] for i in run)
        join, n = tg.most_common(1)[0]
        if n < 4:
            continue
        # the guards of the chain: from the first branch to the join label on; a guard in front of it whose target is another
        # label belongs to the chain when exactly four jumps to the join label would otherwise be in front of a pair's guard
        first = next(k for k, i in enumerate(run) if insts[i][1] == join)
        inner = [k for k, i in enumerate(run[first:]) if insts[i][1] != join]
        if inner and inner[0] == 4 and first > 0:
            first -= 1
        guards = [i for i in range(run[first], labels[join]) if insts[i][0] in GUARD_BRANCHES and labels.get(insts[i][1], -1) > i]
        out.append((guards, labels[join]))
    return out


def line_search(lines_, insts, labels):
    """[lo, hi) of the line search: from the first saveexec in front of the innermost loop to the label that joins behind it"""
    # the innermost loop's header is the one label the compiler comments as a child loop of the Newton loop
    hdr = None
    for raw in lines_:
        m = re.match(r"^(\.LBB\d+_\d+):.*Parent Loop", raw)
        if m:
            hdr = m.group(1)
    if hdr is None:
        return None
    h = labels[hdr]
    lo = max(i for i in range(h) if insts[i][0].startswith("s_and_saveexec") and insts[i + 1][0] == "s_cbranch_execz" and labels.get(insts[i + 1][1], -1) > h)
    hi = labels[insts[lo + 1][1]]
    return lo, hi


def inventory(path):
    lines_ = loop_lines(path)
    insts, labels = parse(lines_)
    tag = ["common"] * len(insts)
    ls = line_search(lines_, insts, labels)
    if ls:
        for i in range(ls[0], ls[1]):
            tag[i] = "line search"
    for guards, join in chains(insts, labels):
        for k, g in enumerate(guards):
            end = guards[k + 1] + 1 if k < 4 else join
            name = f"slot {k}" if k < 4 else "slots 4+"
            for i in range(g + 1, end):
                tag[i] = name
    table = collections.OrderedDict((t, collections.Counter()) for t in ["common", "slot 0", "slot 1", "slot 2", "slot 3", "slots 4+", "line search"])
    mnem = collections.Counter()
    for (mn, ops, lab), t in zip(insts, tag):
        table[t][classify(mn)] += 1
        if classify(mn) == "float arithmetic":
            mnem[mn] += 1
    return insts, tag, table, mnem


def paths(table):
    """class counts of one iteration without a line search, by the number of contact slots the wave runs"""
    out = collections.OrderedDict()
    for name, parts in (("<= 2 slots", ["common", "slot 0", "slot 1"]), ("3 slots", ["common", "slot 0", "slot 1", "slot 2"]),
                        ("4 slots", ["common", "slot 0", "slot 1", "slot 2", "slot 3"])):
        c = collections.Counter()
        for p in parts:
            c.update(table[p])
        out[name] = c
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm", help=".s of ant_step_kernel<0, 16, false, 0> (tools/isa_one.sh 0 16 false 0)")
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    insts, tag, table, mnem = inventory(args.asm)
    pt = paths(table)
    cols = list(table) + list(pt)
    data = dict(table)
    data.update(pt)
    sep = " | " if args.markdown else "  "
    head = ["class"] + cols
    rows = [[c] + [str(data[k][c]) for k in cols] for c in CLASSES]
    rows.append(["all"] + [str(sum(data[k].values())) for k in cols])
    rows.append(["not float arithmetic"] + [str(sum(data[k].values()) - data[k]["float arithmetic"]) for k in cols])
    if args.markdown:
        print("| " + sep.join(head) + " |")
        print("|" + "---|" * len(head))
        for r in rows:
            print("| " + sep.join(r) + " |")
    else:
        w = [max(len(r[i]) for r in [head] + rows) for i in range(len(head))]
        for r in [head] + rows:
            print(sep.join(x.ljust(w[i]) if i == 0 else x.rjust(w[i]) for i, x in enumerate(r)))
    print()
    print(f"loop region: {len(insts)} instructions; float arithmetic {sum(mnem.values())}, the rest {len(insts) - sum(mnem.values())}")
    print("float-arithmetic mnemonics: " + ", ".join(f"{k} {v}" for k, v in sorted(mnem.items())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
