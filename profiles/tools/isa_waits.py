#!/usr/bin/env python3
"""Exposed-latency census of one kernel in a gfx950 assembly listing (hipcc --cuda-device-only -S): every s_waitcnt that
waits for a counter to reach 0 and stands within WINDOW instructions behind a load of that counter (ds_read* for lgkmcnt,
global_load* / flat_load* for vmcnt) -- a wait with nothing to hide the round trip.  Printed with the basic block it sits
in and whether that block belongs to a loop (range label .. backward branch).
Usage: isa_waits.py engine.s '<demangled substring>' [window=3]"""
import re
import subprocess
import sys


def kernel_body(path, want):
    lines = open(path).read().splitlines()
    for i, l in enumerate(lines):
        if "@function" in l and ".type" in l:
            name = l.split()[1].rstrip(",").split(",")[0]
            dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
            if want in dem:
                end = next(j for j in range(i, len(lines)) if lines[j].strip().startswith(".Lfunc_end"))
                return dem, lines[i:end]
    raise SystemExit("not found")


def main():
    path, want = sys.argv[1], sys.argv[2]
    window = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    dem, body = kernel_body(path, want)
    print("kernel:", dem[:200])
    labels, instrs, block_of, block = {}, [], [], "entry"
    for l in body:
        t = l.strip()
        m = re.match(r"(\.LBB\d+_\d+):", t)
        if m:
            labels[m.group(1)] = len(instrs)
            block = m.group(1)
            continue
        if not t or t.startswith(";") or t.startswith("."):
            continue
        instrs.append(t.split(";")[0].strip())
        block_of.append(block)
    loops = []
    for k, ins in enumerate(instrs):
        m = re.match(r"s_c?branch\S*\s+(\.LBB\d+_\d+)", ins)
        if m and m.group(1) in labels and labels[m.group(1)] <= k:
            loops.append((labels[m.group(1)], k, m.group(1)))

    def innermost(k):
        inside = [(b - a, lab, b - a + 1) for a, b, lab in loops if a <= k <= b]
        return min(inside)[1:] if inside else None

    total = {"lgkmcnt": 0, "vmcnt": 0}
    tight = {"lgkmcnt": 0, "vmcnt": 0}
    rows = []
    for k, ins in enumerate(instrs):
        if not ins.startswith("s_waitcnt"):
            continue
        for cnt, loads in (("lgkmcnt", ("ds_read",)), ("vmcnt", ("global_load", "flat_load", "buffer_load"))):
            if cnt + "(0)" not in ins:
                continue
            total[cnt] += 1
            back = [j for j in range(max(0, k - window), k) if instrs[j].startswith(loads)]
            if back:
                tight[cnt] += 1
                lp = innermost(k)
                rows.append((k, cnt, k - back[-1], instrs[back[-1]].split()[0], block_of[k],
                             "loop %s (%d instr)" % lp if lp else "straight-line"))
    print("instructions: %d   s_waitcnt lgkmcnt(0): %d, of them within %d of a ds_read: %d   vmcnt(0): %d, within %d of a load: %d"
          % (len(instrs), total["lgkmcnt"], window, tight["lgkmcnt"], total["vmcnt"], window, tight["vmcnt"]))
    for r in rows:
        print("  instr %5d  %-7s  %d behind %-20s block %-12s %s" % r)


if __name__ == "__main__":
    main()
