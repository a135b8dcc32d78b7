#!/usr/bin/env python3
"""List what the wait-count pass made of the loops of named kernels.

    hipcc -O3 --offload-arch=gfx950 -std=c++17 -fno-slp-vectorize -fPIC --cuda-device-only -S -o dsx.s dsx.hip
    tools/loop_waits.py dsx.s 'k_rowfinal<18, 4, 1, 0, 1>' 'k_fwd_march<0, true, 8>'

For every kernel whose (demangled) name contains one of the patterns, every loop is printed with nothing but its
vector-memory instructions, its s_waitcnt lines, its labels and its branches, in program order.  Loops are the cycles
of the function's block graph (strongly connected components, then the same again inside each with its entry blocks
taken out), so blocks that the compiler placed elsewhere do not drag unrelated code in.  An inner loop is printed on its own and shown as one line inside the loop around it.  A
steady-state loop that prefetches must show counted waits (vmcnt(N), N > 0); `vmcnt(0)` inside it means that every
trip drains the memory queue.  The last line per loop counts them; --summary prints only the
header and that line of every loop.

A listing tool, not a test: it reads the text the compiler wrote and judges nothing.
"""

import argparse
import re
import shutil
import subprocess
import sys

VMEM = re.compile(r"^\s+(buffer_|global_|flat_|scratch_)(load|store|atomic)\S*")
WAIT = re.compile(r"^\s+s_waitcnt\b")
BRANCH = re.compile(r"^\s+(s_cbranch_\w+|s_branch)\s+(\.LBB\w+)")
LABEL = re.compile(r"^(\.LBB\w+):")
FUNC = re.compile(r"^(_Z\w+):")
END = re.compile(r"^\.Lfunc_end\d+:")
VMCNT = re.compile(r"vmcnt\((\d+)\)")


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool or not names:
        return dict((n, n) for n in names)
    out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.splitlines()))


def functions(lines):
    """(mangled name, first line, last line) of every function of the file."""
    found, name, start = [], None, 0
    for i, line in enumerate(lines):
        m = FUNC.match(line)
        if m and name is None:
            name, start = m.group(1), i
        elif END.match(line) and name is not None:
            found.append((name, start, i))
            name = None
    return found


TERMINATOR = re.compile(r"^\s+(s_branch|s_endpgm|s_setpc_b64|s_trap)\b")


def blocks_of(lines, start, end):
    """Basic blocks of a function as [first line, last line] plus the successor lists (indices into the block list)."""
    cuts = set([start + 1])
    for i in range(start + 1, end):
        if LABEL.match(lines[i]):
            cuts.add(i)
        if BRANCH.match(lines[i]) or TERMINATOR.match(lines[i]):
            cuts.add(i + 1)
    firsts = sorted(c for c in cuts if c < end)
    blocks = [(f, (firsts[k + 1] if k + 1 < len(firsts) else end) - 1) for k, f in enumerate(firsts)]
    at = {}
    for k, (f, _) in enumerate(blocks):
        m = LABEL.match(lines[f])
        if m:
            at[m.group(1)] = k
    succ = []
    for k, (f, l) in enumerate(blocks):
        out = []
        m = BRANCH.match(lines[l])
        if m and m.group(2) in at:
            out.append(at[m.group(2)])
        if not TERMINATOR.match(lines[l]) and k + 1 < len(blocks):
            out.append(k + 1)
        succ.append(out)
    return blocks, succ


def sccs(nodes, succ):
    """Strongly connected components with a cycle in them, over the blocks in `nodes` only (iterative Tarjan)."""
    nodes = set(nodes)
    index, low, on, stack, found, n = {}, {}, set(), [], [], [0]
    for root in sorted(nodes):
        if root in index:
            continue
        work = [(root, iter([s for s in succ[root] if s in nodes]))]
        index[root] = low[root] = n[0]; n[0] += 1
        stack.append(root); on.add(root)
        while work:
            v, it = work[-1]
            for w in it:
                if w not in index:
                    index[w] = low[w] = n[0]; n[0] += 1
                    stack.append(w); on.add(w)
                    work.append((w, iter([s for s in succ[w] if s in nodes])))
                    break
                if w in on:
                    low[v] = min(low[v], index[w])
            else:
                work.pop()
                if work:
                    low[work[-1][0]] = min(low[work[-1][0]], low[v])
                if low[v] == index[v]:
                    comp = []
                    while True:
                        w = stack.pop(); on.discard(w); comp.append(w)
                        if w == v:
                            break
                    if len(comp) > 1 or v in succ[v]:
                        found.append(sorted(comp))
    return sorted(found)


def loop_tree(nodes, succ, depth=0):
    """[(depth, blocks of the loop, [blocks of each loop directly inside it])], outer loops before their inner ones."""
    out = []
    for comp in sccs(nodes, succ):
        inside = set(comp)
        heads = [b for b in comp if any(b in succ[p] for p in range(len(succ)) if p not in inside)] or comp[:1]
        inner = loop_tree([b for b in comp if b not in heads], succ, depth + 1)
        out.append((depth, comp, [c for d, c, _ in inner if d == depth + 1]))
        out += inner
    return out


def brief(line):
    return " ".join(line.split(";")[0].split())


def list_loop(lines, blocks, comp, inner, out, summary=False):
    """Print the blocks of a loop in program order; a loop directly inside it is one line.  summary: the last line only."""
    waits, hidden = [], {}
    for c in inner:
        for b in c:
            hidden[b] = c
    told = set()
    for b in comp:
        if b in hidden:
            c = hidden[b]
            if c[0] not in told:
                told.add(c[0])
                if not summary:
                    out.write("      %7d  [inner loop at %s]\n" % (blocks[c[0]][0] + 1, brief(lines[blocks[c[0]][0]])))
            continue
        for i in range(blocks[b][0], blocks[b][1] + 1):
            line = lines[i]
            if LABEL.match(line) or VMEM.match(line) or WAIT.match(line) or BRANCH.match(line):
                if not summary:
                    out.write("      %7d  %s\n" % (i + 1, brief(line)))
                if WAIT.match(line):
                    waits += [int(n) for n in VMCNT.findall(line)]
    counted = sorted(set(n for n in waits if n > 0))
    out.write("      -> own vmcnt waits: %d, of them vmcnt(0): %d; counted: %s\n"
              % (len(waits), sum(1 for n in waits if n == 0), ", ".join(map(str, counted)) or "none"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm", help="device assembly (hipcc --cuda-device-only -S)")
    ap.add_argument("kernels", nargs="+", help="substrings of demangled kernel names, e.g. 'k_fwd_march<0, true, 8>'")
    ap.add_argument("--min-vmem", type=int, default=1, help="skip loops with fewer vector-memory instructions (default 1)")
    ap.add_argument("--max-vmem", type=int, default=None, help="skip loops with more vector-memory instructions")
    ap.add_argument("--summary", action="store_true", help="per loop only its header and the count of its waits")
    args = ap.parse_args()
    with open(args.asm) as f:
        lines = f.read().splitlines()
    funcs = functions(lines)
    names = demangle([n for n, _, _ in funcs])
    pats = [p.replace(" ", "") for p in args.kernels]
    out = sys.stdout
    hit = set()
    for name, start, end in funcs:
        shown = names[name]
        flat = shown.replace(" ", "")
        mine = [p for p in pats if p in flat or p in name]
        if not mine:
            continue
        hit.update(mine)
        out.write("%s\n  (%s, lines %d-%d)\n" % (shown, name, start + 1, end + 1))
        blocks, succ = blocks_of(lines, start, end)
        n = 0
        for depth, comp, inner in loop_tree(range(len(blocks)), succ):
            vmem = sum(1 for b in comp for i in range(blocks[b][0], blocks[b][1] + 1) if VMEM.match(lines[i]))
            if vmem < args.min_vmem or (args.max_vmem is not None and vmem > args.max_vmem):
                continue
            n += 1
            first = blocks[comp[0]][0]
            out.write("  loop at %s  line %d  depth %d  %d blocks  %d vector-memory instructions\n"
                      % (brief(lines[first]), first + 1, depth, len(comp), vmem))
            list_loop(lines, blocks, comp, inner, out, args.summary)
        if n == 0:
            out.write("  no loop with vector memory in it\n")
        out.write("\n")
    missing = [p for p in pats if p not in hit]
    if missing:
        sys.exit("no kernel matches: " + ", ".join(missing))


if __name__ == "__main__":
    main()
