#!/usr/bin/env python3
"""How many dependent scalar round trips lie in front of the first per-env row load of the step kernels?

Cross-compiles the default kernel variant to gfx950 assembly (no GPU needed) and, for the plain step kernel, the EMIT step kernel
and the persistent rollout kernel of the metric configuration, prints the instructions from the kernel's entry to the first row
`global_load_dwordx4` of the fast staging path with three blob units per lane, and counts

  s_load before the first s_waitcnt lgkmcnt      the first batch of kernel-argument loads
  s_load between that wait and the row loads     argument loads that cost a wait of their own (0 = one batch)
  scalar waits before the first row load         dependent round trips (1 = the kernel arguments, once)

The path: basic blocks are split at labels and branches; the block of the row loads is the one with exactly nine
global_load_dwordx4 in a row (3 blob units, y, x, target, 2 x sections, parameters: the action rows follow behind the decode
branch; the 8- and 20-unit instances have 14 and 26), and the path printed is the one with the fewest instructions from the entry
to it, whichever way the branches on it go.

  tools/stage_prologue.py                      compile mop-truss-marl_amd/csrc/truss_hip.hip
  tools/stage_prologue.py --source FILE.hip    another source tree's truss_hip.hip (e.g. a checkout of the parent commit)
  tools/stage_prologue.py --asm FILE.s         parse assembly that was compiled before
  --brief                                      counts only"""
import argparse
import heapq
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-munsafe-fp-atomics", "-DTRUSS_ONLY_DEFAULT_VARIANT",
         "--cuda-device-only", "-S"]
KERNELS = (("step<16,8,1,5>", "_Z17truss_step_kernelILi16ELi8ELi1ELi5ELb0EE"),
           ("step<16,8,1,5,EMIT>", "_Z17truss_step_kernelILi16ELi8ELi1ELi5ELb1EE"),
           ("rollout<16,8,1,5>", "_Z20truss_rollout_kernelILi16ELi8ELi1ELi5EE"))
ROW_LOADS = 9
BRANCH = re.compile(r"^s_(cbranch_\w+|branch)\s+(\S+)")


def compile_asm(source):
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc] + FLAGS + ["-o", out, os.path.basename(source)], cwd=os.path.dirname(os.path.abspath(source)),
                          stderr=subprocess.DEVNULL)
    return out


def kernel_text(lines, prefix):
    """instructions and labels of the kernel whose symbol begins with `prefix`"""
    start = next(i for i, l in enumerate(lines) if l.startswith(prefix) and ":" in l)
    body = []
    for l in lines[start + 1:]:
        s = l.split(";")[0].strip()
        if s.startswith(".Lfunc_end"):
            break
        if s and not s.startswith(".") or re.match(r"^\.LBB\w+:", s):
            body.append(s)
    return body


def blocks_of(body):
    """-> list of (label or None, [instructions]); a block ends behind a branch"""
    blocks, cur, label = [], [], None
    for s in body:
        if s.endswith(":"):
            if cur or label:
                blocks.append((label, cur))
            cur, label = [], s[:-1]
            continue
        cur.append(s)
        if BRANCH.match(s):
            blocks.append((label, cur))
            cur, label = [], None
    blocks.append((label, cur))
    return blocks


def path_to_row_loads(blocks):
    index = {lab: i for i, (lab, _) in enumerate(blocks) if lab}

    def succ(i):
        ins = blocks[i][1]
        m = BRANCH.match(ins[-1]) if ins else None
        out = []
        if m and m.group(2) in index:
            out.append(index[m.group(2)])
        if not (m and m.group(1) == "branch") and i + 1 < len(blocks):
            out.append(i + 1)
        return out

    def is_target(i):
        return sum(s.startswith("global_load_dwordx4") for s in blocks[i][1]) == ROW_LOADS

    dist, prev, heap = {0: 0}, {}, [(0, 0)]
    while heap:
        d, i = heapq.heappop(heap)
        if d > dist.get(i, 1 << 60):
            continue
        if is_target(i):
            path = [i]
            while path[-1] in prev:
                path.append(prev[path[-1]])
            return path[::-1]
        for j in succ(i):
            nd = d + len(blocks[i][1])
            if nd < dist.get(j, 1 << 60):
                dist[j], prev[j] = nd, i
                heapq.heappush(heap, (nd, j))
    raise SystemExit("no block with %d row loads found" % ROW_LOADS)


def report(name, body, brief):
    blocks = blocks_of(body)
    path = path_to_row_loads(blocks)
    text = []
    for i in path:
        lab, ins = blocks[i]
        if lab:
            text.append(lab + ":")
        for s in ins:
            text.append("\t" + s)
            if i == path[-1] and s.startswith("global_load_dwordx4"):
                break
    ins = [t.strip() for t in text if t.startswith("\t")]
    waits = [k for k, s in enumerate(ins) if s.startswith("s_waitcnt") and "lgkmcnt" in s]
    loads = [k for k, s in enumerate(ins) if s.startswith("s_load") or s.startswith("s_buffer_load")]
    first = waits[0] if waits else len(ins)
    print(f"== {name}")
    if not brief:
        print("\n".join(text))
    print(f"   s_load before the first s_waitcnt lgkmcnt    : {sum(k < first for k in loads)}")
    print(f"   s_load between that wait and the row loads   : {sum(k > first for k in loads)}")
    print(f"   scalar waits before the first row load       : {len(waits)}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--source", default=os.path.join(ROOT, "mop-truss-marl_amd", "csrc", "truss_hip.hip"))
    ap.add_argument("--asm", default=None)
    ap.add_argument("--brief", action="store_true")
    a = ap.parse_args()
    asm = a.asm or compile_asm(a.source)
    lines = open(asm).read().splitlines()
    for name, prefix in KERNELS:
        report(name, kernel_text(lines, prefix), a.brief)
    if not a.asm:
        os.unlink(asm)


if __name__ == "__main__":
    sys.exit(main())
