#!/usr/bin/env python3
"""What a kernel does with its own arguments before its first loads: hipcc -S for one .hip file, then per kernel the kernarg size, the
kernarg preload length (dwords the dispatcher puts into user SGPRs), the s_load count, and the number of s_waitcnt on lgkmcnt in front of
the first vector-memory load (vm) and in front of the first non-temporal load (nt: the weight burst of the decode kernels).
With a preload length > 0 a kernel has two entries: the fall-back stub (s_load of the same SGPRs, one wait, a branch: taken where the
firmware does not preload) and the preloaded entry 256 bytes further on; waits are given as "preloaded entry / fall-back entry".
Counted in program-text order from the entry label (branches are not followed: a prologue with an early loop shows the loop's waits too).
Usage: python tools/kernel_entry.py uniaudio2_amd/csrc/ua2_gemv.hip [--filter SUBSTR]... [--flags ...hipcc flags, to the end of the line]"""
import os, re, subprocess, sys, tempfile

argv = sys.argv[1:]
flags = []
if "--flags" in argv:
    flags = argv[argv.index("--flags") + 1:]
    argv = argv[:argv.index("--flags")]
flt = [argv[i + 1] for i, v in enumerate(argv) if v == "--filter"]
src = argv[0]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
if src.endswith(".s"):                               # an ISA listing made earlier (a minute per file saved)
    lines = open(src).read().splitlines()
else:
  with tempfile.TemporaryDirectory() as d:
    asm = os.path.join(d, "k.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only", "-Wno-unused-command-line-argument",
                    *flags, src, "-o", asm], check=True)
    lines = open(asm).read().splitlines()

VM = re.compile(r"^\s*(global|buffer|flat|scratch)_load")
meta, body, cur = {}, {}, None
for l in lines:
    m = re.match(r"^(\w+):\s*; @", l)
    if m:
        cur = m.group(1)
        body[cur] = []
        continue
    m = re.match(r"^\s*\.amdhsa_kernel (\w+)", l)
    if m:
        cur = None
        meta[m.group(1)] = k = {}
        continue
    m = re.match(r"^\s*\.amdhsa_(kernarg_size|user_sgpr_kernarg_preload_length) (\d+)", l)
    if m and meta:
        k[m.group(1)] = int(m.group(2))
    if cur is not None:
        if l.startswith(".Lfunc_end"):
            cur = None
        elif re.match(r"^\s+[a-z]", l) and not l.lstrip().startswith("."):
            body[cur].append(l.strip())
        elif ".p2align\t8" in l:
            body[cur].append(".entry")          # the preloaded entry starts behind the stub's padding


def waits(ins):
    """(s_waitcnt on lgkmcnt before the first vm load, before the first nt load); None = no such load"""
    n, first_vm, first_nt = 0, None, None
    for i in ins:
        if i.startswith("s_waitcnt") and "lgkmcnt" in i:
            n += 1
        elif VM.match(i):
            if first_vm is None:
                first_vm = n
            if first_nt is None and re.search(r"\bnt\b", i):
                first_nt = n
                break
    return first_vm, first_nt


names = subprocess.run(["c++filt"], input="\n".join(meta), capture_output=True, text=True).stdout.splitlines()
print(f"{'kernel':64s} kernarg preload s_load  waits before first vm / nt load")
for sym, name in zip(meta, names):
    name = re.sub(r"\(.*", "", name.replace("(anonymous namespace)::", "").replace("void ", ""))
    if flt and not any(f in name for f in flt):
        continue
    ins = body.get(sym, [])
    pre = meta[sym].get("user_sgpr_kernarg_preload_length", 0)
    nload = sum(i.startswith("s_load") for i in ins)
    if ".entry" in ins:
        cut = ins.index(".entry")
        stub, main = [i for i in ins[:cut] if not i.startswith("s_branch")], ins[cut + 1:]
        nload -= sum(i.startswith("s_load") for i in stub)      # the stub's loads are the preload's stand-in, not the kernel's own
        a, b = waits(main), waits(stub + main)
        w = f"vm {a[0]} / {b[0]}   nt {a[1]} / {b[1]}"
    else:
        a = waits(ins)
        w = f"vm {a[0]}   nt {a[1]}"
    print(f"{name:64s} {meta[sym].get('kernarg_size', 0):7d} {pre:7d} {nload:6d}  {w}")
