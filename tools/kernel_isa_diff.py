#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 code hipcc emits for two versions of
a .hip file: the check the mfma_gemm.hip header asks for before and after
any change to its kernels. Needs hipcc and c++filt, no GPU.

    git show HEAD:distributedllm_amd/ops/csrc/mfma_gemm.hip > /tmp/old.hip
    tools/kernel_isa_diff.py /tmp/old.hip distributedllm_amd/ops/csrc/mfma_gemm.hip \\
        --map 'k_ffn16_mt<(.*)>$=k_ffn16<\\1, true>'

Kernels are matched by demangled name without the argument list; --map
(a regex on the OLD name = its replacement, first match wins) follows
renames. Two kernels are `same` when their instruction streams (comments
stripped, .LBBn_ labels normalised, lines naming the kernel itself dropped)
and the five resource fields below are equal. Whole streams are compared;
nothing here looks for particular instructions.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

CSRC = Path(__file__).resolve().parent.parent / "distributedllm_amd/ops/csrc"
# the code-generation flags of distributedllm_amd/ops/build.py
CFLAGS = ["-O3", "-std=c++17", "-fno-gpu-rdc", "-Wno-ignored-attributes",
          "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1"]
META = ["next_free_vgpr", "next_free_sgpr", "accum_offset",
        "group_segment_fixed_size", "private_segment_fixed_size"]


def kernels(src, arch):
    """{demangled name: (instruction lines, {field: value})} of one file."""
    with tempfile.TemporaryDirectory() as tmp:
        asm = Path(tmp) / "out.s"
        subprocess.run(
            [os.environ.get("HIPCC", "hipcc"), *CFLAGS,
             f"--offload-arch={arch}", "--cuda-device-only", "-S",
             f"-I{Path(src).resolve().parent}", f"-I{CSRC}", str(src),
             "-o", str(asm)], check=True)
        lines = asm.read_text().splitlines()
    body, meta, cur, desc = {}, {}, None, None
    for raw in lines:
        line = raw.split(";")[0].strip()
        m = re.match(r"\.amdhsa_kernel (\S+)", line)
        if m:
            desc = meta.setdefault(m.group(1), {})
        elif line == ".end_amdhsa_kernel":
            desc = None
        elif desc is not None:
            m = re.match(r"\.amdhsa_(\w+) (\S+)", line)
            if m and m.group(1) in META:
                desc[m.group(1)] = m.group(2)
        elif re.match(r"\.type\s+\S+,@function", line):
            cur = re.match(r"\.type\s+(\S+),", line).group(1)
            body[cur] = []
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur and line and cur not in line and (
                not line.startswith(".") or line.startswith(".LBB")):
            body[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", line))
    names = sorted(meta)
    dem = subprocess.run(["c++filt"], input="\n".join(names), text=True,
                         capture_output=True, check=True).stdout.split("\n")
    # "void k<int=1>(args)" -> "k<1>": the arguments are not compared
    # (kernels in an anonymous namespace keep their bare name)
    short = [re.sub(r"^void |\(.*\)$", "",
                    d.replace("(anonymous namespace)::", "")).replace(
        "(WType)", "").replace("(GemmMode)", "") for d in dem]
    return {s: (body[n], meta[n]) for s, n in zip(short, names)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--map", action="append", default=[],
                    metavar="OLD_REGEX=NEW", help="rename rule, repeatable")
    ap.add_argument("--arch", default=os.environ.get("PYTORCH_ROCM_ARCH",
                                                     "gfx950"))
    args = ap.parse_args()
    rules = [m.split("=", 1) for m in args.map]
    old, new = kernels(args.old, args.arch), kernels(args.new, args.arch)
    count = {"same": 0, "diff": 0, "only in old": 0}
    matched = set()
    for name, (ins, meta) in sorted(old.items()):
        target = name
        for pat, rep in rules:
            if re.search(pat, name):
                target = re.sub(pat, rep, name)
                break
        label = name if target == name else f"{name} -> {target}"
        if target not in new:
            count["only in old"] += 1
            print(f"only in old  {label}")
            continue
        matched.add(target)
        ins2, meta2 = new[target]
        if ins == ins2 and meta == meta2:
            count["same"] += 1
            print(f"same  {label}")
            continue
        count["diff"] += 1
        fields = " ".join(f"{k}={meta.get(k)}/{meta2.get(k)}" for k in META)
        print(f"diff  {label}: instructions {len(ins)}/{len(ins2)} {fields}")
    only_new = sorted(set(new) - matched)
    for name in only_new:
        print(f"only in new  {name}")
    print(f"{len(old)} old, {len(new)} new kernels: {count['same']} same, "
          f"{count['diff']} diff, {count['only in old']} only in old, "
          f"{len(only_new)} only in new")
    return 1 if count["diff"] else 0


if __name__ == "__main__":
    sys.exit(main())
