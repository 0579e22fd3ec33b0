"""Vector-memory waits and direct-to-LDS loads of the counted-wait gemm8
kernels, in program order, from a gfx950 cross-compile of ops/csrc/gemm8.hip.

    python tools/gemm8_waits_isa.py [label] >> profiles/gemm8_waits_isa.txt

Needs hipcc and no GPU.  Per kernel: every `s_waitcnt` that names vmcnt, every
`global_load_lds_dwordx4` (runs of them folded to a count), loop labels and
backward branches, so the steady loop and the tail can be told apart.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "vescale_amd", "ops", "csrc", "gemm8.hip")
KERNELS = ("gemm8_tn_bf16_rot", "gemm8_tn_bf16_rot3", "gemm8_tn_bf16_rot3np",
           "gemm8_tn_bf16_rot3u2", "gemm8_tn_bf16_rot3ra", "gemm8_tn_bf16_rot8",
           "gemm8_tn_bf16_rot9")


def main():
    label = sys.argv[1] if len(sys.argv) > 1 else "working tree"
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "gemm8.s")
        subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip",
                        "--cuda-device-only", "-S", SRC, "-o", asm], check=True)
        lines = open(asm).read().splitlines()
    print(f"==== {label}: hipcc --offload-arch=gfx950 -O3, gemm8.hip ====")
    kernel, run = None, 0

    def flush():
        nonlocal run
        if run:
            print(f"    global_load_lds_dwordx4 x{run}")
            run = 0

    for ln in lines:
        s = ln.strip()
        m = re.match(r"^(\w+):", s)
        if m and m.group(1) in KERNELS:
            kernel = m.group(1)
            print(f"\n-- {kernel}")
            continue
        if kernel is None:
            continue
        if s.startswith("s_endpgm"):
            flush()
            kernel = None
        elif s.startswith("global_load_lds"):
            run += 1
        elif s.startswith("s_waitcnt") and "vmcnt" in s:
            flush()
            print("    " + s.split(";")[0].strip())
        elif re.match(r"^\.LBB\d+_\d+:", s):
            flush()
            print("  " + s.split(";")[0].strip())
        elif s.startswith("s_cbranch") or s.startswith("s_branch"):
            flush()
            print("      " + s.split(";")[0].strip())


if __name__ == "__main__":
    main()
