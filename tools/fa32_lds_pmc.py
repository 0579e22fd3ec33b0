"""One call of each 32x32 flash kernel at the Llama-8B bench shape, for a
counter run of its own:

    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_VALU_MFMA_BF16 \
        -d OUT --output-format csv -- python tools/fa32_lds_pmc.py

fa_fwd_bf16 and its no-PV / no-QK^T ablations (the forward driver's,
tools/fa_fwd_profile.py), then fa2_dq / fa2_dk / fa2_dv through fa_bwd2.
`python tools/fa32_lds_pmc.py --table OUT` sums the counters per kernel from
the csv files under OUT and prints conflicts per MFMA."""
import csv
import glob
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNELS = ("fa_fwd_bf16", "fa_fwd_bf16_ab2", "fa_fwd_bf16_ab3",
           "fa2_dq_bf16", "fa2_dk_bf16", "fa2_dv_bf16")


def run():
    import torch
    import vescale_amd.ops as ops

    C = ops.require_ext()
    B, Hq, Hkv, S = 4, 32, 8, 8192
    torch.manual_seed(0)
    q = torch.randn(B, Hq, S, 128, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, Hkv, S, 128, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, Hkv, S, 128, device="cuda", dtype=torch.bfloat16)
    dy = torch.randn(B, Hq, S, 128, device="cuda", dtype=torch.bfloat16)
    sc = 1.0 / math.sqrt(128)
    for mode in (2, 3):
        C.fa_fwd_ablate(q, k, v, sc, mode)
    o, lse = C.fa_fwd(q, k, v, sc)
    C.fa_bwd2(q, k, v, o, dy, lse, sc, False)
    torch.cuda.synchronize()
    print("done")


def table(out_dir):
    tot = {}
    for path in glob.glob(os.path.join(out_dir, "**", "*counter_collection.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row["Kernel_Name"].split("(")[0].strip()
                if name in KERNELS:
                    d = tot.setdefault(name, {})
                    d[row["Counter_Name"]] = d.get(row["Counter_Name"], 0.0) + float(row["Counter_Value"])
    counters = sorted({c for d in tot.values() for c in d})
    mfma = "SQ_INSTS_VALU_MFMA_BF16"
    print(f"{'kernel':<18}" + "".join(f"{c:>30}" for c in counters) + f"{'LDSconf/MFMA':>14}{'LDSidx/MFMA':>13}")
    for name in KERNELS:
        if name not in tot:
            continue
        d = tot[name]
        n = d.get(mfma, float("nan"))
        print(f"{name:<18}" + "".join(f"{d.get(c, float('nan')):>30.4e}" for c in counters)
              + f"{d.get('SQ_LDS_BANK_CONFLICT', float('nan')) / n:>14.3f}"
              + f"{d.get('SQ_LDS_IDX_ACTIVE', float('nan')) / n:>13.3f}")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--table":
        table(sys.argv[2])
    else:
        run()
