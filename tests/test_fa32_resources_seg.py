"""Register and LDS budget of the 32x32 flash kernels, packed-document (SEG)
instantiations included, in the style of test_fa32_resources.py.

The direct, double-buffered staging (ff_stage_async) trades staging registers
for LDS: every kernel still has to run at 2 waves per SIMD with no scratch, and
its LDS must leave it the blocks per CU it runs at.  A CU has 160 KiB: fa_fwd
runs two 4-wave blocks per CU, so a block may take at most 80 KiB; the backward
kernels run one 8-wave block per CU (their registers decide that) and may take
the whole 160 KiB.  Compiles attention_fwd.hip and attention_bwd2.hip
device-only for gfx950 with the extension's flags (setup.py) and reads the
compiler's per-kernel resource remarks; it needs hipcc, not a GPU.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vescale_amd", "ops", "csrc")
KIB = 1024


def _build_flags():
    """The device compile flags of the shipped build: setup.py's "nvcc" list,
    read from its text (importing setup.py would run the build)."""
    with open(os.path.join(ROOT, "setup.py")) as f:
        m = re.search(r'"nvcc"\s*:\s*\[([^\]]*)\]', f.read())
    assert m, 'no "nvcc" flag list in setup.py'
    flags = re.findall(r'"([^"]+)"', m.group(1))
    assert "--offload-arch=gfx950" in flags, flags
    return flags


FLAGS = _build_flags()
# kernel -> (source, waves per SIMD of its __launch_bounds__, LDS bytes per block at most)
KERNELS = {
    "fa_fwd_bf16": ("attention_fwd.hip", 2, 80 * KIB),
    "fa_fwd_seg_bf16": ("attention_fwd.hip", 2, 80 * KIB),
    "fa2_dq_bf16": ("attention_bwd2.hip", 2, 160 * KIB),
    "fa2_dq_seg_bf16": ("attention_bwd2.hip", 2, 160 * KIB),
    "fa2_dk_bf16": ("attention_bwd2.hip", 2, 160 * KIB),
    "fa2_dk_seg_bf16": ("attention_bwd2.hip", 2, 160 * KIB),
    "fa2_dv_bf16": ("attention_bwd2.hip", 2, 160 * KIB),
    "fa2_dv_seg_bf16": ("attention_bwd2.hip", 2, 160 * KIB),
}


def _hipcc():
    found = shutil.which("hipcc")
    if found:
        return found
    cand = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    return cand if os.path.exists(cand) else None


def _parse(remarks):
    """{kernel: {field: int}} from -Rpass-analysis=kernel-resource-usage output."""
    out, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: \S*\s+([A-Za-z][A-Za-z /\[\]]*?): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    tmp = tmp_path_factory.mktemp("fa32_resources_seg")
    procs = {}
    for src in sorted({s for s, _, _ in KERNELS.values()}):
        cmd = [hipcc, *FLAGS, "-S", "--cuda-device-only",
               "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, src),
               "-o", str(tmp / (src + ".s"))]
        procs[src] = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                      text=True)
    found = {}
    for src, proc in procs.items():
        text = proc.communicate()[0]
        assert proc.returncode == 0, f"{src} did not compile:\n{text[-4000:]}"
        found.update(_parse(text))
    return found


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_kernel_fits_its_registers_and_lds(usage, kernel):
    assert kernel in usage, f"no resource remark for {kernel}: {sorted(usage)}"
    u = usage[kernel]
    print(kernel, u)
    _, waves, lds = KERNELS[kernel]
    assert u["ScratchSize [bytes/lane]"] == 0, u
    assert u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, u
    assert u["VGPRs"] <= 256, u
    assert u["Occupancy [waves/SIMD]"] >= waves, u
    assert u["LDS Size [bytes/block]"] <= lds, u
