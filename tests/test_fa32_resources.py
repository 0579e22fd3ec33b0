"""Register budget of the four 32x32 flash kernels on the benchmark path.

They run at 2 waves per SIMD (their __launch_bounds__), i.e. on at most 256
VGPRs, and fa2_dq and fa2_dk use nearly all of them: a change to the tile loop
or to a shared helper can push a few registers into scratch without any test of
the results noticing.  This compiles attention_fwd.hip and attention_bwd2.hip
device-only for gfx950 with the extension's flags (setup.py) and reads the
compiler's own per-kernel resource remarks; it needs hipcc, not a GPU.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vescale_amd", "ops", "csrc")


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
# kernel -> waves per SIMD its __launch_bounds__(threads, 2) asks for
KERNELS = {
    "fa_fwd_bf16": ("attention_fwd.hip", 2),
    "fa2_dq_bf16": ("attention_bwd2.hip", 2),
    "fa2_dk_bf16": ("attention_bwd2.hip", 2),
    "fa2_dv_bf16": ("attention_bwd2.hip", 2),
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
    tmp = tmp_path_factory.mktemp("fa32_resources")
    procs = {}
    for src in sorted({s for s, _ in KERNELS.values()}):
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
def test_kernel_fits_its_launch_bounds(usage, kernel):
    assert kernel in usage, f"no resource remark for {kernel}: {sorted(usage)}"
    u = usage[kernel]
    print(kernel, u)
    assert u["ScratchSize [bytes/lane]"] == 0, u
    assert u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, u
    assert u["VGPRs"] <= 256, u
    assert u["Occupancy [waves/SIMD]"] >= KERNELS[kernel][1], u
