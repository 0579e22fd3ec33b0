"""The source side of the 32x32 flash family's LDS tile image (csrc/fa32_lds_map.h),
on the host.

ff_stage_async (csrc/fa32_common.h) stages a tile by direct global -> LDS loads:
the LDS side of such a load is linear, so the swizzle is applied to the address
a lane reads from.  Builds tests/fa32_async_stage_model.cpp, a stand-alone
program that includes the address header the kernels are built on and walks the
helper's lane-to-position arithmetic, with the host compiler of the machine and
runs it.  For tiles of 64 and 256 rows, 256 and 512 threads, contiguous and
with a [B,S,H,D] row stride it fails unless every 16-byte position of the image
is assigned exactly once, holds the chunk ff_map_chunk_byte puts there, a
quarter-wave reads one whole 256-byte row, and every global offset formed lies
inside the tile."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "vescale_amd", "ops", "csrc")


def _host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        path = shutil.which(name) if name else None
        if path:
            return path
    return None


def test_direct_staging_writes_the_register_path_image(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path / "fa32_async_stage_model")
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-Wall", "-I", CSRC,
         os.path.join(HERE, "fa32_async_stage_model.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    out = run.stdout
    for rows in (64, 256):
        for threads in (256, 512):
            for hq in (1, 2, 4, 32):
                loads = rows * 256 // (threads * 16)
                assert (f"rows {rows} threads {threads} stride {hq * 128}: "
                        f"{loads} loads per thread, image equal") in out
    assert "all checks passed" in out
