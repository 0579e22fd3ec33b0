"""The LDS tile map of the 32x32 flash family (csrc/fa32_lds_map.h) against the
CDNA4 LDS bank rules, on the host.

Builds tests/fa32_lds_bank_model.cpp, a stand-alone program that includes the
address header the kernels are built on, with the host compiler of the machine
and runs it.  The program enumerates the lane addresses of every ff_afrag /
ff_bfrag row fragment, every ff_tr_read8 read and every staging store, applies
the lane groups and bank rules, and fails unless a ds_read_b128 takes 4 LDS
cycles, a ds_read_b64_tr_b16 takes 2, the stores' array cycles are no worse
than the previous map's, and the map is a bijection of the tile.  4, 2 and
"bijection" are conditions, not measurements."""
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


def test_tile_map_is_bank_conflict_free(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path / "fa32_lds_bank_model")
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-Wall", "-I", CSRC,
         os.path.join(HERE, "fa32_lds_bank_model.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    out = run.stdout
    assert "ds_read_b128 fragments: 4..4 cycles" in out
    assert "ds_read_b64_tr_b16: 2..2 cycles" in out
    for threads in (128, 256, 512):
        assert f"ds_write_b128, {threads} threads: 8 array cycles" in out
    assert "bijection: ok" in out and "all checks passed" in out
