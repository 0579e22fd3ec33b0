"""The counted vector-memory waits of the gemm8 region-rotation schedules
(csrc/gemm8_sched.h), on the host.

A wait vmcnt(n) only says that all but the n youngest loads of a wave have
landed; whether that covers the region a phase reads depends on which slots
were issued since, and near the end of K some were not.  A numerical test
catches a short count only by luck (the loads were issued three or four phases
earlier).  Builds tests/gemm8_wait_model.cpp, a stand-alone program that
includes the table the kernels are built on and walks one wave's queue of
outstanding loads for every schedule and every allowed K-tile count in 1..12,
with the host compiler of the machine and runs it.  It fails unless every
region read holds its tile with nothing in flight and a barrier between the
wait and the read (a wave's wait covers its own loads only), and no slot
issues into a region that is still being read."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "vescale_amd", "ops", "csrc")

# schedule -> allowed K-tile counts (the host guards of gemm_tn8)
ALLOWED = {"rot": range(1, 13), "rot-u2": range(2, 13, 2), "rot-ra": range(1, 13),
           "rot8": range(4, 13, 2), "rot9": range(4, 13, 2)}


def _host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        path = shutil.which(name) if name else None
        if path:
            return path
    return None


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("gemm8") / "gemm8_wait_model")
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-Wall", "-I", CSRC,
         os.path.join(HERE, "gemm8_wait_model.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    return exe


def test_every_read_is_covered_and_no_slot_overwrites_a_live_region(model):
    run = subprocess.run([model], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    for sched, counts in ALLOWED.items():
        for ntile in counts:
            assert f"{sched} ntile {ntile}: ok" in run.stdout
    assert "FAIL" not in run.stdout
    assert "all checks passed" in run.stdout


def test_model_reports_steady_counts_on_the_last_tiles(model):
    """The negative control: with the steady loop's counts on every tile (what
    the kernels did before the tail rule) the model must name the reads that
    the short queue of the last tile leaves uncovered, and only those tiles."""
    run = subprocess.run([model, "--steady-only"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 1, run.stdout + run.stderr
    out = run.stdout
    assert "FAIL rot ntile 3: tile 2 p0 reads B h1 with 2 loads in flight (last wait vmcnt(4))" in out
    assert "FAIL rot ntile 3: tile 2 p2 reads A q1 with 2 loads in flight (last wait vmcnt(8))" in out
    assert "FAIL rot-ra ntile 3: tile 2 p0 reads B h1" in out
    assert "FAIL rot8 ntile 4: tile 3 p0 reads B h1" in out
    assert "FAIL rot9 ntile 4: tile 3 p0 reads A q0" in out
    # ntile 1 has no counted wait at all
    assert "rot ntile 1: ok" in out and "rot-ra ntile 1: ok" in out
    for line in out.splitlines():
        if line.startswith("FAIL"):
            words = line.split()
            ntile, tile = int(words[3].rstrip(":")), int(words[5])
            assert tile == ntile - 1, line


def test_model_reports_waits_with_no_barrier_before_the_reads(model):
    """The second negative control: a counted wait at the start of the phase
    whose reads it gates (where the kernels once had it) covers one wave's
    loads; the other waves' shares of the region are read before any barrier.
    On an MI355X with every CU starting cold this summed stale rows.  The
    read-ahead form, which reads after the phase's first barrier, passes."""
    run = subprocess.run([model, "--waits-open-the-phase"], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 1, run.stdout + run.stderr
    out = run.stdout
    assert ("FAIL rot ntile 3: tile 1 p0 reads B h0 straight after the wait vmcnt(4) that "
            "retired it, no barrier between") in out
    assert "FAIL rot8 ntile 4: tile 2 p0 reads" in out and "FAIL rot9 ntile 4: tile 2 p0 reads" in out
    for ntile in ALLOWED["rot-ra"]:
        assert f"rot-ra ntile {ntile}: ok" in out
    assert "in flight" not in out.replace("loads in flight\n", "")
