"""The host-side planning of the nearest-neighbour lists -- the call's own refusals, the strips, per strip the overlap's
tiles and parts, the key, the eligibility and the steps of the radix select the kernel shares with the host
(kwage_amd/csrc/neighbors_plan.hpp over overlap_plan.hpp) -- built with g++ -fsanitize=address,undefined as a stand-alone
program (tests/sanitize/neighbors_sanitize.cpp).  The program walks the strips, walks the select kernel's workgroup lane
by lane over cell rows whose allocation ends where the strip's rows end, compares every list with a plain sort under the
exact order, and checks the offsets of a strip beyond 4 GiB as pure arithmetic.  CPU only: no device is touched, nothing
is loaded into python."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

REPORTS = ("AddressSanitizer", "runtime error", "LeakSanitizer", "FAILED")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_neighbors_planning_under_sanitizers(tmp_path):
    exe = str(tmp_path / "neighbors_sanitize")
    csrc = os.path.join(ROOT, "kwage_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(csrc, "host.cpp"),
           os.path.join(ROOT, "tests", "sanitize", "neighbors_sanitize.cpp"), "-o", exe, "-lz", "-lpthread"]
    b = subprocess.run(cmd, capture_output=True, text=True, cwd=csrc)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    if r.returncode != 0 and ("unexpected memory mapping" in r.stderr or "Shadow memory range interleaves" in r.stderr or "ReserveShadowMemoryRange failed" in r.stderr):
        pytest.skip("the sanitizer runtime cannot start here: " + r.stderr.strip().splitlines()[0][:200])
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    assert "no report" in r.stdout and not any(x in r.stderr for x in REPORTS), r.stderr[-4000:]
    checks, refused, lists, strips = [int(x) for x in r.stdout.split("sanitizers:")[1].split(":")[0].replace(",", "").split()[::2]]
    assert checks > 1000000 and refused == 10 and lists > 10000 and strips > 100
