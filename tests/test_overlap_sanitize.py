"""The host-side planning of the overlap matrix -- the refusals in their order, the straight and gathered blocks, the tile
and split schedules, the staging functions and the spreading the kernel shares with the host
(kwage_amd/csrc/overlap_plan.hpp) -- built with g++ -fsanitize=address,undefined as a stand-alone program
(tests/sanitize/overlap_sanitize.cpp).  The program walks the kernel's workgroups lane by lane over matrices whose
allocations end where the matrices end, multiplies the spread operands byte by byte, sums the parts, compares every cell
and the sentinels behind them with a bit-by-bit count, and checks the offsets at row 2^32 - 1 of 12544-byte rows as pure
arithmetic.  CPU only: no device is touched, nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

REPORTS = ("AddressSanitizer", "runtime error", "LeakSanitizer", "FAILED")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_overlap_planning_under_sanitizers(tmp_path):
    exe = str(tmp_path / "overlap_sanitize")
    csrc = os.path.join(ROOT, "kwage_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(csrc, "host.cpp"),
           os.path.join(ROOT, "tests", "sanitize", "overlap_sanitize.cpp"), "-o", exe, "-lz", "-lpthread"]
    b = subprocess.run(cmd, capture_output=True, text=True, cwd=csrc)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    if r.returncode != 0 and ("unexpected memory mapping" in r.stderr or "Shadow memory range interleaves" in r.stderr or "ReserveShadowMemoryRange failed" in r.stderr):
        pytest.skip("the sanitizer runtime cannot start here: " + r.stderr.strip().splitlines()[0][:200])
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    assert "no report" in r.stdout and not any(x in r.stderr for x in REPORTS), r.stderr[-4000:]
    checks, refused = [int(x) for x in r.stdout.split("sanitizers:")[1].replace(" checks,", "").split(" refusals")[0].split()]
    assert checks > 1000000 and refused == 27
