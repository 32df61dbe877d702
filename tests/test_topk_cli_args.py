"""kwage_top's argument errors (no GPU): a missing, zero, too large or non-numeric -k, and a threshold outside [0, 1],
end the program with a non-zero status and a message before any device is opened."""
import subprocess

import pytest


@pytest.fixture(scope="module")
def kwage_top():
    from kwage_amd import native
    native.ensure_built()
    return native.KWAGE_TOP_BIN


@pytest.mark.parametrize("args, text", [
    (["-d", "db", "ACGT"], "-k"),
    (["-k", "0", "-d", "db", "ACGT"], "1 <= -k <= 1024"),
    (["-k", "1025", "-d", "db", "ACGT"], "1 <= -k <= 1024"),
    (["-k", "abc", "-d", "db", "ACGT"], "1 <= -k <= 1024"),
    (["-k", "-3", "-d", "db", "ACGT"], "1 <= -k <= 1024"),
    (["-d", "db", "ACGT", "-k"], "1 <= -k <= 1024"),
    (["-k", "5", "-t", "1.5", "-d", "db", "ACGT"], "threshold"),
    (["-k", "5", "-t", "-0.5", "-d", "db", "ACGT"], "threshold"),
])
def test_kwage_top_argument_errors(kwage_top, tmp_path, args, text):
    # HIP_VISIBLE_DEVICES=-1: were a device opened, the run would fail with a device error instead of the message
    r = subprocess.run([kwage_top] + args, cwd=tmp_path, capture_output=True, text=True,
                       env={"PATH": "/usr/bin:/bin", "HIP_VISIBLE_DEVICES": "-1"}, timeout=60)
    assert r.returncode != 0, r
    assert text in r.stderr, r.stderr
    assert r.stdout == ""
