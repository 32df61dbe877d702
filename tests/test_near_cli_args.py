"""kwage_near's usage and argument errors (no GPU): the program ends with its message before any device is opened, and
prints nothing on stdout.  It has kwage's -d and -o, -k (default 10) and run accessions, positional or with -s; anything
else shows the usage text."""
import os
import subprocess

import pytest

from cli_early_exits import EARLY_EXITS, check_early_exit
from conftest import GOLDEN

USAGE = ("Usage for kwage_near (the samples most like given samples of the database, by Jaccard index of their Bloom filters):\n"
         "\t[-k <number of samples per query sample>] (1 to 1024, default is 10)\n"
         "\t[-o <output file>] (default is stdout)\n"
         "\t-d <database search path> (can be repeated)\n"
         "\t[-s <run accession>] (can be repeated)\n"
         "\t[<run accession>] (can be repeated)\n")

BASIC = os.path.join(GOLDEN, "basic", "db")


@pytest.fixture(scope="module")
def kwage_near():
    from kwage_amd import native
    native.ensure_built()
    return native.KWAGE_NEAR_BIN


def run(exe, args, cwd):
    # HIP_VISIBLE_DEVICES=-1: were a device opened, the run would fail with a device error instead of the message
    return subprocess.run([exe] + args, cwd=cwd, capture_output=True, text=True,
                          env={"PATH": "/usr/bin:/bin", "HIP_VISIBLE_DEVICES": "-1"}, timeout=60)


@pytest.mark.parametrize("args, status", [
    ([], 1),
    (["-h"], 0),
    (["-t", "0.5", "-d", BASIC, "SRR0001000"], 1),
    (["-i", "reads.fa", "-d", BASIC, "SRR0001000"], 1),
    (["--o.csv", "-d", BASIC, "SRR0001000"], 1),
    (["-d"], 1),
])
def test_kwage_near_usage(kwage_near, tmp_path, args, status):
    r = run(kwage_near, args, tmp_path)
    assert r.returncode == status, r
    assert r.stderr == USAGE and r.stdout == ""


@pytest.mark.parametrize("args, text", [
    (["-d", BASIC], "Please provide at least one run accession of a sample of the database\n"),
    (["-d", BASIC, "-k", "5"], "Please provide at least one run accession of a sample of the database\n"),
    (["-d", BASIC, "-k", "0", "SRR0001000"], "Please provide: 1 <= -k <= 1024 (got \"0\")\n"),
    (["-d", BASIC, "-k", "1025", "SRR0001000"], "Please provide: 1 <= -k <= 1024 (got \"1025\")\n"),
    (["-d", BASIC, "-k", "ten", "-s", "SRR0001000"], "Please provide: 1 <= -k <= 1024 (got \"ten\")\n"),
    (["-d", BASIC, "SRR0001000", "-k"], "Please provide: 1 <= -k <= 1024 (got \"\")\n"),
    (["SRR0001000"], "Please provide at least one database file to search (-d)\n"),
    (["-d", "empty", "SRR0001000"], "Please provide at least one database file to search (-d)\n"),
    (["-d", BASIC, "SRR0001000", "-s", "NOSUCH42", "SRR0001001"], "No sample with the run accession NOSUCH42 in the database\n"),
    (["-d", BASIC, "srr0001000"], "No sample with the run accession srr0001000 in the database\n"),
    # an unknown accession is reported before -o is opened
    (["-d", BASIC, "-o", "no_such_dir/out.txt", "SRR0001000", "NOSUCH42"], "No sample with the run accession NOSUCH42 in the database\n"),
    (["-d", BASIC, "-k", "0"], "Please provide: 1 <= -k <= 1024 (got \"0\")\n"),                 # -k before the accessions
])
def test_kwage_near_argument_errors(kwage_near, tmp_path, args, text):
    (tmp_path / "empty").mkdir()                       # a database directory without a single .db file
    r = run(kwage_near, args, tmp_path)
    assert r.returncode == 1, r
    assert r.stderr == text and r.stdout == ""


@pytest.mark.parametrize("which", EARLY_EXITS)
def test_kwage_near_ends_before_a_device(kwage_near, tmp_path, which):
    check_early_exit(kwage_near, which, ["-s", "SRR0001000"], tmp_path)
