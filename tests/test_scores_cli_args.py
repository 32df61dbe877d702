"""kwage_scores' usage and argument errors (no GPU): the program ends with its message before any device is opened, and
prints nothing on stdout.  It has kwage's -d, -i, -o and positional sequences; a -t or a -k shows the usage text."""
import subprocess

import pytest

from cli_early_exits import EARLY_EXITS, check_early_exit

USAGE = ("Usage for kwage_scores (every query's match count for every sample, tab-separated):\n"
         "\t[-o <output file>] (default is stdout)\n"
         "\t-d <database search path> (can be repeated)\n"
         "\t[-i <input sequence file>] (can be repeated)\n"
         "\t[<DNA sequence>] (can be repeated)\n"
         "\t(the whole matrix, queries x samples x 4 bytes, is held in host memory until it is printed)\n")


@pytest.fixture(scope="module")
def kwage_scores():
    from kwage_amd import native
    native.ensure_built()
    return native.KWAGE_SCORES_BIN


def run(exe, args, cwd):
    # HIP_VISIBLE_DEVICES=-1: were a device opened, the run would fail with a device error instead of the message
    return subprocess.run([exe] + args, cwd=cwd, capture_output=True, text=True,
                          env={"PATH": "/usr/bin:/bin", "HIP_VISIBLE_DEVICES": "-1"}, timeout=60)


@pytest.mark.parametrize("args, status", [
    ([], 1),
    (["-h"], 0),
    (["-t", "0.5", "-d", "db", "ACGT"], 1),
    (["-k", "5", "-d", "db", "ACGT"], 1),
    (["--o.csv", "-d", "db", "ACGT"], 1),
    (["-d"], 1),
])
def test_kwage_scores_usage(kwage_scores, tmp_path, args, status):
    (tmp_path / "db").mkdir()
    r = run(kwage_scores, args, tmp_path)
    assert r.returncode == status, r
    assert r.stderr == USAGE and r.stdout == ""


@pytest.mark.parametrize("args, text", [
    (["-d", "db", "ACGT"], "Please provide at least one database file to search (-d)\n"),
    (["ACGT"], "Please provide at least one database file to search (-d)\n"),
    (["-d", "db"], "Please provide at least one query sequence or file\n"),
    (["-d", "db", "-i", "reads.txt"], "The query sequence file name, reads.txt, does not have an allowed file extension\n"),
    (["-d", "db", "-i", "reads.fa.fa"], "The query sequence file name, reads.fa.fa, does not have an allowed file extension\n"),
])
def test_kwage_scores_argument_errors(kwage_scores, tmp_path, args, text):
    (tmp_path / "db").mkdir()                          # a database directory without a single .db file
    r = run(kwage_scores, args, tmp_path)
    assert r.returncode == 1, r
    assert r.stderr == text and r.stdout == ""


@pytest.mark.parametrize("which", EARLY_EXITS)
def test_kwage_scores_ends_before_a_device(kwage_scores, tmp_path, which):
    check_early_exit(kwage_scores, which, ["ACGT"], tmp_path)
