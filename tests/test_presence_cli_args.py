"""kwage_presence's usage and argument errors (no GPU): the program ends with its message before any device is opened,
and prints nothing on stdout.  It has kwage's -d, -i, -o, -t and positional sequences; a -k or a report format shows the
usage text."""
import subprocess

import pytest

from cli_early_exits import EARLY_EXITS, check_early_exit

USAGE = ("Usage for kwage_presence (which samples hold each query: a tab-separated 0/1 matrix):\n"
         "\t[-o <output file>] (default is stdout)\n"
         "\t[-t <search threshold>] (default is 1)\n"
         "\t-d <database search path> (can be repeated)\n"
         "\t[-i <input sequence file>] (can be repeated)\n"
         "\t[<DNA sequence>] (can be repeated)\n"
         "\t(the whole matrix, samples / 8 bytes per query, is held in host memory until it is printed)\n")
BAD_T = "Please provide: 0.0 < search threshold <= 1.0\n"


@pytest.fixture(scope="module")
def kwage_presence():
    from kwage_amd import native
    native.ensure_built()
    return native.KWAGE_PRESENCE_BIN


def run(exe, args, cwd):
    # HIP_VISIBLE_DEVICES=-1: were a device opened, the run would fail with a device error instead of the message
    return subprocess.run([exe] + args, cwd=cwd, capture_output=True, text=True,
                          env={"PATH": "/usr/bin:/bin", "HIP_VISIBLE_DEVICES": "-1"}, timeout=60)


@pytest.mark.parametrize("args, status", [
    ([], 1),
    (["-h"], 0),
    (["-k", "5", "-d", "db", "ACGT"], 1),
    (["--o.csv", "-d", "db", "ACGT"], 1),
    (["-d"], 1),
    (["-d", "db", "ACGT", "-t"], 1),
])
def test_kwage_presence_usage(kwage_presence, tmp_path, args, status):
    (tmp_path / "db").mkdir()
    r = run(kwage_presence, args, tmp_path)
    assert r.returncode == status, r
    assert r.stderr == USAGE and r.stdout == ""


@pytest.mark.parametrize("args, text", [
    (["-t", "0", "-d", "db", "ACGT"], BAD_T),
    (["-t", "1.5", "-d", "db", "ACGT"], BAD_T),
    (["-t", "-0.5", "-d", "db", "ACGT"], BAD_T),
    (["-t", "nan", "-d", "db", "ACGT"], BAD_T),
    (["-t", "x", "-d", "db", "ACGT"], BAD_T),
    (["-d", "db", "ACGT"], "Please provide at least one database file to search (-d)\n"),
    (["-t", "0.8", "ACGT"], "Please provide at least one database file to search (-d)\n"),
    (["-d", "db"], "Please provide at least one query sequence or file\n"),
    (["-d", "db", "-t", "0.8", "-i", "reads.txt"], "The query sequence file name, reads.txt, does not have an allowed file extension\n"),
    (["-t", "0", "-i", "reads.txt", "-d", "db"], BAD_T),                           # the threshold line, not the name line
])
def test_kwage_presence_argument_errors(kwage_presence, tmp_path, args, text):
    (tmp_path / "db").mkdir()                          # a database directory without a single .db file
    r = run(kwage_presence, args, tmp_path)
    assert r.returncode == 1, r
    assert r.stderr == text and r.stdout == ""


@pytest.mark.parametrize("which", EARLY_EXITS)
def test_kwage_presence_ends_before_a_device(kwage_presence, tmp_path, which):
    check_early_exit(kwage_presence, which, ["-t", "0.8", "ACGT"], tmp_path)
