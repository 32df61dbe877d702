"""What every command-line program does alike between its option reader and its first device call: a -d path that does
not exist, an -o that cannot be opened, a database file too short to hold a header.  Exact stderr, exact status, nothing
on stdout, no device (shared by the test_*_cli_args.py files; each names its program and what makes a run valid)."""
import os
import subprocess

from conftest import GOLDEN

BASIC_DB = os.path.join(GOLDEN, "basic", "db")

# HIP_VISIBLE_DEVICES=-1: were a device opened, the run would fail with a device error instead of the message;
# KWAGE_NODE_RANKS: the one-process-per-GPU programs then count no devices either
NO_GPU = {"PATH": "/usr/bin:/bin", "HIP_VISIBLE_DEVICES": "-1", "KWAGE_NODE_RANKS": "1"}

EARLY_EXITS = ["missing_db_path", "output_in_missing_directory", "short_db_file", "db_file_of_header_only"]


def run(exe, args, cwd):
    return subprocess.run([exe] + args, cwd=cwd, capture_output=True, text=True, env=NO_GPU, timeout=60)


def check_early_exit(exe, which, search_args, tmp_path):
    """`search_args`: what a valid run of `exe` has besides -d and -o (-k, a query or an accession)."""
    if which == "missing_db_path":
        args, want = ["-d", "no_such_dir"], "Caught the error FindFiles::next: Unable to stat entry\n"
    elif which == "output_in_missing_directory":
        args, want = ["-d", BASIC_DB, "-o", "no_such_dir/out.txt"], "Unable to open no_such_dir/out.txt for writing\n"
    elif which == "short_db_file":
        (tmp_path / "dbs").mkdir()
        (tmp_path / "dbs" / "x.db").write_bytes(b"abc")
        args, want = ["-d", "dbs"], "dbs/x.db: Unable to read header\nCaught the error main: I/O error\n"
    else:
        (tmp_path / "dbs").mkdir()
        with open(os.path.join(BASIC_DB, "basic.db"), "rb") as fh:
            (tmp_path / "dbs" / "x.db").write_bytes(fh.read(44))          # the header, and not a byte of what it points to
        args, want = ["-d", "dbs"], "dbs/x.db: metadata index lies outside the file\nCaught the error main: Unable to read header\n"
    r = run(exe, args + search_args, tmp_path)
    assert r.returncode == 1 and r.stdout == "", r
    assert r.stderr == want, r.stderr
