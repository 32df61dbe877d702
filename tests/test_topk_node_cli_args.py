"""kwage_top_node's command line without a GPU: its argument handling is kwage_top's (return code, stdout, stderr) on
kwage_top's hostile argument lines, and KWAGE_NODE_PLAN=1 prints kwage_node's plan.  Neither may open a device.  Also
kwage_node's argument handling, which is kwage's, and how the two end before a device."""
import os
import subprocess

import pytest

from cli_early_exits import EARLY_EXITS, check_early_exit
from conftest import GOLDEN, ROOT

BIN = os.path.join(ROOT, "kwage_amd", "bin")
TOP, TOP_NODE, NODE, KWAGE = (os.path.join(BIN, n) for n in ("kwage_top", "kwage_top_node", "kwage_node", "kwage"))

# HIP_VISIBLE_DEVICES=-1: were a device opened, the run would fail with a device error instead of the message
NO_GPU = {"PATH": "/usr/bin:/bin", "HIP_VISIBLE_DEVICES": "-1", "KWAGE_NODE_RANKS": "1"}


@pytest.mark.parametrize("args", [
    [], ["-h"], ["-?"],
    ["-d", "db", "ACGT"],
    ["-k", "0", "-d", "db", "ACGT"],
    ["-k", "1025", "-d", "db", "ACGT"],
    ["-k", "abc", "-d", "db", "ACGT"],
    ["-k", "-3", "-d", "db", "ACGT"],
    ["-d", "db", "ACGT", "-k"],
    ["-k", "5", "-t", "1.5", "-d", "db", "ACGT"],
    ["-k", "5", "-t", "-0.5", "-d", "db", "ACGT"],
    ["-k", "5", "-d", "no_such_dir", "ACGT"],
    ["-k", "5", "-d", "db"],
    ["-k", "5", "-d", "db", "-i", "reads.txt"],
    ["-k", "5", "--o.cs", "-d", "db", "ACGT"],
])
def test_top_node_argument_handling_is_kwage_tops(args):
    cdir = os.path.join(GOLDEN, "basic")
    a = subprocess.run([TOP] + args, cwd=cdir, capture_output=True, env=NO_GPU, timeout=60)
    b = subprocess.run([TOP_NODE] + args, cwd=cdir, capture_output=True, env=NO_GPU, timeout=60)
    assert (b.returncode, b.stdout, b.stderr) == (a.returncode, a.stdout, a.stderr), args


@pytest.mark.parametrize("ranks, budget", [(1, None), (3, None), (5, None), (2, "200000")])
def test_top_node_plan_is_kwage_nodes(ranks, budget):
    cdir = os.path.join(GOLDEN, "multi")
    env = dict(NO_GPU, KWAGE_NODE_RANKS=str(ranks), KWAGE_NODE_PLAN="1")
    if budget:
        env["KWAGE_MAX_GROUP_BYTES"] = budget
    a = subprocess.run([NODE, "-d", "dbs", "ACGT"], cwd=cdir, capture_output=True, env=env, timeout=60)
    b = subprocess.run([TOP_NODE, "-k", "4", "-d", "dbs", "ACGT"], cwd=cdir, capture_output=True, env=env, timeout=60)
    assert a.returncode == 0 and a.stdout.startswith(b'{"ranks": '), a.stderr
    assert (b.returncode, b.stdout, b.stderr) == (a.returncode, a.stdout, a.stderr)


@pytest.mark.parametrize("args", [
    [], ["-h"], ["-?"], ["--bogus"],
    ["-d", "no_such_dir", "ACGT"],                          # the database walk comes first ...
    ["-d", "no_such_dir", "-t", "2"],
    ["-d", "reads.txt", "-t", "2", "-i", "reads.txt"],      # ... then no database, no query, the name, the threshold
    ["-d", "db", "-t", "2", "-i", "reads.txt"],
    ["-d", "db", "-t", "2", "-i", "reads.txt", "ACGT"],
    ["-d", "db", "-t", "0", "ACGT"],
    ["-d", "db", "-t", "abc", "ACGT"],
    ["ACGT", "-d", "db", "-t"],
    ["--o.cs", "-d", "db"],
])
def test_node_argument_handling_is_kwages(args):
    cdir = os.path.join(GOLDEN, "basic")
    a = subprocess.run([KWAGE] + args, cwd=cdir, capture_output=True, env=NO_GPU, timeout=60)
    b = subprocess.run([NODE] + args, cwd=cdir, capture_output=True, env=NO_GPU, timeout=60)
    assert (b.returncode, b.stdout, b.stderr) == (a.returncode, a.stdout, a.stderr), args
    assert a.stdout == b"" and a.stderr != b""


@pytest.mark.parametrize("program", [KWAGE, NODE], ids=["kwage", "kwage_node"])
@pytest.mark.parametrize("which", EARLY_EXITS)
def test_kwage_and_kwage_node_end_before_a_device(program, tmp_path, which):
    check_early_exit(program, which, ["ACGT"], tmp_path)
