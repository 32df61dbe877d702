"""`kwage_top_node`: kwage_top's command line as one process per GPU (kwage_amd/csrc/kwage_top_node.cpp).  Its report
must be kwage_top's, byte for byte, for any rank count and any pass count: the per-rank top-k lists carry global column
numbers, are merged on the device under the file-order tie table, and are folded across passes on rank 0.  One rank
runs over RCCL; 2, 3 and 5 ranks are rehearsed on device 0 (KWAGE_NODE_REHEARSE=1: the lists travel through a shared
host segment, and rank 0 merges the R lists on the device as it does over RCCL)."""
import os
import re
import subprocess

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "kwage_amd", "bin")
TOP = os.path.join(BIN, "kwage_top")
TOP_NODE = os.path.join(BIN, "kwage_top_node")

# (fixture, arguments): the three reference-written fixtures, each at its own k, threshold and format
CASES = {
    "basic": ["-d", "db", "-i", "q.fa", "-k", "3", "-t", "0.5", "--o.csv",
              "CGGTGTATGTCTTAGTAAATTGTTCAGGACAACTTGTACCCTACTAGGAGGCAGCCGTGTTTGTAAGGCTATTTTGACGTACCGTACTAACATAGCGGCT", "ACGTNACGT"],
    "multi": ["-d", "dbs", "-i", "reads.fastq", "-i", "contigs.fa.gz", "-k", "5", "--o.json"],
    "k32": ["-d", "k32.db", "-i", "q.fna", "-k", "2", "-t", "0.6", "--o.csv"],
}


def _env(**extra):
    env = dict(os.environ, KWAGE_NODE_RANKS="1")
    env.update(extra)
    env.pop("NCCL_DEBUG", None)
    return env


def _secs(b):
    return re.sub(rb"in \d+ sec", b"in N sec", b)


@pytest.fixture(scope="module")
def want():
    out = {}
    for name, args in CASES.items():
        r = subprocess.run([TOP] + args, cwd=os.path.join(GOLDEN, name), capture_output=True, timeout=120)
        assert r.returncode == 0 and r.stdout, r.stderr.decode()
        out[name] = r
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_top_node_report_is_kwage_tops(want, name):
    cdir = os.path.join(GOLDEN, name)
    for ranks in (1, 2, 3, 5):
        extra = {"KWAGE_NODE_REHEARSE": "1"} if ranks > 1 else {}
        r = subprocess.run([TOP_NODE] + CASES[name], cwd=cdir, capture_output=True, timeout=120, env=_env(KWAGE_NODE_RANKS=str(ranks), **extra))
        assert r.returncode == 0, (ranks, r.stderr.decode())
        assert r.stdout == want[name].stdout, (name, ranks)
        assert _secs(r.stderr) == _secs(want[name].stderr), (name, ranks)


def test_top_node_batches_passes_and_device_merges(want):
    """multi/ has two k-mer lengths (some ranks own no file of a group, with 5 ranks some own nothing): small batches,
    passes, and the stats line showing the device merges with the expected number of sources."""
    cdir = os.path.join(GOLDEN, "multi")
    args = CASES["multi"]
    for ranks, env in ((1, {"KWAGE_BATCH_BASES": "300"}), (3, {"KWAGE_BATCH_BASES": "300"}),
                       (1, {"KWAGE_MAX_GROUP_BYTES": "200000"}), (3, {"KWAGE_MAX_GROUP_BYTES": "200000", "KWAGE_BATCH_BASES": "300"})):
        extra = {"KWAGE_NODE_REHEARSE": "1"} if ranks > 1 else {}
        r = subprocess.run([TOP_NODE] + args, cwd=cdir, capture_output=True, timeout=120,
                           env=_env(KWAGE_NODE_RANKS=str(ranks), KWAGE_NODE_STATS="1", **extra, **env))
        assert r.returncode == 0, r.stderr.decode()
        assert r.stdout == want["multi"].stdout, (ranks, env)
        err = r.stderr.decode()
        m = re.search(r"rank 0: (\d+) batches, (\d+) pass\(es\); exchange merges (\d+) of (\d+) sources, (\d+) records merged", err)
        assert m, err
        batches, passes, merges, sources, records = (int(x) for x in m.groups())
        assert sources == ranks and merges >= 1 and records >= 1, err
        if "KWAGE_BATCH_BASES" in env:
            assert batches >= 4, err                        # several exchanges
        passes_seen = [int(x) for x in re.findall(r"bytes per pass, (\d+) pass\(es\)", err)]
        assert len(passes_seen) == ranks and len(set(passes_seen)) == 1 and passes_seen[0] == passes, err
        local = [int(x) for x in re.findall(r"local merges (\d+)", err)]
        assert len(local) == ranks, err
        if "KWAGE_MAX_GROUP_BYTES" in env:
            assert passes >= 2, err
        elif ranks == 1:
            assert local[0] == batches, err                 # one rank holds all three groups: its list is merged before the exchange


def test_top_node_a_failing_rank_ends_the_run():
    cdir = os.path.join(GOLDEN, "multi")
    r = subprocess.run([TOP_NODE, "-d", "dbs", "-i", "reads.fastq", "-k", "5"], cwd=cdir, capture_output=True, timeout=120,
                       env=_env(KWAGE_NODE_RANKS="2", KWAGE_NODE_REHEARSE="1", KWAGE_NODE_REHEARSE_RECORDS="1"))
    assert r.returncode != 0 and b"rehearsal segment is too small" in r.stderr
