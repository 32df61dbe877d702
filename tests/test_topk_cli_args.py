"""kwage_top's and kwage_top_node's usage and argument errors (no GPU): the usage text, a missing, zero, too large or
non-numeric -k, a threshold outside [0, 1], a bad query file name, no query, no database -- the first complaint that
applies, in that order, ends the program with its exact message and status before any device is opened."""
import pytest

from cli_early_exits import EARLY_EXITS, check_early_exit, run

USAGE = ("Usage for kwage_top (the k best-scoring samples per query):\n"
         "\t-k <number of samples per query> (1 to 1024)\n"
         "\t[-o <output file>] (default is stdout)\n"
         "\t[--o.csv (output CSV) | --o.json (output JSON)]\n"
         "\t[-t <search threshold>] (default is 0: the k best, whatever their score)\n"
         "\t-d <database search path> (can be repeated)\n"
         "\t[-i <input sequence file>] (can be repeated)\n"
         "\t[<DNA sequence>] (can be repeated)\n")
NO_K = "Please provide the number of samples per query (-k)\n"
BAD_K = "Please provide: 1 <= -k <= 1024 (got \"%s\")\n"
BAD_T = "Please provide: 0.0 <= search threshold <= 1.0\n"
BAD_NAME = "The query sequence file name, reads.txt, does not have an allowed file extension\n"
NO_QUERY = "Please provide at least one query sequence or file\n"
NO_DB = "Please provide at least one database file to search (-d)\n"


@pytest.fixture(scope="module")
def kwage_top():
    from kwage_amd import native
    native.ensure_built()
    return native.KWAGE_TOP_BIN


@pytest.fixture(scope="module", params=["kwage_top", "kwage_top_node"])
def program(request, kwage_top):
    from kwage_amd import native
    return {"kwage_top": kwage_top, "kwage_top_node": native.KWAGE_TOP_NODE_BIN}[request.param]


def exact_message(args, text):
    """The whole line that a case of test_kwage_top_argument_errors names by a piece of it."""
    if text == "-k":
        return NO_K
    if text == "threshold":
        return BAD_T
    return BAD_K % (args + [""])[args.index("-k") + 1]


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
    r = run(kwage_top, args, tmp_path)
    assert r.returncode == 1, r
    assert r.stderr == exact_message(args, text), r.stderr
    assert r.stdout == ""


@pytest.mark.parametrize("args, status, stderr", [
    ([], 1, USAGE),
    (["-h"], 0, USAGE),
    (["--bogus"], 0, USAGE),
    (["-k", "5", "-d", "db", "ACGT", "-x"], 0, USAGE),
    (["-k", "0", "-t", "2", "-d", "db", "ACGT"], 1, BAD_K % "0"),                  # the -k line only
    (["-t", "2", "-i", "reads.txt"], 1, NO_K),
    (["-k", "5", "-t", "2", "-i", "reads.txt", "-d", "db"], 1, BAD_T),            # the threshold before the name
    (["-k", "5", "-t", "nan", "-d", "db", "ACGT"], 1, BAD_T),
    (["-k", "5", "-d", "db", "-i", "reads.txt"], 1, BAD_NAME),                    # the name before the empty database
    (["-k", "5", "-d", "db"], 1, NO_QUERY),
    (["-k", "5", "-d", "db", "ACGT"], 1, NO_DB),
    (["-k", "5", "ACGT"], 1, NO_DB),
    (["-k", "5", "-t", "0", "-d", "db", "ACGT"], 1, NO_DB),                       # t = 0 is allowed here
    (["-k", "5", "--o.cs", "-d", "db", "ACGT"], 1, NO_DB),                        # an abbreviated long option is taken
])
def test_top_usage_and_order_of_complaints(program, tmp_path, args, status, stderr):
    (tmp_path / "db").mkdir()                          # a database directory without a single .db file
    r = run(program, args, tmp_path)
    assert (r.returncode, r.stderr, r.stdout) == (status, stderr, ""), r


@pytest.mark.parametrize("which", EARLY_EXITS)
def test_top_ends_before_a_device(program, tmp_path, which):
    check_early_exit(program, which, ["-k", "5", "ACGT"], tmp_path)
