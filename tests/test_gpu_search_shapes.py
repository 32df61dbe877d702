"""kwage_search at every gather-kernel instantiation of engine.hip, against the CPU oracle.

The cases are the table of search_shapes.py (CASES): each one asserts the exact name it reports, compares the whole hit
list (query, column, num_match in (query, column) order) and every query's k-mer count with the oracle's, and each test
checks at its end that it reached all the instantiations of its family.  After every persistent or early-exit form the
exchange buffers must read zero again.

The groups, the batches, the oracle's expectation and the run of one case are search_groups.py's (shared with
test_gpu_search_holes.py, which runs the table again on groups with dead columns): every group here is one block without a
hole.  KWAGE_SEARCH_FULL_GRID=1 adds the threshold sweep and the list-capacity and unit-length knob variants."""
import pytest

import search_shapes as ss
from search_groups import Env, run_family

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ka():
    import kwage_amd as ka
    from kwage_amd import native
    native.ensure_built()
    return ka


@pytest.fixture(scope="module")
def env(ka, oracle):
    e = Env(ka, oracle)
    yield e
    e.close()


def test_and_narrow(env):
    run_family(env, ss.CASES, "and_narrow")


def test_and_screen_then_refine(env):
    run_family(env, ss.CASES, "and_screen")


def test_and_walk(env):
    run_family(env, ss.CASES, "and_walk")


def test_and_band_walk(env):
    run_family(env, ss.CASES, "and_band_walk")


def test_and_kernel(env):
    run_family(env, ss.CASES, "and_kernel")


def test_count_screen_then_refine(env):
    run_family(env, ss.CASES, "count_screen")


def test_count_walk_truncated_then_refine(env):
    run_family(env, ss.CASES, "count_walk_trunc")


def test_count_walk(env):
    run_family(env, ss.CASES, "count_walk_pf")


def test_count_kernel(env):
    run_family(env, ss.CASES, "count_kernel")


def test_count_segments_and_combine(env):
    run_family(env, ss.CASES, "count_segments")


def test_count_narrow(env):
    run_family(env, ss.CASES, "count_narrow")
