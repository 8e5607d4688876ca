"""The corrector's and completion's kernels (csrc/ns_fuzzy.hip) on the directed families of
tests/fuzzy_shapes.py.

1. Each family through raw ns_ac_fuzzy / ns_ac_fuzzy_prefix on the product library, in this process, against the restatements
   tests/correct_ref.py and tests/complete_ref.py: exact in index, distance, count and the ~0u / 0xff tails.
2. ONE child process on the counting build runs all families again and reports ns_debug_fuzzy_counters per family: every
   event a family was built for was reached, and the counts that depend on the table and the queries alone (candidates given
   to the signature test, candidates it rejected, entries the build dropped) equal their restatements exactly."""
import json
import os
import subprocess
import sys

import pytest

import fuzzy_shapes
from conftest import PKG

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT_LIB = os.path.join(PKG, "libnextsearch_hip_count.so")
# A child loads a library, creates a context and runs six small families, 2052 of the calls with one query each.  Measured on an
# MI355X host: 7.7 s in all, most of it the restatement in Python (which alone took 20 s on a slower host CPU).  The limit stays at
# the 30 s of the other children; a family that needs more is made smaller, the limit is not raised.
CHILD_TIMEOUT_S = 30
IN_TEST_BUILD = os.path.basename(os.environ.get("NS_HIP_LIB", "")) not in ("", "libnextsearch_hip.so")


@pytest.mark.parametrize("name", fuzzy_shapes.FAMILIES)
def test_family_equals_the_restatement(name):
    fuzzy_shapes.run_family(name)


def test_the_families_reach_their_paths_in_the_counting_build(tmp_path):
    if IN_TEST_BUILD:
        pytest.skip("this IS a test-build process")
    assert os.path.exists(COUNT_LIB), "libnextsearch_hip_count.so is missing: make -C nextsearch-api_amd all"
    out = str(tmp_path / "fuzzy.json")
    env = dict(os.environ, NS_HIP_LIB=COUNT_LIB)
    env.pop("NS_FUZZY_NO_SIG", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzzy_shapes.py"), out], env=env, capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT_S)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "fuzzy shapes OK" in r.stdout, tail
    with open(out) as f:
        rep = json.load(f)
    print(json.dumps(rep["events"], sort_keys=True))
    assert rep["counting"] and not rep["missed"], rep
    for name in fuzzy_shapes.FAMILIES:
        ev = rep["events"][name]
        for e in fuzzy_shapes.REACHED[name]:
            assert ev[e] > 0, (name, e, ev)
    # what does not depend on how the work is cut, exactly
    assert set(rep["exact"]["queue"]) == {"sig_tested", "sig_rejected"}
    assert set(rep["exact"]["build"]) == {"build_dropped_zero", "build_dropped_repeat"}
    for name, pairs in rep["exact"].items():
        for e, (got, want) in pairs.items():
            assert got == want, (name, e, got, want)
    assert rep["exact"]["queue"]["sig_tested"][1] == 4 * 1024 * 1024
    # anagrams, per call (corrector, then completion): the near candidate's wave runs every row beside 63 dead lanes while the
    # other three waves leave early; with nothing near all four do (tests/test_fuzzy_shapes_cpu.py derives both from the rows' minima)
    for near, none in (rep["anagrams_calls"][0:2], rep["anagrams_calls"][2:4]):
        assert near["dp_early_exit"] == 3 and none["dp_early_exit"] == 4, (near, none)
        assert near["dp_dead_lane_rows"] > 0
        assert near["dp_full_waves"] == none["dp_full_waves"] == 4 and near["sig_rejected"] == none["sig_rejected"] == 0
    # the other events are reached somewhere too
    total = {e: sum(rep["events"][n][e] for n in fuzzy_shapes.FAMILIES) for e in fuzzy_shapes.FUZZY_EVENTS}
    assert all(v > 0 for v in total.values()), total
