"""Directed families of tests/body_shapes.py on the GPU: every family in every scoring mode of the product library against
the numpy restatement (found, nhits, canonical order, score bits), and ONE child process on the counting build that asserts
that the families reached the rare paths they were built for (tests/body_reach.py; profiles/body_shapes/README.md holds a
recorded run of it next to what the generator-based inputs reach)."""
import json
import os
import subprocess
import sys

import pytest

import body_reach
import body_shapes
import join_run
import join_shapes
from conftest import PKG

pytestmark = pytest.mark.gpu

COUNT_LIB = os.path.join(PKG, "libnextsearch_hip_count.so")
# The child's timeout.  The child took 2.2 s on an MI355X before the join families ran in it too (1.8 s of it inside main();
# profiles/body_shapes/README.md holds both times); five times that is 11 s, plus 19 s for what does not scale with the
# work: starting the interpreter, loading the library and the first use of a device that other processes share.
REACH_TIMEOUT_S = 30


@pytest.mark.parametrize("name", list(body_shapes.FAMILIES))
def test_family_equals_numpy_restatement_in_every_mode(name):
    """In-place scoring (OR, AND, merge body on and off, default doc-range cut, the split variant, K around the candidate
    buffer's switch for the families that ask for it), skip tables registered and used / unused, shared term scores
    (NS_INFO_SHARED), packed modes 1 and 2 (NS_INFO_PACKED) and the impact stream (NS_INFO_IMPACTS): one ctx, always released."""
    body_reach.run_family(body_shapes.FAMILIES[name], full=True)


def test_directed_families_reach_their_paths_in_the_counting_build(tmp_path):
    """One fresh child process loads libnextsearch_hip_count.so (built by `make all`), runs every family against the
    restatement again and asserts that every event a family names was counted: pos >= 4 lanes and next-bucket moves for the
    full-bucket families, wrap moves for the wrap families, chunks that continue a bucket for the carry family, every hi
    source, both exhausted-list step kinds and B windows of 1 and 4 chunks for the merge families, shrinks inside a step
    for the flood.  The same child runs the join families of tests/join_shapes.py and one synthetic rank-row case: every
    join counter a family names is above zero, and the number of queries counted on each of the four join paths EQUALS what
    the family declares (which tests/test_join_shapes_cpu.py pins to the planner): a query that silently took another path
    changes a count."""
    if "count" in os.path.basename(os.environ.get("NS_HIP_LIB", "")):
        pytest.skip("this IS a counting-build process")
    assert os.path.exists(COUNT_LIB), "libnextsearch_hip_count.so is missing: make -C nextsearch-api_amd all"
    out = str(tmp_path / "reach.json")
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "body_reach.py"), out],
                       env=dict(os.environ, NS_HIP_LIB=COUNT_LIB), capture_output=True, text=True, timeout=REACH_TIMEOUT_S)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "reach OK" in r.stdout, tail
    with open(out) as f:
        rep = json.load(f)
    assert not rep["missed"] and set(rep["directed"]) == set(body_shapes.FAMILIES)
    for name, fn in body_shapes.FAMILIES.items():
        for e in fn.events:
            assert rep["directed"][name]["events"][e] > 0, (name, e)
    join = rep["join"]
    assert set(join["families"]) == set(join_shapes.FAMILIES)
    for name, fn in join_shapes.FAMILIES.items():
        got, fam = join["families"][name], fn()
        for e in fam.events:
            assert got["events"][e] > 0, (name, e)
        assert [got["events"][p] for p in join_shapes.PATHS] == join_run.predicted_path_counts(name, got["batches_at_k"]), name
        assert sorted(set(got["batches_at_k"])) == sorted(fam.ks)
    assert {e for fn in join_shapes.FAMILIES.values() for e in fn().events} | {"rank_join", "rank_join_tie_rounds"} == set(join_shapes.JOIN_EVENTS)
    assert join["rank_join"]["events"]["rank_join"] == join_shapes.RANK_QUERIES and join["rank_join"]["events"]["rank_join_tie_rounds"] > 0
    keep = os.environ.get("NS_REACH_JSON")   # a recorded run for profiles/body_shapes/
    if keep:
        with open(keep, "w") as f:
            json.dump(rep, f, indent=1, sort_keys=True)
