"""The shapes of tests/window_shapes.py on the GPU: every shape in every mode of the product library against the numpy
restatement (every hit, nhits, found, the padding; OR and AND; K = 1, 10, 33, 100; whole groups and a forced split; scoring
in place, shared term scores, the impact stream), and ONE child process on the counting build that sets the foreign-window
counters of the first general and the first thin shape against the lists and against tools/dbg/window_sim.py
(tests/foreign_reach.py).  tests/test_window_shapes_cpu.py asserts the class of every group through the plan harness."""
import json
import os
import subprocess
import sys

import pytest

import foreign_reach
import window_shapes
from conftest import PKG

pytestmark = pytest.mark.gpu

COUNT_LIB = os.path.join(PKG, "libnextsearch_hip_count.so")
REACH_TIMEOUT_S = 30   # as tests/test_body_shapes_gpu.py: the child's work is two small batches; the rest is start-up on a shared device


@pytest.mark.parametrize("name", list(window_shapes.SHAPES))
def test_shape_equals_numpy_restatement_in_every_mode(name):
    foreign_reach.run_shape(window_shapes.SHAPES[name])


def test_windows_consume_every_posting_once_and_are_used_as_the_model_says(tmp_path):
    if "count" in os.path.basename(os.environ.get("NS_HIP_LIB", "")):
        pytest.skip("this IS a counting-build process")
    assert os.path.exists(COUNT_LIB), "libnextsearch_hip_count.so is missing: make -C nextsearch-api_amd all"
    out = str(tmp_path / "windows.json")
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "foreign_reach.py"), out],
                       env=dict(os.environ, NS_HIP_LIB=COUNT_LIB), capture_output=True, text=True, timeout=REACH_TIMEOUT_S)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "windows OK" in r.stdout, tail
    with open(out) as f:
        rep = json.load(f)
    assert set(rep) == set(window_shapes.COUNTED)
    for name, v in rep.items():
        c, s = v["counted"], v["simulated"]
        assert c["consumed"] == v["foreign postings of the lists"] and c["loaded"] <= v["FB"] * c["super_batches"], name
        assert c["utilisation"] >= s["utilisation"] - foreign_reach.UTIL_MARGIN, (name, c, s)
    keep = os.environ.get("NS_WINDOWS_JSON")   # a recorded run for profiles/window_slack/
    if keep:
        with open(keep, "w") as f:
            json.dump(rep, f, indent=1, sort_keys=True)
