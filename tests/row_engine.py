"""The Engine leg of the shared-top-rows tests: a text search through nsbind.Engine that takes rows, against the C oracle.

Run as a script on the counting build by tests/test_row_sharing_gpu.py, in a process of its own, with NS_SHARE=2,
NS_SHARE_ROWS=2 and NS_ROW_MIN_USERS=1 in the environment (ns_ctx_create reads them: every batch shares its term scores and
every thin group whose hot list has a skip table takes rows).  It generates an index with the repository's generator, runs a
batch of BASELINE's cfg5 law — reduced as tests/test_gpu_parity.py::test_config_shaped_workloads_reduced reduces it — through
Engine.search_batch, compares it with the oracle the way that test does, and writes the consumer's counters."""
import json
import os
import sys

import numpy as np

DOCS, QUERIES = 60_000, 256


def main(out_path, index_dir):
    import nsbind
    import orc
    import row_shapes
    import workloads
    assert hasattr(nsbind.hip_lib(), "ns_debug_counters"), "not the counting build"
    assert os.environ.get("NS_SHARE_ROWS") == "2" and os.environ.get("NS_SHARE") == "2"
    gen, _, k, flags, (nseg, _) = workloads.WORKLOADS["cfg5"]
    nsbind.gen_index(index_dir, nseg, DOCS, 65536, 1337, False)
    queries = gen(QUERIES)
    eng, ora = nsbind.Engine(index_dir, 0), orc.Oracle(index_dir)
    try:
        nsbind.debug_counters(reset=True)
        gh, gn, gf, gu = eng.search_batch(queries, k, flags)
        cnt = nsbind.debug_counters(reset=True)["ns_debug_counters"]
        oh, on, of, ou = ora.search_batch(queries, k, flags)
    finally:
        eng.close()
        ora.close()
    # as tests/test_gpu_parity.py's assert_same
    np.testing.assert_array_equal(gu.astype(bool), ou.astype(bool))
    for q in range(len(queries)):
        if not ou[q]:
            assert gn[q] == 0
            continue
        assert int(gf[q]) == int(of[q]), ("found", q, queries[q], int(gf[q]), int(of[q]))
        assert int(gn[q]) == int(on[q]), ("nhits", q, queries[q])
        n = int(on[q])
        g, o = gh[q, :n], oh[q, :n]
        bad = np.nonzero((g["doc"] != o["doc"]) | (g["seg"] != o["seg"]) | (g["score"].view(np.uint32) != o["score"].view(np.uint32)))[0]
        assert bad.size == 0, ("query", q, queries[q], "rank", int(bad[0]), g[bad[0]], o[bad[0]])
        assert np.all(gh[q, n:]["doc"] == 0xFFFFFFFF) and np.all(np.isneginf(gh[q, n:]["score"]))
    rep = {e: cnt[i] for e, i in row_shapes.EVENTS.items()}
    rep.update(docs=DOCS, queries=QUERIES, k=k)
    with open(out_path, "w") as f:
        json.dump(rep, f, indent=1, sort_keys=True)
    print("rows engine OK", rep)


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "nextsearch-api_amd"))
    sys.path.insert(0, here)
    main(sys.argv[1], sys.argv[2])
