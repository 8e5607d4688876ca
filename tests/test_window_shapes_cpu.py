"""CPU test of tests/window_shapes.py: every shape is planned through tests/plan_harness.cpp and every group takes the
driver-stream class it was sized for, whole and with the forced split the GPU test runs.  No GPU."""
import numpy as np
import pytest

import body_shapes
import rawseg
import window_shapes
from test_batch_plan import SEG_DTYPE, check_exactly_once, harness, plan  # noqa: F401  (harness: fixture)
from test_body_shapes_cpu import WHOLE, body_of, per_query


@pytest.mark.parametrize("name", list(window_shapes.SHAPES))
def test_shape_takes_its_class(name, harness):
    fn = window_shapes.SHAPES[name]
    n, doc_len, lists, queries, idfs, weights = fn()
    assert n == 1 << 17 and len(np.unique(doc_len)) > 100
    flat, offs = rawseg.payload_of(lists)
    qd, refs = rawseg.descriptors(queries, lists, offs, idfs, weights)
    segs = np.zeros(1, SEG_DTYPE)
    segs[0]["n_docs"], segs[0]["n_postings"], segs[0]["norm_safe"] = n, len(flat) // 2, 1
    for q in queries:
        assert body_shapes.plan_rule([len(lists[li][0]) for li in q], n) == fn.cls
        assert q.count(0) == 1 and len(lists[0][0]) > max(len(lists[li][0]) for li in q if li), "list 0 drives"
    for flags in (0, 1):
        for k in (1, 10, 33, 100):
            p = plan(harness, segs, qd, refs, k=k, flags=flags, **WHOLE)
            check_exactly_once(p, segs, len(qd))
            for qi, ws in enumerate(per_query(p, len(queries))):
                assert len(ws) == 1 and int(ws[0]["whole"]) & 1 and body_of(int(ws[0]["whole"])) == fn.cls, (name, qi)
            assert p.n_wide == sum(len(q) > 16 for q in queries)   # 17 terms and more: the 64-term instantiation
            p = plan(harness, segs, qd, refs, k=k, flags=flags, min_items=1, split_postings=window_shapes.SPLIT)
            check_exactly_once(p, segs, len(qd))
            for qi, ws in enumerate(per_query(p, len(queries))):
                assert {body_of(int(w["whole"])) for w in ws} == {fn.cls}, (name, qi)
                assert len(ws) >= 2, (name, qi, len(ws))

