"""The numpy checker of the rank join (ns_merge_rank_rows): the global heap over the ranks' rows in the canonical order —
score desc, GLOBAL segment asc, doc asc.  Shared by tests/test_segment_shard.py and the join tests; exercised against brute
force on the CPU by tests/test_join_shapes_cpu.py."""
import numpy as np


def np_join(g_hits, g_nhits, g_found, seg_map, K):
    """g_hits [W, Q, K, 3] (score bits, local seg, doc), g_nhits [W, Q] (clamped to K, as the kernel does), g_found [W, Q],
    seg_map [W, stride] or None (ids are global already) -> per query ([(score bits, global seg, doc)], found)"""
    W, Q = g_nhits.shape
    out = []
    for q in range(Q):
        cand = []
        for r in range(W):
            for i in range(min(int(g_nhits[r, q]), K)):
                bits, seg, doc = (int(x) & 0xFFFFFFFF for x in g_hits[r, q, i])
                score = np.array([bits], dtype=np.uint32).view(np.float32)[0]
                cand.append((-float(score), seg if seg_map is None else int(seg_map[r, seg]), doc, bits))
        cand.sort()
        out.append(([(c[3], c[1], c[2]) for c in cand[:K]], sum(int(x) for x in g_found[:, q])))
    return out
