"""The sub-batch loop of the eleven batch calls (host/engine.cpp: for_each_sub_batch, ranked_batch): a batch cut into three
sub-batches answers as the same batch in one piece, byte for byte.

NS_SUBBATCH is read once per process and a batch is cut from Q >= 2 x NS_SUBBATCH, so the cut run is a child process started
with NS_SUBBATCH=64; this process, where one sub-batch covers the 130 queries, gives the expected arrays and the cursors."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nextsearch-api_amd"))
import nsbind  # noqa: E402

pytestmark = pytest.mark.gpu

SUB = 64
K = 3
CHILD_TIMEOUT_S = 60
DIALECTS = ("boolean", "grouped", "quorum")


def queries():
    t = lambda i: "t%06d" % (i % 48)
    qs = []
    for i in range(130):
        a, b, c, d = t(i), t(3 * i + 1), t(5 * i + 2), t(7 * i + 3)
        qs.append((f"{a} {b} {c}", f"+{a} {b} -{d}", f"+({a} {b}) {c}", f"{a} {b} {c} ~2", f"+({a} {b} {c})~2 {d}", f"{a} zzzzqq", f"+zzzzqq {a}", "", "the of",
                   f"-{a}")[i % 10])
    return qs


def filter_bits():
    return [np.array([0x5B6DB6DB, 0x1B6D], dtype=np.uint32), np.array([0xDB6DB6DB, 0x0DB6], dtype=np.uint32)]   # 45 documents a segment


def calls(eng, handle, n_buckets):
    """name -> (kind, call(after)); kind: 's' score order, 'd' date order, 'f' facets"""
    qs = queries()
    out = {"search_or": ("s", lambda after: eng.search_after_batch(qs, K, after, nsbind.NS_FLAG_OR, handle)),
           "search_and": ("s", lambda after: eng.search_after_batch(qs, K, after, nsbind.NS_FLAG_AND, handle)),
           "sorted": ("d", lambda after: eng.search_sorted_after_batch(qs, K, after, "newest", nsbind.NS_FLAG_OR, handle))}
    for d in DIALECTS:
        out[d + "_after"] = ("s", lambda after, d=d: getattr(eng, f"search_{d}_after_batch")(qs, K, after, handle))
        out[d + "_facet"] = ("f", lambda after, d=d: getattr(eng, f"facet_{d}_batch")(qs, n_buckets, "year", handle))
        out[d + "_sorted"] = ("d", lambda after, d=d: getattr(eng, f"search_{d}_sorted_batch")(qs, K, after, "oldest", handle))
    assert len(out) == 12   # the eleven calls, search_after in both of its modes
    return out


def cursors_of(kind, first):
    """every third query's first hit of page 1 as its cursor"""
    hits, nhits = first[0], first[2 if kind == "d" else 1]
    rank = first[1] if kind == "d" else hits["score"].view(np.uint32)
    return [(int(rank[q, 0]), int(hits[q, 0]["seg"]), int(hits[q, 0]["doc"])) if q % 3 == 1 and nhits[q] else None for q in range(len(nhits))]


def run(index, cursors):
    """-> ({"<filtered|whole>.<call>.<i>": array}, cursors); cursors None: taken from the first pages"""
    eng = nsbind.Engine(index, 0)
    arrays, taken = {}, {}
    try:
        n_buckets = len(eng.facet_buckets("year")[1])
        for where in ("whole", "filtered"):
            handle = eng.open_filter(bits=filter_bits()) if where == "filtered" else 0
            for name, (kind, call) in calls(eng, handle, n_buckets).items():
                key = where + "." + name
                after = None
                if kind != "f":
                    after = cursors[key] if cursors is not None else cursors_of(kind, call(None))
                    taken[key] = after
                for i, a in enumerate(call(after)):
                    arrays[f"{key}.{i}"] = np.ascontiguousarray(a)
            if handle:
                eng.close_filter(handle)
    finally:
        eng.close()
    return arrays, taken


def test_a_batch_cut_into_sub_batches_answers_as_the_batch_in_one_piece(tmp_path):
    index, cur_file, out_file = str(tmp_path / "index"), str(tmp_path / "cursors.json"), str(tmp_path / "cut.npz")
    nsbind.gen_index(index, 2, 45, 512, 77, False)
    whole, cursors = run(index, None)
    Q = len(queries())
    n_sub = (Q + SUB - 1) // SUB
    assert Q >= 2 * SUB and n_sub == 3                        # the child cuts the batch: [0, 43), [43, 86), [86, 130)
    behind = {key: sum(c is not None for c in cur[Q // n_sub:]) for key, cur in cursors.items()}
    assert len(behind) == 18 and all(n > 0 for n in behind.values()), behind   # every paged call has cursors behind the first sub-batch
    assert max(sum(c is not None for c in cur) for cur in cursors.values()) >= Q // 6, cursors
    assert any(np.any(whole[k] == 0) for k in whole if k.endswith("_after.4")) and any(np.any(whole[k] != 0) for k in whole if k.endswith("_after.4"))   # has_found
    with open(cur_file, "w") as f:
        json.dump(cursors, f)
    env = dict(os.environ, NS_SUBBATCH=str(SUB))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), index, cur_file, out_file], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    assert r.returncode == 0 and "sub-batch child OK" in r.stdout, (r.stdout + r.stderr)[-3000:]
    with np.load(out_file) as cut:
        assert sorted(cut.files) == sorted(whole)
        for key in whole:
            assert cut[key].dtype == whole[key].dtype and cut[key].shape == whole[key].shape and cut[key].tobytes() == whole[key].tobytes(), key


if __name__ == "__main__":
    assert os.environ.get("NS_SUBBATCH") == str(SUB)
    with open(sys.argv[2]) as f:
        given = {k: [None if c is None else tuple(c) for c in v] for k, v in json.load(f).items()}
    got, _ = run(sys.argv[1], given)
    np.savez(sys.argv[3], **got)
    print("sub-batch child OK")
