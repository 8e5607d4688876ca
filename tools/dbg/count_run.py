#!/usr/bin/env python3
"""Diagnostic: event counts of the scoring bodies per query law (needs a GPU).  Runs on the counting build, which
`make -C nextsearch-api_amd all` builds (tests/test_body_shapes_gpu.py asserts on the same counters):
    NS_HIP_LIB=nextsearch-api_amd/libnextsearch_hip_count.so python3 tools/dbg/count_run.py cfg5_gen,cfg5_thin,cfg5
"""
import ctypes as C, os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "nextsearch-api_amd")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import nsbind, law_bench
L = nsbind.hip_lib()
assert hasattr(L, "ns_debug_counters"), "not the counting build: set NS_HIP_LIB to libnextsearch_hip_count.so"
tmp = tempfile.TemporaryDirectory(); idx = os.path.join(tmp.name, "i")
nsbind.gen_index(idx, 1, 1_000_000, 65536, 1337, False)
eng = nsbind.Engine(idx, 0)
laws = law_bench.laws()
names = ["items (driver-stream body)", "super-batches", "super-batches with foreign postings", "foreign postings LOADED (windows)", "foreign postings consumed",
         "foreign chunks", "claim iterations", "rmw term passes", "driver rounds (256 loaded each)", "driver postings consumed", "terms (sum over items)",
         "active foreign terms (sum over sb)", "driver chunks with postings", "driver chunks that probed the table", "driver postings that hit the table", "foreign entries placed WITHOUT a claim (pass A)"]
# the table's rare paths (indices 20 .. 27 of ns_debug_counters), the merge body and the candidate buffer
rare = {20: "pass-A lanes with a full bucket (pos >= 4)", 21: "pass-A chunks that continue the previous chunk's bucket (carry)",
        22: "claim-loop moves to the next bucket", 23: "... of which wrap to bucket 0", 24: "claim-loop lanes that found an owner",
        25: "super-batches without a primary term (wmax < 8)", 26: "super-batches on the T > 8 branch", 27: "span clamps",
        19: "row consumer items (k_rscore)", 28: "row consumer: look-ups of an owner's doc in the hot list", 29: "... that found it",
        30: "row consumer: row entries that probed the table", 31: "... that hit it"}
mnames = ["items (merge body)", "steps", "steps with hi from A's round", "steps with hi from B's window", "steps with hi = end of range",
          "steps with a_rem == 0", "steps with b_rem == 0", "B windows of 1 chunk", "B windows of 2 chunks", "B windows of 3 chunks",
          "B windows of 4 chunks", "docs in both lists"]
knames = ["shrinks between steps", "shrinks INSIDE a step", "final shrinks (one per item)"]
for n in (sys.argv[1] if len(sys.argv) > 1 else "cfg5_gen").split(","):
    qs, k = laws[n]
    b = eng.prepare(qs, k)
    nsbind.debug_counters(reset=True)
    b.run(True); b.sync()
    cs = nsbind.debug_counters(reset=True)
    out, tout, mout, kout = cs["ns_debug_counters"], cs["ns_debug_tile_counters"], cs["ns_debug_merge_counters"], cs["ns_debug_topk_counters"]
    inf = b.info()
    sb = max(out[1], 1)
    print(f"{n}: postings {inf.postings}, kernel {inf.last_score_kernel_ms:.3f} ms")
    for i in range(16):
        print(f"    {names[i]:>40}: {out[i]:>12}  ({out[i] / sb:8.2f} per super-batch)")
    for i, nm in rare.items():
        print(f"    {nm:>60}: {out[i]:>12}")
    for nm, v in zip(mnames, mout):
        print(f"    {'merge body: ' + nm:>60}: {v:>12}")
    for nm, v in zip(knames, kout):
        print(f"    {'candidate buffer: ' + nm:>60}: {v:>12}")
    print(f"    foreign window utilisation {out[4] / max(out[3], 1):.3f}; lanes used in foreign chunks {out[4] / max(out[5] * 64, 1):.3f}; "
          f"driver round utilisation {out[9] / max(out[8] * 256, 1):.3f}; lanes used in driver chunks {out[9] / max(out[12] * 64, 1):.3f}; "
          f"foreign share of consumed postings {out[4] / max(out[4] + out[9], 1):.3f}")
    if out[0] and out[17]:
        print(f"    driver-stream body, shader clocks per item: whole {out[17] / out[0]:.0f}, set-up (term table, range searches, first window plan) {out[16] / out[0]:.0f}, final shrink + rows out {out[18] / out[0]:.0f}")
    if tout[0]:
        t = max(tout[1], 1)
        print(f"    doc-tile body: items {tout[0]}, tiles {tout[1]}, (term, tile) visits {tout[2]} ({tout[2] / t:.2f} per tile), rounds {tout[3]} ({tout[3] / max(tout[2], 1):.2f} per visit), "
              f"chunks loaded {tout[4]} ({tout[4] / t:.2f} per tile), postings taken {tout[5]} ({tout[5] / t:.1f} per tile; lanes used {tout[5] / max(tout[4] * 64, 1):.3f}), terms per item {tout[6] / tout[0]:.2f}")
        if tout[9]:
            print(f"    doc-tile body, shader clocks: item {tout[7] / tout[0]:.0f} per item ({tout[7] / max(tout[5], 1) * 64:.0f} per 64 postings); full rounds {tout[9]}: "
                  f"issue -> data {tout[8] / tout[9]:.0f}, whole round {tout[11] / tout[9]:.0f}; tile read-back (+ shrink) {tout[10] / t:.0f} per tile")
    b.close()
