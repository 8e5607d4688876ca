"""The directed families of tests/fuzzy_shapes.py claim what their names say (no GPU): checked here with the restatements
alone, so that a family that stops building its rare case fails here and not silently on the device."""
import random

import complete_ref
import correct_ref
import fuzzy_shapes as fs


def test_event_names_are_one_per_counter():
    assert sorted(fs.FUZZY_EVENTS.values()) == list(range(17)) == list(range(len(fs.FUZZY_EVENTS)))
    assert set(fs.REACHED) == set(fs.FAMILIES) and all(e in fs.FUZZY_EVENTS for t in fs.REACHED.values() for e in t)


def test_signature_counts_equal_the_scalar_rule():
    fam = fs.slices()
    terms, scores = fam["terms"], fam["scores"]
    cand = correct_ref.candidates(terms, scores)
    for q, e in ((fam["q"], 2), (b"a0x", 1), (b"b" * 62 + b"cb", 2), (b"A-b9_", 1)):
        win = [t for i, t in enumerate(terms) if cand[i] and len(q) - e <= len(t) <= len(q) + e]
        assert fs.sig_counts(terms, scores, [q], [e], False) == (len(win), sum(not fs.sig_pass_fuzzy(q, t, e) for t in win))
        win = [t for i, t in enumerate(terms) if cand[i] and len(t) >= len(q) - e]
        assert fs.sig_counts(terms, scores, [q], [e], True) == (len(win), sum(not fs.sig_pass_prefix(q, t, e) for t in win))
        win = [t for t in win if t.startswith(q[:3])]
        assert fs.sig_counts(terms, scores, [q], [e], True, 3) == (len(win), sum(not fs.sig_pass_prefix(q, t, e) for t in win))
    assert fs.sig_pass_prefix(b"zz", b"a" * 67, 0) and not fs.sig_pass_prefix(b"zz", b"a" * 66, 0)


def test_seam_grid_is_covered_and_every_twin_and_edit_is_there():
    fam = fs.seam()
    terms = fam["terms"]
    assert terms == sorted(terms) and len(set(fam["scores"])) == len(terms)
    assert fs.seam_grid(fam) == {(m, r) for m in fs.SEAM_LENGTHS for r in range(4)}
    offs = fs.pool_offsets(terms)
    stems_at = {(len(s), offs[terms.index(s)] % 4) for s in fam["stems"]}
    assert {m for m, _ in stems_at} == set(fs.SEAM_LENGTHS)
    for m in (12, 16, 20):   # a length that is a multiple of 4: a stem of its own at each offset
        assert {r for k, r in stems_at if k == m} == {0, 1, 2, 3}
    fuzzy_q = set(fam["calls"][0][1])
    prefix_q = set(fam["calls"][1][1])
    for s in fam["stems"]:
        m = len(s)
        want = sorted({7, 8, 9, m - 2, m - 1} & set(range(m)))
        assert sorted(fam["twins"][s]) == want
        for x, t in fam["twins"][s].items():
            assert t in terms and len(t) == m and [j for j in range(m) if t[j] != s[j]] == [x]
        kinds = {(k, i) for k, i, _ in fam["edits"][s]}
        for i in sorted({6, 7, 8, 9, m - 2, m - 1} & set(range(m))):
            assert {("del", i), ("ins", i), ("sub", i)} <= kinds and ((("swap", i) in kinds) == (i + 1 < m))
        for k, i, x in fam["edits"][s]:
            assert correct_ref.osa(x, s) == 1 and x in fuzzy_q and {x[:8], x[:9], x[:10], x} <= prefix_q, (k, i)
            assert len(x) == m + {"del": -1, "ins": 1}.get(k, 0)
    (_, fq, fe, _, _, _), (_, pq, pe, _, _, _) = fam["calls"]
    assert fq[:len(fq) // 2] == fq[len(fq) // 2:] and fe == [1] * (len(fq) // 2) + [2] * (len(fq) // 2)      # every string under both bounds
    assert pq[:len(pq) // 2] == pq[len(pq) // 2:] and pe == [1] * (len(pq) // 2) + [2] * (len(pq) // 2)      # and every cut
    assert all(c[3] == 0 and c[4] == 10 for c in fam["calls"])


def test_queue_each_query_has_exactly_one_answer():
    fam = fs.queue()
    terms = fam["terms"]
    assert len(terms) == len(set(terms)) == 1024 and {len(t) for t in terms} == {12} and len(set(fam["scores"])) == 1
    assert sum(set(t) <= set(b"abcdefghijkl") for t in terms) == 512 and sum(set(t) <= set(b"mnopqrstuvwx") for t in terms) == 512
    want = fs.reference("queue")[0]
    assert {key[0] for key in want} == {"fuzzy", "prefix"}
    for (kind, queries, edits, prefix_len, k), answers in want.items():
        assert list(queries) == [t[:5] + b"z" + t[6:] for t in terms] and set(edits) == {2}
        assert answers == [[(p, 1)] for p in range(1024)], kind
    assert [c[0] for c in fam["calls"]] == ["fuzzy", "fuzzy", "prefix", "prefix"] and [c[5] for c in fam["calls"]] == [False, True, False, True]


def test_queue_answers_land_all_over_the_queue():
    """the scan's queue restated over a sample of the queries: both kinds of DP call happen, and the one right answer sits at
    the first and last lane of a full call and of a remainder somewhere in the sample"""
    fam = fs.queue()
    terms = fam["terms"]
    rng = random.Random(1)
    full = rest = tail = rejected = 0
    lanes = set()
    for p in [0, 511, 512, 1023] + rng.sample(range(1024), 124):
        q = fam["queries"][p]
        passes = [fs.sig_pass_fuzzy(q, t, 2) for t in terms]
        assert passes[p]
        f, r, t, where = fs.queue_trace(passes)
        full, rest, tail, rejected = full + f, rest + r, tail + t, rejected + passes.count(False)
        lanes.add(where[p][2])
    assert full > 0 and rest > 0 and tail > 0 and rejected > 0
    assert len(lanes) >= 32 and 0 in lanes and max(lanes) >= 60, sorted(lanes)


def test_anagrams_near_and_far_share_a_wave_and_all_pass_the_signature():
    fam = fs.anagrams()
    terms = fam["terms"]
    assert len(terms) == 256 and {len(t) for t in terms} == {12} and {bytes(sorted(t)) for t in terms} == {b"abcdefghijkl"}
    near = fam["near"]
    run = range(near // 64 * 64, near // 64 * 64 + 64)       # one length, every entry a candidate: slot = index
    assert all(correct_ref.candidates(terms, fam["scores"])) and near in run and run[-1] < len(terms)
    for q in (fam["q_near"], fam["q_none"]):
        assert all(fs.sig_pass_fuzzy(q, t, 2) and fs.sig_pass_prefix(q, t, 2) for t in terms)
        assert fs.queue_trace([True] * 256)[:3] == (4, 0, 0)  # so each wave's DP call is 64 consecutive slots
    far = [i for i in run if i != near]
    assert len(far) == 63 and all(correct_ref.osa(fam["q_near"], terms[i]) > 2 for i in far)
    assert correct_ref.osa(fam["q_near"], terms[near]) == 1
    # the near query: the near candidate's wave runs every row beside 63 lanes that are past the bound, the other three
    # waves leave early; the far query: all four do
    waves = [terms[w:w + 64] for w in range(0, 256, 64)]
    rows = [fs.early_exit_row(fam["q_near"], w) for w in waves]
    assert rows[near // 64] is None and all(r is not None for k, r in enumerate(rows) if k != near // 64)
    assert fs.early_exit_row(fam["q_near"], [terms[i] for i in far]) is not None
    assert all(fs.early_exit_row(fam["q_none"], w) is not None for w in waves)
    want = fs.reference("anagrams")[0]
    for kind in ("fuzzy", "prefix"):
        assert want[(kind, (fam["q_near"], fam["q_none"]), (2, 2), 0, 10)] == [[(near, 1)], []]


def test_keep_every_term_survives_the_dp():
    for fam in fs.tables_of("keep"):
        tab = correct_ref.Table(fam["terms"], fam["scores"])
        assert len(fam["terms"]) == 1296 and len(tab.within(b"aaaa--", 2, 0)[0]) == 1296
        ptab = complete_ref.Table(fam["terms"], fam["scores"])
        assert len(ptab.within(b"zz", 2, 0)[0]) == 1296
    assert fs.keep(False)["scores"] == fs.keep(True)["scores"][::-1] == list(range(1, 1297))


def test_slices_best_ties_straddle_slot_1024():
    fam = fs.slices()
    terms, scores, q = fam["terms"], fam["scores"], fam["q"]
    assert len(terms) == 4097
    tab, ptab = correct_ref.Table(terms, scores), complete_ref.Table(terms, scores)
    assert len(fs.slot_positions(terms, scores, len(q), 2, False)) > 1024
    assert fs.straddles(terms, scores, tab.fuzzy(q, 2, 0, 10), len(q), 2, False)
    assert fs.straddles(terms, scores, ptab.complete(b"zz", 2, 0, 10), 2, 2, True)
    # with the first three bytes fixed the query keeps some answers, all inside one slice: the later slices are empty
    inside = [t for t in terms if t.startswith(q[:3])]
    assert 0 < len(tab.fuzzy(q, 2, 3, 10)) and len(inside) < 1024
    assert sum(len(t) > 66 for t in terms) >= 4               # the bucket past 66 bytes, in every completion query's window
    assert any(c[0] == "fuzzy" and c[3] == 3 for c in fam["calls"]) and any(c[0] == "prefix" and c[3] == 3 for c in fam["calls"])


def test_build_repeats_and_zero_scores_on_both_sides_of_entry_4096():
    fam = fs.build()
    terms, scores = fam["terms"], fam["scores"]
    C = fs.CHUNK
    assert len(terms) == 4400 and terms == sorted(terms)
    assert len(set(terms[C - 3:C + 4])) == 1 and terms[C - 4] != terms[C - 3] and terms[C + 4] != terms[C + 3]   # a run across the chunks
    assert len(set(terms[60:67])) == 1                                                                        # and one across a wave
    repeats = [i for i in range(1, len(terms)) if terms[i] == terms[i - 1]]
    zeros = [i for i, s in enumerate(scores) if s == 0]
    for where in (repeats, zeros):
        assert any(C - 8 <= i < C for i in where) and any(C <= i < C + 8 for i in where)
    assert any(scores[i] == 0 for i in repeats) and any(scores[i] == 0 and terms[i + 1] == terms[i] != terms[i - 1] for i in range(1, 4399))
    for g in range(0, len(terms), 64):
        assert len({len(t) for t in terms[g:g + 64]}) >= 3
    zero, repeat = fs.build_dropped(fam)
    cand = correct_ref.candidates(terms, scores)
    assert zero == len(zeros) > 100 and repeat == sum(scores[i] != 0 for i in repeats) > 5 and zero + repeat + sum(cand) == len(terms)
    # some answer sits next to the chunk boundary, and some is decided among equal scores by the index
    want = fs.reference("build")[0]
    hit = {i for answers in want.values() for a in answers for i, _ in a}
    assert any(C - 8 <= i < C for i in hit) and any(C <= i < C + 8 for i in hit)
    assert any(a[r][1] == a[r + 1][1] and scores[a[r][0]] == scores[a[r + 1][0]] for answers in want.values() for a in answers for r in range(len(a) - 1))
