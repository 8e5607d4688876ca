"""Filtered search, host side (host/filter.hpp, Engine::filter_bits): the date rules and the keep-bitmaps
against a Python restatement, word for word, on a host-only engine.  No device is touched."""
import os
import random
import re

import numpy as np
import pytest

import nsbind

N_SEG, N_PER_SEG = 3, 203            # 203 documents: 6 whole words and 11 bits of a seventh


def py_date_key(text):
    """the rule as the issue states it: blanks stripped; exactly YYYY, YYYY-MM (01..12) or YYYY-MM-DD (01..31)"""
    m = re.fullmatch(r"(\d{4})(?:-(\d{2})(?:-(\d{2}))?)?", text.strip(" \t\r\n\f\v"), flags=re.ASCII)
    if not m:
        return 0
    y, mo, d = int(m.group(1)), int(m.group(2) or 0), int(m.group(3) or 0)
    if m.group(2) is not None and not 1 <= mo <= 12:
        return 0
    if m.group(3) is not None and not 1 <= d <= 31:
        return 0
    return y * 10000 + mo * 100 + d


def py_bound(text, fill):
    """a bound -> key, missing parts = fill; None: open; ValueError: malformed"""
    t = text.strip(" \t\r\n\f\v")
    if not t:
        return None
    if py_date_key(t) == 0:
        raise ValueError(text)
    parts = t.split("-")
    y, mo, d = int(parts[0]), (int(parts[1]) if len(parts) > 1 else fill), (int(parts[2]) if len(parts) > 2 else fill)
    return y * 10000 + mo * 100 + d


DATE_CASES = [
    ("2020", 20200000), ("2020-03", 20200300), ("2020-03-17", 20200317), ("0999-12-31", 9991231), ("2020-01-01", 20200101),
    ("2020-12", 20201200), ("2020-00", 0), ("2020-13", 0), ("2020-03-00", 0), ("2020-03-32", 0), ("2020-03-31", 20200331),
    ("2020-03-17T00:00", 0), ("2020-03-17 x", 0), ("2020 Mar", 0), ("  2020-03 ", 20200300), ("\t2020\r\n", 20200000),
    ("", 0), ("   ", 0), ("20200317", 0), ("2020-3", 0), ("2020-3-17", 0), ("2020/03/17", 0), ("20x0", 0), ("2020-", 0),
    ("2020-03-", 0), ("-2020", 0), ("٢٠٢٠", 0),
]


@pytest.mark.parametrize("text,want", DATE_CASES)
def test_date_key(text, want):
    assert py_date_key(text) == want      # the restatement agrees with the table
    assert nsbind.date_key(text) == want


def write_metadata(index, seed=5):
    """A seeded metadata.csv for gen_index's uids: full dates, year-month, year only, malformed and empty publish_time,
    and documents without a row.  Returns {uid: publish_time} of the rows written."""
    rng = random.Random(seed)
    rows = {}
    lines = ["cord_uid,title,publish_time,authors,url"]
    for i in range(N_SEG * N_PER_SEG):
        r = rng.random()
        if r < 0.15:
            continue                                             # no row at all
        y = rng.choice([2018, 2019, 2020, 2021])
        if r < 0.55:
            t = "%04d-%02d-%02d" % (y, rng.randint(1, 12), rng.randint(1, 28))
        elif r < 0.65:
            t = "%04d-%02d" % (y, rng.randint(1, 12))
        elif r < 0.80:
            t = "%04d" % y
        elif r < 0.88:
            t = ""
        elif r < 0.94:
            t = rng.choice(["2020 Mar 3", "2020-13-01", "unknown", "2020-02-30x"])
        else:
            t = " %04d-%02d " % (y, rng.randint(1, 12))          # blanks around a date (quoted by the writer below)
        uid = "u%08d" % i
        rows[uid] = t
        lines.append('%s,Title %d,"%s",A B,http://x/%d' % (uid, i, t, i))
    with open(os.path.join(index, "metadata.csv"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return rows


@pytest.fixture(scope="module")
def dated(tmp_path_factory):
    index = str(tmp_path_factory.mktemp("filter_cpu") / "index")
    nsbind.gen_index(index, N_SEG, N_PER_SEG, 512, 77, False)
    rows = write_metadata(index)
    eng = nsbind.Engine(index, -1)
    yield eng, rows
    eng.close()


def want_bits(rows, date_from, date_to, keep_undated):
    lo, hi = py_bound(date_from, 0), py_bound(date_to, 99)
    out = []
    for s in range(N_SEG):
        words = np.zeros((N_PER_SEG + 31) // 32, dtype=np.uint32)
        for d in range(N_PER_SEG):
            t = rows.get("u%08d" % (s * N_PER_SEG + d))
            key = py_date_key(t) if t is not None else 0
            keep = keep_undated if key == 0 else ((lo is None or key >= lo) and (hi is None or key <= hi))
            if keep:
                words[d >> 5] |= np.uint32(1 << (d & 31))
        out.append(words)
    return out


FILTERS = [("", "", False), ("", "", True), ("2020", "2020", False), ("2020", "", False), ("", "2019", True), ("2020-03", "2020-09", False),
           ("2019-06-15", "2020-06-15", False), ("2020-03", "", False), (" 2019 ", "\t2020-02\n", True), ("2030", "", False), ("2021", "2018", False)]


@pytest.mark.parametrize("date_from,date_to,keep_undated", FILTERS)
def test_filter_bits_equal_the_restatement(dated, date_from, date_to, keep_undated):
    eng, rows = dated
    got = eng.filter_bits(date_from, date_to, keep_undated)
    want = want_bits(rows, date_from, date_to, keep_undated)
    assert len(got) == N_SEG
    for s in range(N_SEG):
        assert got[s].dtype == np.uint32 and len(got[s]) == (N_PER_SEG + 31) // 32
        np.testing.assert_array_equal(got[s], want[s], err_msg=str((date_from, date_to, keep_undated, s)))
        assert int(got[s][-1]) >> (N_PER_SEG % 32) == 0           # the tail bits of the last word are zero


def test_the_fixture_holds_every_kind_of_document(dated):
    eng, rows = dated
    kinds = {"full": 0, "month": 0, "year": 0, "undated": 0}
    for t in rows.values():
        k = py_date_key(t)
        kinds["undated" if k == 0 else "year" if k % 10000 == 0 else "month" if k % 100 == 0 else "full"] += 1
    assert all(v >= 10 for v in kinds.values()), kinds
    assert N_SEG * N_PER_SEG - len(rows) >= 10                    # documents without a row
    # the engine's own table agrees on what a document's publish_time is
    for s, d in ((0, 0), (1, 7), (2, N_PER_SEG - 1)):
        md = eng.doc_metadata(s, d)
        t = rows.get("u%08d" % (s * N_PER_SEG + d))
        assert (md is None) == (t is None) and (md is None or md["publish_time"] == t)


def test_date_to_fills_missing_parts_with_99_and_date_from_with_0(dated):
    eng, rows = dated
    count = lambda bits: sum(int(bin(int(w)).count("1")) for b in bits for w in b)
    keys = [py_date_key(t) for t in rows.values()]
    # date_to = "2020" keeps all of 2020, the documents dated just "2020" included
    assert count(eng.filter_bits("2020", "2020")) == sum(1 for k in keys if 20200000 <= k <= 20209999)
    assert count(eng.filter_bits("2020", "2020")) > count(eng.filter_bits("2020-01-01", "2020-12-31")) > 0
    # date_from = "2020-03": a document dated just "2020" (key 20200000) is NOT kept; date_from = "2020" keeps it
    year_only = sum(1 for k in keys if k == 20200000)
    assert year_only > 0
    assert count(eng.filter_bits("2020-03", "2020")) == sum(1 for k in keys if 20200300 <= k <= 20209999)
    assert count(eng.filter_bits("2020", "2020")) - count(eng.filter_bits("2020-01", "2020")) == year_only
    # keep_undated adds exactly the undated documents, the row-less ones included
    undated = N_SEG * N_PER_SEG - sum(1 for k in keys if k)
    assert count(eng.filter_bits("2020", "2020", True)) - count(eng.filter_bits("2020", "2020", False)) == undated
    assert count(eng.filter_bits("", "", False)) == sum(1 for k in keys if k) and count(eng.filter_bits("", "", True)) == N_SEG * N_PER_SEG


@pytest.mark.parametrize("date_from,date_to", [("2020-13", ""), ("", "2020-00"), ("yesterday", ""), ("", "2020-03-17T00"), ("2020-3", "2021")])
def test_a_malformed_bound_is_refused(dated, date_from, date_to):
    eng, _ = dated
    with pytest.raises(RuntimeError, match="is not YYYY, YYYY-MM or YYYY-MM-DD"):
        eng.filter_bits(date_from, date_to)


def test_a_host_only_engine_fails_loudly(dated):
    eng, _ = dated
    with pytest.raises(RuntimeError, match="no device context"):
        eng.open_filter("2020", "2020")
    with pytest.raises(RuntimeError, match="no device context"):
        eng.open_filter(bits=eng.filter_bits("2020", "2020"))
    with pytest.raises(RuntimeError, match="no device context"):
        eng.search_filtered_json("t000001", 10, "2020", "2020")
    body = eng.search_filtered_json("t000001", 10, "2020", "2020", check=False)
    assert body.startswith('{\n  "error": "') and "no device context" in body
    assert eng.open_filters() == 0
    with pytest.raises(RuntimeError, match="stale"):
        eng.close_filter(8)
