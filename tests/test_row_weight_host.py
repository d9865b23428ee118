"""CPU: the structure of the codes of row_weight_cases.py -- what test_row_weight_gpu.py relies on when it says that a row
fills its bucket, its mask or its record exactly -- and the decoder's host tables for every one of them (csrc/graph_tables.h
through tests/graph_tables_driver.cpp, a stand-alone program built under ASan/UBSan)."""
import os
import re
import subprocess
from collections import Counter

import numpy as np
import pytest

import record_flags_cases
import row_weight_cases as rc

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CSRC = os.path.join(ROOT, "ldpc_toolbox_amd", "csrc")


def column_degrees(n, rows):
    deg = Counter(c for cs in rows for c in cs)
    return [deg[c] for c in range(n)]


def levels(n, rows):
    """the layered schedule's dependency levels (csrc/slice_tasks.h, build_levels, restated): a row's level is one more than
    the highest level of the earlier rows it shares a variable with"""
    last = [0] * n
    out = []
    for cs in rows:
        lv = 1 + max(last[c] for c in cs)
        for c in cs:
            last[c] = lv
        out.append(lv)
    return out


@pytest.mark.parametrize("w", rc.WEIGHTS)
def test_staircase_structure(w):
    rows, a = rc.staircase_code(w)
    K, n = rc.staircase_columns(w), rc.columns("staircase", w)
    assert n == K + rc.M and len(rows) == rc.M and n <= 700
    lengths = [len(cs) for cs in rows]
    assert max(lengths) == w and lengths.count(w) >= 10
    assert 4 <= min(lengths) <= 8 and sum(4 <= x <= 8 for x in lengths) >= 10      # short rows beside the full ones
    assert all(len(set(cs)) == len(cs) and cs == sorted(cs) for cs in rows)         # no duplicate entry
    deg = column_degrees(n, rows)
    assert min(deg[:K]) >= 3                                                       # information columns: the variable-node kernel's
    assert set(deg[K:]) == {1, 2} and deg[K:].count(1) == 1                        # the staircase: L-free variables
    assert all(cs[-1] == K + r and (r == 0 or cs[-2] == K + r - 1) for r, cs in enumerate(rows))
    assert levels(n, rows) == list(range(1, rc.M + 1))                             # one row per layered level
    assert a.split("\n", 2)[:2] == [f"{n} {rc.M}", f"{max(deg)} {w}"]


@pytest.mark.parametrize("w", [12, 13])
def test_staircase_is_the_record_flags_code(w):
    """the generalisation deals the two codes test_record_flags_* decode, edge for edge"""
    assert rc.staircase_code(w) == record_flags_cases.staircase_code(w)
    assert rc.staircase_columns(w) == record_flags_cases.K and rc.M == record_flags_cases.M


@pytest.mark.parametrize("w", rc.WEIGHTS)
def test_regular_structure(w):
    rows, a = rc.regular_code(w)
    n = rc.columns("regular", w)
    assert n == 12 * w <= 800
    lengths = [len(cs) for cs in rows]
    assert max(lengths) == w and lengths.count(w) == 12 and min(lengths) >= 2
    assert all(len(set(cs)) == len(cs) and cs == sorted(cs) for cs in rows)
    assert set(column_degrees(n, rows)) == {3, 4}                                   # no degree 0 / 1 / 2: no L-free variable
    lv = levels(n, rows)
    assert sorted(set(lv)) == [1, 2, 3, 4] and lv == sorted(lv)
    assert all(lv[r] == 1 for r in range(len(rows)) if lengths[r] == w)            # one level kernel sees all full rows ...
    assert min(Counter(lv).values()) >= 3                                          # ... and every level several rows
    # a level's kernel is chosen by the level's longest row: beside the full level there is one whose longest row is short
    # of the bucket by one edge and one by two
    assert sorted(max(x for x, l in zip(lengths, lv) if l == k) for k in (1, 2, 3, 4)) == [w - 2, w - 1, w - 1, w]


def test_regular_6_32_structure():
    rows, a = rc.regular_6_32()
    assert rc.columns("regular_6_32") == 512 and len(rows) == 96
    assert {len(cs) for cs in rows} == {32} and all(len(set(cs)) == 32 for cs in rows)
    assert set(column_degrees(512, rows)) == {6}
    assert Counter(levels(512, rows)) == {k: 16 for k in range(1, 7)}


@pytest.mark.parametrize("family", rc.FAMILIES)
def test_frames_reach_the_last_slot(family):
    """In the first iteration a row's inputs are the channel LLRs themselves, so the frames alone show that, for every weight,
    some full row has its smallest magnitude in its LAST slot (argmin = w - 1, the top of the argmin field) and some has a
    negative input there (the top bit of the sign mask, the last flip bit)."""
    for w in rc.WEIGHTS:
        llrs = rc.frames(family, w)
        assert llrs.shape == (rc.FRAMES, rc.columns(family, w)) and llrs.dtype == np.float32 and not llrs.flags.writeable
        assert (llrs[0] > 0).all() and len(set(llrs[0].tolist())) == 1                # noise-free
        argmins, negatives = rc.last_slot_argmins(family, w), rc.last_slot_negatives(family, w)
        print(f"{family} weight {w}: {argmins} argmins and {negatives} negative inputs in the last slot of a full row")
        assert argmins >= 5 and negatives >= 5


def test_graph_tables_under_asan_ubsan(tmp_path):
    """csrc/graph_tables.h on every code: the driver derives each table's invariants from the CSR form alone -- among them
    RowRecordTables::ready (rows of at most 32 / 64 edges and L-free tables), rec_w (3 up to 26 / 58 edges, 4 beyond), the
    sliced and lane-per-edge tables' `ready` (rows of at most 64 edges) -- and with "near:" that the degree-2 variables join
    neighbouring rows (row records by default).  Its report line gives the keep / free split: 120 L-free variables in a
    staircase code, none in a regular one -- where build_lfree_tables is therefore not ready and no record table exists."""
    exe = str(tmp_path / "graph_tables_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "graph_tables_driver.cpp"),
                    os.path.join(CSRC, "sparse.cpp")], check=True, capture_output=True)
    args, want = [], {}
    for family, w in [(f, w) for f in rc.FAMILIES for w in rc.WEIGHTS] + [("regular_6_32", None)]:
        rows, a = rc.code(family, w)
        f = tmp_path / f"{family}_{w}.alist"
        f.write_text(a)
        args.append(("near:" if family == "staircase" else "") + str(f))
        n = rc.columns(family, w)
        free = rc.M if family == "staircase" else 0
        want[str(f)] = f"{len(rows)} rows, {n} columns, {sum(map(len, rows))} edges, {n - free} keep / {free} free variables: ok"
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "graph tables driver: ok" in r.stdout
    reported = dict(re.findall(r"^(\S+\.alist): (.*)$", r.stdout, flags=re.M))
    assert reported == want
