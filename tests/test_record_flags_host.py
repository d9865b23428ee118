"""CPU: the width of a row record's flags word is a pure host decision (csrc/graph_tables.h, record_flag_bits) -- 16 bits
for rows of at most 12 edges, the decoder's own word beyond.  The driver is a stand-alone program built under ASan/UBSan."""
import os
import subprocess

import numpy as np

from record_flags_cases import frames, staircase_code

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CSRC = os.path.join(ROOT, "ldpc_toolbox_amd", "csrc")


def test_record_flag_width_under_asan_ubsan(tmp_path):
    """weights 1..64 in f32 and f64 against a restatement of the rule, both sides of 12 | 13 (16-bit flags or not) and of
    26 | 27 and 58 | 59 (the three- and four-word families, which the narrow flags leave as they were), and the tables
    build_row_record_tables returns for staircase graphs whose longest row has exactly those weights"""
    exe = str(tmp_path / "record_flags_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "record_flags_driver.cpp"),
                    os.path.join(CSRC, "sparse.cpp")], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "longest row 12: ok" in r.stdout and "longest row 13: ok" in r.stdout and "record flags driver: ok" in r.stdout


def test_highest_slot_of_a_twelve_edge_row_is_used():
    """In the weight-12 code of the GPU tests slot 11 of a 12-edge row -- flip bit 11, argmin value 11: the top of both fields
    of the 16-bit word -- is the row's own staircase column K + r (the largest column of the row).  In the first iteration a
    row's inputs are the channel LLRs themselves, so the frames alone show that some 12-edge row has a negative input on
    slot 11 and some has its smallest magnitude there."""
    rows, _ = staircase_code(12)
    llrs = frames()
    negative = argmin = 0
    for cs in rows:
        if len(cs) != 12:
            continue
        x = llrs[:, cs]
        assert cs[11] == max(cs)
        negative += int((x[:, 11] < 0).sum())
        argmin += int((np.abs(x).argmin(axis=1) == 11).sum())
    print(f"slot 11 of the 12-edge rows: {negative} negative inputs, {argmin} argmins")
    assert negative >= 10 and argmin >= 10
