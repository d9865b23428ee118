"""CPU: the byte form of a row record's flags.  Whether it applies is a pure host decision (csrc/graph_tables.h,
record_flag_bytes: rows of at most 7 edges), and what memory holds is the encode / decode pair of csrc/record_flags8.h, which
the kernels run as well.  The driver is a stand-alone program built under ASan/UBSan."""
import os
import subprocess

import numpy as np

from record_flags8_cases import quantised_frames, staircase_code

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CSRC = os.path.join(ROOT, "ldpc_toolbox_amd", "csrc")


def test_byte_flags_under_asan_ubsan(tmp_path):
    """record_flag_bytes for every row weight 0..65 in f32 and f64 (7 | 8 and 12 | 13 spelled out; record_flag_bits as it
    was), and encode -> decode of all 128 flip patterns x argmin 0..6 x magnitudes {+0, smallest subnormal, 1, largest
    finite, +inf}^2 in both types: everything comes back bit for bit, decoded magnitudes have clear sign bits"""
    exe = str(tmp_path / "record_flags8_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "record_flags8_driver.cpp"),
                    os.path.join(CSRC, "sparse.cpp")], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "f32: 22400 records round-trip" in r.stdout and "f64: 22400 records round-trip" in r.stdout
    assert "record flags8 driver: ok" in r.stdout


def test_the_frames_use_both_stolen_bits():
    """In the first iteration a row's inputs are the channel LLRs themselves, so the frames alone show that the 7-edge rows
    have their smallest magnitude on every slot 0..6 -- argmin values with bit 1 and with bit 2 set, the bits that travel
    in the magnitudes' sign bits -- and that the quantised frames have ties, exact zeros and infinities in a row."""
    rows = staircase_code(7)[1]
    assert max(len(cs) for cs in rows) == 7 and min(len(cs) for cs in rows) == 4
    llrs = quantised_frames()
    seen = np.zeros(7, dtype=np.int64)
    ties = zeros = infs = 0
    for cs in rows:
        x = np.abs(llrs[:, cs])
        if len(cs) == 7:
            seen += np.bincount(x.argmin(axis=1), minlength=7)
        s = np.sort(x, axis=1)
        ties += int((s[:, 0] == s[:, 1]).sum())
        zeros += int((s[:, 0] == 0).sum())
        infs += int(np.isinf(s[:, 1]).sum())
    print(f"argmin slots of the 7-edge rows: {seen.tolist()}; rows with min1 == min2: {ties}, min1 == 0: {zeros}, "
          f"min2 == inf: {infs}")
    assert (seen >= 10).all() and ties >= 10 and zeros >= 10
