"""CPU: the kept list of the variable-node kernel's record form in bundles (csrc/graph_tables.h, build_vn_bundles) -- the same
entries, ordered so that aligned groups of W share rows.  The driver is a stand-alone program built under ASan/UBSan."""
import os
import re
import subprocess

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CSRC = os.path.join(ROOT, "ldpc_toolbox_amd", "csrc")


def test_vn_bundles_under_asan_ubsan(tmp_path):
    """a permutation whose entries keep their edges in order, aligned bundles of one degree, W = 1 the identity, list lengths
    and degree classes that are no multiple of W, a variable that shares no row, the counts against a recount -- and at least
    12 % of the record fetches saved on the built-in DVB-S2 1/2 tables with W = 4"""
    exe = str(tmp_path / "vn_bundles_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "vn_bundles_driver.cpp"),
                    os.path.join(CSRC, "sparse.cpp"), os.path.join(CSRC, "codes.cpp")], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for line in ("mixed degrees, 18 kept: ok", "no shared rows, 7 kept: ok", "chain: ok", "vn_bundles driver: ok"):
        assert line in r.stdout
    m = re.search(r"dvbs2:R1_2: W = 4 (\d+) -> (\d+),", r.stdout)
    assert m, r.stdout
    fetches, distinct = int(m.group(1)), int(m.group(2))
    print(f"dvbs2:R1_2, W = 4: {fetches} record fetches, {distinct} distinct per bundle, "
          f"{100.0 * (fetches - distinct) / fetches:.2f} % saved")
    assert fetches == 162000
    assert (fetches - distinct) >= 0.12 * fetches
