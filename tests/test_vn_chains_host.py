"""CPU: the kept list of the variable-node kernel's record form in chains (csrc/graph_tables.h, build_vn_chains) -- the same
entries in blocks of W * L, a wave walking L of them one after the other with the record of a shared row carried in its
registers.  The driver is a stand-alone program built under ASan/UBSan."""
import os
import re
import subprocess

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CSRC = os.path.join(ROOT, "ldpc_toolbox_amd", "csrc")


def test_vn_chains_under_asan_ubsan(tmp_path):
    """a permutation whose entries keep their edges in order; the carry consistent wave by wave (an edge taken from the carry
    names the row the wave's previous entry left there, none at a block's first step, at most one per entry); L = 1 equal to
    build_vn_bundles; kept counts that are no multiple of W * L, W or L, a variable that shares no row, isolated stars; the
    counts against a recount -- and on the built-in DVB-S2 1/2 tables with W = 4, L = 8 at most 0.83 x 162 000 loads issued"""
    exe = str(tmp_path / "vn_chains_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "vn_chains_driver.cpp"),
                    os.path.join(CSRC, "sparse.cpp"), os.path.join(CSRC, "codes.cpp")], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for line in ("mixed degrees, 18 kept: ok", "no shared rows, 7 kept: ok", "isolated stars, 15 kept: ok",
                 "long column, 12 kept: ok", "vn_chains driver: ok"):
        assert line in r.stdout
    found = {int(m.group(1)): tuple(int(x) for x in m.groups()[1:])
             for m in re.finditer(r"dvbs2:R1_2: W = 4, L = (\d+): (\d+) fetches, (\d+) carried, (\d+) issued", r.stdout)}
    assert set(found) == {1, 4, 8, 16}, r.stdout
    for length, (fetches, carried, issued) in sorted(found.items()):
        print(f"dvbs2:R1_2, W = 4, L = {length}: {fetches} record fetches, {carried} carried, {issued} issued, "
              f"{100.0 * (fetches - issued) / fetches:.2f} % spared")
        assert fetches == 162000
    assert found[1][1] == 0
    assert found[8][2] <= 0.83 * 162000
    assert found[16][2] < found[8][2] < found[4][2] < found[1][2]
