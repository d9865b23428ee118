"""CPU: the table the variable-node kernel's record source reads (csrc/graph_tables.h, build_keep_rs) -- one word
row << 6 | slot per edge of the kept list -- against a direct walk of the alist.  The driver is a stand-alone program built
under ASan/UBSan."""
import os
import subprocess

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CSRC = os.path.join(ROOT, "ldpc_toolbox_amd", "csrc")


def test_keep_rs_table_under_asan_ubsan(tmp_path):
    """kept variables of weight 3, 8, 9 and 13, a variable whose edges sit in the first and in the last row, a 12-edge and a
    64-edge row, the padding, and the refusals: a 65-edge row (the slot does not fit), a row count beyond the word, graphs
    without kept or without L-free variables"""
    exe = str(tmp_path / "keep_rs_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "keep_rs_driver.cpp"),
                    os.path.join(CSRC, "sparse.cpp")], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for line in ("weights 3, 8, 9, 13 with a 12-edge row: ok", "64-edge row: ok", "refusals: ok", "keep_rs driver: ok"):
        assert line in r.stdout
