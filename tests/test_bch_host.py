"""CPU: the BCH code's host side (csrc/bch.h) -- spec parsing and every refusal, the generator anchors, the argument
checks -- and a host loop over the functions the kernels themselves run (remainder register and combining table, syndromes
of a remainder, locator, root count) against a syndrome-table decoder, exhaustively on small codes.  The driver is a
stand-alone program built under ASan/UBSan."""
import os
import subprocess

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_bch_host_functions_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "bch_host_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "bch_host_driver.cpp")],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    # every pattern of weight <= 3 on 25 positions is corrected (1 + 25 + 300 + 2300), and the weight-4 split of the
    # 25-bit code (11705 detected, 945 miscorrected) is part of these totals
    assert "bch:5:25:3:25: 41841 patterns up to weight 5: 2626 corrected" in r.stdout
    assert "bch:16:1002D:12:65535: planted errors ok" in r.stdout and "bch:14:402B:12:300: planted errors ok" in r.stdout
    assert "bch host driver: ok" in r.stdout
