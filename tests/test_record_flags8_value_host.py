"""CPU: the value a check row takes from a stored byte-form record (csrc/record_flags8.h, record_flags8_arg and
record_flags8_value -- the code the byte form of cn_minsum_rec_kernel runs) against the 16-bit form's `value` of
record_flags8_decode's output.  The driver is a stand-alone program built under ASan/UBSan."""
import os
import subprocess

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_value_of_a_stored_record_under_asan_ubsan(tmp_path):
    """all 128 flip patterns x argmin 0..6 x magnitudes {+0, smallest subnormal, 1, largest finite, +inf}^2 x slot 0..6 in
    both word types: the value taken from the stored triple equals, bit for bit, the 16-bit form's value of the decoded
    record"""
    exe = str(tmp_path / "record_flags8_value_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "record_flags8_value_driver.cpp")],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "f32: 156800 values equal the 16-bit form's" in r.stdout
    assert "f64: 156800 values equal the 16-bit form's" in r.stdout
    assert "record flags8 value driver: ok" in r.stdout
