"""CPU: the host side of the HARQ simulator (csrc/nr_harq.h) -- the validation of a sequence, its offsets, normal pairs and
per-transmission plans against a literal loop over the concatenated transmitted row, in a stand-alone driver built under
ASan/UBSan that includes that header only -- and the refusals of the three C entries that need no GPU."""
import ctypes as C
import os
import subprocess

import numpy as np

import ldpc_toolbox_amd as lt
from ldpc_toolbox_amd import _capi

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ERR_ARGUMENT = -4       # include/ldpc_toolbox.h
HARQ_SYMBOLS = ("ldpc_toolbox_sim_set_harq", "ldpc_toolbox_sim_run_harq", "ldpc_toolbox_sim_generate_harq")


def test_nr_harq_host_functions_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "nr_harq_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "nr_harq_driver.cpp")],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "sequences: 48 cases" in r.stdout and "agree with the literal row" in r.stdout
    assert "refusals ok" in r.stdout and "nr harq driver: ok" in r.stdout


def test_every_new_symbol_is_exported_and_declared():
    L = _capi.lib()
    header = open(os.path.join(ROOT, "include", "ldpc_toolbox.h")).read()
    for name in HARQ_SYMBOLS:
        assert name in _capi.SYMBOLS and getattr(L, name) is not None and f"int32_t {name}(" in header
    assert {"set_harq", "run_harq", "generate_harq"} <= set(dir(lt.Simulator))


def _arrays(seq):
    return np.array([e for e, _ in seq], dtype=np.uint64), np.array([rv for _, rv in seq], dtype=np.uint32)


def test_refusals_come_before_the_gpu_and_write_nothing():
    """A sequence that is none is refused as such before the simulator handle is looked at, so also where no simulator can
    exist; a null handle is refused by every entry.  Nothing is written to the caller's arrays."""
    L = _capi.lib()
    rm = lt.NrRateMatcher("nr5g:2:16")
    good = [(480, 0), (96, 2), (96, 3), (96, 1)]
    cases = ((good[:0], 1, "1 .. 8 transmissions"), (good * 2 + good[:1], 1, "1 .. 8 transmissions"), ([(480, 0), (96, 4)], 1, "rv must be 0 .. 3"),
             ([(480, 0), (95, 2)], 2, "Qm must divide E"), ([(480, 0), (0, 2)], 1, "E must be positive"),
             ([(0x7fffffff, 0), (1, 2)], 1, "sum above 0x7fffffff"))
    for seq, qm, why in cases:
        e, rv = _arrays(seq + [(7, 7)])             # (never empty: a T of 0 is refused for itself)
        assert L.ldpc_toolbox_sim_set_harq(None, rm._h, e.ctypes.data, rv.ctypes.data, len(seq), qm) == -1, seq
        assert why in _capi.last_error(), (seq, _capi.last_error())
    e, rv = _arrays(good)
    assert L.ldpc_toolbox_sim_set_harq(None, rm._h, None, rv.ctypes.data, 4, 1) == -1 and "null" in _capi.last_error()
    assert L.ldpc_toolbox_sim_set_harq(None, rm._h, e.ctypes.data, None, 4, 1) == -1 and "null" in _capi.last_error()
    # a null simulator handle, with a sequence that is one, and when clearing
    assert L.ldpc_toolbox_sim_set_harq(None, rm._h, e.ctypes.data, rv.ctypes.data, 4, 1) == -1 and _capi.last_error() == "null argument"
    assert L.ldpc_toolbox_sim_set_harq(None, None, None, None, 0, 1) == -1 and _capi.last_error() == "null argument"
    counters = np.full(6, 0xAB, dtype=np.uint64)
    per_tx = np.full((8, 4), 0xAB, dtype=np.uint64)
    llrs = np.full((2, 480), 7.5, dtype=np.float32)
    idx = np.full(2, 0xAB, dtype=np.uint32)
    assert L.ldpc_toolbox_sim_run_harq(None, 1.0, 1, 0, 2, 30, counters.ctypes.data, per_tx.ctypes.data) == -1 and _capi.last_error()
    assert L.ldpc_toolbox_sim_generate_harq(None, 1.0, 1, 0, 2, 0, llrs.ctypes.data, idx.ctypes.data) == -1 and _capi.last_error()
    assert (counters == 0xAB).all() and (per_tx == 0xAB).all() and (llrs == 7.5).all() and (idx == 0xAB).all()
    assert (e == [480, 96, 96, 96]).all() and (rv == [0, 2, 3, 1]).all()
    rm.close()


def test_run_harq_before_set_harq_is_refused():
    """A simulator handle exists on a machine with a GPU only: there, run_harq and generate_harq without a sequence return
    ERR_ARGUMENT, the counters zeroed and per_tx and the LLRs untouched (tests/test_sim_harq_gpu.py repeats this among the
    GPU tests).  Without a GPU the constructor itself refuses, and says why."""
    L = _capi.lib()
    alist = lt.code_alist("nr5g:2:16")
    if L.ldpc_toolbox_device_count() <= 0:
        assert L.ldpc_toolbox_sim_ctor(alist.encode(), b"Minsumf32", b"", 0, 4, 1) is None and _capi.last_error()
        return
    s = lt.Simulator(alist, "Minsumf32", device=0, pool_size=4)
    counters = np.full(6, 0xAB, dtype=np.uint64)
    per_tx = np.full((8, 4), 0xAB, dtype=np.uint64)
    llrs = np.full((2, 832), 7.5, dtype=np.float32)
    assert s.get("harq") == 0 and s.harq() == []
    assert L.ldpc_toolbox_sim_run_harq(s._h, 1.0, 1, 0, 2, 30, counters.ctypes.data, per_tx.ctypes.data) == ERR_ARGUMENT
    assert "no HARQ sequence" in _capi.last_error() and (counters == 0).all() and (per_tx == 0xAB).all()
    assert L.ldpc_toolbox_sim_generate_harq(s._h, 1.0, 1, 0, 2, 0, llrs.ctypes.data, None) == ERR_ARGUMENT
    assert "no HARQ sequence" in _capi.last_error() and (llrs == 7.5).all()
    s.close()
