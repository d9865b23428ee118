"""The row-shape form of the flooding min-sum check-node kernel ("cn_row_shape": cn_minsum_rec_kernel's SHAPE forms, a
straight-line row step in the runs of the walk whose rows all have the graph's dominant shape, the generic step in every
other run of the same launch) against the same decoder with "cn_row_shape" 0 and against the CPU reference, bit for bit:
hard decisions, iteration counts and posterior LLRs with np.array_equal, no tolerance -- NaN frames included, compared bit
pattern for bit pattern between the two forms.

Codes and frames: cn_row_shape_cases.py.  The hand-built code of 7-edge rows (kind PN) and the same code with its staircase
columns numbered backwards (kind NP, DVB-S2's) have runs that conform and runs that do not; the staircase codes with rows of
3 to 7 edges have none, and the form must not run on them.  Run lengths 8 (the default: one conforming run, walked downwards),
4 (three: up, down, up) and 3 (six, and run boundaries inside conforming stretches); batches 1, 65 and 257 with packs of 1, 2
and 4 codewords per lane (lanes with frozen codewords, a partial last tile); iteration limits 1 (the first iteration alone,
which has no row-shape form: the key must say so), 2, 5 and 40.  "last_cn_row_shape", "cn_row_shape_runs" and
"cn_row_shape_rows" are compared with a count made here from the codes' rows.  One more case runs DVB-S2 1/2 normal frames on
64 frames of the benchmark's own stream."""
import functools
import itertools

import numpy as np
import pytest

import corrected_minsum_restatement as cm
import ldpc_toolbox_amd as lt
from cn_row_shape_cases import CODES, ORACLE_ALWAYS, ORACLE_ONCE, code, conforming_runs, fitting_rows, frames

pytestmark = pytest.mark.gpu

RULES = ("Minsumf32", "NormMinsumf32", "OffsetMinsumf32")
BATCHES = (1, 65, 257)
LIMITS = (1, 2, 5, 40)
RUNS = (8, 4, 3)
VECS = (1, 2, 4)


@functools.lru_cache(maxsize=None)
def reference(oracle, name, rule, limit):
    """(frame indices, bits, iterations, posterior) of the frames the CPU reference holds for at this limit"""
    llrs, kind = frames(name)
    index = np.flatnonzero((kind == ORACLE_ALWAYS) | ((kind == ORACLE_ONCE) & (limit == 1)))
    a = code(name)[2]
    if rule.startswith(("Norm", "Offset")):
        bits, its, post = cm.decode(a, rule, llrs[index], limit)
    else:
        bits, its, post = oracle.decode_batch(oracle.Graph(a), rule, llrs[index], limit, threads=8)
    assert not np.isnan(post).any()
    return index, bits, its, post.astype(np.float32)


def decoder(alist, rule, shape):
    dec = lt.LdpcDecoder(alist, rule)
    dec.set("latency", 0)              # the batched kernels at every batch size
    dec.set("vn_records", 1)
    dec.set("flags8", 1)
    dec.set("cn_row_shape", shape)
    assert dec.get("cn_row_shape") == shape and dec.get("row_records") == 3
    return dec


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", CODES)
def test_row_shape_form_decodes_as_the_generic_form_and_as_the_reference(oracle, name, rule):
    llrs, kind = frames(name)
    llrs = np.array(llrs, dtype=np.float32)
    n, rows, alist = code(name)
    shape_kind, fits = fitting_rows(n, rows)
    shaped, generic = decoder(alist, rule, 1), decoder(alist, rule, 0)
    ran = 0
    for run, batch, limit, vec in itertools.product(RUNS, BATCHES, LIMITS, VECS):
        what = (run, batch, limit, vec)
        got = {}
        for key, dec in ((1, shaped), (0, generic)):
            dec.set("rec_run", run)
            dec.set("vec", vec)
            got[key] = dec.decode_batch(llrs[:batch], limit, want_posterior=True)
            assert dec.get("last_record_flag_bytes") == 1 and dec.get("last_vn_records") == 1, what
        # what the call says it ran, against the count made from the code's rows: the form runs behind the first iteration,
        # and only where some run of this length conforms
        want = conforming_runs(fits, run)
        expect = 1 if (want and limit > 1) else 0
        assert shaped.get("last_cn_row_shape") == expect, what
        assert shaped.get("cn_row_shape_runs") == (len(want) if expect else 0), what
        assert shaped.get("cn_row_shape_rows") == (sum(min(r * run + run, len(rows)) - r * run for r in want) if expect else 0), what
        assert generic.get("last_cn_row_shape") == 0 and generic.get("cn_row_shape_runs") == 0, what
        ran += expect
        # the same decoder with the key off: every frame, NaNs included, bit pattern for bit pattern
        assert np.array_equal(got[1][1], got[0][1]), ("iterations, against cn_row_shape = 0", what)
        assert np.array_equal(got[1][0], got[0][0]), ("bits, against cn_row_shape = 0", what)
        assert np.array_equal(got[1][2].view(np.uint32), got[0][2].view(np.uint32)), ("posterior, against cn_row_shape = 0", what)
        # the CPU reference
        index, bits, its, post = reference(oracle, name, rule, limit)
        here = index < batch
        at = index[here]
        assert np.array_equal(got[1][1][at], its[here]), ("iterations", what)
        assert np.array_equal(got[1][0][at], bits[here]), ("bits", what)
        assert got[1][2].dtype == post.dtype
        assert np.array_equal(got[1][2][at], post[here]), ("posterior", what)
    if shape_kind == "none":
        assert ran == 0                    # a code with no conforming run: the form never ran
    else:
        # every run length has conforming runs here, in both walk directions (even runs walk upwards, odd ones downwards)
        assert ran == len(RUNS) * len(BATCHES) * (len(LIMITS) - 1) * len(VECS)
        directions = {r % 2 for run in RUNS for r in conforming_runs(fits, run)}
        assert directions == {0, 1}
        assert any(conforming_runs(fits, run) and len(conforming_runs(fits, run)) < (len(rows) + run - 1) // run for run in RUNS)


def test_row_shape_form_on_dvbs2_half_rate_frames_of_the_benchmark():
    """DVB-S2 n = 64800, rate 1/2 (kind PN: the decoder's graph comes from the alist; all runs but the first and the last conform): 64 frames of the benchmark's stream
    -- the library's own generator, seed 1000, Eb/N0 = 0 dB -- at 3 iterations, against the key off"""
    import torch
    alist = lt.code_alist("dvbs2:R1_2")
    gen = lt.Simulator(alist, "Minsumf32", "", device=0, pool_size=64, pool_seed=1000)
    d_llrs = torch.empty((64, gen.n_tx), dtype=torch.float32, device="cuda:0")
    gen.generate_into(d_llrs.data_ptr(), 0.0, 1000, 0, 64)
    torch.cuda.synchronize()
    gen.close()
    llrs = d_llrs.cpu().numpy()
    got = {}
    for key in (1, 0):
        dec = lt.LdpcDecoder(alist, "Minsumf32")
        dec.set("latency", 0)
        dec.set("cn_row_shape", key)
        assert dec.get("flags8") == 1      # the timed configuration's defaults: records read by the variable nodes, byte flags
        got[key] = dec.decode_batch(llrs, 3, want_posterior=True)
        assert dec.get("last_vn_records") == 1 and dec.get("last_record_flag_bytes") == 1
        assert dec.get("last_cn_row_shape") == key
        if key:
            runs, in_rows = dec.get("cn_row_shape_runs"), dec.get("cn_row_shape_rows")
            print(f"dvbs2:R1_2, run 8: {runs} conforming runs of {(32400 + 7) // 8}, {in_rows} rows of 32400")
            assert runs == (32400 + 7) // 8 - 2 and in_rows == 32400 - 16
    assert np.array_equal(got[1][1], got[0][1])
    assert np.array_equal(got[1][0], got[0][0])
    assert np.array_equal(got[1][2].view(np.uint32), got[0][2].view(np.uint32))
