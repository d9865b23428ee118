"""GPU: the host entries of the NR rate matcher and the NR transport block handle on calls that need more than one stage
(include/ldpc_toolbox.h, PART 6 and 7), bit for bit against the numpy restatements.  A host entry stages 2^28 bytes of its
longest side at a time; every call here is one stage and a ragged rest of three rows, tiled from P + a few restated rows
(tests/tiled_cases.py) with np.take.  What only a later stage runs: the host offsets b0 * row, DeviceNrTb::copy_rows and
copy_packed, which cut block-major host arrays into one strided copy per block, the flag copies at tb_ok + b0 and
cb_ok + b0 * C, and recover with `into`, which brings the old buffer in one stage at a time."""
import numpy as np
import pytest

import ldpc_toolbox_amd as lt
import nr_rate_match_reference as rr
import nr_transport_block_reference as tr
import tiled_cases as tc
from ldpc_toolbox_amd import _capi
from test_nr_rate_match_gpu import bits_of, soft_values
from test_nr_transport_block_gpu import dirty
from tiled_cases import BYTES, flip

pytestmark = pytest.mark.gpu

# mirrored from device_nr_rm.h / device_nr_tb.h; every test asserts it against the handle's getter
STAGE_BYTES = 1 << 28
Q = 2


def stage_of(side_bytes):
    """the rows of a stage as the entries compute them, and a batch of one stage and a ragged rest of three"""
    stage = max(STAGE_BYTES // side_bytes, 1)
    assert stage * side_bytes <= STAGE_BYTES < (stage + 1) * side_bytes
    return stage, stage + 3


def same(got, want_patterns, ids):
    return got.dtype == want_patterns.dtype and np.array_equal(bits_of(got) if got.dtype.kind == "f" else got,
                                                               np.take(bits_of(want_patterns) if want_patterns.dtype.kind == "f" else want_patterns,
                                                                       ids, axis=0))


@pytest.fixture(scope="module")
def rm_case():
    ref = rr.Config(2, 2, 4, 93)
    rm = lt.NrRateMatcher(ref.spec, device=0)
    assert rm.get("stage_bytes") == STAGE_BYTES and (rm.n, ref.n) == (104, 104)
    yield ref, rm
    rm.close()


def test_match_over_two_stages(rm_case):
    ref, rm = rm_case
    e, rv, qm = 104, 3, 4
    stage, batch = stage_of(max(ref.n, e))
    t = tc.Tiling(batch, [stage])
    ids = t.ids()
    cws = np.random.default_rng(1).choice(BYTES, (t.patterns, ref.n))
    got = rm.match(np.take(cws, ids, axis=0), e, rv, qm)
    assert got.shape == (batch, e) and same(got, ref.match(cws, e, rv, qm), ids)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_recover_over_stages_and_into_the_first_result(rm_case, dtype):
    """E = 104, rv 2, Qm 2 into a fresh buffer: two stages.  Then rv 0, Qm 4, E = 208 with into = that result: rows twice
    as long, so three stages, and the old buffer is copied in stage by stage."""
    ref, rm = rm_case
    el = np.dtype(dtype).itemsize
    (e1, rv1, qm1, fill1), (e2, rv2, qm2, fill2) = (104, 2, 2, np.inf), (208, 0, 4, 9.0)
    stage1, batch = stage_of(max(ref.n, e1) * el)
    stage2 = STAGE_BYTES // (max(ref.n, e2) * el)
    cuts2 = list(range(stage2, batch, stage2))
    assert len(cuts2) == 2, "the second transmission takes three stages"
    t = tc.Tiling(batch, [stage1] + cuts2)
    ids = t.ids()
    rng = np.random.default_rng(el)
    rx1, rx2 = soft_values(rng, (t.patterns, e1), dtype), soft_values(rng, (t.patterns, e2), dtype)
    want1 = ref.recover(rx1, rv1, qm1, fill1)
    want2 = ref.recover(rx2, rv2, qm2, fill2, old=want1)
    buf = rm.recover(np.take(rx1, ids, axis=0), rv1, qm1, filler_llr=fill1)
    assert buf.shape == (batch, ref.n) and same(buf, want1, ids), "the first transmission"
    again = rm.recover(np.take(rx2, ids, axis=0), rv2, qm2, filler_llr=fill2, into=buf)
    assert again is buf and same(buf, want2, ids), "the second transmission, combined"


@pytest.fixture(scope="module")
def tb_case():
    stage, batch = stage_of(2 * 2080)
    t = tc.Tiling(batch, [stage])
    ref, raw, rows = tc.two_block_patterns(t.patterns)
    tb = lt.NrTransportBlock(ref.spec, device=0)
    assert tb.get("stage_bytes") == STAGE_BYTES and (tb.c, tb.k) == (ref.c, ref.k) == (2, 2080)
    yield ref, tb, t, raw, rows
    tb.close()


def tiled_rows(rows, c, ids):
    """block-major [C * patterns][K] -> block-major [C * batch][K]"""
    return np.concatenate([np.take(block, ids, axis=0) for block in rows.reshape(c, rows.shape[0] // c, -1)])


def test_segment_over_two_stages(tb_case):
    ref, tb, t, raw, rows = tb_case
    ids = t.ids()
    got = tb.segment(np.take(raw, ids, axis=0))
    assert got.dtype == np.uint8 and np.array_equal(got, tiled_rows(rows, ref.c, ids))


def test_desegment_over_two_stages(tb_case):
    """flipped: a payload bit in block 0 of transport block stage - 1, one in block 1 of transport block stage, and a
    CRC24B bit of block 0 of the last.  Once with cb_ok and once without."""
    ref, tb, t, raw, rows = tb_case
    c, pats, stage, batch = ref.c, t.patterns, t.boundaries[0], t.batch
    take = ref.k_prime - ref.l_cb
    received = dirty(rows, ref, np.random.default_rng(64))
    flip(received, 0 * pats + t.pattern_of(stage - 1), 700)
    flip(received, 1 * pats + t.pattern_of(stage), 1900)
    flip(received, 0 * pats + t.pattern_of(batch - 1), take + 3)
    want_payload, want_tb, want_cb = ref.desegment(received)
    ids = t.ids()
    big = tiled_rows(received, c, ids)
    payload, tb_ok, cb_ok = tb.desegment(big)
    assert same(payload, want_payload, ids) and same(tb_ok, want_tb, ids) and same(cb_ok, want_cb, ids)
    assert np.nonzero(tb_ok != 1)[0].tolist() == [stage - 1, stage] and not tb_ok[[stage - 1, stage]].any()
    assert list(zip(*(x.tolist() for x in np.nonzero(cb_ok != 1)))) == [(stage - 1, 0), (stage, 1), (batch - 1, 0)]
    assert not cb_ok[[stage - 1, stage, batch - 1], [0, 1, 0]].any()
    # cb_ok omitted
    payload2 = np.full((batch, ref.a), 0xEE, dtype=np.uint8)
    tb_ok2 = np.full(batch, 0xEE, dtype=np.uint8)
    rc = _capi.lib().ldpc_toolbox_nr_tb_desegment(tb._h, payload2.ctypes.data, ref.a, tb_ok2.ctypes.data, None, big.ctypes.data, ref.k, batch)
    assert rc == 0 and np.array_equal(payload2, payload) and np.array_equal(tb_ok2, tb_ok)


@pytest.fixture(scope="module", params=[(3826, 14, [6, 8]), (7641, 20, [6, 6, 8])], ids=["two blocks", "three blocks"])
def packed_case(request, tb_case):
    """(2, 3826) at (G, q) = (14, 2): one block of each length.  (2, 7641), C = 3, at (20, 2): two blocks of the shorter
    length, so that copy_packed's strided copies reach a second block of one length (r * batch with r > 0)."""
    a, g, lengths = request.param
    if a == 3826:
        ref, tb = tb_case[:2]
        yield ref, tb, g, lengths
        return
    ref = tr.Config(2, a)
    tb = lt.NrTransportBlock(ref.spec, device=0)
    assert tb.get("stage_bytes") == STAGE_BYTES and tb.c == ref.c == len(lengths)
    yield ref, tb, g, lengths
    tb.close()


def test_concatenate_over_two_stages(packed_case):
    ref, tb, G, LENGTHS = packed_case
    assert ref.block_lengths(G, Q) == LENGTHS
    stage, batch = stage_of(G)
    t = tc.Tiling(batch, [stage])
    ids = t.ids()
    packed = np.random.default_rng(G).choice(BYTES, t.patterns * G)
    big = np.empty(batch * G, dtype=np.uint8)
    for view, block in zip(tc.packed_views(big, LENGTHS, batch), ref.unpack(packed, t.patterns, G, Q)):
        view[:] = np.take(block, ids, axis=0)
    got = tb.concatenate(big, G, Q)
    assert got.shape == (batch, G) and same(got, ref.concatenate(packed, t.patterns, G, Q), ids)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_split_over_two_stages(packed_case, dtype):
    ref, tb, G, LENGTHS = packed_case
    assert ref.block_lengths(G, Q) == LENGTHS
    stage, batch = stage_of(G * np.dtype(dtype).itemsize)
    t = tc.Tiling(batch, [stage])
    ids = t.ids()
    rx = soft_values(np.random.default_rng(G), (t.patterns, G), dtype)
    rx[0, 0] = np.nan
    want = ref.unpack(ref.split(rx, Q), t.patterns, G, Q)
    got = tb.split(np.take(rx, ids, axis=0), Q)
    assert got.dtype == dtype and got.shape == (batch * G,)
    for r, view in enumerate(tc.packed_views(got, LENGTHS, batch)):
        assert same(view, want[r], ids), f"block {r}"
