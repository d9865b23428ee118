"""GPU: rate recovery / HARQ combining and the NR demapper on 8-bit soft bits (include/ldpc_toolbox.h, PART 9), byte for byte
against the numpy restatement (tests/nr_soft_i8_restatement.py, pinned on the CPU by tests/test_nr_soft_i8_restatement.py).
There is no tolerance anywhere: saturating integer sums in a fixed order, and one quantiser.

Recovery runs on nr5g:2:2:4:93 (n = 104, 4 fillers, a limited buffer of 93 bits, L = 89) at five (E, rv, Qm) from one
repeat per column to 75.  A thread of the kernel owns four output bytes aligned to a dword of the output, so every device
call is made with the output at all four byte offsets into a dword, guard bytes on both sides, and batches of 3 (a pass of
78 dwords and two ragged ends) and 67 (more than one workgroup)."""
import numpy as np
import pytest
import torch

import ldpc_toolbox_amd as lt
import nr_qam_reference as nq
import nr_rate_match_reference as rr
import nr_soft_i8_restatement as sr
import tiled_cases as tc
from ldpc_toolbox_amd import _capi

pytestmark = pytest.mark.gpu

# (E, rv, Qm, the most repeats of a column, columns no selection index carries -- the fillers among them)
CASES = [(60, 0, 1, 1, 44), (104, 2, 2, 2, 15), (208, 0, 4, 3, 15), (372, 1, 6, 5, 15), (6656, 1, 8, 75, 15)]
SECOND = (96, 3, 2)             # the second transmission of every case: (E, rv, Qm), combined into the first one's buffer
BATCHES = (3, 67)
GUARD = 0x6E
STAGE_BYTES = 1 << 28           # mirrored from device_nr_rm.h; asserted against the handle's getter


@pytest.fixture(scope="module")
def rm_case():
    ref = rr.Config(2, 2, 4, 93)
    rm = lt.NrRateMatcher(ref.spec, device=0)
    assert (rm.n, ref.n, ref.L) == (104, 104, 89)
    yield ref, rm
    rm.close()


def all_bytes(rng, shape):
    """int8 values that cover all 256 bytes (when there is room for them), in random order"""
    size = int(np.prod(shape))
    v = np.resize(np.arange(-128, 128), max(size, 256))[:size]
    if size > 256:
        v[256:] = rng.integers(-128, 128, size - 256)
    v = rng.permutation(v).astype(np.int8).reshape(shape)
    assert len(np.unique(v)) == min(256, size)
    return v


def dirty_old(buf):
    """a soft buffer whose bytes include -128 and +-127"""
    old = buf.copy()
    old[:, 0::7] = -128
    old[:, 1::7] = 127
    old[:, 2::7] = -127
    return old


@pytest.fixture(scope="module")
def restated(rm_case):
    """per (case, batch): the inputs and the restatement's outputs of both transmissions, computed once and left unchanged"""
    ref, rm = rm_case
    out = {}
    for ci, (e, rv, qm, max_repeats, idle) in enumerate(CASES):
        repeats = ref.repeats(e, rv)
        assert (int(repeats.max()), int((repeats == 0).sum())) == (max_repeats, idle), (e, rv, qm)
        carried = repeats > 0
        for batch in BATCHES:
            rng = np.random.default_rng(1000 * ci + batch)
            rx1, rx2 = all_bytes(rng, (batch, e)), all_bytes(rng, (batch, SECOND[0]))
            sat = np.zeros((batch, ref.n), dtype=bool)
            want1 = sr.recover_i8(ref, rx1, rv, qm, 127, saturated=sat)
            if e >= 208:
                # (a column saturates when a partial sum of one of the batch's frames leaves +-127; the first transmission alone)
                assert sat.any(axis=0)[carried].mean() >= 0.25, (e, rv, qm, batch, sat.any(axis=0)[carried].mean())
            old = dirty_old(want1)
            want2 = sr.recover_i8(ref, rx2, SECOND[1], SECOND[2], 99, old=old, saturated=sat)
            assert sat.any(axis=0)[carried].mean() >= 0.25, "combining into +-127 saturates"
            for a in (rx1, rx2, want1, old, want2):
                a.setflags(write=False)
            out[ci, batch] = (rx1, want1, rx2, old, want2)
    return out


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_recover_equals_the_restatement_on_the_host_entry(rm_case, restated, ci, batch):
    ref, rm = rm_case
    e, rv, qm = CASES[ci][:3]
    rx1, want1, rx2, old, want2 = restated[ci, batch]
    got = rm.recover_i8(rx1, rv, qm)
    assert got.dtype == np.int8 and np.array_equal(got, want1)
    assert (got[:, ref.k - 4:ref.k] == 127).all()
    buf = old.copy()
    assert rm.recover_i8(rx2, SECOND[1], SECOND[2], filler=99, into=buf) is buf and np.array_equal(buf, want2)
    assert (buf[:, ref.k - 4:ref.k] == 99).all() and buf.min() >= -127, "a filler is the filler; -128 never leaves"
    assert buf[0, 0] == -127 and old[0, 0] == -128, "column 0 is never sent: clip(old)"


@pytest.mark.parametrize("own_stream", [False, True], ids=["handle's stream", "caller's stream"])
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_recover_device_at_every_byte_offset(rm_case, restated, ci, batch, own_stream):
    """the output at offsets 4 .. 7 of a 256-byte aligned allocation -- all four positions in a dword -- and the input one
    byte into its own; guard bytes before and behind both stay as they were"""
    ref, rm = rm_case
    e, rv, qm = CASES[ci][:3]
    n = ref.n
    rx1, want1, rx2, old, want2 = restated[ci, batch]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev) if own_stream else None
    st = stream.cuda_stream if own_stream else 0
    d_rx1 = torch.full((batch * e + 2,), GUARD, dtype=torch.int8, device=dev)
    d_rx1[1:-1] = torch.from_numpy(rx1.copy()).to(dev).reshape(-1)
    d_rx2 = torch.from_numpy(rx2.copy()).to(dev)
    results = []
    for off in (4, 5, 6, 7):
        d_out = torch.full((batch * n + 12,), GUARD, dtype=torch.int8, device=dev)
        assert d_out.data_ptr() % 256 == 0
        torch.cuda.synchronize()
        rm.recover_i8_device(d_rx1.data_ptr() + 1, d_out.data_ptr() + off, batch, e, rv, qm, stream=st)
        if own_stream:
            stream.synchronize()
        first = d_out.cpu().numpy()
        d_out[off:off + batch * n] = torch.from_numpy(old.copy()).to(dev).reshape(-1)
        torch.cuda.synchronize()
        rm.recover_i8_device(d_rx2.data_ptr(), d_out.data_ptr() + off, batch, SECOND[0], SECOND[1], SECOND[2], filler=99, combine=True, stream=st)
        if own_stream:
            stream.synchronize()
        results.append((off, first, d_out.cpu().numpy()))
    for off, first, second in results:
        for got, want in ((first, want1), (second, want2)):
            assert (got[:off] == GUARD).all() and (got[off + batch * n:] == GUARD).all(), f"guard bytes at offset {off}"
            assert np.array_equal(got[off:off + batch * n].reshape(batch, n), want), (off, e, rv, qm)
    assert (d_rx1.cpu().numpy()[[0, -1]] == GUARD).all()


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_low_amplitude_equals_the_float_recovery(rm_case, ci):
    """|v| <= 127 // (max repeats + 1) in the received rows and in the old buffer: no partial sum leaves +-127 (asserted from
    the restatement), and the soft bits are the float32 recovery of the same integers -- the restated one and the library's"""
    ref, rm = rm_case
    e, rv, qm, max_repeats, _ = CASES[ci]
    bound = 127 // (max_repeats + 1)
    rng = np.random.default_rng(50 + ci)
    rx = rng.integers(-bound, bound + 1, (67, e)).astype(np.int8)
    old = rng.integers(-bound, bound + 1, (67, ref.n)).astype(np.int8)
    sat = np.zeros((67, ref.n), dtype=bool)
    want = sr.recover_i8(ref, rx, rv, qm, 127, old=old, saturated=sat)
    assert not sat.any()
    got = rm.recover_i8(rx, rv, qm, into=old.copy())
    assert np.array_equal(got, want)
    as_float = ref.recover(rx.astype(np.float32), rv, qm, 127.0, old=old.astype(np.float32))
    lib_float = rm.recover(rx.astype(np.float32), rv, qm, filler_llr=127.0, into=old.astype(np.float32))
    assert np.array_equal(got.astype(np.float32), as_float) and np.array_equal(lib_float, as_float)


def test_recover_host_entry_over_two_stages(rm_case):
    """E = 208, Qm 4: a stage is 2^28 / 208 rows; one stage and a ragged rest of three rows, tiled from 61 + 3 restated rows
    (tests/tiled_cases.py), first into a fresh buffer and then combined into it -- the old buffer goes in stage by stage"""
    ref, rm = rm_case
    e, rv, qm = 208, 0, 4
    assert rm.get("stage_bytes") == STAGE_BYTES and rm.get("pass_elements") == 1 << 30
    stage = STAGE_BYTES // max(ref.n, e)
    batch = stage + 3
    t = tc.Tiling(batch, [stage])
    ids = t.ids()
    rng = np.random.default_rng(208)
    rx1, rx2 = all_bytes(rng, (t.patterns, e)), all_bytes(rng, (t.patterns, e))
    want1 = sr.recover_i8(ref, rx1, rv, qm)
    want2 = sr.recover_i8(ref, rx2, 2, qm, old=want1)
    buf = rm.recover_i8(np.take(rx1, ids, axis=0), rv, qm)
    assert buf.shape == (batch, ref.n) and np.array_equal(buf, np.take(want1, ids, axis=0)), "the first transmission"
    again = rm.recover_i8(np.take(rx2, ids, axis=0), 2, qm, into=buf)
    assert again is buf and np.array_equal(buf, np.take(want2, ids, axis=0)), "the second transmission, combined"


# ---- the demapper ----------------------------------------------------------------------------------------------------------

SIGMA_CLIPPING = {2: 0.25, 4: 0.18, 6: 0.12, 8: 0.08}     # a tenth or more of the LLRs reach +-127 (asserted from the f32 result)
SIGMA_NO_CLIPPING = 1.0                                   # none does (asserted)
CLIP_AT = 127 / 8 - 1 / 16                                # Q(x) = +-127 from |x| = 15.8125 on


@pytest.fixture(scope="module")
def awgn():
    d = lt.Demodulator("QPSK", device=0)
    yield d
    d.close()


@pytest.mark.parametrize("c_init", [-1, 0x5A5A5])
@pytest.mark.parametrize("max_log", [False, True], ids=["exact", "max-log"])
@pytest.mark.parametrize("qm", [2, 4, 6, 8])
def test_demap_i8_is_the_quantised_f32_demapper(awgn, qm, max_log, c_init):
    """3 x 52 symbols from the mapper plus the AWGN channel, at two noise levels; the soft bits equal quantise(demod_f32) on
    the host entry and on the device entry, with the output on a dword and at three other byte addresses"""
    qam = lt.NrQam(qm, device=0)
    batch, S = 3, 52
    bits = np.random.default_rng(qm).integers(0, 2, (batch, S * qm), dtype=np.uint8)
    clean = qam.modulate(bits, c_init, f64=False)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    for sigma in (SIGMA_CLIPPING[qm], SIGMA_NO_CLIPPING):
        sym = awgn.add_noise(clean, sigma, seed=17 + qm, first_frame=5)
        assert sym.dtype == np.complex64
        f32 = qam.demodulate(sym, sigma, max_log, c_init)
        assert f32.dtype == np.float32 and np.array_equal(f32.view(np.uint32), nq.demodulate(sym, sigma, qm, max_log, c_init).view(np.uint32))
        clipped = float((np.abs(f32) >= CLIP_AT).mean())
        assert clipped >= 0.1 if sigma != SIGMA_NO_CLIPPING else clipped == 0.0, (qm, sigma, clipped)
        want = sr.quantise(f32)
        assert (np.abs(want) == 127).mean() == clipped and len(np.unique(want)) > 20
        got = qam.demap_i8(sym, sigma, max_log, c_init)
        assert got.dtype == np.int8 and np.array_equal(got, want), (qm, max_log, c_init, sigma)
        d_sym = torch.from_numpy(sym.view(np.float32).copy()).to(dev)
        for off, st in ((8, 0), (9, stream.cuda_stream), (10, 0), (11, stream.cuda_stream)):
            d_out = torch.full((batch * S * qm + 16,), GUARD, dtype=torch.int8, device=dev)
            assert d_out.data_ptr() % 256 == 0
            torch.cuda.synchronize()
            qam.demap_i8_device(d_sym.data_ptr(), d_out.data_ptr() + off, batch, S, sigma, max_log, c_init, stream=st)
            stream.synchronize()
            out = d_out.cpu().numpy()
            assert (out[:off] == GUARD).all() and (out[off + want.size:] == GUARD).all(), f"guard bytes at offset {off}"
            assert np.array_equal(out[off:off + want.size].reshape(want.shape), want), (qm, max_log, c_init, sigma, off)
    qam.close()


def test_demap_i8_refuses_what_the_float_entry_refuses():
    qam = lt.NrQam(4, device=0)
    L = _capi.lib()
    dev = torch.device("cuda", 0)
    d_sym = torch.zeros((3, 52, 2), dtype=torch.float32, device=dev)
    d_out = torch.full((3 * 52 * 4,), GUARD, dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    for llrs_len, S, sigma, c_init in ((207, 52, 1.0, -1), (208, 51, 1.0, -1), (208, 52, 0.0, -1), (208, 52, float("inf"), -1), (208, 52, 1.0, -2)):
        assert L.ldpc_toolbox_nr_demap_i8_device(qam._h, d_out.data_ptr(), llrs_len, d_sym.data_ptr(), S, 3, sigma, 0, c_init, None) == -4
    assert L.ldpc_toolbox_nr_demap_i8_device(qam._h, d_out.data_ptr(), 208, d_sym.data_ptr() + 4, 52, 3, 1.0, 0, -1, None) == -4
    assert "symbol buffer is not aligned" in _capi.last_error()
    torch.cuda.synchronize()
    assert (d_out == GUARD).all()
    assert qam.demap_i8(np.zeros((0, 52), dtype=np.complex64), 1.0).shape == (0, 208)
    qam.close()
