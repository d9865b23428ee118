"""GPU: one NrQam handle on two streams.  The handle caches the scrambling sequence of the last (c_init, row length) on the
device and orders that cache across streams itself (include/ldpc_toolbox.h, PART 8): a call that generates another
sequence must run after every launch that still reads the one it replaces, whatever stream that launch is on.

The sequence of calls, from one host thread:
  0. choose X so that step 3's stream runs beside it and not behind it on one hardware queue (shown with a short delay);
  1. warm the cache with c_init A on stream X, and wait;
  2. on X a bounded device delay (torch.cuda._sleep, its cycle count calibrated here to about 0.3 s), then a reader of A,
     then the event x_done;
  3. on another stream a call with A (a cache hit) and a call with B (a regeneration, which overwrites the cached words);
  4. X's reader must still have been pending while step 3 was enqueued -- else the test has shown nothing and fails;
  5. wait for everything;
  6. X's result is the restatement's for A, and both results of step 3 are their own restatements', bit for bit.
A handle that orders the regeneration only after the LAST reader lets it overwrite the words under X's delayed launch,
which then descrambles with B's sequence."""
import time

import numpy as np
import pytest
import torch

import channel_restatement as cr
import demod_restatement as dr
import ldpc_toolbox_amd as lt
import nr_qam_reference as nq

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
QM, B, S = 4, 3, 173                  # the shape of test_nr_qam_gpu.py
A_INIT, B_INIT = 0x2A5A5A5, 0x1234567
SIGMA = 0.3
DELAY_MS = 300.0
PROBE_CYCLES = 2_000_000


@pytest.fixture(scope="module")
def case():
    """bits, noisy symbols (complex64) and the restated LLRs and symbols per c_init"""
    rng = np.random.default_rng(173)
    bits = rng.integers(0, 2, (B, QM * S)).astype(np.uint8)
    sym = cr.awgn(nq.modulate(bits, QM, A_INIT), SIGMA, 5, 9).astype(np.complex64)
    llrs = {c: nq.demodulate(sym, SIGMA, QM, False, c) for c in (A_INIT, B_INIT)}
    mapped = {c: nq.modulate(bits, QM, c, np.float32).view(np.float32) for c in (A_INIT, B_INIT)}
    assert not np.array_equal(llrs[A_INIT], llrs[B_INIT]) and not np.array_equal(mapped[A_INIT], mapped[B_INIT])
    return bits, sym, llrs, mapped


@pytest.fixture(scope="module")
def delay_cycles():
    """the argument of torch.cuda._sleep for about DELAY_MS: a short sleep timed with events, scaled"""
    stream = torch.cuda.Stream(device=DEV)
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        torch.cuda._sleep(PROBE_CYCLES)             # (loads the kernel)
        begin.record()
        torch.cuda._sleep(PROBE_CYCLES)
        end.record()
    stream.synchronize()
    ms = begin.elapsed_time(end)
    assert ms > 0.05, f"a sleep of {PROBE_CYCLES} cycles took {ms} ms: too short to scale from"
    cycles = int(PROBE_CYCLES * DELAY_MS / ms)
    print(f"{PROBE_CYCLES} cycles of torch.cuda._sleep took {ms:.3f} ms: {cycles} cycles for {DELAY_MS:.0f} ms")
    return cycles


def llr_buffer():
    return torch.full((B, QM * S), 12345.0, dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("step3", ["a stream", "the handle's stream"])
@pytest.mark.parametrize("reader", ["demodulate_device", "modulate_device"])
def test_regeneration_waits_for_a_reader_on_another_stream(case, delay_cycles, reader, step3):
    """step3 = "a stream": the hit and the regeneration are enqueued on a second stream Y of the caller's, and x_done must
    still be pending when they have returned.  step3 = "the handle's stream": they go through the NULL-stream entry, which
    is synchronous -- a handle that orders the regeneration behind X's reader returns only when that reader is done, so
    there the precondition is that X was pending when step 3 began, and that step 3 began in the first half of X's delay
    (the host's clock against the delay's length as the events measured it)."""
    bits, sym, want_llrs, want_mapped = case
    q = lt.NrQam(QM, device=0)
    y = torch.cuda.Stream(device=DEV)
    st = y.cuda_stream if step3 == "a stream" else 0
    d_bits = torch.from_numpy(bits).to(DEV)
    d_sym = torch.from_numpy(sym.view(np.float32)).to(DEV)
    d_warm, d_hit, d_regen = llr_buffer(), llr_buffer(), llr_buffer()
    d_x = llr_buffer() if reader == "demodulate_device" else torch.full((B, 2 * S), 12345.0, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()

    def demod(out, c_init, stream):
        q.demodulate_device(d_sym.data_ptr(), out.data_ptr(), False, B, S, SIGMA, False, c_init, stream)

    # X: a stream beside which step 3's stream really runs.  The runtime maps streams onto a few hardware queues; two
    # streams on one queue run one after the other, which would order the calls by accident and show nothing.  So an
    # unscrambled call (it touches no sequence and no event of the cache) on step 3's stream must finish under a short
    # delay on X; else the next stream is tried.
    demod(d_warm, -1, st)                # (loads the kernel)
    y.synchronize()
    for attempt in range(8):
        x = torch.cuda.Stream(device=DEV)
        probe_done = torch.cuda.Event()
        with torch.cuda.stream(x):
            torch.cuda._sleep(delay_cycles // 10)
        probe_done.record(x)
        demod(d_warm, -1, st)
        y.synchronize()
        beside = not probe_done.query()
        x.synchronize()
        if beside and x.cuda_stream != y.cuda_stream:
            break
    else:
        pytest.fail("inconclusive: no stream was found beside which step 3's stream runs")
    print(f"stream X found at attempt {attempt}")
    # 1
    demod(d_warm, A_INIT, x.cuda_stream)
    x.synchronize()
    launches = q.get("sequence_launches")
    assert launches == 1
    # 2
    x_begin, x_done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t_delay = time.perf_counter()
    with torch.cuda.stream(x):
        x_begin.record()
        torch.cuda._sleep(delay_cycles)
    if reader == "demodulate_device":
        demod(d_x, A_INIT, x.cuda_stream)
    else:
        q.modulate_device(d_bits.data_ptr(), d_x.data_ptr(), False, B, QM * S, A_INIT, x.cuda_stream)
    x_done.record(x)
    # 3
    pending_before = not x_done.query()
    t_step3 = time.perf_counter()
    demod(d_hit, A_INIT, st)
    demod(d_regen, B_INIT, st)
    # 4
    pending_after = not x_done.query()
    # 5
    x.synchronize()
    y.synchronize()
    torch.cuda.synchronize()
    delay_ms = x_begin.elapsed_time(x_done)
    began_ms = (t_step3 - t_delay) * 1e3
    print(f"X's delay and reader took {delay_ms:.1f} ms; step 3 began {began_ms:.2f} ms after the delay was enqueued; "
          f"x_done pending before step 3: {pending_before}, after: {pending_after}")
    if step3 == "a stream":
        assert pending_after, "inconclusive: X's reader was no longer pending when step 3 had been enqueued"
    else:
        assert pending_before and began_ms < 0.5 * delay_ms, "inconclusive: X's reader was not pending while step 3 ran"
    assert q.get("sequence_launches") == launches + 1, "the hit generates nothing, the other c_init once"
    # 6
    got_x = d_x.cpu().numpy()
    want_x = want_llrs[A_INIT] if reader == "demodulate_device" else want_mapped[A_INIT]
    assert dr.same_bits(got_x, want_x), "X's launch read a sequence that a later call on another stream had overwritten"
    assert dr.same_bits(d_warm.cpu().numpy(), want_llrs[A_INIT])
    assert dr.same_bits(d_hit.cpu().numpy(), want_llrs[A_INIT]), "the cache hit"
    assert dr.same_bits(d_regen.cpu().numpy(), want_llrs[B_INIT]), "the regeneration"
    q.close()
