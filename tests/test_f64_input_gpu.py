"""Decode parity on TRUE f64 channel LLRs through every entry that takes f64: the frames of f64_input_cases.py (plain f64
AWGN, scales down to the float-subnormal range and up beyond the float range, f64 subnormals, signed zeros, infinities, and
the ties of the conversion to float and of the 8-bit quantiser with their f64 neighbours) against the oracle's one-codeword
f64 entry, for all 40 names of lt.ALL_IMPLEMENTATIONS on both codes.  Every comparison is bit equality -- hard decisions,
iteration counts and the f64 posterior (NaNs equal) -- there is no tolerance anywhere.

The kernels that convert f64 input, each of which a name reaches below: ingest_kernel<double, T> (kernels_group.hip.h) and
ingest_i8_kernel / i8_quantize(double) (kernels_i8.hip.h) from the batched entries, the ingest of latency.hip.h (flooding
Minsumf32's single launch) and edge_quantize<T, double> (latency_edge.hip.h, every other name's) from the small batches;
emit_kernel<P, double> writes the f64 posterior.  test_f64_input_host.py shows from the reference alone that narrowing
the input early would change the result on these frames."""
import numpy as np
import pytest

import f64_input_cases as fc
import ldpc_toolbox_amd as lt
from f64_input_cases import ITERATIONS

pytestmark = pytest.mark.gpu

# the small batches, by size -- one codeword, fewer than the 8 XCDs, one per XCD -- as frame ranges: the float ties and the
# deeper subnormal frame alone; the quantiser's ties and whole-frame scales; per-position scales, the huge / tiny / infinite
# values, and the last eight frames
SMALL = {1: (slice(24, 25), slice(33, 34)), 3: (slice(27, 30), slice(12, 15)), 8: (slice(6, 14), slice(16, 24), slice(26, 34))}


def assert_same(got, want, sl, what):
    bits, its, post = got
    assert np.array_equal(its, want[1][sl]), ("iterations", what, its.tolist(), want[1][sl].tolist())
    assert np.array_equal(bits, want[0][sl]), ("bits", what)
    # f32 and 8-bit rules return their posterior widened to the caller's f64 (as test_gpu_parity.py compares
    # `post.astype(np.float64)` of the f32 entry with the oracle's)
    assert post.dtype == np.float64
    assert np.array_equal(post, want[2][sl], equal_nan=True), ("posterior", what, np.argwhere(post != want[2][sl])[:8].tolist())


def device_entry(dec, llrs, iterations):
    import torch
    batch = len(llrs)
    d_llrs = torch.from_numpy(np.ascontiguousarray(llrs).copy()).cuda()
    d_bits = torch.zeros((batch, dec.n), dtype=torch.uint8, device="cuda")
    d_its = torch.zeros(batch, dtype=torch.int32, device="cuda")
    d_post = torch.zeros((batch, dec.n), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dec.decode_batch_device(d_llrs.data_ptr(), True, batch, iterations, d_bits.data_ptr(), dec.n, d_its.data_ptr(),
                            d_post.data_ptr(), 0)
    torch.cuda.synchronize()
    return d_bits.cpu().numpy(), d_its.cpu().numpy(), d_post.cpu().numpy()


@pytest.mark.parametrize("code", fc.CODES)
@pytest.mark.parametrize("name", lt.ALL_IMPLEMENTATIONS)
def test_f64_llrs_through_every_entry(oracle, name, code):
    llrs = fc.frames(code)
    runs = [(ITERATIONS, fc.reference(oracle, code, name))]
    if fc.is_f64(name):
        runs.append((0, fc.reference(oracle, code, name, 0)))
    # the batched kernels at every batch size ...
    batched = lt.LdpcDecoder(fc.alist(code), name)
    batched.set("group_size", 64)
    batched.set("latency", 0)
    batched.set("latency_edge", 0)
    # ... and the default options: every one of the 40 names has a single-launch path on these codes (flooding Minsumf32
    # latency.hip.h, all others latency_edge.hip.h: four and 120 layered levels are within the 512 it takes), and a call
    # that took it reports the batch itself as its group (latency_paths.hip:44)
    small = lt.LdpcDecoder(fc.alist(code), name)
    for iterations, want in runs:
        what = (name, code, iterations)
        got = batched.decode_batch(llrs, iterations, want_posterior=True)
        assert batched.get("last_group") >= 64
        assert_same(got, want, slice(0, fc.FRAMES), what + ("batched",))
        for batch, slices in SMALL.items():
            for sl in slices:
                got = small.decode_batch(llrs[sl], iterations, want_posterior=True)
                assert small.get("last_group") == batch, what
                assert_same(got, want, sl, what + ("small batch", sl.start, batch))
        for sl in (slice(0, 8), slice(24, 32)):
            assert_same(device_entry(small, llrs[sl], iterations), want, sl, what + ("device entry, small-batch path", sl.start))
            assert small.get("last_group") == 8, what
            assert_same(device_entry(batched, llrs[sl], iterations), want, sl, what + ("device entry, batched kernels", sl.start))
            assert batched.get("last_group") >= 64
    want = runs[0][1]
    for dec in (small, batched):
        for f in fc.SCALAR_FRAMES:
            ok, out = dec.decode(llrs[f], ITERATIONS)
            assert ok == (want[1][f] >= 0) and out.iterations == (want[1][f] if ok else ITERATIONS), (name, code, "scalar", f)
            assert np.array_equal(out.codeword, want[0][f]), (name, code, "scalar", f)
    batched.close()
    small.close()
