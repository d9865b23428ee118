"""GPU: the 8-bit soft-bit decode entries (include/ldpc_toolbox.h, PART 9) against their definition: bits, iterations and
posterior are exactly those of the f32 entry of the same decoder on the rows clip(v) / 8 as float32, the posterior as the
int16 word the f32 entry converts to float.  Every path a call can take is run: the single-launch path of small synchronised
calls (1 and 3 frames, host and device entries), a ragged last 64-slot block (257), the straggler pool copying byte rows
(1100 frames with "pooling" and groups of 256, 30 iterations), two lanes, a decoder with a puncturing pattern, and a device
call on the caller's stream with the input one byte into its allocation and guard bytes around every output.

The rows hold all 256 byte values (-128 among them) and are of three kinds: noisy codewords, quantised; codewords with random
magnitudes, valid at iteration 0; and random bytes, which never converge."""
import numpy as np
import pytest
import torch

import ldpc_toolbox_amd as lt
import nr_soft_i8_restatement as sr
from frames import alist, awgn_frames

pytestmark = pytest.mark.gpu

FRAMES = 1100
GUARD = 0x6E
# one of each rule x schedule, and variants with the clipping options
NAMES = ["Minsumi8", "HLMinsumi8Offset", "Minstarapproxi8", "HLMinstarapproxi8PartialHardLimit", "Aminstari8JonesDeg1Clip", "HLAminstari8",
         "Minsumi8OffsetPartialHardLimitDeg1Clip"]
# (Eb/N0 where the noisy rows converge in a few iterations: the straggler pool then runs its chunks on a reduced budget)
CODES = [("nr5g:2:2", "", 4.0), ("ar4ja:1/2:1024", "", 4.5), ("ar4ja:1/2:1024", "1,1,1,1,0", 4.5)]
CASES = [(name, spec, punct, ebn0) for spec, punct, ebn0 in CODES[:2] for name in NAMES] + [("Minsumi8Offset", *CODES[2]), ("HLAminstari8", *CODES[2])]

_SAMPLES = {}


def sample(spec, punct, ebn0):
    """int8 rows [FRAMES][input_len], built once per code and left unchanged"""
    key = (spec, punct)
    if key not in _SAMPLES:
        msgs, llrs, _ = awgn_frames(spec, FRAMES, ebn0, 808, punct)
        rng = np.random.default_rng(len(spec) + len(punct))
        v = sr.quantise(llrs)
        # every fourth row from row 1 on: the codeword's signs (those of the noisy row wherever the noise did not flip them:
        # taken from a noiseless pass) with random magnitudes 1 .. 127, and -128 for some of the ones
        _, clean, _ = awgn_frames(spec, FRAMES, 60.0, 808, punct)
        sign = np.where(clean < 0, -1, 1)
        mags = rng.integers(1, 128, v.shape)
        valid = (sign * mags).astype(np.int8)
        valid[(sign < 0) & (rng.random(v.shape) < 0.1)] = -128
        v[1::4] = valid[1::4]
        # sparse rows of random bytes: they never converge, and there are few enough for the pool's reduced budget
        random_rows = np.arange(3, FRAMES, 24)
        v[random_rows] = rng.integers(-128, 128, (len(random_rows), v.shape[1])).astype(np.int8)
        assert len(np.unique(v)) == 256 and (v[:257] == -128).any()
        v.setflags(write=False)
        _SAMPLES[key] = v
    return _SAMPLES[key]


def assert_defined(got, want, what):
    bits, its, post = got
    wbits, wits, wpost = want
    assert np.array_equal(its, wits), (what, "iterations")
    assert np.array_equal(bits, wbits), (what, "bits")
    if post is not None:
        assert post.dtype == np.int16 and np.array_equal(wpost, np.rint(wpost)) and np.array_equal(post, wpost.astype(np.int16)), (what, "posterior")


def device_decode(dec, v, max_iter, stream=None, offset=0, want_posterior=True):
    """the device entry on torch buffers: the input `offset` bytes into its allocation, guard bytes around every output"""
    B, n = len(v), dec.n
    dev = torch.device("cuda", 0)
    d_in = torch.full((v.size + offset + 1,), GUARD, dtype=torch.int8, device=dev)
    d_in[offset:offset + v.size] = torch.from_numpy(v.copy()).to(dev).reshape(-1)
    d_bits = torch.full((B * n + 16,), GUARD, dtype=torch.uint8, device=dev)
    d_its = torch.full((B + 8,), GUARD, dtype=torch.int32, device=dev)
    d_post = torch.full((B * n + 8,), GUARD, dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    dec.decode_batch_device(d_in.data_ptr() + offset, False, B, max_iter, d_bits.data_ptr() + 8, n, d_its.data_ptr() + 16,
                            d_post.data_ptr() + 8 if want_posterior else 0, stream.cuda_stream if stream else 0, i8=True)
    if stream:
        stream.synchronize()
    bits, its, post = d_bits.cpu().numpy(), d_its.cpu().numpy(), d_post.cpu().numpy()
    assert (bits[:8] == GUARD).all() and (bits[8 + B * n:] == GUARD).all() and (its[:4] == GUARD).all() and (its[4 + B:] == GUARD).all()
    assert (post[:4] == GUARD).all() and (post[4 + B * n:] == GUARD).all() and (want_posterior or (post == GUARD).all())
    return bits[8:8 + B * n].reshape(B, n), its[4:4 + B], post[4:4 + B * n].reshape(B, n) if want_posterior else None


@pytest.mark.parametrize("name,spec,punct,ebn0", CASES)
def test_soft_bit_input_equals_the_f32_entry_on_every_path(name, spec, punct, ebn0):
    v = sample(spec, punct, ebn0)
    dec = lt.LdpcDecoder(alist(spec), name, punct, device=0)
    assert v.shape == (FRAMES, dec.input_len)
    as_float = sr.dequantise(v)
    assert as_float.dtype == np.float32 and np.array_equal(sr.quantise(as_float), sr.clip(v).astype(np.int8))

    def defined(rows, max_iter, want_posterior=True):
        return dec.decode_batch(as_float[rows], max_iter, want_posterior=want_posterior)

    # 257 frames: a ragged last 64-slot block; the three kinds of rows are all there
    rows = slice(0, 257)
    want = defined(rows, 12)
    assert (want[1] > 0).any() and (want[1] < 0).any() and (punct or (want[1] == 0).any()), np.bincount(want[1] + 1)
    assert_defined(dec.decode_batch(v[rows], 12, want_posterior=True), want, "257, host entry")
    assert_defined(device_decode(dec, v[rows], 12), want, "257, device entry")
    # ... on the caller's stream, the input one byte into its allocation; and without a posterior
    stream = torch.cuda.Stream(device=torch.device("cuda", 0))
    assert_defined(device_decode(dec, v[rows], 12, stream=stream, offset=1), want, "257, caller's stream, odd address")
    assert_defined(device_decode(dec, v[rows], 12, stream=stream, offset=3, want_posterior=False), want, "257, no posterior")
    got = dec.decode_batch(v[rows], 12, output_len=dec.k)
    assert got[2] is None and np.array_equal(got[0], want[0][:, :dec.k]) and np.array_equal(got[1], want[1])
    # 1 and 3 frames: small synchronised calls (the single-launch path where the decoder has one), host and device entries
    for batch in (1, 3):
        want_small = defined(slice(0, batch), 12)
        assert_defined(dec.decode_batch(v[:batch], 12, want_posterior=True), want_small, (batch, "host entry"))
        assert_defined(device_decode(dec, v[:batch], 12), want_small, (batch, "device entry"))
        assert_defined(device_decode(dec, v[:batch], 12, offset=1), want_small, (batch, "device entry, odd address"))
    # with the small-batch paths off the same frames take the batched kernels
    dec.set("latency", 0)
    dec.set("latency_edge", 0)
    assert_defined(dec.decode_batch(v[:3], 12, want_posterior=True), defined(slice(0, 3), 12), "3, batched kernels")
    dec.set("latency", 32)
    dec.set("latency_edge", 256)
    # two lanes: 600 frames in groups of 256
    dec.set("group_size", 256)
    dec.set("lanes", 2)
    want_lanes = defined(slice(0, 600), 12)
    assert dec.get("last_lanes") == 2
    assert_defined(device_decode(dec, v[:600], 12, offset=1), want_lanes, "two lanes, device entry")
    assert dec.get("last_lanes") == 2
    assert_defined(dec.decode_batch(v[:600], 12, want_posterior=True), want_lanes, "two lanes, host entry")
    # the straggler pool: 1100 frames, 30 iterations; the pooled rows are gathered and scattered as bytes
    dec.set("pooling", 1)
    want_pool = defined(slice(0, FRAMES), 30)
    got_pool = device_decode(dec, v, 30, offset=1)
    pooled = dec.get("last_pooled")
    assert_defined(got_pool, want_pool, "pooled")
    print(f"{name} on {spec}: {pooled} of {FRAMES} frames through the straggler pool; iterations {np.bincount(want_pool[1] + 1).tolist()}")
    assert pooled > 0, "no frame went through the straggler pool"
    assert_defined(device_decode(dec, v, 30, offset=2, want_posterior=False), want_pool, "pooled, no posterior")
    dec.close()


def test_a_float_decoder_and_a_wrong_length_are_refused():
    spec = "nr5g:2:2"
    v = sample(spec, "", 4.0)[:5]
    dec = lt.LdpcDecoder(alist(spec), "Minsumf32", device=0)
    with pytest.raises(RuntimeError, match=r"\(-3\).*8-bit"):
        dec.decode_batch(v, 10)
    dec.close()
    dec = lt.LdpcDecoder(alist(spec), "Minsumi8", device=0)
    with pytest.raises(RuntimeError, match=r"\(-4\)"):
        dec.decode_batch(v[:, :-1], 10)
    assert dec.decode_batch(v[:0], 10)[0].shape == (0, dec.n)
    dec.close()
