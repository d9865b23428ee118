"""GPU parity tests proper: the HIP path, called through the C ABI, against the CPU oracle on
the same seeded frames.  Bar: BIT-IDENTICAL for every implementation name -- hard decisions,
success flag, iteration count and posterior LLRs -- in f32, f64 and the 8-bit rules alike: the
transcendental rules use glibc-identical exp/log/log1p/tanh on the device (csrc/exact_math.h), so
no tolerance is needed and none is applied (north_star's 1e-5 relative bound on the soft outputs is
met with zero error).  At BASELINE's full sizes the oracle would take minutes, so those tests use
size-independent properties (round trips, symmetry, position and shard invariance) plus a small
oracle sample.
"""
import os

import numpy as np
import pytest

import ldpc_toolbox_amd as lt
from frames import alist, awgn_frames

pytestmark = pytest.mark.gpu


def run_both(oracle, spec, impl, batch, ebn0, max_iter, seed, puncturing="", group=None):
    msgs, llrs, full = awgn_frames(spec, batch, ebn0, seed, puncturing)
    dec = lt.LdpcDecoder(alist(spec), impl, puncturing)
    if group:
        dec.set("group_size", group)
    # f64 arithmetics are driven through the f64 entry so that the posterior comes back in f64
    gpu_in = llrs.astype(np.float64) if impl.endswith("f64") else llrs
    bits, its, post = dec.decode_batch(gpu_in, max_iter, want_posterior=True)
    g = oracle.Graph(alist(spec))
    obits, oits, opost = oracle.decode_batch(g, impl, full, max_iter, threads=8)
    return msgs, (bits, its, post), (obits, oits, opost)


# ---- the reference's own known answers, through the C ABI on the GPU -----------------------

def to_llrs(bits):
    return np.array([1.3863 if b == 0 else -1.3863 for b in bits])


def test_reference_kat_no_errors(toy_h):
    """src/decoder/flooding.rs:161-172"""
    dec = lt.DecoderImplementation("Phif64").build_decoder(toy_h)
    codeword = [0, 0, 1, 0, 1, 1]
    ok, out = dec.decode(to_llrs(codeword), 100)
    assert ok
    assert list(out.codeword) == codeword
    assert out.iterations == 0


def test_reference_kat_single_error(toy_h):
    """src/decoder/flooding.rs:174-189"""
    dec = lt.DecoderImplementation("Phif64").build_decoder(toy_h)
    good = [0, 0, 1, 0, 1, 1]
    for j in range(len(good)):
        bad = list(good)
        bad[j] ^= 1
        ok, out = dec.decode(to_llrs(bad), 100)
        assert ok
        assert list(out.codeword) == good
        assert out.iterations == 1


@pytest.mark.parametrize("impl", lt.IMPLEMENTATIONS)
def test_toy_all_implementations_match_oracle(oracle, toy_h, impl):
    dec = lt.DecoderImplementation(impl).build_decoder(toy_h)
    odec = oracle.Decoder(oracle.Graph(toy_h.alist()), impl)
    rng = np.random.default_rng(7)
    for trial in range(6):
        llrs = rng.normal(1.0, 1.2, size=6) if trial else to_llrs([0, 0, 1, 0, 1, 1])
        ok, out = dec.decode(llrs, 20)
        ook, obits, oit, _ = odec.decode(llrs, 20)
        assert ok == ook
        assert list(out.codeword) == list(obits)
        assert out.iterations == oit


# ---- bit-exact: min-sum -----------------------------------------------------------------------

@pytest.mark.parametrize("impl", ["Minsumf32", "Minsumf64", "HLMinsumf32", "HLMinsumf64"])
@pytest.mark.parametrize("spec,punct,ebn0", [("ar4ja:1/2:1024", "1,1,1,1,0", 2.1),
                                              ("dvbs2:R1_2short", "", 1.6),
                                              ("nr5g:2:24", "", 1.0)])
def test_minsum_bit_exact(oracle, impl, spec, punct, ebn0):
    # (HL on the staircase code: a length-m serial chain of layers, SURVEY F9 -- slow, and exact like the others)
    batch = 200
    msgs, (bits, its, post), (obits, oits, opost) = run_both(oracle, spec, impl, batch, ebn0, 30, seed=11,
                                                            puncturing=punct)
    assert np.array_equal(its, oits)
    assert np.array_equal(bits, obits)
    assert post.dtype == (np.float64 if impl.endswith("f64") else np.float32)
    assert np.array_equal(post, opost.astype(post.dtype))
    assert (its >= 0).any() and (its != 0).any()


def test_minsum_group_sizes_and_ragged_batch(oracle):
    """batch not a multiple of the wave tile, several groups, every vector width"""
    spec = "ar4ja:1/2:1024"
    for group, batch in ((64, 100), (128, 300), (256, 257), (512, 513)):
        msgs, (bits, its, post), (obits, oits, opost) = run_both(oracle, spec, "Minsumf32", batch, 2.2, 25,
                                                                seed=group, puncturing="1,1,1,1,0",
                                                                group=group)
        assert np.array_equal(its, oits), (group, batch)
        assert np.array_equal(bits, obits), (group, batch)
        assert np.array_equal(post, opost.astype(np.float32)), (group, batch)


@pytest.mark.parametrize("impl", ["Minsumf32", "HLMinsumf32", "Aminstari8"])
def test_default_group_grows_for_small_graphs_and_changes_nothing(oracle, impl):
    """A small graph's launches are short, so a large call is cut into larger groups by default (up to 65536 codewords;
    4096 for a graph of DVB-S2's size): "preferred_group" says which, and the grouping is invisible in the results --
    host and device entries, against explicit groups of 4096 and 1024, and against the oracle on a sample."""
    import torch
    spec, punct = "ar4ja:1/2:1024", "1,1,1,1,0"
    big = lt.LdpcDecoder(alist("dvbs2:R1_2"), "Minsumf32")
    assert big.get("preferred_group") == 4096
    big.close()
    dec = lt.LdpcDecoder(alist(spec), impl, punct)
    assert dec.get("preferred_group") == 65536
    msgs, llrs, full = awgn_frames(spec, 9000, 2.0, 41, punct)
    want = dec.decode_batch(llrs, 20, want_posterior=True)
    assert dec.get("last_group") > 4096
    d = torch.from_numpy(llrs).cuda()
    bits = torch.zeros((len(llrs), dec.n), dtype=torch.uint8, device="cuda")
    its = torch.zeros(len(llrs), dtype=torch.int32, device="cuda")
    dec.decode_batch_device(d.data_ptr(), False, len(llrs), 20, bits.data_ptr(), dec.n, its.data_ptr(), 0, 0)
    torch.cuda.synchronize()
    assert dec.get("last_group") > 4096
    assert np.array_equal(bits.cpu().numpy(), want[0]) and np.array_equal(its.cpu().numpy(), want[1])
    for group in (4096, 1024):
        dec.set("group_size", group)
        assert dec.get("preferred_group") == group
        got = dec.decode_batch(llrs, 20, want_posterior=True)
        for a, b in zip(got, want):
            assert np.array_equal(a, b), (impl, group)
    g = oracle.Graph(alist(spec))
    sub = slice(0, 9000, 75)
    ob_, oi_, op_ = oracle.decode_batch(g, impl, full[sub], 20, threads=8)
    assert np.array_equal(want[1][sub], oi_) and np.array_equal(want[0][sub], ob_)
    assert np.array_equal(want[2][sub].astype(np.float64), op_)
    assert (want[1] > 0).any()


def test_minsum_dvbs2_normal_bit_exact(oracle):
    """the headline code (n = 64800, rate 1/2) at a size the oracle finishes in seconds"""
    msgs, (bits, its, post), (obits, oits, opost) = run_both(oracle, "dvbs2:R1_2", "Minsumf32", 64, 1.45, 30,
                                                            seed=3)
    assert np.array_equal(its, oits)
    assert np.array_equal(bits, obits)
    assert np.array_equal(post, opost.astype(np.float32))


def test_minsum_headline_operating_point_matches_oracle(oracle):
    """bench.py's fixed-work point itself (BASELINE.json configs[1] at P1 of SURVEY.md section 8(d)): DVB-S2 n = 64800 rate
    1/2, Minsumf32, Eb/N0 = 0 dB, 50 iterations -- no frame converges, every one runs all iterations -- 256 frames of the
    library's own Philox stream (the frames bench.py decodes: seed 1000) against the oracle: hard decisions, the -1 flags
    and the posterior after 50 iterations, bit for bit.  bench.py's `cpu_baseline.matches_gpu_output` is this check inside
    the benchmark; here it runs in the driver's suite."""
    spec, impl, frames = "dvbs2:R1_2", "Minsumf32", 256
    gen = lt.Simulator(alist(spec), impl, "", device=0, pool_size=64, pool_seed=1000)
    llrs, idx = gen.generate(0.0, 1000, 0, frames)
    gen.close()
    dec = lt.LdpcDecoder(alist(spec), impl)
    bits, its, post = dec.decode_batch(llrs, 50, want_posterior=True)
    assert dec.get("row_records") == 3                      # the headline kernel family ran
    obits, oits, opost = oracle.decode_batch(oracle.Graph(alist(spec)), impl, llrs, 50, threads=os.cpu_count() or 8)
    assert (oits == -1).all(), "P1 must be a fixed-work point: no frame converges"
    assert np.array_equal(its, oits)
    assert np.array_equal(bits, obits)
    assert np.array_equal(post, opost.astype(np.float32))


# ---- transcendental rules (bit-exact) ----------------------------------------------------------

TRANSCENDENTAL = [p + r + s for p in ("", "HL") for r in ("Phi", "Tanh", "Minstarapprox", "Aminstar")
                  for s in ("f32", "f64")]


@pytest.mark.parametrize("impl", TRANSCENDENTAL)
@pytest.mark.parametrize("spec,punct,ebn0", [("ar4ja:1/2:1024", "1,1,1,1,0", 1.6), ("nr5g:2:24", "", 1.2)])
def test_transcendental_rules(oracle, impl, spec, punct, ebn0):
    """the device uses glibc-identical exp/log/log1p/tanh in both precisions (csrc/exact_math.h), so
    Phi/Tanh/Minstarapprox/Aminstar are BIT-IDENTICAL to the CPU oracle, posterior LLRs included"""
    msgs, (bits, its, post), (obits, oits, opost) = run_both(oracle, spec, impl, 128, ebn0, 20, seed=5,
                                                            puncturing=punct)
    assert np.array_equal(its, oits)
    assert np.array_equal(bits, obits)
    assert np.array_equal(post, opost.astype(post.dtype))


def test_transcendental_f32_bit_exact_on_dvbs2_short(oracle):
    """a larger code (n = 16200, check degrees up to 7+) for the two sum-product rules"""
    for impl in ("Tanhf32", "Phif32", "Aminstarf32"):
        msgs, (bits, its, post), (obits, oits, opost) = run_both(oracle, "dvbs2:R1_2short", impl, 96, 0.9, 25,
                                                                seed=17)
        assert np.array_equal(its, oits), impl
        assert np.array_equal(bits, obits), impl
        assert np.array_equal(post, opost.astype(np.float32)), impl


def test_committed_golden_vectors():
    """HIP path against tests/golden/oracle_vectors.npz (self-generated by the oracle)"""
    import os
    v = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_vectors.npz"))
    spec, max_iter = str(v["spec"]), int(v["max_iterations"])
    for impl in lt.ALL_IMPLEMENTATIONS:
        dec = lt.LdpcDecoder(alist(spec), impl)
        llrs = v["llrs"].astype(np.float64) if impl.endswith("f64") else v["llrs"]
        bits, its, post = dec.decode_batch(llrs, max_iter, want_posterior=True)
        obits = np.unpackbits(v[impl + "/bits"], axis=1)[:, :dec.n]
        oits, opost = v[impl + "/iterations"], v[impl + "/posterior"]
        assert np.array_equal(its, oits) and np.array_equal(bits, obits), impl
        assert (its == 0).any() and (its > 0).any(), impl          # the pre-check path and the iterative one
        assert np.array_equal(post.astype(np.int8) if "i8" in impl else post, opost), impl


# ---- contract details of the boundary -----------------------------------------------------------

def test_scalar_and_batch_calls_agree(oracle):
    spec, punct = "ar4ja:1/2:1024", "1,1,1,1,0"
    msgs, llrs, full = awgn_frames(spec, 6, 2.3, 21, punct)
    dec = lt.LdpcDecoder(alist(spec), "Minsumf32", punct)
    bits, its, _ = dec.decode_batch(llrs, 40)
    for b in range(len(llrs)):
        ok, out = dec.decode(llrs[b], 40)                       # _decode_f32
        ok64, out64 = dec.decode(llrs[b].astype(np.float64), 40)  # _decode_f64 (lossless widening)
        assert ok == (its[b] >= 0) and ok64 == ok
        assert np.array_equal(out.codeword, bits[b]) and np.array_equal(out64.codeword, bits[b])
        assert out.iterations == (its[b] if ok else 40)


@pytest.mark.parametrize("spec,punct,ebn0", [("ar4ja:1/2:1024", "1,1,1,1,0", 2.0), ("dvbs2:R1_2short", "", 1.6),
                                             ("dvbs2:R1_2", "", 1.7), ("nr5g:1:24", "", 1.0)])
def test_small_batch_latency_path_equals_batch_path(oracle, spec, punct, ebn0):
    """Batches of up to 8 codewords of flooding Minsumf32 -- the reference's one-codeword-per-call pattern
    (c_api/decoder.rs:50-67) -- take the single-launch path with the lanes across one codeword's rows
    (csrc/latency.hip.h).  Same bits, iteration counts and posterior LLRs as the batched kernels ("latency" = 0)
    and as the oracle: f32 and f64 entries, pre-check hits, failures, max_iterations = 0, more codewords than
    XCDs (they take turns), host and device buffers."""
    import torch
    msgs, llrs, full = awgn_frames(spec, 19, ebn0, 77, punct)
    from ldpc_toolbox_amd import simulation as sim
    tx = lt.Encoder(alist(spec), punct).encode(msgs[0], llrs.shape[1])
    llrs[5] = np.where(tx == 1, -4.0, 4.0)                         # a transmitted codeword, noise-free
    full = sim.depuncture(llrs, sim.parse_puncturing_pattern(punct)) if punct else llrs
    dec = lt.LdpcDecoder(alist(spec), "Minsumf32", punct)
    g = oracle.Graph(alist(spec))
    for max_it in (25, 0):
        dec.set("latency", 0)
        want = dec.decode_batch(llrs, max_it, want_posterior=True)
        ob_, oi_, op_ = oracle.decode_batch(g, "Minsumf32", full[:8], max_it, threads=8)
        assert np.array_equal(want[1][:8], oi_) and np.array_equal(want[0][:8], ob_)
        if max_it:
            assert (want[1] > 1).any() and (punct or want[1][5] == 0)     # (a punctured bit's LLR 0 reads as bit 1)
        for latency, sizes in ((8, (1, 3, 8)), (32, (11, 19)), (0, (2,))):
            dec.set("latency", latency)
            for B in sizes:
                got = dec.decode_batch(llrs[:B], max_it, want_posterior=True)
                for a_, b_ in zip(got, want):
                    assert np.array_equal(a_, b_[:B]), (spec, max_it, B)
                got64 = dec.decode_batch(llrs[:B].astype(np.float64), max_it, want_posterior=True)
                assert np.array_equal(got64[0], want[0][:B]) and np.array_equal(got64[1], want[1][:B])
                assert np.array_equal(got64[2], want[2][:B].astype(np.float64))
        # device-resident entry
        dec.set("latency", 8)
        d = torch.from_numpy(llrs[:8]).cuda()
        bits = torch.zeros((8, dec.n), dtype=torch.uint8, device="cuda")
        its = torch.zeros(8, dtype=torch.int32, device="cuda")
        post = torch.zeros((8, dec.n), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        dec.decode_batch_device(d.data_ptr(), False, 8, max_it, bits.data_ptr(), dec.n, its.data_ptr(), post.data_ptr(), 0)
        torch.cuda.synchronize()
        assert np.array_equal(bits.cpu().numpy(), want[0][:8]) and np.array_equal(its.cpu().numpy(), want[1][:8])
        assert np.array_equal(post.cpu().numpy(), want[2][:8])
    # the scalar entries themselves, many calls on one handle
    dec.set("latency", 0)
    wb, wi, _ = dec.decode_batch(llrs, 25)
    dec.set("latency", 8)
    for b in range(19):
        ok, out = dec.decode(llrs[b], 25)
        assert ok == (wi[b] >= 0) and np.array_equal(out.codeword, wb[b]) and out.iterations == (wi[b] if ok else 25)


EDGE_LATENCY_IMPLS = ["HLMinsumf32", "HLTanhf32", "HLPhif32", "HLMinstarapproxf32", "HLAminstarf32",     # layered, f32
                      "HLPhif64", "HLTanhf64", "HLMinsumf64", "HLAminstarf64",                              # layered, f64
                      "Phif64", "Phif32", "Tanhf32", "Tanhf64", "Minstarapproxf32", "Aminstarf32", "Aminstarf64",
                      "Minstarapproxf64", "Minsumf64"]                                                        # flooding


@pytest.mark.parametrize("impl", EDGE_LATENCY_IMPLS + list(lt.I8_IMPLEMENTATIONS))
@pytest.mark.parametrize("spec,punct,ebn0", [("nr5g:1:24", "", 1.0), ("nr5g:2:24", "", 1.2), ("ar4ja:1/2:1024", "1,1,1,1,0", 2.2)])
def test_small_batch_edge_latency_path_equals_batch_path(oracle, spec, punct, ebn0, impl):
    """Small batches of the layered schedule (every float rule, the 8-bit rules) and of the flooding schedule's
    sum-product family and 8-bit rules --
    among them flooding Phif64, the decoder the reference's command line defaults to (src/cli/ber.rs:49) -- take one
    persistent launch with the lanes across the EDGES of one codeword's rows (csrc/latency_edge.hip.h; the
    reference's one-codeword-per-call pattern, c_api/decoder.rs:50-67).  Same bits, iteration counts and posterior
    LLRs as the batched kernels ("latency" = 0) and as the oracle: f32 and f64 entries, pre-check hits, failures,
    max_iterations = 0, more codewords than XCDs, host and device buffers, scalar calls."""
    import torch
    f64 = impl.endswith("f64")
    base_t, other_t = (np.float64, np.float32) if f64 else (np.float32, np.float64)
    msgs, llrs, full = awgn_frames(spec, 19, ebn0, 78, punct)
    from ldpc_toolbox_amd import simulation as sim
    tx = lt.Encoder(alist(spec), punct).encode(msgs[0], llrs.shape[1])
    llrs[5] = np.where(tx == 1, -4.0, 4.0)                         # a transmitted codeword, noise-free
    full = sim.depuncture(llrs, sim.parse_puncturing_pattern(punct)) if punct else llrs
    llrs = llrs.astype(base_t)
    dec = lt.LdpcDecoder(alist(spec), impl, punct)
    g = oracle.Graph(alist(spec))
    for max_it in (20, 0):
        dec.set("latency", 0)
        want = dec.decode_batch(llrs, max_it, want_posterior=True)
        ob_, oi_, op_ = oracle.decode_batch(g, impl, full[:8], max_it, threads=8)
        assert np.array_equal(want[1][:8], oi_) and np.array_equal(want[0][:8], ob_)
        assert np.array_equal(want[2][:8].astype(np.float64), op_)
        if max_it:
            assert (want[1] > 1).any() and (punct or want[1][5] == 0)
        # (up to 8 codewords: one per XCD; more: bundles of up to 8 per XCD that share every phase and barrier)
        for latency, sizes in ((64, (1, 3, 8, 11, 19)), (0, (2,))):
            dec.set("latency", latency)
            for B in sizes:
                got = dec.decode_batch(llrs[:B], max_it, want_posterior=True)
                assert dec.get("last_group") == (B if latency else dec.get("last_group"))
                for a_, b_ in zip(got, want):
                    assert np.array_equal(a_, b_[:B]), (spec, impl, max_it, B)
                # the other entry (f64 LLRs into an f32 rule / f32 LLRs into an f64 rule)
                if not f64 or np.array_equal(llrs[:B].astype(np.float32).astype(np.float64), llrs[:B]):
                    goto = dec.decode_batch(llrs[:B].astype(other_t), max_it, want_posterior=True)
                    assert np.array_equal(goto[0], want[0][:B]) and np.array_equal(goto[1], want[1][:B])
                    assert np.array_equal(goto[2], want[2][:B].astype(other_t))
        dec.set("latency", 8)
        d = torch.from_numpy(llrs[:8]).cuda()
        bits = torch.zeros((8, dec.n), dtype=torch.uint8, device="cuda")
        its = torch.zeros(8, dtype=torch.int32, device="cuda")
        post = torch.zeros((8, dec.n), dtype=torch.float64 if f64 else torch.float32, device="cuda")
        torch.cuda.synchronize()
        dec.decode_batch_device(d.data_ptr(), f64, 8, max_it, bits.data_ptr(), dec.n, its.data_ptr(), post.data_ptr(), 0)
        torch.cuda.synchronize()
        assert np.array_equal(bits.cpu().numpy(), want[0][:8]) and np.array_equal(its.cpu().numpy(), want[1][:8])
        assert np.array_equal(post.cpu().numpy(), want[2][:8])
    dec.set("latency", 0)
    wb, wi, _ = dec.decode_batch(llrs, 20)
    dec.set("latency", 8)
    for b in range(19):
        ok, out = dec.decode(llrs[b], 20)
        assert ok == (wi[b] >= 0) and np.array_equal(out.codeword, wb[b]) and out.iterations == (wi[b] if ok else 20)
    # a larger call: 64 codewords = 8 XCDs x bundles of 8 (frames repeated: the results must repeat)
    dec.set("latency", 64)
    big = np.concatenate([llrs, llrs, llrs, llrs[:7]])
    gb, gi, _ = dec.decode_batch(big, 20)
    assert "Aminstar" in impl or dec.get("last_group") == 64       # (A-Min* takes the path up to 32 codewords)
    rep = np.concatenate([np.arange(19)] * 3 + [np.arange(7)])
    assert np.array_equal(gb, wb[rep]) and np.array_equal(gi, wi[rep])
    # the layered schedule's sum-product and 8-bit rules keep the path for further rounds inside the launch
    if impl.startswith("HL") and "Minsum" not in impl:
        dec.set("latency", 256)
        B = 50 if "Aminstar" in impl else 100
        rep = np.arange(B) % 19
        gb, gi, _ = dec.decode_batch(llrs[rep], 20)
        assert dec.get("last_group") == B
        assert np.array_equal(gb, wb[rep]) and np.array_equal(gi, wi[rep])


@pytest.mark.parametrize("impl", lt.FAST_IMPLEMENTATIONS)
def test_fast_variants_are_opt_in_and_statistically_equivalent(impl):
    """"@fast" (this build's addition): the Tanh / Phi rules with the GPU's native exp2 / log2 / rcp.  NOT bit-identical to
    the reference and never the default -- only the explicit name selects it.  What is asserted is what a user of such a
    variant relies on: the same decoding performance (frame and bit error counts within a small statistical margin of
    the exact implementation on the same 2048 frames in the waterfall), nearly every frame with the same iteration
    count, soft outputs close; and that the plain name still gives the exact path (bit-identical to the oracle: every
    other test).  tools/fast_probe.py prints the full statistics and the speed (profiles/r03_fast_variants.txt)."""
    exact = impl.split("@")[0]
    assert impl not in lt.ALL_IMPLEMENTATIONS and exact in lt.ALL_IMPLEMENTATIONS
    spec = "nr5g:1:24"
    dec_exact, dec_fast = lt.LdpcDecoder(alist(spec), exact), lt.LdpcDecoder(alist(spec), impl)
    for ebn0 in (1.0, 0.6, 0.2, -0.2, -0.6):                          # down to a waterfall point of this rule
        msgs, llrs, _ = awgn_frames(spec, 2048, ebn0, 99)
        ref = dec_exact.decode_batch(llrs, 30, want_posterior=True)
        k = msgs.shape[1]
        fe_ref = int((ref[0][:, :k] != msgs).any(axis=1).sum())
        if fe_ref >= 40:
            break
    assert 40 <= fe_ref <= 1600                                       # some frames fail, a good part decode
    got = dec_fast.decode_batch(llrs, 30, want_posterior=True)
    fe_got = int((got[0][:, :k] != msgs).any(axis=1).sum())
    be_ref, be_got = int((ref[0][:, :k] != msgs).sum()), int((got[0][:, :k] != msgs).sum())
    assert abs(fe_got - fe_ref) <= max(10, 0.10 * fe_ref), (ebn0, fe_ref, fe_got)
    assert abs(be_got - be_ref) <= max(300, 0.15 * be_ref), (ebn0, be_ref, be_got)
    same_it = float((ref[1] == got[1]).mean())
    assert same_it >= 0.75, same_it
    if "Tanh" in impl:   # (the Phi rule's soft outputs of decoded frames sit on its clamp plateaus, which the native log moves)
        ok = (ref[1] >= 0) & (got[1] >= 0) & (ref[1] == got[1])
        rel = np.abs(ref[2][ok] - got[2][ok]) / (np.abs(ref[2][ok]) + 1.0)
        assert np.median(rel) < 1e-3, float(np.median(rel))
    with pytest.raises(lt.DecoderUnavailable):
        lt.LdpcDecoder(alist(spec), "Minsumf32@fast")               # only the Tanh / Phi f32 rules have such a variant
    with pytest.raises(lt.DecoderUnavailable):
        lt.LdpcDecoder(alist(spec), "Tanhf64@fast")


def test_scalar_calls_from_two_threads_on_two_handles(oracle):
    """The reference's BER driver runs one decoder per worker thread, all calling decode at once
    (simulation/ber.rs:304-310, 462-466).  Two threads, two handles, scalar calls in parallel (ctypes releases
    the GIL): the single-launch path serialises its launches per process -- its workgroups must all be resident
    together -- and every call still returns what the batched kernels return."""
    import threading
    spec = "dvbs2:R1_2short"
    msgs, llrs, full = awgn_frames(spec, 24, 1.6, 91)
    ref = lt.LdpcDecoder(alist(spec), "Minsumf32")
    ref.set("latency", 0)
    wb, wi, _ = ref.decode_batch(llrs, 30)
    results, errors = {}, []

    def worker(t):
        try:
            dec = lt.LdpcDecoder(alist(spec), "Minsumf32")
            for rep in range(3):
                for b in range(t, 24, 2):
                    ok, out = dec.decode(llrs[b], 30)
                    results[(t, rep, b)] = (ok, out.iterations, out.codeword.copy())
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert len(results) == 72
    for (t, rep, b), (ok, its, cw) in results.items():
        assert ok == (wi[b] >= 0) and its == (wi[b] if ok else 30) and np.array_equal(cw, wb[b]), (t, rep, b)


def test_output_len_prefix_and_failure_flag():
    spec = "dvbs2:R1_2short"
    msgs, llrs, _ = awgn_frames(spec, 70, -1.0, 2)   # far below threshold: every frame fails
    dec = lt.LdpcDecoder(alist(spec), "Minsumf32")
    full_bits, its, _ = dec.decode_batch(llrs, 5)
    assert (its == -1).all()
    k_bits, its2, _ = dec.decode_batch(llrs, 5, output_len=dec.k)
    assert np.array_equal(its, its2)
    assert np.array_equal(k_bits, full_bits[:, :dec.k])


def test_precheck_zero_iterations_and_zero_llrs():
    """valid codeword in -> 0 iterations; punctured (0.0) LLRs decide bit 1 (arithmetic.rs:199)"""
    spec, punct = "ar4ja:1/2:1024", "1,1,1,1,0"
    msgs, llrs, full = awgn_frames(spec, 65, 12.0, 9, punct)   # essentially noiseless
    dec = lt.LdpcDecoder(alist(spec), "Minsumf32", punct)
    bits, its, _ = dec.decode_batch(llrs, 10)
    assert (its >= 0).all()
    assert np.array_equal(bits[:, :dec.k], msgs)
    # all-zero codeword with strong positive LLRs and no puncturing: pre-check passes
    dec2 = lt.LdpcDecoder(alist(spec), "Minsumf32")
    ok, out = dec2.decode(np.full(dec2.n, 4.0), 10)
    assert ok and out.iterations == 0 and not out.codeword.any()


def test_max_iterations_zero_matches_reference_semantics(oracle):
    spec = "dvbs2:R1_2short"
    msgs, llrs, full = awgn_frames(spec, 64, 0.5, 4)
    for impl in ("Minsumf32", "HLPhif32"):
        if impl.startswith("HL"):
            spec2, (m2, l2, f2) = "nr5g:2:24", awgn_frames("nr5g:2:24", 64, 0.5, 4)
        else:
            spec2, (m2, l2, f2) = spec, (msgs, llrs, full)
        dec = lt.LdpcDecoder(alist(spec2), impl)
        bits, its, _ = dec.decode_batch(l2, 0)
        g = oracle.Graph(alist(spec2))
        obits, oits, _ = oracle.decode_batch(g, impl, f2, 0, threads=2)
        assert np.array_equal(its, oits)
        assert np.array_equal(bits, obits)


def test_errors_are_loud():
    spec = "ar4ja:1/2:1024"
    with pytest.raises(lt.DecoderUnavailable):
        lt.LdpcDecoder(alist(spec), "NoSuchRulef32")
    with pytest.raises(lt.DecoderUnavailable):
        lt.LdpcDecoder(alist(spec), "HLMinstarapproxi8Jones")   # not one of the reference's 36 names
    with pytest.raises(lt.DecoderUnavailable):
        lt.LdpcDecoder("not an alist", "Minsumf32")
    with pytest.raises(lt.DecoderUnavailable):
        lt.LdpcDecoder(alist(spec), "Minsumf32", "1,1,x")
    dec = lt.LdpcDecoder(alist(spec), "Minsumf32", "1,1,1,1,0")
    assert dec.input_len == 2048 and dec.n == 2560
    L = lt._capi.lib()
    out = np.zeros(dec.n, dtype=np.uint8)
    bad = np.zeros(100, dtype=np.float32)
    assert L.ldpc_toolbox_decoder_decode_f32(dec._h, out.ctypes.data, dec.n, bad.ctypes.data, 100, 5) == -4  # LDPC_TOOLBOX_ERR_ARGUMENT: below -1, never a "decoding failure"
    assert "length" in lt._capi.last_error()
    assert (out == 0).all()                                   # nothing written
    # the batch and syndrome entries speak the same error vocabulary as the scalar ones
    its = np.zeros(2, dtype=np.int32)
    bad2 = np.zeros((2, 100), dtype=np.float32)
    assert L.ldpc_toolbox_decoder_decode_batch_f32(dec._h, out.ctypes.data, dec.n, bad2.ctypes.data, 100, 2, 5,
                                                   its.ctypes.data, None) == -4
    assert L.ldpc_toolbox_decoder_decode_batch_f32(None, out.ctypes.data, dec.n, bad2.ctypes.data, 100, 2, 5,
                                                   its.ctypes.data, None) == -4
    assert L.ldpc_toolbox_decoder_syndrome(dec._h, out.ctypes.data, 100, 1, None, None) == -4


# ---- full-size properties (no oracle: it would take minutes) ----------------------------------

def test_full_size_round_trip_dvbs2():
    """encode -> AWGN above threshold -> decode returns the message; batch = several tiles"""
    spec = "dvbs2:R1_2"
    msgs, llrs, _ = awgn_frames(spec, 320, 2.0, 31)
    dec = lt.LdpcDecoder(alist(spec), "Minsumf32")
    bits, its, _ = dec.decode_batch(llrs, 50, output_len=dec.k)
    assert (its >= 0).mean() > 0.98
    ok = its >= 0
    assert np.array_equal(bits[ok], msgs[ok])
    # decoding is deterministic and independent of grouping
    dec.set("group_size", 64)
    bits2, its2, _ = dec.decode_batch(llrs, 50, output_len=dec.k)
    assert np.array_equal(its, its2) and np.array_equal(bits, bits2)


def test_device_resident_entry_matches_host_entry():
    torch = pytest.importorskip("torch")
    spec = "dvbs2:R1_2short"
    msgs, llrs, _ = awgn_frames(spec, 300, 1.7, 8)
    dec = lt.LdpcDecoder(alist(spec), "Minsumf32", device=0)
    bits, its, post = dec.decode_batch(llrs, 30, want_posterior=True)
    dev = torch.device("cuda:0")
    d_llrs = torch.from_numpy(llrs).to(dev)
    d_bits = torch.zeros((300, dec.n), dtype=torch.uint8, device=dev)
    d_its = torch.zeros(300, dtype=torch.int32, device=dev)
    d_post = torch.zeros((300, dec.n), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev)
    dec.decode_batch_device(d_llrs.data_ptr(), False, 300, 30, d_bits.data_ptr(), dec.n, d_its.data_ptr(),
                            d_post.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(d_its.cpu().numpy(), its)
    assert np.array_equal(d_bits.cpu().numpy(), bits)
    assert np.array_equal(d_post.cpu().numpy(), post)
    # the f64 entry (f64 LLR rows in, f64 posterior out), float / double / 8-bit arithmetics, null stream
    l64 = llrs.astype(np.float64)
    d_l64 = torch.from_numpy(l64).to(dev)
    d_p64 = torch.zeros((300, dec.n), dtype=torch.float64, device=dev)
    for impl in ("Phif64", "HLMinsumf32", "Aminstari8Jones"):
        d2 = lt.LdpcDecoder(alist(spec), impl, device=0)
        want = d2.decode_batch(l64, 12, output_len=d2.k, want_posterior=True)
        d_b2 = torch.zeros((300, d2.k), dtype=torch.uint8, device=dev)
        d2.decode_batch_device(d_l64.data_ptr(), True, 300, 12, d_b2.data_ptr(), d2.k, d_its.data_ptr(), d_p64.data_ptr(), 0)
        assert np.array_equal(d_its.cpu().numpy(), want[1]), impl       # own stream: synchronised on return
        assert np.array_equal(d_b2.cpu().numpy(), want[0]) and np.array_equal(d_p64.cpu().numpy(), want[2]), impl


# ---- BER driver on the GPU path vs the same driver on the oracle --------------------------------

def test_ber_driver_config1_matches_oracle(oracle):
    """BASELINE config 1: CCSDS AR4JA r=1/2 k=1024, puncturing 1,1,1,1,0, flooding min-sum,
    50 iterations, Eb/N0 = 2 dB -- identical frames => identical counters (BER to every digit)."""
    from ldpc_toolbox_amd import simulation as sim
    spec, punct = "ar4ja:1/2:1024", "1,1,1,1,0"
    a = alist(spec)
    pattern = sim.parse_puncturing_pattern(punct)
    enc = lt.Encoder(a)
    dec = lt.LdpcDecoder(a, "Minsumf32", punct)
    g = oracle.Graph(a)

    def gpu_decode(llrs, it):
        bits, its, _ = dec.decode_batch(llrs, it, output_len=dec.k)
        return bits, its

    def cpu_decode(llrs, it):
        bits, its, _ = oracle.decode_batch(g, "Minsumf32", sim.depuncture(llrs, pattern), it, threads=8,
                                           want_posterior=False)
        return bits, its

    common = dict(k=dec.k, n=dec.n, ebn0s_db=[2.0, 2.4], max_iterations=50, puncturing_pattern=pattern,
                  max_frames=768, max_frame_errors=10 ** 9, frames_per_batch=256, seed=77)
    rg = sim.BerTest(a, lambda m: enc.encode(m, dec.n), gpu_decode, **common).run()
    rc = sim.BerTest(a, lambda m: enc.encode(m, dec.n), cpu_decode, **common).run()
    for x, y in zip(rg, rc):
        assert x.num_frames == y.num_frames == 768
        assert (x.ldpc.bit_errors, x.ldpc.frame_errors, x.false_decodes, x.total_iterations,
                x.ldpc.correct_iterations) == (y.ldpc.bit_errors, y.ldpc.frame_errors, y.false_decodes,
                                               y.total_iterations, y.ldpc.correct_iterations)
        assert x.ldpc.ber == y.ldpc.ber and x.ldpc.fer == y.ldpc.fer
    assert rg[0].ldpc.frame_errors > 0            # 2 dB is inside the waterfall of unscaled min-sum
    print(sim.format_header())
    for x in rg:
        print(sim.format_progress(x))


# ---- more of BASELINE.json's configurations and edge cases ----------------------------------------

DVBS2_NORMAL = ["R1_4", "R1_3", "R2_5", "R1_2", "R3_5", "R2_3", "R3_4", "R4_5", "R5_6", "R8_9", "R9_10"]


@pytest.mark.parametrize("code", DVBS2_NORMAL)
def test_all_dvbs2_normal_rates_bit_exact(oracle, code):
    """config 5's codes: every DVB-S2 normal-frame rate (check degrees 4..30), a few frames each"""
    spec = "dvbs2:" + code
    n, m = (int(x) for x in alist(spec).split("\n", 1)[0].split())
    rate = (n - m) / n
    # a point inside each code's waterfall region for unscaled min-sum (Shannon limit + ~1.3 dB)
    ebn0 = 10 * np.log10((2 ** (2 * rate) - 1) / (2 * rate)) + 1.6
    msgs, (bits, its, post), (obits, oits, opost) = run_both(oracle, spec, "Minsumf32", 8, ebn0, 12, seed=41)
    assert np.array_equal(its, oits)
    assert np.array_equal(bits, obits)
    assert np.array_equal(post, opost.astype(np.float32))


def test_config3_nr5g_bg1_zc384_layered_tanh_bit_exact(oracle):
    """config 3's code and rule at a size the oracle finishes in seconds: 5G NR BG1 Zc=384
    (n = 26112, check degree up to 19), HLTanhf32"""
    msgs, (bits, its, post), (obits, oits, opost) = run_both(oracle, "nr5g:1:384", "HLTanhf32", 24, 0.6, 12,
                                                            seed=43)
    assert np.array_equal(its, oits)
    assert np.array_equal(bits, obits)
    assert np.array_equal(post, opost.astype(np.float32))
    assert (its > 0).any()


def test_batch_edge_sizes(oracle):
    """empty batch, one frame, one more than a group, groups of 192 codewords"""
    spec, punct = "ar4ja:1/2:1024", "1,1,1,1,0"
    dec = lt.LdpcDecoder(alist(spec), "Minsumf32", punct)
    bits, its, post = dec.decode_batch(np.zeros((0, dec.input_len), dtype=np.float32), 10, want_posterior=True)
    assert bits.shape == (0, dec.n) and its.shape == (0,)
    for batch in (1, 257, 130, 190):
        # 130, 190 in one group: a 192-codeword tile, which 128-codeword wave slices do not divide
        dec.set("group_size", 256 if batch in (1, 257) else 0)
        msgs, llrs, full = awgn_frames(spec, batch, 2.2, 100 + batch, punct)
        bits, its, post = dec.decode_batch(llrs, 20, want_posterior=True)
        g = oracle.Graph(alist(spec))
        obits, oits, opost = oracle.decode_batch(g, "Minsumf32", full, 20, threads=8)
        assert np.array_equal(its, oits) and np.array_equal(bits, obits)
        assert np.array_equal(post, opost.astype(np.float32))


def test_full_size_codeword_symmetry_property():
    """Size-independent property at BASELINE's full size (DVB-S2 n=64800, 4096 frames, 50
    iterations): the decoder is symmetric, so decoding y for transmitted codeword c equals
    decoding the all-zero-codeword equivalent y * (1 - 2c) XOR c -- same iterations, same error
    pattern -- for every frame, with early termination active."""
    spec = "dvbs2:R1_2"
    B = 4096
    dec = lt.LdpcDecoder(alist(spec), "Minsumf32")
    enc = lt.Encoder(alist(spec))
    rng = np.random.Generator(np.random.Philox(key=[7, 7]))
    from ldpc_toolbox_amd import simulation as sim
    sigma = sim.noise_sigma(0.5, 1.75)
    noise = (sigma * rng.standard_normal((B, dec.n))).astype(np.float32)
    cws = np.zeros((B, dec.n), dtype=np.uint8)
    base = np.stack([enc.encode(rng.integers(0, 2, dec.k, dtype=np.uint8), dec.n) for _ in range(16)])
    cws[:] = base[np.arange(B) % 16]
    sign = 1.0 - 2.0 * cws.astype(np.float32)                    # bit 0 -> +1 (LLR > 0 <=> bit 0)
    scale = np.float32(2.0 / sigma ** 2)
    llr_zero = scale * (1.0 + noise)                             # all-zero codeword
    llr_cw = llr_zero * sign                                     # exact: multiplication by +-1
    b0, i0, _ = dec.decode_batch(llr_zero, 50)
    b1, i1, _ = dec.decode_batch(llr_cw, 50)
    assert np.array_equal(i0, i1)
    assert np.array_equal(b0 ^ cws, b1)
    ok = i0 >= 0
    assert 0.5 < ok.mean() <= 1.0
    assert not b0[ok].any()                                      # converged frames are the codeword


def _device_frames(dec, enc, batch, ebn0_db, seed, pool=16):
    """frames resident in HBM (torch): `pool` random codewords repeated over the batch, BPSK over AWGN in f32.
    -> (codewords [batch][n] u8 numpy, llrs [batch][n] f32 cuda tensor)"""
    import torch
    from ldpc_toolbox_amd import simulation as sim
    rng = np.random.Generator(np.random.Philox(key=[seed, 1]))
    base = np.stack([enc.encode(rng.integers(0, 2, dec.k, dtype=np.uint8), dec.n) for _ in range(pool)])
    idx = np.arange(batch) % pool
    sigma = sim.noise_sigma(dec.k / dec.n, ebn0_db)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(seed)
    sym = torch.from_numpy(base).to(dev)[torch.from_numpy(idx).to(dev)].to(torch.float32) * 2.0 - 1.0
    y = sym + sigma * torch.randn(sym.shape, generator=g, device=dev, dtype=torch.float32)
    llrs = ((-2.0 / (sigma * sigma)) * y).contiguous()
    torch.cuda.synchronize()
    return base[idx], llrs


def _decode_device(dec, llrs, max_iter, out_len):
    import torch
    B = llrs.shape[0]
    bits = torch.zeros((B, out_len), dtype=torch.uint8, device=llrs.device)
    its = torch.zeros(B, dtype=torch.int32, device=llrs.device)
    dec.decode_batch_device(llrs.data_ptr(), False, B, max_iter, bits.data_ptr(), out_len, its.data_ptr(), 0, 0)
    torch.cuda.synchronize()
    return bits, its


def test_config3_full_size_properties(oracle):
    """BASELINE config 3 at its full size -- 5G NR BG1 Zc=384, HLTanhf32, 8192 frames, 50 iterations, early
    termination active -- through properties that need no oracle pass over the whole batch:
      * round trip: every frame reported as decoded is a codeword (zero syndrome) and, at this Eb/N0, the
        transmitted one; every frame reported as failed has a non-zero syndrome;
      * position invariance: the same frames in another order (other tiles, other execution lane, other
        compaction history) give the same per-frame bits and iteration counts;
      * a 12-frame sample is bit-identical to the oracle (bits, iterations).
    (The codeword-symmetry property used for min-sum below does not hold bit for bit for this rule: Rust's
    atanh, 0.5 * ln_1p(2x / (1 - x)), is not an odd function in floating point, so the reference decoder
    itself is not sign-symmetric.)"""
    import torch
    spec, impl, B, max_iter = "nr5g:1:384", "HLTanhf32", 8192, 50
    dec = lt.LdpcDecoder(alist(spec), impl)
    enc = lt.Encoder(alist(spec))
    # the waterfall: the first Eb/N0 of a coarse scan (256 frames each) at which 30 % or more decode
    ebn0 = None
    for cand in (-0.4, -0.1, 0.2, 0.5, 0.8, 1.1, 1.4, 1.7, 2.0):
        _, probe = _device_frames(dec, enc, 256, cand, seed=908)
        _, pits = _decode_device(dec, probe, max_iter, dec.n)
        if (pits >= 0).float().mean().item() >= 0.3:
            ebn0 = cand
            break
    assert ebn0 is not None
    cws, llrs = _device_frames(dec, enc, B, ebn0, seed=909)          # decoded and failed frames, a spread of iterations
    bits, its = _decode_device(dec, llrs, max_iter, dec.n)
    its_np, bits_np = its.cpu().numpy(), bits.cpu().numpy()
    ok = its_np >= 0
    assert 0.05 < ok.mean() < 0.9999, (ebn0, ok.mean())
    assert (its_np[ok] > 0).all() and its_np[ok].max() > its_np[ok].min() + 5
    weights = np.zeros(B, dtype=np.uint32)
    L = lt._capi.lib()
    for b0 in range(0, B, 2048):                                     # the syndrome operator: H x of the outputs
        part = np.ascontiguousarray(bits_np[b0:b0 + 2048])
        w = np.zeros(len(part), dtype=np.uint32)
        assert L.ldpc_toolbox_decoder_syndrome(dec._h, part.ctypes.data, dec.n, len(part), None, w.ctypes.data) == 0
        weights[b0:b0 + 2048] = w
    assert (weights[ok] == 0).all() and (weights[~ok] > 0).all()
    assert np.array_equal(bits_np[ok], cws[ok])                      # no undetected errors at this size / Eb/N0
    # position invariance
    perm = torch.from_numpy(np.random.Generator(np.random.Philox(key=[3, 3])).permutation(B)).to(llrs.device)
    bits_p, its_p = _decode_device(dec, llrs[perm].contiguous(), max_iter, dec.n)
    assert torch.equal(its_p, its[perm]) and torch.equal(bits_p, bits[perm])
    # oracle sample: a few decoded early, a few late, a few failed
    order = np.argsort(its_np, kind="stable")
    sample = np.concatenate([order[:4], order[len(order) // 2: len(order) // 2 + 4], order[-4:]])
    g = oracle.Graph(alist(spec))
    ob_, oi_, _ = oracle.decode_batch(g, impl, llrs[torch.from_numpy(sample).to(llrs.device)].cpu().numpy(), max_iter,
                                      threads=8, want_posterior=False)
    assert np.array_equal(oi_, its_np[sample]) and np.array_equal(ob_, bits_np[sample])


def test_config4_shard_invariance_one_gpu():
    """BASELINE config 4 on one GPU: 32 768 DVB-S2 rate-1/2 frames decoded as 8 contiguous shards of 4096,
    each by a FRESH decoder handle (what 8 ranks do, one shard each: sharding.shard_range), give exactly
    what one 32 768-frame call gives -- bits and iteration counts, early termination active.  Codewords are
    independent; nothing in the device layout (groups, tiles, compaction) may couple them."""
    import torch
    from ldpc_toolbox_amd import sharding
    spec, B, world, max_iter = "dvbs2:R1_2", 32768, 8, 50
    a = alist(spec)
    dec = lt.LdpcDecoder(a, "Minsumf32")
    enc = lt.Encoder(a)
    cws, llrs = _device_frames(dec, enc, B, 1.6, seed=4242)         # waterfall of this code / rule
    bits, its = _decode_device(dec, llrs, max_iter, dec.k)
    its_np = its.cpu().numpy()
    assert (its_np >= 0).any() and (its_np < 0).any()
    del dec
    for rank in range(world):
        b, e = sharding.shard_range(B, rank, world)
        assert e - b == 4096
        shard_dec = lt.LdpcDecoder(a, "Minsumf32")
        sb, si = _decode_device(shard_dec, llrs[b:e], max_iter, shard_dec.k)
        assert torch.equal(si, its[b:e]) and torch.equal(sb, bits[b:e]), rank
        del shard_dec
    ok = its_np >= 0
    assert np.array_equal(bits.cpu().numpy()[ok], cws[ok][:, :bits.shape[1]])   # systematic: message = first k bits


def test_batch_compaction_is_invisible(oracle):
    """Early termination with batch compaction (finished codewords are retired and the live ones
    re-packed at device-decided checkpoints) returns exactly what the un-compacted decode and the
    oracle return: bits, iteration counts, posterior LLRs, in the caller's row order."""
    spec = "dvbs2:R1_2short"
    msgs, llrs, full = awgn_frames(spec, 1024, 1.45, 555)       # waterfall: a wide spread of iteration counts
    dec = lt.LdpcDecoder(alist(spec), "Minsumf32")
    dec.set("group_size", 1024)
    dec.set("compact", 1)
    b1, i1, p1 = dec.decode_batch(llrs, 40, want_posterior=True)
    dec.set("compact", 0)
    b0, i0, p0 = dec.decode_batch(llrs, 40, want_posterior=True)
    assert np.array_equal(i0, i1) and np.array_equal(b0, b1) and np.array_equal(p0, p1)
    spread = i1[i1 >= 0]
    assert spread.max() - spread.min() >= 10 and (i1 < 0).any()   # converged early, late and never
    g = oracle.Graph(alist(spec))
    sub = slice(0, 1024, 4)
    ob_, oi_, op_ = oracle.decode_batch(g, "Minsumf32", full[sub], 40, threads=8)
    assert np.array_equal(i1[sub], oi_) and np.array_equal(b1[sub], ob_)
    assert np.array_equal(p1[sub], op_.astype(np.float32))
    # the paced host (option "throttle", round 5: the host follows the group's progress word two iterations ahead and,
    # once the first codewords have converged, asks for a checkpoint after EVERY iteration), with records and with
    # per-edge messages, several groups per call, device-resident entry on the caller's stream: the same again
    import torch
    d_llrs = torch.from_numpy(llrs).cuda()
    for records, group in ((2, 1024), (0, 512), (2, 256)):
        dec.set("compact", 1)
        dec.set("throttle", 1)
        dec.set("records", records)
        dec.set("group_size", group)
        d_bits = torch.zeros((len(llrs), dec.n), dtype=torch.uint8, device="cuda")
        d_its = torch.zeros(len(llrs), dtype=torch.int32, device="cuda")
        d_post = torch.zeros((len(llrs), dec.n), dtype=torch.float32, device="cuda")
        dec.decode_batch_device(d_llrs.data_ptr(), False, len(llrs), 40, d_bits.data_ptr(), dec.n, d_its.data_ptr(),
                                d_post.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(d_its.cpu().numpy(), i0) and np.array_equal(d_bits.cpu().numpy(), b0), (records, group)
        assert np.array_equal(d_post.cpu().numpy(), p0), (records, group)
    # layered schedule as well
    decl = lt.LdpcDecoder(alist("nr5g:2:24"), "HLMinsumf32")
    m2, l2, f2 = awgn_frames("nr5g:2:24", 1024, 0.9, 556)
    decl.set("compact", 1)
    b1, i1, p1 = decl.decode_batch(l2, 40, want_posterior=True)
    decl.set("compact", 0)
    b0, i0, p0 = decl.decode_batch(l2, 40, want_posterior=True)
    assert np.array_equal(i0, i1) and np.array_equal(b0, b1) and np.array_equal(p0, p1)


@pytest.mark.parametrize("spec,impl,ebn0", [("dvbs2:R8_9short", "Minsumf32", 4.2), ("nr5g:2:24", "Tanhf32", 1.4)])
def test_flooding_two_lanes_with_paced_threads_are_invisible(spec, impl, ebn0):
    """Two execution lanes of the flooding schedule under option "throttle" (round 5): a host thread per lane, each following
    its own group's progress word two iterations ahead and ending every iteration with a checkpoint once convergence has
    begun -- against one thread enqueuing both lanes blind (lane_threads = 0) and against one lane: the same bits, iteration
    counts and posteriors on the device-resident entry (caller's stream), whole and ragged groups."""
    import torch
    msgs, llrs, full = awgn_frames(spec, 2304, ebn0, 4711)
    dec = lt.LdpcDecoder(alist(spec), impl)
    dec.set("lanes", 1)
    dec.set("group_size", 4096)
    want = dec.decode_batch(llrs, 30, want_posterior=True)
    assert (want[1] >= 0).any()
    d_llrs = torch.from_numpy(llrs).cuda()
    for threads, throttle, group in ((1, 1, 1024), (0, 1, 1024), (1, 1, 768), (1, 0, 512)):
        for key, v in (("lanes", 2), ("lane_threads", threads), ("throttle", throttle), ("group_size", group)):
            dec.set(key, v)
        d_bits = torch.zeros((len(llrs), dec.n), dtype=torch.uint8, device="cuda")
        d_its = torch.zeros(len(llrs), dtype=torch.int32, device="cuda")
        d_post = torch.zeros((len(llrs), dec.n), dtype=torch.float32, device="cuda")
        dec.decode_batch_device(d_llrs.data_ptr(), False, len(llrs), 30, d_bits.data_ptr(), dec.n, d_its.data_ptr(),
                                d_post.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert dec.get("last_lanes") == 2
        assert np.array_equal(d_its.cpu().numpy(), want[1]), (threads, throttle, group)
        assert np.array_equal(d_bits.cpu().numpy(), want[0]) and np.array_equal(d_post.cpu().numpy(), want[2]), (threads, throttle, group)


@pytest.mark.parametrize("spec,impl,ebn0,puncturing", [
    ("dvbs2:R1_2short", "Minsumf32", 1.45, ""),      # staircase: peers are the neighbouring rows (the fast path)
    ("dvbs2:R8_9short", "Minsumf32", 4.2, ""),       # rows of 27 edges: four-word records, several rounds per row
    ("dvbs2:R1_4short", "Minsumf64", 1.6, ""),       # f64 records (64-bit flip word)
    ("nr5g:2:24", "Minsumf32", 1.2, ""),             # degree-1 variables (no peer), peers far from the row
    ("ar4ja:1/2:1024", "Minsumf32", 2.2, "1,1,1,1,0"),  # punctured degree-1/2 mix
])
def test_row_records_are_invisible(oracle, spec, impl, ebn0, puncturing):
    """Flooding min-sum with the check rows' messages kept as records {min1, min2, flip bits, argmin}
    (cn_minsum_rec_kernel, the default) returns exactly what the per-edge message kernels and the oracle
    return -- bits, iteration counts, posterior LLRs -- with and without the deferred L-free posterior stores
    ("rec_quiet"), with and without batch compaction, for every run length of the row walk."""
    msgs, llrs, full = awgn_frames(spec, 768, ebn0, 4242, puncturing)
    gpu_in = llrs.astype(np.float64) if impl.endswith("f64") else llrs
    dec = lt.LdpcDecoder(alist(spec), impl, puncturing)
    dec.set("group_size", 768)
    dec.set("records", 0)
    ref = dec.decode_batch(gpu_in, 30, want_posterior=True)
    spread = ref[1][ref[1] >= 0]
    assert len(spread) and spread.max() - spread.min() >= 5        # convergences spread over the iterations
    # ("records" = 2: also on graphs whose degree-2 variables join distant rows, where the default keeps per-edge messages)
    # ("vn_event": the first convergences' L-free posteriors rebuilt inside the variable-node launch -- the default -- or by a
    # launch of their own)
    for opts in ({"records": 2}, {"records": 2, "vn_event": 0}, {"records": 2, "vn_event": 0, "compact": 0},
                 {"records": 2, "vn_event": 1, "rec_quiet": 0}, {"records": 2, "rec_quiet": 1, "compact": 0, "vn_event": 1},
                 {"records": 2, "compact": 1, "rec_run": 1}, {"records": 2, "rec_run": 3},
                 {"records": 2, "rec_run": 64, "vec": 2}, {"records": 2, "rec_run": 8, "vec": 1}):
        for k, v in opts.items():
            dec.set(k, v)
        got = dec.decode_batch(gpu_in, 30, want_posterior=True)
        for a, b in zip(ref, got):
            assert np.array_equal(a, b), (opts,)
        assert dec.get("row_records") in (3, 4)
    g = oracle.Graph(alist(spec))
    sub = slice(0, 768, 6)
    ob_, oi_, op_ = oracle.decode_batch(g, impl, full[sub], 30, threads=8)
    assert np.array_equal(ref[1][sub], oi_) and np.array_equal(ref[0][sub], ob_)
    assert np.array_equal(ref[2][sub].astype(np.float64), op_)


@pytest.mark.parametrize("impl", ["HLMinsumf32", "HLMinsumf64", "HLTanhf32", "HLMinstarapproxi8"])
def test_layered_execution_choices_are_invisible(oracle, impl):
    """The layered schedule's launch-level choices -- register-resident rows (hl_reg) versus the
    two-pass form, row records versus per-edge messages for min-sum (hl_records), with and without batch compaction,
    one execution lane versus two half-batches on two streams (enqueued by one host thread or two) -- change nothing in
    what the caller gets, on the host-buffer and on the device-resident entry, and match the oracle."""
    import torch
    spec = "nr5g:1:16"                                            # BG1: rows of degree 3..19, both buckets
    msgs, llrs, full = awgn_frames(spec, 2304, 1.0, 777)
    dec = lt.LdpcDecoder(alist(spec), impl)
    want = None
    # (hl_records: layered min-sum keeps a row's messages R as one record {min1, min2, flip bits | argmin})
    # (threads: the two lanes' launches enqueued by two host threads or by one; throttle: the device-resident entry
    # paces itself on the groups' progress words too)
    for hl_reg, lanes, group, hl_rec, compact, threads, throttle in (
            (1, 1, 4096, 1, 1, 1, 0), (0, 1, 4096, 1, 1, 1, 0), (1, 2, 4096, 0, 1, 1, 1), (1, 2, 1024, 1, 0, 1, 0),
            (0, 2, 512, 0, 1, 0, 1), (1, 2, 768, 1, 1, 0, 0), (1, 1, 2304, 1, 1, 1, 1), (1, 1, 2304, 0, 0, 0, 0)):
        dec.set("lane_threads", threads)
        dec.set("throttle", throttle)
        dec.set("lane_pace", 1 - throttle)              # a lane's own thread following its group's progress, or not
        dec.set("lead", (group // 256) % 4)             # ... 1-3 iterations behind (0: the default)
        dec.set("hl_reg", hl_reg)
        dec.set("lanes", lanes)
        dec.set("group_size", group)
        dec.set("hl_records", hl_rec)
        dec.set("compact", compact)
        got = dec.decode_batch(llrs, 12, want_posterior=True)
        d_llrs = torch.from_numpy(llrs).cuda()
        d_bits = torch.zeros((len(llrs), dec.k), dtype=torch.uint8, device="cuda")
        d_its = torch.zeros(len(llrs), dtype=torch.int32, device="cuda")
        dec.decode_batch_device(d_llrs.data_ptr(), False, len(llrs), 12, d_bits.data_ptr(), dec.k, d_its.data_ptr(), 0,
                                torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(d_its.cpu().numpy(), got[1])
        assert np.array_equal(d_bits.cpu().numpy(), got[0][:, : dec.k])
        if want is None:
            want = got
        else:
            for a, b in zip(want, got):
                assert np.array_equal(a, b)
    g = oracle.Graph(alist(spec))
    sub = slice(0, 2304, 9)
    ob_, oi_, _ = oracle.decode_batch(g, impl, full[sub], 12, threads=8)
    assert np.array_equal(want[1][sub], oi_) and np.array_equal(want[0][sub], ob_)
    assert (want[1] >= 0).any() and (want[1] < 0).any()


@pytest.mark.parametrize("spec,impl,frames,ebn0", [("dvbs2:R1_2short", "Tanhf32", 520, 1.4), ("ar4ja:1/2:1024", "Tanhf32", 700, 1.8),
                                                   ("dvbs2:R1_4short", "Tanhf64", 300, 0.8), ("nr5g:2:24", "Tanhf32", 600, 1.5)])
def test_register_resident_flooding_tanh_rows_are_invisible(oracle, spec, impl, frames, ebn0):
    """`cn_reg` (default on): the flooding Tanh rule on graphs whose rows have at most 12 edges takes cn_reg_kernel -- a record
    per row, the row's values in registers, a straight-line block per degree -- instead of cn_staged_kernel; hard decisions,
    iteration counts and posteriors are bit for bit the same, and the oracle's.  (DVB-S2 1/2 short: rows of 7 edges, the
    10-edge bucket; 1/4 short: 4; AR4JA 1/2: 6; 5G NR BG2: rows of 10, the table-driven mix of 3..10.)"""
    msgs, llrs, full = awgn_frames(spec, frames, ebn0, 4242)
    dec = lt.LdpcDecoder(alist(spec), impl)
    dec.set("latency", 0)                       # (the small-batch paths would take these calls)
    gpu_in = llrs.astype(np.float64) if impl.endswith("f64") else llrs
    outs = []
    for cn_reg, compact in ((1, 1), (0, 1), (1, 0)):
        dec.set("cn_reg", cn_reg)
        dec.set("compact", compact)
        outs.append(dec.decode_batch(gpu_in, 20, want_posterior=True))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert np.array_equal(a, b)
    g = oracle.Graph(alist(spec))
    sub = slice(0, frames, 5)
    ob_, oi_, op_ = oracle.decode_batch(g, impl, full[sub], 20, threads=8)
    assert np.array_equal(outs[0][1][sub], oi_) and np.array_equal(outs[0][0][sub], ob_)
    assert np.array_equal(outs[0][2][sub].astype(np.float64), op_.astype(outs[0][2].dtype).astype(np.float64))
    assert (outs[0][1] >= 0).any()


def test_wrong_result_switches_are_not_in_the_product():
    """include/ldpc_toolbox.h promises that no tunable changes a result: the experiment switches that did are gone -- and
    so are the opt-in forms that measured level or behind (round 5): the slice-persistent layered kernel's options are
    unknown to the product, and "streaming" on the simulator changes nothing"""
    dec = lt.LdpcDecoder(alist("dvbs2:R1_2short"), "Minsumf32")
    for key in ("rec_dbg", "lat_debug", "hl_persist", "hl_slice"):
        with pytest.raises(KeyError):
            dec.set(key, 1)
    s = lt.Simulator(alist("dvbs2:R1_2short"), "Minsumf32", "", device=0, pool_size=8, pool_seed=2)
    s.set("records", 2)
    s.set("streaming", 1)
    a = s.run(1.8, seed=3, first_frame=0, frames=4096 + 700, max_iterations=25)
    assert s.get("streamed_frames") == 0
    s.set("streaming", 0)
    assert np.array_equal(a, s.run(1.8, seed=3, first_frame=0, frames=4096 + 700, max_iterations=25))


@pytest.mark.parametrize("impl", ["HLMinsumf32", "HLMinsumf64", "HLTanhf64"])
def test_layered_long_rows(oracle, impl):
    """rows of 27 edges (DVB-S2 short 8/9): the layered min-sum takes its 32-edge register bucket in
    f32 and the two-pass kernel in f64 (no register form fits); the staircase makes every row its own
    dependency level, so this is also the launch-bound corner of the layered schedule"""
    spec = "dvbs2:R8_9short"
    msgs, llrs, full = awgn_frames(spec, 96, 4.2, 31)
    dec = lt.LdpcDecoder(alist(spec), impl)
    assert dec.get("max_check_degree") == 27
    bits, its, post = dec.decode_batch(llrs.astype(np.float64) if impl.endswith("f64") else llrs, 6, want_posterior=True)
    ob_, oi_, op_ = oracle.decode_batch(oracle.Graph(alist(spec)), impl, full, 6, threads=8)
    assert np.array_equal(its, oi_) and np.array_equal(bits, ob_)
    assert np.array_equal(post, op_ if impl.endswith("f64") else op_.astype(np.float32))
    assert (its >= 0).any()


@pytest.mark.parametrize("impl", ["Minsumf32", "HLMinsumf32", "Tanhf32", "Minstarapproxi8"])
def test_rows_longer_than_64_edges(oracle, impl):
    """a matrix with check rows of 70-90 edges: beyond the 64-bit sign mask of the streaming min-sum
    kernel (it takes the LDS-staged kernel instead) and beyond every register bucket"""
    rng = np.random.default_rng(12)
    n, m = 400, 24
    h = lt.SparseMatrix(m, n)
    for r in range(m):
        for c in rng.choice(n, size=70 + (r % 3) * 10, replace=False):
            h.insert(r, int(c))
    for c in range(n):                                            # no empty column
        if h.col_weight(c) == 0:
            h.insert(int(rng.integers(m)), c)
    a = h.alist()
    dec = lt.LdpcDecoder(a, impl)
    assert dec.get("max_check_degree") >= 90
    llrs = (2.5 + 2.0 * rng.standard_normal((200, n))).astype(np.float32)   # all-zero codeword, noisy
    bits, its, post = dec.decode_batch(llrs, 8, want_posterior=True)
    ob_, oi_, op_ = oracle.decode_batch(oracle.Graph(a), impl, llrs, 8, threads=8)
    assert np.array_equal(its, oi_) and np.array_equal(bits, ob_)
    assert np.array_equal(post, op_.astype(np.float32))


@pytest.mark.parametrize("impl", ["Minsumf32", "Phif32", "Tanhf64", "Aminstarf64", "HLMinstarapproxf32", "HLPhif64", "HLMinsumf64",
                                  "Minstarapproxi8", "HLAminstari8PartialHardLimit"])
@pytest.mark.parametrize("batch", [40, 600])
def test_rows_beyond_the_lds_limit(oracle, impl, batch):
    """The reference takes any alist (/root/reference/src/sparse.rs:352-389, flooding.rs:26-39: no degree limit).  A matrix
    with check rows of 330-420 edges: beyond the 160 KB of LDS the staged check-node kernels keep a row's two columns in
    (320 edges in f32 and the 8-bit rules, 160 in f64; one column for Tanh) -- those launches keep the columns in a
    per-wavefront region of HBM instead (cn_staged_kernel / hl_level_kernel / cn_i8_kernel / hl_i8_kernel, SCRATCH), beside
    short rows that stay in the LDS and in registers in the same decoder.  Small and large batch, bit for bit the oracle."""
    rng = np.random.default_rng(5)
    n, m = 1500, 14
    h = lt.SparseMatrix(m, n)
    for r in range(m):
        deg = (330 + 30 * (r % 4)) if r < 8 else (5 + r)                   # eight very long rows, six short ones
        for c in rng.choice(n, size=deg, replace=False):
            h.insert(r, int(c))
    for c in range(n):                                                      # no empty column
        if h.col_weight(c) == 0:
            h.insert(int(rng.integers(m)), c)
    a = h.alist()
    dec = lt.LdpcDecoder(a, impl)
    assert dec.get("max_check_degree") >= 420
    llrs = (3.0 + 2.0 * rng.standard_normal((batch, n))).astype(np.float32)   # all-zero codeword, noisy
    f64 = impl.endswith("f64")
    bits, its, post = dec.decode_batch(llrs.astype(np.float64) if f64 else llrs, 6, want_posterior=True)
    ob_, oi_, op_ = oracle.decode_batch(oracle.Graph(a), impl, llrs, 6, threads=8)
    assert np.array_equal(its, oi_) and np.array_equal(bits, ob_)
    if "i8" in impl:
        run = its != 0
        assert np.array_equal(post[run].astype(np.float64), op_[run])
    else:
        assert np.array_equal(post, op_ if f64 else op_.astype(np.float32))
    if "Minsum" in impl:
        # min-sum through the generic LDS-staged kernel ("staged_minsum", an execution choice): the same rows beyond the LDS,
        # both schedules (round 5's advisor: the layered form skipped the scratch allocation and failed its launch)
        dec.set("staged_minsum", 1)
        b2, i2, p2 = dec.decode_batch(llrs.astype(np.float64) if f64 else llrs, 6, want_posterior=True)
        assert np.array_equal(i2, its) and np.array_equal(b2, bits) and np.array_equal(p2, post)


@pytest.mark.parametrize("impl", ["Minsumf32", "Minsumf64", "Phif32", "HLMinsumf32", "HLPhif64", "Aminstari8", "HLMinstarapproxi8"])
def test_isolated_and_low_degree_variables(oracle, impl):
    """variables with no check at all (their posterior is the channel LLR, they never change a
    syndrome), with one and with two checks (the L-free path of the flooding min-sum), next to
    ordinary ones"""
    rng = np.random.default_rng(21)
    n, m = 150, 40
    h = lt.SparseMatrix(m, n)
    for c in range(n):
        deg = 0 if c % 10 == 0 else (1 if c % 10 == 1 else (2 if c % 10 in (2, 3) else 3 + c % 3))
        for r in rng.choice(m, size=deg, replace=False):
            h.insert(int(r), c)
    for r in range(m):                                            # every rule needs rows of degree >= 2
        while h.row_weight(r) < 2:
            h.insert(r, int(rng.integers(n)))
    a = h.alist()
    dec = lt.LdpcDecoder(a, impl)
    llrs = (1.5 + 2.0 * rng.standard_normal((130, n))).astype(np.float32)
    llrs[0] = 4.0                                                 # a clean frame: pre-check, 0 iterations
    f64 = impl.endswith("f64")
    bits, its, post = dec.decode_batch(llrs.astype(np.float64) if f64 else llrs, 15, want_posterior=True)
    ob_, oi_, op_ = oracle.decode_batch(oracle.Graph(a), impl, llrs, 15, threads=8)
    assert np.array_equal(its, oi_) and np.array_equal(bits, ob_)
    assert np.array_equal(post, op_ if f64 else op_.astype(np.float32))
    assert its[0] == 0
    if "i8" not in impl:
        isolated = np.arange(0, n, 10)
        assert np.array_equal(post[:, isolated], llrs[:, isolated].astype(post.dtype))


@pytest.mark.parametrize("impl", ["Minsumf32", "HLMinsumf32", "Minstarapproxf32", "Phif32", "Tanhf32", "HLTanhf32",
                                  "Minsumf64", "HLMinsumf64", "Aminstari8Jones", "HLMinstarapproxi8"])
def test_infinite_and_huge_llrs(oracle, impl):
    """known bits (shortening) arrive as +/-inf or huge LLRs: the reference's arithmetic then runs
    through inf - finite, inf - inf = NaN, min with inf, the tanh clamp, exp(-inf) and the 8-bit
    saturation; the HIP path follows the oracle bit for bit, NaNs included.  (Aminstarf32/f64 are left
    out: the reference panics on a NaN there, arithmetic.rs:947-951, and the oracle reports that.)"""
    spec = "nr5g:2:24"
    msgs, llrs, full = awgn_frames(spec, 140, 1.2, 404)
    enc = lt.Encoder(alist(spec))
    sign = np.where(np.stack([enc.encode(m, llrs.shape[1]) for m in msgs]) == 1, -1.0, 1.0).astype(np.float32)
    rng = np.random.default_rng(5)
    known = rng.random(llrs.shape) < 0.06
    llrs = llrs.copy()
    llrs[known] = (sign * np.float32(np.inf))[known]
    llrs[3] = np.where(rng.random(llrs.shape[1]) < 0.5, np.float32(1e30) * sign[3], llrs[3]).astype(np.float32)
    llrs[4, ::5] = np.float32(3.0e38) * sign[4, ::5]
    llrs[5, ::7] = np.float32(-1.0e-40)                            # denormals
    f64 = impl.endswith("f64")
    dec = lt.LdpcDecoder(alist(spec), impl)
    with np.errstate(all="ignore"):
        bits, its, post = dec.decode_batch(llrs.astype(np.float64) if f64 else llrs, 12, want_posterior=True)
        ob_, oi_, op_ = oracle.decode_batch(oracle.Graph(alist(spec)), impl, llrs, 12, threads=8)
        want = op_ if f64 else op_.astype(np.float32)
    assert np.array_equal(its, oi_) and np.array_equal(bits, ob_)
    assert np.array_equal(post, want, equal_nan=True)
    assert (its >= 0).any()
    if "Minsum" in impl:
        assert np.isnan(post).any()                               # the inf - inf rows were exercised
        dec.set("staged_minsum", 1)                               # the LDS-staged form of the same rule
        with np.errstate(all="ignore"):
            b2, i2, p2 = dec.decode_batch(llrs.astype(np.float64) if f64 else llrs, 12, want_posterior=True)
        assert np.array_equal(i2, its) and np.array_equal(b2, bits) and np.array_equal(p2, post, equal_nan=True)


@pytest.mark.parametrize("impl", ["Minsumf32", "Phif32", "Tanhf32", "Minstarapproxf32", "HLMinstarapproxf32", "Phif64",
                                  "Minstarapproxi8", "HLAminstari8"])
def test_nan_llrs_follow_the_reference_arithmetic(oracle, impl):
    """NaN channel values: hard decision 0 (NaN <= 0 is false), `x < 0` false, the clamps and the
    transcendental functions propagate them as glibc does; bits, iterations and the NaN pattern of
    the soft output equal the oracle's.  (A-Min* in floating point panics on NaN in the reference.)"""
    spec = "nr5g:2:24"
    msgs, llrs, full = awgn_frames(spec, 70, 2.5, 77)
    llrs = llrs.copy()
    llrs[1::3, ::97] = np.nan
    llrs[2, :] = np.nan                                           # a frame of nothing but NaNs
    f64 = impl.endswith("f64")
    dec = lt.LdpcDecoder(alist(spec), impl)
    with np.errstate(all="ignore"):
        bits, its, post = dec.decode_batch(llrs.astype(np.float64) if f64 else llrs, 10, want_posterior=True)
        ob_, oi_, op_ = oracle.decode_batch(oracle.Graph(alist(spec)), impl, llrs, 10, threads=8)
        want = op_ if f64 else op_.astype(np.float32)
    assert np.array_equal(its, oi_) and np.array_equal(bits, ob_)
    assert np.array_equal(post, want, equal_nan=True)
    assert (its[0::3] >= 0).all()                                  # the NaN-free frames decode (Eb/N0 2.5 dB)


def test_all_frames_clean_and_handle_reuse(oracle):
    """a batch whose every frame passes the pre-check (nothing to iterate: the group is finished
    before the first launch), then the same handle over changing batch sizes, schedules of options
    and entry points: each result equals a fresh handle's"""
    import torch
    spec = "nr5g:2:24"
    a = alist(spec)
    msgs, llrs, full = awgn_frames(spec, 1100, 1.4, 88)
    enc = lt.Encoder(a)
    clean = np.stack([np.where(enc.encode(m, llrs.shape[1]) == 1, -3.0, 3.0) for m in msgs[:200]]).astype(np.float32)
    for impl in ("Minsumf32", "HLMinsumf32", "HLTanhf32", "Minstarapproxi8"):
        dec = lt.LdpcDecoder(a, impl)
        bits, its, post = dec.decode_batch(clean, 50, want_posterior=True)
        assert (its == 0).all() and np.array_equal(bits[:, : dec.k], msgs[:200])
        if "i8" not in impl:
            assert np.array_equal(post, clean)
        for batch, opts in ((300, {}), (64, {"group_size": 64}), (1100, {"group_size": 512, "lanes": 2}), (130, {"group_size": 0}),
                            (1, {}), (700, {"compact": 0, "lanes": 1, "poll": 0})):
            for k, v in opts.items():
                dec.set(k, v)
            got = dec.decode_batch(llrs[:batch], 20, want_posterior=True)
            fresh = lt.LdpcDecoder(a, impl).decode_batch(llrs[:batch], 20, want_posterior=True)
            for x, y in zip(got, fresh):
                assert np.array_equal(x, y), (impl, batch)
        d_llrs = torch.from_numpy(llrs[:257]).cuda()
        d_bits = torch.zeros((257, dec.n), dtype=torch.uint8, device="cuda")
        d_its = torch.zeros(257, dtype=torch.int32, device="cuda")
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):                             # a caller-owned stream, two calls back to back
            for _ in range(2):
                dec.decode_batch_device(d_llrs.data_ptr(), False, 257, 20, d_bits.data_ptr(), dec.n, d_its.data_ptr(), 0,
                                        side.cuda_stream)
        side.synchronize()
        assert np.array_equal(d_its.cpu().numpy(), fresh[1][:257] if batch >= 257 else d_its.cpu().numpy())
        want = lt.LdpcDecoder(a, impl).decode_batch(llrs[:257], 20)
        assert np.array_equal(d_its.cpu().numpy(), want[1]) and np.array_equal(d_bits.cpu().numpy(), want[0])


def test_two_handles_from_two_threads(oracle):
    """distinct handles are independent (the reference's Send-not-Sync contract): two Python threads
    decode different batches at the same time on one GPU"""
    import threading
    spec = "nr5g:2:24"
    a = alist(spec)
    jobs = [("HLMinsumf32", awgn_frames(spec, 600, 1.3, 5)[1]), ("Minsumf32", awgn_frames(spec, 500, 1.5, 6)[1])]
    want = [lt.LdpcDecoder(a, impl).decode_batch(l, 25, want_posterior=True) for impl, l in jobs]
    got = [None, None]

    def work(i):
        dec = lt.LdpcDecoder(a, jobs[i][0])
        for _ in range(3):
            got[i] = dec.decode_batch(jobs[i][1], 25, want_posterior=True)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for g_, w_ in zip(got, want):
        for x, y in zip(g_, w_):
            assert np.array_equal(x, y)


def test_file_path_decoder_constructor(tmp_path, oracle):
    """include/ldpc_toolbox.h:12: the reference's alist-file constructor, with a puncturing pattern,
    driven through the scalar f64 call as a C caller of the reference would"""
    import ctypes as C
    L = lt._capi.lib()
    spec, punct = "ar4ja:1/2:1024", "1,1,1,1,0"
    path = tmp_path / "h.alist"
    path.write_text(alist(spec))
    h = L.ldpc_toolbox_decoder_ctor(str(path).encode(), b"Phif64", punct.encode())
    assert h
    msgs, llrs, full = awgn_frames(spec, 4, 2.5, 17, punct, dtype=np.float64)
    dec = oracle.Decoder(oracle.Graph(alist(spec)), "Phif64")
    for i in range(4):
        out = np.zeros(1024, dtype=np.uint8)
        it = L.ldpc_toolbox_decoder_decode_f64(h, out.ctypes.data, 1024, llrs[i].ctypes.data, llrs.shape[1], 30)
        ok, obits, oit, _ = dec.decode(full[i], 30)
        assert (it >= 0) == ok and (it == oit or not ok) and np.array_equal(out, obits[:1024])
    assert L.ldpc_toolbox_decoder_decode_f64(h, out.ctypes.data, 1024, llrs[0].ctypes.data, 100, 30) == -4   # wrong length: LDPC_TOOLBOX_ERR_ARGUMENT
    L.ldpc_toolbox_decoder_dtor(h)


@pytest.mark.parametrize("impl", ["HLMinsumf32", "HLTanhf32", "HLMinsumf64", "HLAminstari8"])
def test_row_serial_mode_equals_level_launches(oracle, impl):
    """DVB-S2's staircase gives one dependency level per row; beyond 512 levels the layered decoder
    walks all rows with one wave per codeword slice (one launch per iteration).  Same results as one
    launch per level, and as the oracle."""
    spec = "dvbs2:R1_2short"
    msgs, llrs, full = awgn_frames(spec, 300, 1.9, 61)
    dec = lt.LdpcDecoder(alist(spec), impl)
    assert dec.get("layers") > 512
    f64 = impl.endswith("f64")
    gin = llrs.astype(np.float64) if f64 else llrs
    serial = dec.decode_batch(gin, 8, want_posterior=True)
    dec.set("serial_levels", 10 ** 6)                              # force one launch per level
    levels = dec.decode_batch(gin, 8, want_posterior=True)
    for a_, b_ in zip(serial, levels):
        assert np.array_equal(a_, b_)
    sub = slice(0, 300, 5)
    ob_, oi_, op_ = oracle.decode_batch(oracle.Graph(alist(spec)), impl, full[sub], 8, threads=8)
    assert np.array_equal(serial[1][sub], oi_) and np.array_equal(serial[0][sub], ob_)
    assert (serial[1] >= 0).any() and (serial[1] < 0).any()


def test_c_program_written_against_the_reference_header(tmp_path):
    """examples/reference_abi_roundtrip.c uses only the nine symbols of the reference's header; built
    with gcc and linked against this library it encodes, adds noise and decodes on the GPU"""
    import subprocess
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    lib = os.path.join(root, "ldpc_toolbox_amd", "lib")
    exe = str(tmp_path / "roundtrip")
    subprocess.run(["gcc", "-O2", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "reference_abi_roundtrip.c"),
                    "-L" + lib, "-lldpc_toolbox", "-Wl,-rpath," + lib, "-lm", "-o", exe], check=True, capture_output=True)
    path = tmp_path / "h.alist"
    path.write_text(alist("ar4ja:1/2:1024"))
    for impl in ("Phif64", "HLMinstarapproxi8"):
        r = subprocess.run([exe, str(path), impl], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.count("message recovered") == 8


def test_c_worker_replacing_the_one_frame_loop(tmp_path):
    """examples/batched_worker.c: what a C caller writes in place of the reference's one-frame loop (ber.rs:462-466) -- one call of
    the batched extension, host buffers, the decoder's own straggler pooling -- against the scalar symbol of the reference's header on
    the same frames: identical results three ways (the program exits 0 only then)"""
    import subprocess
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    lib = os.path.join(root, "ldpc_toolbox_amd", "lib")
    exe = str(tmp_path / "batched_worker")
    subprocess.run(["gcc", "-O2", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "batched_worker.c"),
                    "-L" + lib, "-lldpc_toolbox", "-Wl,-rpath," + lib, "-lm", "-o", exe], check=True, capture_output=True)
    path = tmp_path / "h.alist"
    path.write_text(alist("nr5g:2:52"))
    for impl, sigma in (("HLMinsumf32", "1.34"), ("Minsumf32", "1.30")):      # Eb/N0 about 1.6 / 1.9 dB on this rate-0.19 code: a few per cent of slow frames
        r = subprocess.run([exe, str(path), impl, "20000", sigma], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "results identical" in r.stdout
        print(r.stdout.strip())


def test_syndrome_operator_matches_oracle(oracle):
    """ldpc_toolbox_decoder_syndrome (the reference's check_llrs, decoder.rs:157-164, with the
    parities returned) equals the oracle's on random words and on the decoder's own output: a frame
    reported converged has syndrome zero, a failed one has not."""
    import torch
    spec = "dvbs2:R1_2short"
    msgs, llrs, full = awgn_frames(spec, 300, 1.3, 99)
    dec = lt.LdpcDecoder(alist(spec), "Minsumf32")
    g = oracle.Graph(alist(spec))
    bits, its, _ = dec.decode_batch(llrs, 20)
    syn, weight = dec.syndrome(bits)
    osyn, oweight = oracle.syndrome(g, bits)
    assert np.array_equal(syn, osyn) and np.array_equal(weight, oweight)
    assert (its >= 0).any() and (its < 0).any()
    assert np.array_equal(weight == 0, its >= 0)
    rnd = np.random.default_rng(3).integers(0, 2, size=(65, dec.n)).astype(np.uint8)
    syn, weight = dec.syndrome(rnd)
    osyn, oweight = oracle.syndrome(g, rnd)
    assert np.array_equal(syn, osyn) and np.array_equal(weight, oweight)
    # device-resident form, weights only
    d_bits = torch.from_numpy(rnd).cuda()
    d_w = torch.full((65,), 12345, dtype=torch.int32, device="cuda")
    rc = lt._capi.lib().ldpc_toolbox_decoder_syndrome_device(dec._h, d_bits.data_ptr(), dec.n, 65, None,
                                                             d_w.data_ptr(), None)
    assert rc == 0 and np.array_equal(d_w.cpu().numpy().astype(np.uint32), oweight)
    with pytest.raises(RuntimeError):
        dec.syndrome(rnd[:, :100])                               # must cover the whole codeword


# ---- the reference's 8-bit quantised arithmetics: integer arithmetic, exact by construction -------

@pytest.mark.parametrize("impl", lt.I8_IMPLEMENTATIONS)
def test_i8_implementations_bit_exact(oracle, impl):
    """all 20 i8 names of src/decoder/factory.rs:246-263, 270-275.  AR4JA r=1/2 has degree-1
    variables (Deg1Clip), punctured zero LLRs and saturating channel values (Jones,
    PartialHardLimit matter once |llr| reaches the 8-bit range)."""
    cases = [("ar4ja:1/2:1024", "1,1,1,1,0", 1.9, 25), ("nr5g:2:24", "", 1.4, 20)]
    if not impl.startswith("HL"):
        cases.append(("dvbs2:R1_2short", "", 1.5, 15))
    # long check rows (the O(d^2) fold from its identity, the argmin key, the register forms up to 24 edges
    # and the two-pass form beyond): BG1 has rows of 19, DVB-S2 8/9 short of 27 edges
    if impl in ("Minstarapproxi8", "Aminstari8JonesPartialHardLimitDeg1Clip", "HLMinstarapproxi8", "HLAminstari8",
                "Aminstari8PartialHardLimit", "HLMinstarapproxi8PartialHardLimit"):
        cases += [("nr5g:1:8", "", 3.0, 12), ("dvbs2:R8_9short", "", 3.6, 10)]
    for spec, punct, ebn0, iters in cases:
        msgs, (bits, its, post), (obits, oits, opost) = run_both(oracle, spec, impl, 300, ebn0, iters, seed=91,
                                                                puncturing=punct)
        assert np.array_equal(its, oits), (impl, spec)
        assert np.array_equal(bits, obits), (impl, spec)
        assert np.array_equal(post.astype(np.float64), opost), (impl, spec)
        assert (its > 0).any(), (impl, spec)


def test_i8_options_change_results_where_they_should(oracle):
    """strong LLRs (saturation at +-127) make Jones / PartialHardLimit / Deg1Clip differ from the
    plain rule -- and the GPU follows the oracle in each case"""
    spec, punct = "ar4ja:1/2:1024", "1,1,1,1,0"
    msgs, llrs, full = awgn_frames(spec, 256, 6.5, 33, punct)      # high SNR: LLRs far beyond 127/8
    llrs = llrs.copy()
    llrs[:, ::3] *= -0.02                                           # plant weak wrong symbols so that decoding iterates
    from ldpc_toolbox_amd import simulation as sim
    full = sim.depuncture(llrs, sim.parse_puncturing_pattern(punct))
    g = oracle.Graph(alist(spec))
    outs = {}
    for impl in ("Minstarapproxi8", "Minstarapproxi8Jones", "Minstarapproxi8PartialHardLimit", "Minstarapproxi8Deg1Clip",
                 "Aminstari8", "Aminstari8JonesPartialHardLimitDeg1Clip"):
        dec = lt.LdpcDecoder(alist(spec), impl, punct)
        bits, its, post = dec.decode_batch(llrs, 12, want_posterior=True)
        obits, oits, opost = oracle.decode_batch(g, impl, full, 12, threads=8)
        assert np.array_equal(its, oits) and np.array_equal(bits, obits), impl
        assert np.array_equal(post.astype(np.float64), opost), impl
        outs[impl] = (its.copy(), post.copy())
        # the same saturating frames as small calls (lane-per-edge path, csrc/latency_edge.hip.h)
        for B in (1, 11):
            sb, si, sp = dec.decode_batch(llrs[:B], 12, want_posterior=True)
            assert dec.get("last_group") == B
            assert np.array_equal(si, its[:B]) and np.array_equal(sb, bits[:B]) and np.array_equal(sp, post[:B]), (impl, B)
    base = outs["Minstarapproxi8"]
    differing = [k for k, v in outs.items() if k != "Minstarapproxi8" and not (np.array_equal(v[0], base[0]) and
                                                                               np.array_equal(v[1], base[1]))]
    assert len(differing) >= 3, differing


# ---- on-device frame generation + error counting -----------------------------------

def test_device_frame_generator_matches_oracle(oracle):
    """the HIP generator (Philox4x32-10 + polar method + glibc-identical logf) and the oracle's C
    restatement produce the same LLRs, bit for bit"""
    spec, punct = "ar4ja:1/2:1024", "1,1,1,1,0"
    sim_ = lt.Simulator(alist(spec), "Minsumf32", punct, device=0, pool_size=8, pool_seed=3)
    msgs, tx = sim_.pool_data()
    assert tx.shape == (8, 2048) and msgs.shape == (8, 1024)
    enc = lt.Encoder(alist(spec), punct)
    assert np.array_equal(enc.encode(msgs[5], 2048), tx[5])
    for ebn0, seed, first, frames in ((2.0, 11, 0, 40), (-1.5, 2 ** 40 + 7, 2 ** 33, 9)):
        llrs, idx = sim_.generate(ebn0, seed, first, frames)
        ollrs, oidx = oracle.generate_llrs(tx, sim_.rate, ebn0, seed, first, frames)
        assert np.array_equal(idx, oidx)
        assert np.array_equal(llrs, ollrs)
        # the same frames written in place into a buffer of the simulator's GPU (what bench.py fills its batch with: no host
        # round trip), 8PSK with the interleaver included below
        import torch
        d = torch.full((frames, sim_.n_tx), 7.0, dtype=torch.float32, device="cuda")
        didx = sim_.generate_into(d.data_ptr(), ebn0, seed, first, frames)
        torch.cuda.synchronize()
        assert np.array_equal(didx, oidx) and np.array_equal(d.cpu().numpy(), ollrs)
    psk = lt.Simulator(alist("dvbs2:R2_3short"), "Minsumf32", "", device=0, pool_size=4, pool_seed=1, modulation="8PSK", interleaving=3)
    h_llrs, h_idx = psk.generate(6.5, 5, 100, 12)
    import torch
    d = torch.zeros((12, psk.n_tx), dtype=torch.float32, device="cuda")
    d_idx = psk.generate_into(d.data_ptr(), 6.5, 5, 100, 12)
    torch.cuda.synchronize()
    assert np.array_equal(d_idx, h_idx) and np.array_equal(d.cpu().numpy(), h_llrs)


def test_device_simulation_counters_match_cpu_pipeline(oracle):
    """sim_run's six counters == the oracle decoding the same (regenerated) frames and the host-side
    Statistics fold (ber.rs:313-338), across several chunks and with a frame offset"""
    from ldpc_toolbox_amd import sharding, simulation as sim
    spec, punct = "ar4ja:1/2:1024", "1,1,1,1,0"
    pattern = sim.parse_puncturing_pattern(punct)
    s = lt.Simulator(alist(spec), "Minsumf32", punct, device=0, pool_size=16, pool_seed=9)
    s.set("group_size", 256)
    msgs, tx = s.pool_data()
    g = oracle.Graph(alist(spec))
    for ebn0, frames in ((2.0, 700), (2.6, 300)):
        got = s.run(ebn0, seed=77, first_frame=1000, frames=frames, max_iterations=30)
        llrs, idx = oracle.generate_llrs(tx, s.rate, ebn0, 77, 1000, frames)
        bits, its, _ = oracle.decode_batch(g, "Minsumf32", sim.depuncture(llrs, pattern), 30, threads=8,
                                           want_posterior=False)
        st = sim.fold_statistics(ebn0, s.k, msgs[idx], bits, its, 30, 1.0)
        assert np.array_equal(got, sharding.counters_from_statistics(st)), (ebn0, got)
    assert got[0] == 300


@pytest.mark.parametrize("spec,ebn0s,max_it", [("dvbs2:R1_2", (1.5, 1.4, 1.8), 200), ("dvbs2:R9_10", (4.0, 3.8, 4.2), 100)])
def test_config5_simulator_on_dvbs2_normal_frames(oracle, spec, ebn0s, max_it):
    """BASELINE config 5's workload as the driver runs it: the SIMULATOR (frames generated, decoded and scored on the
    device; straggler pooling on; the reference's Worker::simulate, /root/reference/src/simulation/ber.rs:436-481, with
    its stop-rule inputs :522-531) on DVB-S2 NORMAL-frame codes -- the shortest rows (R1_2: 7 edges) and the longest
    (R9_10: 30 edges, 4-word row records) -- at the foot of the waterfall (frames converge well inside the budget: the pool
    is in use), inside it (most frames fail: pooling switches itself off) and above it.  Three groups
    and a ragged rest per call, 100 iterations at most (the reference CLI's default, src/cli/ber.rs:55-56; 200 for R1_2,
    whose waterfall frames need 35 on average) so that later chunks run the reduced budget (2 x average + 8, taken when it
    is below 0.7 of the limit) and the pool fills.  The nine counters
    (BCH view included) equal (a) the same call with pooling off and (b), on a 256-frame sample, the CPU pipeline:
    the oracle decoding the regenerated Philox frames + the host-side Statistics fold (ber.rs:313-338)."""
    from ldpc_toolbox_amd import sharding, simulation as sim
    s = lt.Simulator(alist(spec), "Minsumf32", "", device=0, pool_size=8, pool_seed=3)
    msgs, tx = s.pool_data()
    g = oracle.Graph(alist(spec))
    frames = 3 * 4096 + 1000
    for ebn0 in ebn0s:
        s.set("pooling", 1)
        got = s.run(ebn0, seed=11, first_frame=500, frames=frames, max_iterations=max_it, bch_max_errors=12)
        pooled = s.get("pooled_frames")
        s.set("pooling", 0)
        want = s.run(ebn0, seed=11, first_frame=500, frames=frames, max_iterations=max_it, bch_max_errors=12)
        assert s.get("pooled_frames") == 0
        assert np.array_equal(got, want), (spec, ebn0, got, want)
        assert got[0] == frames
        if ebn0 == ebn0s[0]:
            assert pooled > 0, (pooled, got)                   # the foot of the waterfall: stragglers went through the pool
        if ebn0 == ebn0s[1]:
            assert got[2] > frames // 4, got                   # inside the waterfall: many frames fail
        # the CPU pipeline on the first 256 frames of the same stream
        s.set("pooling", 1)
        part = s.run(ebn0, seed=11, first_frame=500, frames=256, max_iterations=max_it, bch_max_errors=12)
        llrs, idx = oracle.generate_llrs(tx, s.rate, ebn0, 11, 500, 256)
        bits, its, _ = oracle.decode_batch(g, "Minsumf32", llrs, max_it, threads=32, want_posterior=False)
        st = sim.fold_statistics(ebn0, s.k, msgs[idx], bits, its, max_it, 1.0, bch_max_errors=12)
        assert np.array_equal(part, sharding.counters_from_statistics(st)), (spec, ebn0, part)


@pytest.mark.parametrize("spec,punct,impl,ebn0s", [("ar4ja:1/2:1024", "1,1,1,1,0", "Minsumf32", (1.6, 2.0, 2.4, 3.0, 0.0)),
                                                   ("nr5g:2:24", "", "HLTanhf32", (0.4, 1.2, 2.4)),
                                                   ("nr5g:1:16", "", "HLMinstarapproxi8", (1.2,))])
def test_straggler_pooling_counts_the_same_frames_the_same_way(oracle, spec, punct, impl, ebn0s):
    """sim_run over more than one chunk: once the call has seen how many iterations its frames take, later chunks run a
    reduced iteration budget and the frames that have not converged by then are pooled and decoded together with the
    full budget (csrc/simulator.h).  Per frame that is the result of one full-budget decode, so the counters equal
    those of "pooling" = 0 -- in the waterfall (where it pools), where nearly every frame fails (where it must not),
    where every frame converges at once -- and, on the small code, those of the oracle over the regenerated frames."""
    from ldpc_toolbox_amd import sharding, simulation as sim
    pattern = sim.parse_puncturing_pattern(punct) if punct else None
    s = lt.Simulator(alist(spec), impl, punct, device=0, pool_size=16, pool_seed=9)
    s.set("group_size", 1024)                  # chunks of 1024 frames
    msgs, tx = s.pool_data()
    pooled_somewhere = False
    for ebn0 in ebn0s:
        frames = 6 * 1024 + 300
        s.set("pooling", 1)
        got = s.run(ebn0, seed=5, first_frame=77, frames=frames, max_iterations=60)
        pooled = s.get("pooled_frames")
        s.set("pooling", 0)
        want = s.run(ebn0, seed=5, first_frame=77, frames=frames, max_iterations=60)
        assert s.get("pooled_frames") == 0
        assert np.array_equal(got, want), (ebn0, pooled, got, want)
        assert got[0] == frames
        fer = want[2] / frames
        pooled_somewhere = pooled_somewhere or pooled > 0
        if 0 < fer < 0.03:
            assert pooled > 0, (ebn0, fer)     # a few slow frames per chunk: they were set aside
        if fer > 0.6:
            assert pooled < 0.4 * frames       # where most frames fail, pooling switches itself off after the first chunk
    assert pooled_somewhere
    # a sweep calls run() chunk by chunk at one Eb/N0: the budget carries over from call to call (and not to another point)
    e = ebn0s[-2] if spec.startswith("ar4ja") else ebn0s[0]
    for pooling in (1, 0):
        s.set("pooling", pooling)
        s.run(e + 1.0, seed=9, first_frame=0, frames=1024, max_iterations=60)
        calls = [s.run(e, seed=9, first_frame=1024 * c, frames=1024, max_iterations=60) for c in range(5)]
        if pooling:
            with_pool = calls
        else:
            for a, b in zip(with_pool, calls):
                assert np.array_equal(a, b)
    # the outer-BCH accounting (ber.rs:328-337) of the pooled frames
    nine = {}
    for pooling in (1, 0):
        s.set("pooling", pooling)
        nine[pooling] = s.run(e, seed=11, first_frame=0, frames=5 * 1024 + 77, max_iterations=60, bch_max_errors=12)
    assert len(nine[1]) == 9 and np.array_equal(nine[1], nine[0])
    if spec.startswith("ar4ja"):
        g = oracle.Graph(alist(spec))
        frames = 5000
        s.set("pooling", 1)
        got = s.run(2.4, seed=6, first_frame=40, frames=frames, max_iterations=60)
        assert s.get("pooled_frames") > 0
        llrs, idx = oracle.generate_llrs(tx, s.rate, 2.4, 6, 40, frames)
        bits, its, _ = oracle.decode_batch(g, impl, sim.depuncture(llrs, pattern), 60, threads=8, want_posterior=False)
        st = sim.fold_statistics(2.4, s.k, msgs[idx], bits, its, 60, 1.0)
        assert np.array_equal(got, sharding.counters_from_statistics(st)), got


@pytest.mark.parametrize("spec,punct,impl,ebn0s", [("ar4ja:1/2:1024", "1,1,1,1,0", "Minsumf32", (2.0, 2.4, 3.0, 0.0)),
                                                   ("nr5g:2:24", "", "HLTanhf32", (1.2, 2.4)),
                                                   ("nr5g:1:16", "", "Aminstari8", (1.4, 2.2, 3.0)),
                                                   ("dvbs2:R1_2short", "", "Phif64", (1.6, 2.0))])
def test_straggler_pooling_inside_the_batch_entries_is_invisible(oracle, spec, punct, impl, ebn0s):
    """Option "pooling" of the decoder itself (round 6; the simulation driver has had it since round 3): a call of several
    chunks runs its later chunks with a reduced iteration budget and decodes the frames that have not converged by then
    again, together, with the full budget -- per frame the result of one full-budget decode
    (/root/reference/src/simulation/ber.rs:462-466 calls decode once per frame with max_iterations).  Hard decisions,
    iteration counts and posteriors of both batch entries (host buffers, device buffers on the library's stream and on the
    caller's with "throttle") equal those of "pooling" = 0 -- in the waterfall (where it pools), where nearly every frame
    fails (where it must switch itself off) and where every frame converges at once -- and the oracle's on a sample."""
    import torch
    group, chunks, max_it = 512, 9, 60
    frames = chunks * group + 100
    dec = lt.LdpcDecoder(alist(spec), impl, punct)
    dec.set("group_size", group)
    dec.set("lanes", 1)
    f64 = impl.endswith("f64")
    pooled_somewhere = False
    for ebn0 in ebn0s:
        msgs, llrs, full = awgn_frames(spec, frames, ebn0, 31, punct)
        gin = llrs.astype(np.float64) if f64 else llrs
        dec.set("pooling", 0)
        want = dec.decode_batch(gin, max_it, want_posterior=True)
        assert dec.get("last_pooled") == 0
        fer = float((want[1] < 0).mean())
        dec.set("pooling", 1)
        got = dec.decode_batch(gin, max_it, want_posterior=True)                        # host buffers
        pooled_host = dec.get("last_pooled")
        for name, a, b in zip(("bits", "iterations", "posterior"), want, got):
            assert np.array_equal(a, b, equal_nan=True), (ebn0, "host entry", name, pooled_host)
        d_in = torch.from_numpy(gin).cuda()
        d_bits = torch.zeros((frames, dec.k), dtype=torch.uint8, device="cuda")
        d_its = torch.zeros(frames, dtype=torch.int32, device="cuda")
        d_post = torch.zeros((frames, dec.n), dtype=torch.float64 if f64 else torch.float32, device="cuda")
        stream = torch.cuda.Stream()
        for how in ("own stream", "caller's stream + throttle", "caller's stream, no iteration counts asked for"):
            d_bits.zero_(), d_its.fill_(-7), d_post.zero_()
            torch.cuda.synchronize()
            dec.set("throttle", 0 if how == "own stream" else 1)
            dec.decode_batch_device(d_in.data_ptr(), f64, frames, max_it, d_bits.data_ptr(), dec.k,
                                    0 if how.endswith("asked for") else d_its.data_ptr(), d_post.data_ptr(),
                                    0 if how == "own stream" else stream.cuda_stream)
            torch.cuda.synchronize()
            pooled_dev = dec.get("last_pooled")
            assert np.array_equal(d_bits.cpu().numpy(), want[0][:, :dec.k]), (ebn0, how)
            if not how.endswith("asked for"):
                assert np.array_equal(d_its.cpu().numpy(), want[1]), (ebn0, how)
            assert np.array_equal(d_post.cpu().numpy(), want[2], equal_nan=True), (ebn0, how)
            if 0 < fer < 0.03 and want[1][want[1] >= 0].mean() * 2 + 8 < 0.7 * max_it:
                assert pooled_dev > 0, (ebn0, fer, how)       # a few slow frames per chunk: they were set aside
            if fer > 0.6:
                assert pooled_dev < 0.4 * frames, (ebn0, fer, how)
        dec.set("throttle", 0)
        # a call on the caller's stream without "throttle" only enqueues: it cannot pool, and says so
        dec.decode_batch_device(d_in.data_ptr(), f64, frames, max_it, d_bits.data_ptr(), dec.k, d_its.data_ptr(), 0, stream.cuda_stream)
        torch.cuda.synchronize()
        assert dec.get("last_pooled") == 0 and np.array_equal(d_its.cpu().numpy(), want[1])
        pooled_somewhere = pooled_somewhere or pooled_host > 0 or pooled_dev > 0
        if 0 < fer < 0.03 and want[1][want[1] >= 0].mean() * 2 + 8 < 0.7 * max_it:
            assert pooled_host > 0, (ebn0, fer)           # (a budget of 2 x average + 8 that is worth reducing to)
    # (whether a point pools depends on its iteration statistics; the first two cases are known to -- the simulation driver's
    # test pools there -- the others must above all give identical outputs)
    assert pooled_somewhere or impl in ("Aminstari8", "Phif64")
    # a sample against the oracle (the first chunk and the tail)
    sub = np.r_[0:40, frames - 40:frames]
    ob_, oi_, op_ = oracle.decode_batch(oracle.Graph(alist(spec)), impl, full[sub], max_it, threads=8)
    assert np.array_equal(got[1][sub], oi_) and np.array_equal(got[0][sub], ob_)


def test_device_8psk_generator_matches_oracle(oracle):
    """8PSK with the DVB-S2 bit interleaver on the device (interleave -> Gray 8PSK -> complex AWGN ->
    exact max* demodulation in f64 -> deinterleave) against the oracle's restatement of
    modulation.rs / interleaving.rs over the same Philox noise: bit for bit"""
    spec = "nr5g:2:6"                                             # n = 312 = 3 * 104
    a = alist(spec)
    for interleaving in (0, 3, -3, 8):
        s = lt.Simulator(a, "Minsumf32", device=0, pool_size=5, pool_seed=4, modulation="8PSK", interleaving=interleaving)
        msgs, tx = s.pool_data()
        for ebn0, seed, first, frames in ((4.0, 21, 0, 33), (-2.0, 2 ** 41 + 5, 2 ** 34, 7)):
            llrs, idx = s.generate(ebn0, seed, first, frames)
            ollrs, oidx = oracle.generate_llrs_psk8(tx, s.rate, ebn0, interleaving, seed, first, frames)
            assert np.array_equal(idx, oidx)
            assert np.array_equal(llrs, ollrs), (interleaving, ebn0)
        # high Eb/N0: the LLR signs are the transmitted bits, in codeword order (the deinterleaver undid the interleaver)
        llrs, idx = s.generate(30.0, 1, 0, 8)
        assert np.array_equal((llrs <= 0).astype(np.uint8), tx[idx])
    with pytest.raises(ValueError):
        lt.Simulator(alist("ar4ja:1/2:1024"), "Minsumf32", device=0, modulation="8PSK")     # 2560 % 3 != 0
    with pytest.raises(ValueError):
        lt.Simulator(a, "Minsumf32", device=0, modulation="8PSK", interleaving=7)            # 312 % 7 != 0
    with pytest.raises(ValueError):
        lt.Simulator(a, "Minsumf32", device=0, modulation="16APSK")


def test_device_8psk_simulation_counters_match_cpu_pipeline(oracle):
    """sim_run with 8PSK + interleaver: the six counters equal the oracle decoding the regenerated
    frames; and 8PSK needs more Eb/N0 than BPSK for the same frame error rate"""
    from ldpc_toolbox_amd import sharding, simulation as sim
    spec = "nr5g:2:24"                                            # n = 1248 = 3 * 416
    a = alist(spec)
    s = lt.Simulator(a, "HLMinsumf32", device=0, pool_size=16, pool_seed=9, modulation="8PSK", interleaving=-3)
    msgs, tx = s.pool_data()
    g = oracle.Graph(a)
    got = s.run(1.5, seed=5, first_frame=100, frames=600, max_iterations=25)
    llrs, idx = oracle.generate_llrs_psk8(tx, s.rate, 1.5, -3, 5, 100, 600)
    bits, its, _ = oracle.decode_batch(g, "HLMinsumf32", llrs, 25, threads=8, want_posterior=False)
    st = sim.fold_statistics(1.5, s.k, msgs[idx], bits, its, 25, 1.0)
    assert np.array_equal(got, sharding.counters_from_statistics(st)), got
    assert 0 < got[2] < 600                                        # some frame errors, not all
    bpsk = lt.Simulator(a, "HLMinsumf32", device=0, pool_size=16, pool_seed=9)
    assert bpsk.run(1.5, 5, 100, 600, 25)[2] < got[2]
    # outer-BCH accounting on the device (ber.rs:328-337) against the host-side fold
    got9 = s.run(1.5, seed=5, first_frame=100, frames=600, max_iterations=25, bch_max_errors=12)
    st = sim.fold_statistics(1.5, s.k, msgs[idx], bits, its, 25, 1.0, bch_max_errors=12)
    assert np.array_equal(got9, sharding.counters_from_statistics(st)), got9
    assert np.array_equal(got9[:6], got) and 0 < got9[7] < got9[2]


def test_ber_sweep_on_device():
    """the sweep driver end to end on one GPU: BER falls with Eb/N0, the stop rules hold, and the
    run is reproducible from its seed"""
    from ldpc_toolbox_amd import ber
    s = lt.Simulator(alist("ar4ja:1/2:1024"), "Minsumf32", "1,1,1,1,0", device=0)
    res = ber.sweep(s, [1.5, 2.5, 3.5], max_iterations=50, max_frame_errors=40, max_frames=8192, frames_per_batch=1024,
                    seed=5)
    assert [r.ebn0_db for r in res] == [1.5, 2.5, 3.5]
    assert res[0].ldpc.ber > res[1].ldpc.ber >= res[2].ldpc.ber
    assert res[0].num_frames == 1024 and res[0].ldpc.frame_errors >= 40      # stopped after the first batch
    assert res[2].num_frames == 8192                                         # ran to --max-frames
    again = ber.sweep(s, [2.5], max_iterations=50, max_frame_errors=40, max_frames=8192, frames_per_batch=1024, seed=5)
    assert again[0].ldpc.bit_errors == res[1].ldpc.bit_errors and again[0].num_frames == res[1].num_frames


def test_handles_give_their_device_memory_back():
    """Constructing, using and closing decoders, encoders and simulators in a loop leaves the device's free memory where it
    was: every workspace (both execution lanes' joint slab, row records, level records, pinned rings) is released by the
    destructor (the reference's contract: src/c_api/decoder.rs:93-101, the dtor frees everything the ctor made)."""
    import torch
    specs = [("dvbs2:R1_2short", "Minsumf32"), ("nr5g:1:16", "HLTanhf32"), ("ar4ja:1/2:1024", "Tanhf32"),
             ("nr5g:2:24", "HLMinstarapproxi8"), ("dvbs2:R1_4short", "Phif64")]

    def cycle():
        for spec, impl in specs:
            two_lanes = impl == "HLTanhf32"      # (both execution lanes' joint workspace and the lane threads)
            msgs, llrs, full = awgn_frames(spec, 2304 if two_lanes else 300, 2.0, 5)
            dec = lt.LdpcDecoder(alist(spec), impl)
            dec.set("latency", 0)
            if two_lanes:
                dec.set("lanes", 2)
                dec.set("group_size", 1024)
            gpu_in = llrs.astype(np.float64) if impl.endswith("f64") else llrs
            dec.decode_batch(gpu_in, 5)
            dec.close()
        s = lt.Simulator(alist("ar4ja:1/2:1024"), "Minsumf32", "1,1,1,1,0", device=0)
        s.run(2.0, 1, 0, 512, 10)
        s.close()

    cycle()                                   # first use: the runtime's own pools, module loading
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(3):
        cycle()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < 64 * 1024 * 1024, (free0, free1)
