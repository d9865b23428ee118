"""Normalized and offset min-sum on the GPU against the numpy restatement (corrected_minsum_restatement.py): bits, iteration
counts and posterior LLRs with np.array_equal -- no tolerance -- on every path a min-sum name can take."""
import numpy as np
import pytest

import corrected_minsum_restatement as cm
import ldpc_toolbox_amd as lt
from frames import alist, awgn_frames

pytestmark = pytest.mark.gpu

RULES = lt.CORRECTED_MINSUM_IMPLEMENTATIONS + ("NormMinsumf32:0.8", "HLOffsetMinsumf64:0.3")
# (code, puncturing, Eb/N0, iterations): the waterfall of each code and an iteration budget that lets the sample converge
# over several iterations (the restatement on these samples: DVB-S2 1/2 short converges at iterations 8-30 by rule, 8/9 short
# at 3-11; test_parity asserts the spread)
CODES = [("ar4ja:1/2:1024", "1,1,1,1,0", 1.9, 20), ("nr5g:2:24", "", 1.6, 14), ("dvbs2:R1_2short", "", 1.7, 30),
         ("dvbs2:R8_9short", "", 4.1, 12)]


def plain_of(name):
    return name.split(":")[0].replace("Norm", "").replace("Offset", "")


def gpu_decode(dec, name, llrs, max_iter):
    f64 = plain_of(name).endswith("f64")
    return dec.decode_batch(llrs.astype(np.float64) if f64 else llrs, max_iter, want_posterior=True)


def want_of(ref, name):
    bits, its, post = ref
    return bits, its, (post if plain_of(name).endswith("f64") else post.astype(np.float32))


def assert_same(got, want, what=""):
    assert np.array_equal(got[1], want[1]), ("iterations", what)
    assert np.array_equal(got[0], want[0]), ("bits", what)
    assert got[2].dtype == want[2].dtype
    assert np.array_equal(got[2], want[2], equal_nan=True), ("posterior", what)


def sample(spec, punct, ebn0, batch, seed=11):
    """seeded AWGN frames plus, where nothing is punctured, a clean frame (pre-check hit: 0 iterations); frame 1 is noise that
    belongs to no codeword (a failure)"""
    msgs, llrs, full = awgn_frames(spec, batch, ebn0, seed, punct)
    llrs = llrs.copy()
    rng = np.random.default_rng(seed)
    if not punct:
        enc = lt.Encoder(alist(spec))
        llrs[0] = np.where(enc.encode(msgs[0], llrs.shape[1]) == 1, -4.0, 4.0)
    llrs[1] = rng.standard_normal(llrs.shape[1]).astype(np.float32)
    if punct:
        from ldpc_toolbox_amd import simulation as sim
        full = sim.depuncture(llrs, sim.parse_puncturing_pattern(punct))
    else:
        full = llrs
    return llrs, full


@pytest.mark.parametrize("spec,punct,ebn0,max_iter", CODES)
@pytest.mark.parametrize("name", RULES)
def test_parity(name, spec, punct, ebn0, max_iter):
    batch = 40
    llrs, full = sample(spec, punct, ebn0, batch)
    dec = lt.LdpcDecoder(alist(spec), name, punct)
    assert dec.get("minsum_correction") == (1 if "Norm" in name else 2)
    got = gpu_decode(dec, name, llrs, max_iter)
    want = want_of(cm.decode(alist(spec), name, full, max_iter), name)
    its = want[1]
    print(f"{name} {spec}: iterations {sorted(set(its.tolist()))}")
    assert_same(got, want)
    assert (its < 0).any()                                        # failures
    assert len(set(its[its > 0].tolist())) >= 3                    # convergences spread over several iterations
    if not punct:
        assert its[0] == 0                                         # a pre-check hit
    if not plain_of(name).startswith("HL") and spec.startswith("dvbs2"):
        # the record kernels ran: rows of 27 edges take a fourth word in f32 (26 flip bits beside the argmin), not in f64 (58)
        assert dec.get("row_records") == (4 if spec == "dvbs2:R8_9short" and plain_of(name).endswith("f32") else 3)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("schedule", ["", "HL"])
def test_identity_with_plain_minsum(schedule, prec):
    spec, punct = "ar4ja:1/2:1024", "1,1,1,1,0"
    _, llrs, _ = awgn_frames(spec, 300, 1.9, 11, punct)
    plain_name = f"{schedule}Minsum{prec}"
    plain = gpu_decode(lt.LdpcDecoder(alist(spec), plain_name, punct), plain_name, llrs, 20)
    assert (plain[1] > 0).any() and (plain[1] < 0).any()
    for name in (f"{schedule}NormMinsum{prec}:1", f"{schedule}OffsetMinsum{prec}:0", f"{schedule}NormMinsum{prec}:1.000",
                 f"{schedule}OffsetMinsum{prec}:0.0"):
        dec = lt.LdpcDecoder(alist(spec), name, punct)
        for opts in ({}, {"records": 0}, {"staged_minsum": 1}):
            for k, v in opts.items():
                dec.set(k, v)
            got = gpu_decode(dec, name, llrs, 20)
            assert_same(got, plain, (name, opts))
            assert np.array_equal(np.signbit(got[2]), np.signbit(plain[2]))
    for name in (f"{schedule}NormMinsum{prec}", f"{schedule}OffsetMinsum{prec}"):
        got = gpu_decode(lt.LdpcDecoder(alist(spec), name, punct), name, llrs, 20)
        assert not np.array_equal(got[2], plain[2])               # the correction is live
        assert not np.array_equal(got[1], plain[1])


FLOODING_OPTS = ({"records": 0}, {"records": 0, "lfree": 0}, {"records": 2}, {"records": 2, "vn_event": 0},
                 {"records": 2, "vn_event": 0, "compact": 0}, {"records": 2, "vn_event": 1, "rec_quiet": 0},
                 {"records": 2, "rec_quiet": 1, "compact": 0, "vn_event": 1}, {"records": 2, "compact": 1, "rec_run": 1},
                 {"records": 2, "rec_run": 3}, {"records": 2, "rec_run": 64, "vec": 2}, {"records": 2, "rec_run": 8, "vec": 1},
                 {"records": 2, "rec_long": 1, "vec": 0}, {"staged_minsum": 1}, {"staged_minsum": 0, "pooling": 1},
                 {"pooling": 0, "group_size": 256})
LAYERED_OPTS = tuple({"hl_reg": a, "lanes": b, "group_size": c, "hl_records": d, "compact": e, "lane_threads": f, "throttle": g}
                     for a, b, c, d, e, f, g in ((1, 1, 4096, 1, 1, 1, 0), (0, 1, 4096, 1, 1, 1, 0), (1, 2, 4096, 0, 1, 1, 1),
                                                 (1, 2, 256, 1, 0, 1, 0), (0, 2, 512, 0, 1, 0, 1), (1, 1, 640, 0, 0, 0, 0))) + (
    {"staged_minsum": 1, "hl_reg": 1}, {"staged_minsum": 1, "hl_reg": 0}, {"staged_minsum": 0, "pooling": 1})


# (the layered schedule on a staircase code is one launch per row and level: test_parity has it, this test does not)
PATH_CASES = [(name, spec, punct, ebn0)
              for name in ("NormMinsumf32:0.8", "OffsetMinsumf64", "HLNormMinsumf64", "HLOffsetMinsumf32:0.3")
              for spec, punct, ebn0 in (("ar4ja:1/2:1024", "1,1,1,1,0", 1.9), ("dvbs2:R1_2short", "", 1.7), ("nr5g:1:16", "", 1.3))
              if not (name.startswith("HL") and spec.startswith("dvbs2"))]


@pytest.mark.parametrize("name,spec,punct,ebn0", PATH_CASES)
def test_every_path_returns_the_same(name, spec, punct, ebn0):
    """batch sizes that take the two single-launch paths (1, 8, 40) and the batched one (600, and 640 in groups of 256), the
    execution choices of the existing min-sum tests, the LDS-staged form, the small-batch paths on and off, pooling, the
    device-resident entry: one result, the restatement's"""
    import torch
    layered = name.startswith("HL")
    max_iter = 30 if spec.startswith("dvbs2") else 12
    llrs, full = sample(spec, punct, ebn0, 640)
    dec = lt.LdpcDecoder(alist(spec), name, punct)
    dec.set("latency", 0)
    dec.set("latency_edge", 0)
    ref = gpu_decode(dec, name, llrs, max_iter)                   # the batched kernels, defaults
    sub = 24
    want = want_of(cm.decode(alist(spec), name, full[:sub], max_iter), name)
    assert_same(tuple(x[:sub] for x in ref), want, "restatement")
    assert (ref[1] > 0).any() and (ref[1] < 0).any()
    f64 = plain_of(name).endswith("f64")
    for lat, edge in ((0, 0), (8, 0), (0, 64), (32, 256)):         # both off, row-lane only, lane-per-edge only, defaults
        dec.set("latency", lat)
        dec.set("latency_edge", edge)
        for batch in (1, 8, 40, 600):
            got = gpu_decode(dec, name, llrs[:batch], max_iter)
            assert_same(got, tuple(x[:batch] for x in ref), (lat, edge, batch))
    dec.set("latency", 0)
    dec.set("latency_edge", 0)
    for opts in (LAYERED_OPTS if layered else FLOODING_OPTS):
        for k, v in opts.items():
            dec.set(k, v)
        assert_same(gpu_decode(dec, name, llrs, max_iter), ref, opts)
        if not f64:
            d_llrs = torch.from_numpy(llrs).cuda()
            d_bits = torch.zeros((len(llrs), dec.n), dtype=torch.uint8, device="cuda")
            d_its = torch.zeros(len(llrs), dtype=torch.int32, device="cuda")
            d_post = torch.zeros((len(llrs), dec.n), dtype=torch.float32, device="cuda")
            dec.decode_batch_device(d_llrs.data_ptr(), False, len(llrs), max_iter, d_bits.data_ptr(), dec.n, d_its.data_ptr(),
                                    d_post.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert_same((d_bits.cpu().numpy(), d_its.cpu().numpy(), d_post.cpu().numpy()), ref, ("device", opts))


def _long_row_graph(seed, n, m, degree_of):
    rng = np.random.default_rng(seed)
    h = lt.SparseMatrix(m, n)
    for r in range(m):
        for c in rng.choice(n, size=degree_of(r), replace=False):
            h.insert(r, int(c))
    for c in range(n):
        if h.col_weight(c) == 0:
            h.insert(int(rng.integers(m)), c)
    return h.alist(), rng


@pytest.mark.parametrize("name", ["NormMinsumf32:0.8", "OffsetMinsumf32", "HLNormMinsumf32", "HLOffsetMinsumf64:0.3", "OffsetMinsumf64"])
@pytest.mark.parametrize("batch", [40, 600])
def test_long_rows(name, batch):
    """rows of 70-90 edges (beyond the streaming kernels' sign mask in the flooding schedule) and of 330-420 edges (beyond the
    LDS: the staged kernels' columns in HBM), built as test_rows_longer_than_64_edges / test_rows_beyond_the_lds_limit do"""
    for a, rng, n, mean in (_long_row_graph(12, 400, 24, lambda r: 70 + (r % 3) * 10) + (400, 2.5),
                            _long_row_graph(5, 1500, 14, lambda r: (330 + 30 * (r % 4)) if r < 8 else (5 + r)) + (1500, 3.0)):
        dec = lt.LdpcDecoder(a, name)
        llrs = (mean + 2.0 * rng.standard_normal((batch, n))).astype(np.float32)
        got = gpu_decode(dec, name, llrs, 6)
        sub = min(batch, 64)
        want = want_of(cm.decode(a, name, llrs[:sub], 6), name)
        assert_same(tuple(x[:sub] for x in got), want, n)
        dec.set("staged_minsum", 1)
        assert_same(gpu_decode(dec, name, llrs, 6), got, (n, "staged"))


@pytest.mark.parametrize("name", ["NormMinsumf32", "OffsetMinsumf32", "HLNormMinsumf32:0.8", "HLOffsetMinsumf32", "NormMinsumf64",
                                  "OffsetMinsumf64:0.3", "HLNormMinsumf64", "HLOffsetMinsumf64", "OffsetMinsumf32:1000"])
def test_special_inputs(name):
    """+-inf and huge LLRs (inf - inf = NaN inside), exact zeros and -0.0, subnormal LLRs (alpha * m is then a subnormal),
    an offset larger than every magnitude (all messages zero): the restatement's values, NaNs and signs of zero"""
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
    llrs[5, ::7] = np.float32(-1.0e-40)
    llrs[6] = (np.float32(1.0e-40) * rng.integers(1, 200, llrs.shape[1]) * sign[6]).astype(np.float32)   # all subnormal
    llrs[7, ::3] = 0.0
    llrs[7, 1::3] = -0.0
    llrs[8] = 0.0
    llrs[9] = -0.0
    dec = lt.LdpcDecoder(alist(spec), name)
    with np.errstate(all="ignore"):
        want = want_of(cm.decode(alist(spec), name, llrs, 12), name)
        for opts in ({}, {"staged_minsum": 1}, {"staged_minsum": 0, "records": 0, "hl_records": 0}, {"latency": 0, "latency_edge": 0}):
            for k, v in opts.items():
                dec.set(k, v)
            for batch in (140, 8):
                got = gpu_decode(dec, name, llrs[:batch], 12)
                w = tuple(x[:batch] for x in want)
                assert_same(got, w, (opts, batch))
                finite = np.isfinite(w[2])
                assert np.array_equal(np.signbit(got[2])[finite], np.signbit(w[2])[finite]), (opts, batch)
    assert (want[1] > 0).any()
    if not name.endswith(":1000"):
        assert np.isnan(want[2]).any()                             # the inf - inf rows were exercised


def test_what_the_feature_is_for():
    """256 frames of ar4ja:1/2:1024 at 1.75 dB, 30 flooding iterations in f32: plain min-sum loses most of them, the corrected
    rules few.  The GPU's frame-error counts are the restatement's, and each corrected count is at most half the plain one
    (the restatement gave 179, 12 and 8 when this was written: more than a factor of ten)."""
    import independent_restatement as ir
    spec, punct = "ar4ja:1/2:1024", "1,1,1,1,0"
    msgs, llrs, full = awgn_frames(spec, 256, 1.75, 11, punct)
    errors, ref_errors = {}, {}
    for name in ("Minsumf32", "NormMinsumf32", "OffsetMinsumf32"):
        dec = lt.LdpcDecoder(alist(spec), name, punct)
        bits, its, _ = dec.decode_batch(llrs, 30)
        k = msgs.shape[1]
        errors[name] = int((bits[:, :k] != msgs).any(axis=1).sum())
        rb, ri, _ = ir.decode(alist(spec), name, full, 30) if name == "Minsumf32" else cm.decode(alist(spec), name, full, 30)
        ref_errors[name] = int((rb[:, :k] != msgs).any(axis=1).sum())
        assert np.array_equal(bits, rb) and np.array_equal(its, ri), name
    print("frame errors of 256:", errors)
    assert errors == ref_errors
    assert 2 * errors["NormMinsumf32"] <= errors["Minsumf32"] and 2 * errors["OffsetMinsumf32"] <= errors["Minsumf32"]


def test_minsum_correction_key():
    a = alist("ar4ja:1/2:1024")
    for name, value in (("Minsumf32", 0), ("HLMinsumf64", 0), ("Tanhf32", 0), ("NormMinsumf32", 1), ("HLNormMinsumf64:0.9", 1),
                        ("OffsetMinsumf64", 2), ("HLOffsetMinsumf32:0.25", 2)):
        dec = lt.LdpcDecoder(a, name, "1,1,1,1,0")
        assert dec.get("minsum_correction") == value
        dec.close()


def test_simulator_takes_the_names():
    s = lt.Simulator(alist("dvbs2:R1_2short"), "OffsetMinsumf32:0.4", "", device=0, pool_size=8, pool_seed=2)
    a = s.run(1.8, seed=3, first_frame=0, frames=512, max_iterations=25)
    p = lt.Simulator(alist("dvbs2:R1_2short"), "Minsumf32", "", device=0, pool_size=8, pool_seed=2)
    b = p.run(1.8, seed=3, first_frame=0, frames=512, max_iterations=25)
    assert not np.array_equal(a, b)
    z = lt.Simulator(alist("dvbs2:R1_2short"), "OffsetMinsumf32:0", "", device=0, pool_size=8, pool_seed=2)
    assert np.array_equal(z.run(1.8, seed=3, first_frame=0, frames=512, max_iterations=25), b)
