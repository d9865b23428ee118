"""The 8-bit min-sum family on the GPU against the numpy restatement (minsum_i8_restatement.py): bits, iteration counts and
the posterior (the clipped i8 value, in quantiser units) with np.array_equal -- no tolerance -- on every path the names take.

The restatement decodes run in a pool of CPU processes (spawned: they never touch the GPU) while the GPU decodes run; every
decode is submitted once, under a key, when the first test asks for one."""
import multiprocessing
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import independent_restatement as ir
import ldpc_toolbox_amd as lt
import minsum_i8_restatement as mi
from frames import alist, awgn_frames
from test_corrected_minsum_gpu import _long_row_graph, sample

pytestmark = pytest.mark.gpu

STEMS = ("Minsumi8", "Minsumi8Norm", "Minsumi8Offset", "Minsumi8Norm:0.8125", "Minsumi8Offset:0.25")
RULES = STEMS + tuple("HL" + s for s in STEMS)
OPTION_RULES = ("Minsumi8NormJones", "Minsumi8OffsetPartialHardLimitDeg1Clip", "Minsumi8JonesPartialHardLimitDeg1Clip",
                "HLMinsumi8NormPartialHardLimit")
CORRECTION_INT = {"Minsumi8": 0, "Minsumi8Norm": 12, "Minsumi8Offset": 4, "Minsumi8Norm:0.8125": 13, "Minsumi8Offset:0.25": 2}
# (code, puncturing, Eb/N0, iterations)
CODES = [("ar4ja:1/2:1024", "1,1,1,1,0", 1.9, 20), ("nr5g:2:24", "", 1.6, 14), ("dvbs2:R1_2short", "", 1.7, 30),
         ("dvbs2:R8_9short", "", 4.1, 12)]
PARITY_CASES = [(name, spec, punct, ebn0, it) for spec, punct, ebn0, it in CODES for name in RULES + OPTION_RULES
                if not (spec.startswith("dvbs2") and (name.startswith("HL") or name in OPTION_RULES))]
PATH_CASES = [(name, spec, punct, ebn0) for name in ("Minsumi8Norm", "HLMinsumi8Offset:0.25")
              for spec, punct, ebn0 in (("ar4ja:1/2:1024", "1,1,1,1,0", 1.9), ("dvbs2:R1_2short", "", 1.7), ("nr5g:1:16", "", 1.3))
              if not (name.startswith("HL") and spec.startswith("dvbs2"))]
OPTION_CASES = ("Minsumi8", "Minsumi8Jones", "Minsumi8PartialHardLimit", "Minsumi8Deg1Clip", "Minsumi8NormJonesPartialHardLimitDeg1Clip",
                "Minsumi8OffsetPartialHardLimit", "HLMinsumi8", "HLMinsumi8PartialHardLimit")
PURPOSE = ("Minsumi8", "Minsumi8Norm", "Minsumi8Offset", "Minstarapproxi8")


def _strong_sample():
    """the strong-LLR sample of test_i8_options_change_results_where_they_should: saturation at +-127, weak wrong symbols"""
    spec, punct = "ar4ja:1/2:1024", "1,1,1,1,0"
    _, llrs, _ = awgn_frames(spec, 256, 6.5, 33, punct)
    llrs = llrs.copy()
    llrs[:, ::3] *= -0.02
    from ldpc_toolbox_amd import simulation as sim
    return llrs, sim.depuncture(llrs, sim.parse_puncturing_pattern(punct))


def _path_iterations(spec):
    return 30 if spec.startswith("dvbs2") else 12


_POOL = None
_JOBS = {}


def _submit_all():
    """every restatement decode of this file, the longest first (DVB-S2 short: half a minute each in the closed form)"""
    global _POOL
    ir._libm()                                                     # built once, before the workers want it
    _POOL = ProcessPoolExecutor(max_workers=12, mp_context=multiprocessing.get_context("spawn"))
    jobs = []
    for name, spec, punct, ebn0, it in PARITY_CASES:
        jobs.append((("parity", name, spec), mi.decode, (alist(spec), name, sample(spec, punct, ebn0, 40)[1], it)))
    for name, spec, punct, ebn0 in PATH_CASES:
        jobs.append((("path", name, spec), mi.decode, (alist(spec), name, sample(spec, punct, ebn0, 640)[1][:24], _path_iterations(spec))))
    strong = _strong_sample()[1]
    for name in OPTION_CASES:
        jobs.append((("options", name), mi.decode, (alist("ar4ja:1/2:1024"), name, strong, 12)))
    full = awgn_frames("ar4ja:1/2:1024", 256, 1.75, 11, "1,1,1,1,0")[2]
    for name in PURPOSE:
        jobs.append((("purpose", name), ir.decode if name == "Minstarapproxi8" else mi.decode, (alist("ar4ja:1/2:1024"), name, full, 30)))
    cost = lambda j: (0 if j[0][-1].startswith("dvbs2:R1_2") else 1 if j[0][0] == "purpose" else 2 if j[0][-1].startswith("dvbs2") else 3)
    for key, fn, args in sorted(jobs, key=cost):
        _JOBS[key] = _POOL.submit(fn, *args)


def reference(*key):
    if _POOL is None:
        _submit_all()
    return _JOBS[key].result()


@pytest.fixture(scope="module", autouse=True)
def _pool_cleanup():
    yield
    if _POOL is not None:
        _POOL.shutdown(wait=True, cancel_futures=True)


def gpu_decode(dec, llrs, max_iter):
    return dec.decode_batch(llrs, max_iter, want_posterior=True)


def want_of(ref, dtype=np.float32):
    return ref[0], ref[1], ref[2].astype(dtype)


def assert_same(got, want, what=""):
    assert np.array_equal(got[1], want[1]), ("iterations", what)
    assert np.array_equal(got[0], want[0]), ("bits", what)
    assert got[2].dtype == want[2].dtype, what
    assert np.array_equal(got[2], want[2]), ("posterior", what)


@pytest.mark.parametrize("name,spec,punct,ebn0,max_iter", PARITY_CASES)
def test_parity(name, spec, punct, ebn0, max_iter):
    llrs, full = sample(spec, punct, ebn0, 40)
    dec = lt.LdpcDecoder(alist(spec), name, punct)
    got = gpu_decode(dec, llrs, max_iter)
    want = want_of(reference("parity", name, spec))
    its = want[1]
    print(f"{name} {spec}: {int((its < 0).sum())} failures, iterations {sorted(set(its[its > 0].tolist()))}")
    assert_same(got, want)
    if name in OPTION_RULES:
        return                                                     # equality only
    assert dec.get("minsum_correction_int") == CORRECTION_INT[name[2:] if name.startswith("HL") else name]
    assert (its < 0).any()                                         # a failure is present
    assert len(set(its[its > 0].tolist())) >= 3                    # convergences spread over several iterations
    if not punct:
        assert its[0] == 0                                         # a pre-check hit
    assert (np.abs(want[2]) == 127).any()                          # the clip was reached


@pytest.mark.parametrize("schedule", ["", "HL"])
def test_identity_and_defaults(schedule):
    """Norm:1 and Offset:0 are plain Minsumi8 (a = 16, b = 0); the defaults differ from plain; plain differs from Minstarapproxi8"""
    spec, punct = "ar4ja:1/2:1024", "1,1,1,1,0"
    _, llrs, _ = awgn_frames(spec, 300, 1.9, 11, punct)
    for opt in ("", "PartialHardLimit"):
        plain = gpu_decode(lt.LdpcDecoder(alist(spec), f"{schedule}Minsumi8{opt}", punct), llrs, 20)
        assert (plain[1] > 0).any() and (plain[1] < 0).any()
        for name in (f"{schedule}Minsumi8Norm{opt}:1", f"{schedule}Minsumi8Offset{opt}:0", f"{schedule}Minsumi8Norm{opt}:1.000",
                     f"{schedule}Minsumi8Offset{opt}:0.0"):
            assert_same(gpu_decode(lt.LdpcDecoder(alist(spec), name, punct), llrs, 20), plain, name)
        for name in (f"{schedule}Minsumi8Norm{opt}", f"{schedule}Minsumi8Offset{opt}", f"{schedule}Minstarapproxi8{opt}"):
            got = gpu_decode(lt.LdpcDecoder(alist(spec), name, punct), llrs, 20)
            assert not np.array_equal(got[2], plain[2]), name
            assert not np.array_equal(got[1], plain[1]), name


def test_options_change_results_where_they_should():
    """strong LLRs (saturation at +-127) make Jones / PartialHardLimit / Deg1Clip differ from the plain rule, and the GPU
    follows the restatement in each case, at the large batch and as small calls"""
    spec, punct = "ar4ja:1/2:1024", "1,1,1,1,0"
    llrs, _ = _strong_sample()
    outs = {}
    for name in OPTION_CASES:
        dec = lt.LdpcDecoder(alist(spec), name, punct)
        got = gpu_decode(dec, llrs, 12)
        assert_same(got, want_of(reference("options", name)), name)
        outs[name] = got
        for B in (1, 11):
            assert_same(gpu_decode(dec, llrs[:B], 12), tuple(x[:B] for x in got), (name, B))
    differs = lambda a, b: not (np.array_equal(outs[a][1], outs[b][1]) and np.array_equal(outs[a][2], outs[b][2]))
    assert (outs["Minsumi8"][1] != 0).all()                        # every frame iterates
    for name in ("Minsumi8Jones", "Minsumi8PartialHardLimit", "Minsumi8Deg1Clip"):
        assert differs(name, "Minsumi8"), name
    assert differs("HLMinsumi8PartialHardLimit", "HLMinsumi8")


@pytest.mark.parametrize("name,spec,punct,ebn0", PATH_CASES)
def test_every_path_returns_the_same(name, spec, punct, ebn0):
    """batches of 1, 8, 40, 600, and 640 in groups of 256; the small-batch switches on and off (these names take the batched
    kernels at every size); compaction, lanes, pooling, the row-serial and two-pass layered forms; the device-resident entry
    with f32 and f64 LLRs: one result, the restatement's"""
    import torch
    layered = name.startswith("HL")
    max_iter = _path_iterations(spec)
    llrs, _ = sample(spec, punct, ebn0, 640)
    dec = lt.LdpcDecoder(alist(spec), name, punct)
    ref = gpu_decode(dec, llrs, max_iter)
    assert_same(tuple(x[:24] for x in ref), want_of(reference("path", name, spec)), "restatement")
    assert (ref[1] > 0).any() and (ref[1] < 0).any()
    for lat, edge in ((0, 0), (32, 256)):
        dec.set("latency", lat)
        dec.set("latency_edge", edge)
        for batch in (1, 8, 40, 600):
            assert_same(gpu_decode(dec, llrs[:batch], max_iter), tuple(x[:batch] for x in ref), (lat, edge, batch))
    got64 = gpu_decode(dec, llrs.astype(np.float64), max_iter)
    assert_same(got64, want_of(ref, np.float64), "f64 LLRs")
    options = [{"group_size": 256}, {"compact": 0}, {"compact": 1, "lanes": 2}, {"lanes": 1, "pooling": 1}, {"pooling": 0, "group_size": 640}]
    if layered:
        options += [{"hl_reg": 0, "group_size": 4096}, {"hl_reg": 1, "lanes": 2, "lane_threads": 0, "throttle": 1}]
    for opts in options:
        for k, v in opts.items():
            dec.set(k, v)
        assert_same(gpu_decode(dec, llrs, max_iter), ref, opts)
        for f64 in (False, True):
            t = torch.float64 if f64 else torch.float32
            d_llrs = torch.from_numpy(llrs.astype(np.float64) if f64 else llrs).cuda()
            d_bits = torch.zeros((len(llrs), dec.n), dtype=torch.uint8, device="cuda")
            d_its = torch.zeros(len(llrs), dtype=torch.int32, device="cuda")
            d_post = torch.zeros((len(llrs), dec.n), dtype=t, device="cuda")
            dec.decode_batch_device(d_llrs.data_ptr(), f64, len(llrs), max_iter, d_bits.data_ptr(), dec.n, d_its.data_ptr(),
                                    d_post.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert_same((d_bits.cpu().numpy(), d_its.cpu().numpy(), d_post.cpu().numpy()), want_of(ref, np.float64 if f64 else np.float32),
                        ("device", f64, opts))


@pytest.mark.parametrize("name", ["Minsumi8Norm", "Minsumi8OffsetPartialHardLimit", "HLMinsumi8", "HLMinsumi8Norm:0.8125"])
@pytest.mark.parametrize("batch", [40, 600])
def test_long_rows(name, batch):
    """rows of 70-90 edges and of 330-420 edges (the generator of test_long_rows), and rows of 31-34 edges: either side of the
    32 edges whose input signs the flooding kernel keeps in registers"""
    for a, rng, n, mean in (_long_row_graph(12, 400, 24, lambda r: 70 + (r % 3) * 10) + (400, 2.5),
                            _long_row_graph(5, 1500, 14, lambda r: (330 + 30 * (r % 4)) if r < 8 else (5 + r)) + (1500, 3.0),
                            _long_row_graph(7, 300, 16, lambda r: 31 + r % 4) + (300, 2.0)):
        dec = lt.LdpcDecoder(a, name)
        llrs = (mean + 2.0 * rng.standard_normal((batch, n))).astype(np.float32)
        got = gpu_decode(dec, llrs, 6)
        sub = min(batch, 64)
        assert_same(tuple(x[:sub] for x in got), want_of(mi.decode(a, name, llrs[:sub], 6)), n)
        assert (got[1] != 0).any()
        if name.startswith("HL"):
            dec.set("hl_reg", 0)
            assert_same(gpu_decode(dec, llrs, 6), got, (n, "hl_reg 0"))


@pytest.mark.parametrize("name", ["Minsumi8", "Minsumi8OffsetJonesPartialHardLimitDeg1Clip", "HLMinsumi8Norm", "HLMinsumi8OffsetPartialHardLimit"])
def test_special_inputs(name):
    """+-inf and huge LLRs (the quantiser's clamp), NaN (quantised to 0, hard decision of the raw input 0), exact zeros and
    -0.0, whole frames of each"""
    spec = "nr5g:2:24"
    msgs, llrs, _ = awgn_frames(spec, 140, 1.2, 404)
    enc = lt.Encoder(alist(spec))
    sign = np.where(np.stack([enc.encode(m, llrs.shape[1]) for m in msgs]) == 1, -1.0, 1.0).astype(np.float32)
    rng = np.random.default_rng(5)
    known = rng.random(llrs.shape) < 0.06
    llrs = llrs.copy()
    llrs[known] = (sign * np.float32(np.inf))[known]
    llrs[3] = np.where(rng.random(llrs.shape[1]) < 0.5, np.float32(1e30) * sign[3], llrs[3]).astype(np.float32)
    llrs[4, ::5] = np.float32(3.0e38) * sign[4, ::5]
    llrs[5, ::7] = np.float32(np.nan)
    llrs[6, ::2] = np.float32(np.nan)
    llrs[7, ::3] = 0.0
    llrs[7, 1::3] = -0.0
    llrs[8] = 0.0
    llrs[9] = -0.0
    llrs[10] = np.float32(np.nan)
    llrs[11] = np.float32(np.inf) * sign[11]
    llrs[12] = np.float32(-np.inf)
    llrs[13] = np.float32(1.0e-40) * sign[13]
    with np.errstate(all="ignore"):
        want = mi.decode(alist(spec), name, llrs, 12)
    assert (want[1] > 0).any() and (want[1] < 0).any() and want[1][11] == 0
    dec = lt.LdpcDecoder(alist(spec), name)
    for batch in (140, 8):
        assert_same(gpu_decode(dec, llrs[:batch], 12), tuple(x[:batch] for x in want_of(want)), batch)
        assert_same(gpu_decode(dec, llrs[:batch].astype(np.float64), 12), tuple(x[:batch] for x in want_of(want, np.float64)), (batch, "f64"))


def test_what_the_feature_is_for():
    """256 frames of ar4ja:1/2:1024 at 1.75 dB, 30 flooding iterations: plain 8-bit min-sum loses most of them, the corrected
    rules few -- close to Minstarapproxi8, at a fraction of its arithmetic.  The GPU's frame-error counts are the restatement's,
    and each corrected count is at most half the plain one (the restatement gave 179, 14, 8, and 3 for Minstarapproxi8)."""
    spec, punct = "ar4ja:1/2:1024", "1,1,1,1,0"
    msgs, llrs, _ = awgn_frames(spec, 256, 1.75, 11, punct)
    k = msgs.shape[1]
    errors, ref_errors = {}, {}
    for name in PURPOSE:
        bits, its, _ = lt.LdpcDecoder(alist(spec), name, punct).decode_batch(llrs, 30)
        errors[name] = int((bits[:, :k] != msgs).any(axis=1).sum())
        rb, ri, _ = reference("purpose", name)
        ref_errors[name] = int((rb[:, :k] != msgs).any(axis=1).sum())
        assert np.array_equal(bits, rb) and np.array_equal(its, ri), name
    print("frame errors of 256:", errors)
    assert errors == ref_errors
    assert 2 * errors["Minsumi8Norm"] <= errors["Minsumi8"] and 2 * errors["Minsumi8Offset"] <= errors["Minsumi8"]


def test_simulator_and_keys():
    a = alist("dvbs2:R1_2short")
    run = lambda name: lt.Simulator(a, name, "", device=0, pool_size=8, pool_seed=2).run(1.8, seed=3, first_frame=0, frames=512,
                                                                                       max_iterations=25)
    plain = run("Minsumi8")
    assert plain[0] == 512
    assert np.array_equal(run("Minsumi8Norm:1"), plain) and np.array_equal(run("Minsumi8Offset:0"), plain)
    assert not np.array_equal(run("Minsumi8Norm"), plain) and not np.array_equal(run("Minsumi8Offset"), plain)
    assert not np.array_equal(run("Minstarapproxi8"), plain)
    hl = lt.Simulator(alist("nr5g:2:24"), "HLMinsumi8Norm", "", device=0, pool_size=8, pool_seed=2)
    assert hl.run(1.6, seed=3, first_frame=0, frames=512, max_iterations=14)[0] == 512
    a = alist("ar4ja:1/2:1024")
    for name, kind, value in (("Minsumi8", 0, 0), ("HLMinsumi8PartialHardLimit", 0, 0), ("Minsumi8Norm", 1, 12), ("HLMinsumi8Norm:0.8125", 1, 13),
                              ("Minsumi8OffsetJones", 2, 4), ("HLMinsumi8Offset:0.25", 2, 2), ("Minsumi8Norm:1", 1, 16), ("Minsumi8Offset:0", 2, 0),
                              ("Minstarapproxi8", 0, 0), ("Minsumf32", 0, 0), ("NormMinsumf32", 1, 0)):
        dec = lt.LdpcDecoder(a, name, "1,1,1,1,0")
        assert dec.get("minsum_correction") == kind and dec.get("minsum_correction_int") == value, name
        dec.close()
