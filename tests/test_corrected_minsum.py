"""Normalized and offset min-sum ([HL]NormMinsum / [HL]OffsetMinsum), the part that needs no GPU: the names through the
Python layer and the C ABI, and the numpy restatement the GPU tests compare against (corrected_minsum_restatement.py) --
its literal, combined and closed forms against each other, and alpha = 1 / beta = 0 against plain Minsum."""
import numpy as np
import pytest

import corrected_minsum_restatement as cm
import independent_restatement as ir
import ldpc_toolbox_amd as lt
from frames import alist, awgn_frames
from ldpc_toolbox_amd import _capi

DEFAULT_NAMES = ("NormMinsumf64", "NormMinsumf32", "OffsetMinsumf64", "OffsetMinsumf32",
                 "HLNormMinsumf64", "HLNormMinsumf32", "HLOffsetMinsumf64", "HLOffsetMinsumf32")
VALUED = ("NormMinsumf32:0.8125", "HLOffsetMinsumf64:0.3", "NormMinsumf32:1", "OffsetMinsumf32:0", "NormMinsumf64:0.8",
          "HLNormMinsumf32:1.0", "OffsetMinsumf64:12", "OffsetMinsumf32:0.000", "NormMinsumf32:0.001")
BAD = ("NormMinsumf32:0", "NormMinsumf32:1.5", "OffsetMinsumf32:-1", "NormMinsumf32:", "NormMinsumf32:.5", "NormMinsumf32:1e-1",
       "NormMinsumf32:0.5x", "OffsetMinsumf32:", "OffsetMinsumf32:.5", "OffsetMinsumf32:1e-1", "OffsetMinsumf32:0.5x",
       "NormMinsumf32:1.", "NormMinsumf32:+0.5", "NormMinsumf32:0.0", "OffsetMinsumf32:inf", "OffsetMinsumf32:nan",
       "NormMinsumf32@fast", "OffsetMinsumf64@fast", "HLNormMinsumf32@fast", "NormMinsumi8", "HLOffsetMinsumi8",
       "NormMinsum", "OffsetMinsumf16", "normminsumf32", "NormMinsumf32:0.5:0.5", "NormMinsumf32 ",
       # invalid before, invalid now
       "Minsumf32@fast", "HLMinsum", "Minsumf32:0.5")


def test_names_in_python():
    assert lt.CORRECTED_MINSUM_IMPLEMENTATIONS == DEFAULT_NAMES
    for name in DEFAULT_NAMES + VALUED:
        assert str(lt.DecoderImplementation(name)) == name
    for name in BAD:
        with pytest.raises(ValueError, match="invalid decoder implementation"):
            lt.DecoderImplementation(name)
    # the reference's tuples keep their contents
    assert len(lt.IMPLEMENTATIONS) == 20 and len(lt.I8_IMPLEMENTATIONS) == 20 and len(lt.ALL_IMPLEMENTATIONS) == 40
    assert lt.ALL_IMPLEMENTATIONS == lt.IMPLEMENTATIONS + lt.I8_IMPLEMENTATIONS
    assert lt.FAST_IMPLEMENTATIONS == ("Tanhf32@fast", "HLTanhf32@fast", "Phif32@fast", "HLPhif32@fast")
    assert not set(DEFAULT_NAMES) & set(lt.ALL_IMPLEMENTATIONS)
    assert sorted(lt.IMPLEMENTATIONS) == sorted(p + r + s for p in ("", "HL") for r in ("Phi", "Tanh", "Minstarapprox", "Aminstar", "Minsum")
                                                for s in ("f32", "f64"))


def test_names_through_the_c_abi():
    """a valid name gets as far as the device (and constructs when there is one); an invalid one stops at the parser"""
    a = alist("ar4ja:1/2:1024")
    have_gpu = _capi.lib().ldpc_toolbox_device_count() > 0
    for name in DEFAULT_NAMES + VALUED + ("NormMinsumf32:0.8125@hip", "OffsetMinsumf64:0.3@hip:0"):
        if have_gpu:
            dec = lt.LdpcDecoder(a, name, "1,1,1,1,0")
            assert dec.get("minsum_correction") == (1 if "Norm" in name else 2)
            dec.close()
        else:
            with pytest.raises(lt.DecoderUnavailable, match="no HIP device"):
                lt.LdpcDecoder(a, name, "1,1,1,1,0")
    for name in BAD + ("NormMinsumf32:1.5@hip", "OffsetMinsumf32:x@hip:0"):
        with pytest.raises(lt.DecoderUnavailable, match="invalid decoder implementation"):
            lt.LdpcDecoder(a, name, "1,1,1,1,0")


def _special_frames(full, rng):
    """subnormal, zero and negative-zero LLRs among ordinary ones"""
    full = full.copy()
    full[1, ::3] = np.float32(1.0e-40) * np.where(rng.random(full[1, ::3].shape) < 0.5, -1, 1)
    full[2, ::4] = 0.0
    full[2, 1::4] = -0.0
    full[3] *= np.float32(1.0e-38)
    return full


@pytest.mark.parametrize("schedule", ["", "HL"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_restatement_forms_agree(schedule, prec):
    """whole decodes: the combined form max(alpha * m - beta, 0) equals the two separate definitions, and the closed form
    (min1, min2, first argmin) equals the literal fold -- bits, iterations, and the final LLRs bit for bit with the sign of
    zero; alpha = 1 and beta = 0 equal plain Minsum"""
    spec, punct = "nr5g:2:8", ""
    rng = np.random.default_rng(3)
    _, _, full = awgn_frames(spec, 24, 1.5, 11, punct)
    full = _special_frames(full, rng)
    a = alist(spec)
    for stem, value in (("NormMinsum", "0.75"), ("OffsetMinsum", "0.5"), ("NormMinsum", "0.8"), ("OffsetMinsum", "0.3")):
        name = f"{schedule}{stem}{prec}:{value}"
        lit = cm.decode(a, name, full, 8, fast=False)
        assert (lit[1] > 0).any()
        for other in (cm.decode(a, name, full, 8, fast=False, combined=True), cm.decode(a, name, full, 8, fast=True),
                      cm.decode(a, name, full, 8, fast=True, combined=True)):
            assert np.array_equal(lit[0], other[0]) and np.array_equal(lit[1], other[1])
            assert cm.same(lit[2], other[2])
    plain = ir.decode(a, f"{schedule}Minsum{prec}", full, 8)
    changed = False
    for name in (f"{schedule}NormMinsum{prec}:1", f"{schedule}OffsetMinsum{prec}:0"):
        for fast in (False, True):
            got = cm.decode(a, name, full, 8, fast=fast)
            assert np.array_equal(plain[0], got[0]) and np.array_equal(plain[1], got[1]) and cm.same(plain[2], got[2])
    for name in (f"{schedule}NormMinsum{prec}", f"{schedule}OffsetMinsum{prec}"):
        changed = changed or not np.array_equal(plain[2], cm.decode(a, name, full, 8)[2], equal_nan=True)
    assert changed                                   # the default values do something


def test_restatement_plain_equals_the_oracle(oracle):
    """... and through independent_restatement.decode, the C oracle (what the GPU's plain Minsum is pinned to)"""
    spec = "nr5g:2:8"
    _, _, full = awgn_frames(spec, 16, 1.5, 12)
    a = alist(spec)
    for name, plain in (("NormMinsumf32:1", "Minsumf32"), ("HLOffsetMinsumf64:0", "HLMinsumf64")):
        got = cm.decode(a, name, full, 6)
        ob, oi, op = oracle.decode_batch(oracle.Graph(a), plain, full, 6, threads=4)
        assert np.array_equal(got[0], ob) and np.array_equal(got[1], oi)
        run = oi != 0
        assert np.array_equal(got[2][run], op[run])


def test_restatement_message_values():
    """the rule on one row, by hand: magnitudes, the clamp at zero and its signed zeros, a row of +inf"""
    f = np.float32
    x = np.array([[2.0, -0.5, 3.0, -0.25]], dtype=f)
    norm = cm.CorrectedMinsum(f, "Norm", 0.75)._all(x)
    assert np.array_equal(norm, np.array([[f(0.75) * f(0.25), -f(0.75) * f(0.25), f(0.75) * f(0.25), -f(0.75) * f(0.5)]], dtype=f))
    off = cm.CorrectedMinsum(f, "Offset", 0.3)._all(x)
    assert np.array_equal(off, np.array([[0.0, -0.0, 0.0, -(f(0.5) - f(0.3))]], dtype=f))
    assert np.array_equal(np.signbit(off), np.array([[False, True, False, True]]))
    x = np.array([[np.inf, -np.inf, 1.0]], dtype=f)
    assert np.array_equal(cm.CorrectedMinsumFast(f, "Offset", 0.5)._all(x), np.array([[-0.5, 0.5, -np.inf]], dtype=f))
