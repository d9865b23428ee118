"""The 8-bit min-sum family ([HL]Minsumi8[Norm|Offset]<options>[:value]), the part that needs no GPU: the names through the
Python layer, the C ABI and the parser under ASan / UBSan, and the numpy restatement the GPU tests compare against
(minsum_i8_restatement.py) -- its literal fold against its closed form, Norm:1 / Offset:0 against plain, and plain against
independent_restatement.I8Arithmetic with a zeroed lookup table."""
import os
import subprocess

import numpy as np
import pytest

import independent_restatement as ir
import ldpc_toolbox_amd as lt
import minsum_i8_restatement as mi
from frames import alist, awgn_frames
from ldpc_toolbox_amd import _capi

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
STEMS = ("Minsumi8", "Minsumi8Norm", "Minsumi8Offset")
DEFAULT_NAMES = tuple(n for b in STEMS for n in
                      tuple(b + j + h + d for j in ("", "Jones") for h in ("", "PartialHardLimit") for d in ("", "Deg1Clip"))
                      + ("HL" + b, "HL" + b + "PartialHardLimit"))
# (name, minsum_correction, minsum_correction_int)
VALUED = (("Minsumi8Norm:0.8125", 1, 13), ("Minsumi8Offset:0.25", 2, 2), ("HLMinsumi8Norm:1", 1, 16), ("Minsumi8Offset:0", 2, 0),
          ("Minsumi8Norm:0.0625", 1, 1), ("Minsumi8Offset:15.875", 2, 127), ("Minsumi8NormJonesPartialHardLimitDeg1Clip:0.5", 1, 8),
          ("HLMinsumi8OffsetPartialHardLimit:1.000", 2, 8), ("Minsumi8Norm:1.0", 1, 16), ("Minsumi8OffsetDeg1Clip:0.125", 2, 1))
BAD = ("Minsumi8:0.5", "Minsumi8Norm:0.8", "Minsumi8Norm:0", "Minsumi8Norm:1.5", "Minsumi8Offset:0.3", "Minsumi8Offset:16",
       "Minsumi8JonesNorm", "HLMinsumi8Jones", "HLMinsumi8NormDeg1Clip", "Minsumi8Norm:", "Minsumi8Norm:.5", "Minsumi8Norm:1e-1",
       "NormMinsumi8",
       # and their like
       "HLOffsetMinsumi8", "Minsumi8Jones:0.5", "Minsumi8Norm:0.03125", "Minsumi8Norm:1.0625", "Minsumi8Offset:-1",
       "Minsumi8Offset:0.5x", "Minsumi8Norm:0.75:0.75", "Minsumi8NormOffset", "Minsumi8OffsetNorm", "Minsumi8Deg1ClipJones",
       "Minsumi8PartialHardLimitJones", "Minsumi8Norm ", "minsumi8", "Minsumi8@fast", "Minsumi16", "HLMinsumi8OffsetJones:0.5",
       "Minsumi8Norm:+0.5", "Minsumi8Offset:inf", "Minsumi8Norm:nan", "Minsumi8Norm:0.75Jones", "Phii8", "Tanhi8Norm")


def test_names_in_python():
    assert lt.MINSUM_I8_IMPLEMENTATIONS == DEFAULT_NAMES and len(DEFAULT_NAMES) == 30
    assert "MINSUM_I8_IMPLEMENTATIONS" in lt.__all__
    for name in DEFAULT_NAMES + tuple(v[0] for v in VALUED):
        assert str(lt.DecoderImplementation(name)) == name
        mi.parse(name)
    for name in BAD:
        with pytest.raises(ValueError, match="invalid decoder implementation"):
            lt.DecoderImplementation(name)
        with pytest.raises(ValueError, match="invalid decoder implementation"):
            mi.parse(name)
    for name, _, value in VALUED:
        assert mi.parse(name)[2] == value
    assert mi.parse("Minsumi8Norm")[2] == 12 and mi.parse("HLMinsumi8Offset")[2] == 4 and mi.parse("Minsumi8Jones")[1:3] == (None, 0)
    # the other tuples keep their contents
    assert len(lt.IMPLEMENTATIONS) == 20 and len(lt.I8_IMPLEMENTATIONS) == 20 and len(lt.ALL_IMPLEMENTATIONS) == 40
    assert lt.ALL_IMPLEMENTATIONS == lt.IMPLEMENTATIONS + lt.I8_IMPLEMENTATIONS
    assert len(lt.CORRECTED_MINSUM_IMPLEMENTATIONS) == 8
    assert not set(DEFAULT_NAMES) & (set(lt.ALL_IMPLEMENTATIONS) | set(lt.CORRECTED_MINSUM_IMPLEMENTATIONS))


def test_names_through_the_c_abi():
    """a valid name gets as far as the device (and constructs when there is one); an invalid one stops at the parser"""
    a = alist("ar4ja:1/2:1024")
    have_gpu = _capi.lib().ldpc_toolbox_device_count() > 0
    cases = [(n, 1 if "Norm" in n else (2 if "Offset" in n else 0), 12 if "Norm" in n else (4 if "Offset" in n else 0))
             for n in DEFAULT_NAMES] + list(VALUED) + [("Minsumi8Norm:0.8125@hip", 1, 13), ("HLMinsumi8Offset:0.25@hip:0", 2, 2),
                                                       ("Minsumi8@hip", 0, 0)]
    for name, kind, value in cases:
        if have_gpu:
            dec = lt.LdpcDecoder(a, name, "1,1,1,1,0")
            assert dec.get("minsum_correction") == kind and dec.get("minsum_correction_int") == value, name
            dec.close()
        else:
            with pytest.raises(lt.DecoderUnavailable, match="no HIP device"):
                lt.LdpcDecoder(a, name, "1,1,1,1,0")
    for name in BAD + ("Minsumi8Norm:1.5@hip", "Minsumi8Offset:x@hip:0", "NormMinsumi8@hip"):
        with pytest.raises(lt.DecoderUnavailable, match="invalid decoder implementation"):
            lt.LdpcDecoder(a, name, "1,1,1,1,0")
    for name in BAD[:6]:
        with pytest.raises(lt.DecoderUnavailable, match="invalid decoder implementation"):
            lt.Simulator(a, name, "1,1,1,1,0", device=0, pool_size=8, pool_seed=2)


def test_parser_is_clean_under_asan_ubsan(tmp_path):
    """the parser (csrc/implementation.cpp) with AddressSanitizer + UBSan over the names given on the command line: "+name" must
    parse to the stated integers, "-name" must be refused; and the name lists keep their sizes (40, 8, 30)"""
    exe = str(tmp_path / "minsum_i8_name_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "minsum_i8_name_driver.cpp"),
                    os.path.join(ROOT, "ldpc_toolbox_amd", "csrc", "implementation.cpp")], check=True, capture_output=True)
    args = [f"+{n}={1 if 'Norm' in n else (2 if 'Offset' in n else 0)},{12 if 'Norm' in n else (4 if 'Offset' in n else 0)}"
            for n in DEFAULT_NAMES]
    args += [f"+{n}={k},{v}" for n, k, v in VALUED] + ["-" + n for n in BAD]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + args, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"minsum i8 name driver: ok ({len(args)} names)" in r.stdout


def _frames(spec):
    """noisy frames, a saturating one (the clip at +-127 and the hard limit at 100 matter), zeros, and a clean one"""
    msgs, _, full = awgn_frames(spec, 24, 1.5, 11)
    full = full.copy()
    full[2] *= 6.0
    full[3, ::4] = 0.0
    full[3, 1::4] = -0.0
    enc = lt.Encoder(alist(spec))
    full[4] = np.where(enc.encode(msgs[4], full.shape[1]) == 1, -4.0, 4.0)
    return full


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("schedule", ["", "HL"])
def test_restatement_forms_agree(schedule):
    """whole decodes on nr5g:2:8: the literal fold equals the closed form (bits, iterations, posterior); Norm:1 and Offset:0
    equal plain; plain equals I8Arithmetic with a zeroed table; the defaults do something"""
    spec = "nr5g:2:8"
    a = alist(spec)
    full = _frames(spec)
    options = ("", "PartialHardLimit") if schedule else ("", "JonesPartialHardLimitDeg1Clip", "Jones", "Deg1Clip")
    for opt in options:
        plain = mi.decode(a, f"{schedule}Minsumi8{opt}", full, 8, fast=False)
        assert (plain[1] > 0).any() and plain[1][4] == 0
        assert np.abs(plain[2]).max() == 127
        for stem, values in (("", ("",)), ("Norm", ("", ":0.8125", ":0.0625")), ("Offset", ("", ":0.25", ":15.875"))):
            for value in values:
                name = f"{schedule}Minsumi8{stem}{opt}{value}"
                lit = mi.decode(a, name, full, 8, fast=False)
                assert _same(lit, mi.decode(a, name, full, 8, fast=True)), name
        for name in (f"{schedule}Minsumi8Norm{opt}:1", f"{schedule}Minsumi8Offset{opt}:0", f"{schedule}Minsumi8Norm{opt}:1.00"):
            for fast in (False, True):
                assert _same(plain, mi.decode(a, name, full, 8, fast=fast)), name
        # the definition's one changed line: the lookup term gone
        A = ir.I8Arithmetic(False, "Jones" in opt, "PartialHardLimit" in opt, "Deg1Clip" in opt)
        A.table[:] = 0
        assert _same(plain, mi.decode_with(A, bool(schedule), a, full, 8)), opt
        star = mi.decode_with(ir.I8Arithmetic(False, "Jones" in opt, "PartialHardLimit" in opt, "Deg1Clip" in opt), bool(schedule),
                              a, full, 8)
        assert not np.array_equal(star[2], plain[2])
        for stem in ("Norm", "Offset"):
            assert not np.array_equal(mi.decode(a, f"{schedule}Minsumi8{stem}{opt}", full, 8)[2], plain[2])


def test_restatement_message_values():
    """the rule on one row, by hand: first argmin on a tie, rounding of (a m + 8) >> 4, the clamp of the offset at zero, the
    hard limit after the correction, zero stays zero"""
    x = np.array([[40, -3, 3, -127]], dtype=np.int32)
    for cls in (mi.MinsumI8, mi.MinsumI8Fast):
        assert np.array_equal(cls(None, 0, False, False, False)._minstar_all(x), [[3, -3, 3, -3]])
    x = np.array([[-120, 127, 110, -127]], dtype=np.int32)
    for cls in (mi.MinsumI8, mi.MinsumI8Fast):
        assert np.array_equal(cls(None, 0, False, False, False)._minstar_all(x), [[-110, 110, 120, -110]])
        assert np.array_equal(cls("Norm", 12, False, False, False)._minstar_all(x), [[-83, 83, 90, -83]])       # (12*110+8)>>4 = 83
        assert np.array_equal(cls("Norm", 12, False, True, False)._minstar_all(x), [[-83, 83, 90, -83]])
        assert np.array_equal(cls("Norm", 15, False, True, False)._minstar_all(x), [[-127, 127, 127, -127]])    # 103, 113 -> 127
        assert np.array_equal(cls("Offset", 12, False, True, False)._minstar_all(x), [[-98, 98, 127, -98]])     # 108 -> 127, 98 stays
        assert np.array_equal(cls("Offset", 127, False, False, False)._minstar_all(x), [[0, 0, 0, 0]])
        y = np.array([[5, -1, 9]], dtype=np.int32)
        assert np.array_equal(cls("Norm", 1, False, False, False)._minstar_all(y), [[0, 0, 0]])                 # (1*5+8)>>4 = 0
        assert np.array_equal(cls("Norm", 8, False, False, False)._minstar_all(y), [[-1, 3, -1]])               # (8+8)>>4 = 1, (40+8)>>4 = 3
        assert np.array_equal(cls("Offset", 2, False, False, False)._minstar_all(y), [[0, 3, 0]])


def test_quantiser_special_values():
    A = mi.MinsumI8(None, 0, False, False, False)
    with np.errstate(all="ignore"):
        q = A.input_llr_quantize(np.array([np.nan, np.inf, -np.inf, 1e300, -0.0, 0.0625, -0.0625, 0.06, 15.875, 15.9, -3.0e38]))
    assert np.array_equal(q, [0, 127, -127, 127, 0, 1, -1, 0, 127, 127, -127])
