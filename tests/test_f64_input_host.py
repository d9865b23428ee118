"""CPU: the premises of the f64-input parity tests (f64_input_cases.py, test_f64_input_gpu.py), from the reference alone --
the oracle's one-codeword f64 entry on every frame, for all 40 names of lt.ALL_IMPLEMENTATIONS and both codes.  What is
asserted here is what makes the GPU comparison mean something: the frames decode (no panic), they iterate, converge and
fail, and an entry that narrowed the input to float before the decoder's own conversion would return something else."""
import numpy as np
import pytest

import f64_input_cases as fc
import ldpc_toolbox_amd as lt

NAMES = lt.ALL_IMPLEMENTATIONS


def _rounded_first(code):
    with np.errstate(over="ignore"):
        return fc.frames(code).astype(np.float32).astype(np.float64)


def _changed(oracle, code, name):
    """the frames on which the reference returns something else (bits, iterations or posterior; or panics) once the frame
    has been rounded to float"""
    want = fc.reference(oracle, code, name)
    panics = []
    got = fc.decode_reference(oracle, code, name, _rounded_first(code), panics=panics)
    return [f for f in range(fc.FRAMES)
            if f in panics or got[1][f] != want[1][f] or not np.array_equal(got[0][f], want[0][f])
            or not np.array_equal(got[2][f], want[2][f], equal_nan=True)]


def test_the_frames_are_true_doubles():
    for code in fc.CODES:
        x = fc.frames(code)
        assert x.dtype == np.float64 and x.shape == (fc.FRAMES, fc.rc.columns(code, fc.WEIGHT))
        plain = x[:6]
        assert (plain.astype(np.float32).astype(np.float64) == plain).mean() < 0.02      # (measured: 0.7 %)
        assert np.isinf(x[23]).any() and (np.abs(x[20]) == 5e-324).any() and np.signbit(x[21][x[21] == 0]).any()
        with np.errstate(over="ignore"):
            assert (x[30] == fc.FLOAT_INF_THRESHOLD).any() and np.isinf(x[30].astype(np.float32)).any()
        assert np.isfinite(x[31].astype(np.float32)).all() and (x[31].astype(np.float32) == np.finfo(np.float32).max).any()
        tiny = np.finfo(np.float32).tiny
        assert (np.abs(x[32]) < tiny).all() and (np.abs(x[33]) < tiny).all() and (x[33].astype(np.float32) != 0).any()


def test_frame_24_tells_the_rounding_modes_apart():
    """Every position of frame 24 is the exact midpoint of two adjacent floats, so truncation (the neighbour towards zero)
    and round-half-away (the other one) differ on EVERY position, and round-to-nearest-even -- numpy's conversion, and the
    reference's `as f32` -- agrees with exactly one of them: with truncation where the inner neighbour is the even one,
    with half-away elsewhere.  Both happen on at least a quarter of the positions, so a conversion in either wrong mode
    changes many inputs.  (Nearest-even cannot differ from truncation on every position AND from half-away on some: where
    it differs from one it equals the other.)"""
    for code in fc.CODES:
        x = fc.frames(code)[24]
        even = x.astype(np.float32)
        towards = np.where(np.abs(even.astype(np.float64)) > np.abs(x), np.nextafter(even, np.float32(0.0)), even)
        away = np.nextafter(towards, np.copysign(np.float32(np.inf), towards))
        assert np.array_equal(0.5 * (towards.astype(np.float64) + away.astype(np.float64)), x)      # ties, every one
        assert ((even == towards) != (even == away)).all()
        n = len(x)
        assert (even != towards).sum() >= n // 4 and (even != away).sum() >= n // 4, ((even != towards).sum(), n)


@pytest.mark.parametrize("code", fc.CODES)
def test_reference_premises(oracle, code):
    for name in NAMES:
        bits, its, post = fc.reference(oracle, code, name)           # (a panic of the reference raises here)
        main = its[:fc.MAIN]
        assert (main >= 2).sum() >= 4 and (main < 0).sum() >= 4, (code, name, its.tolist())
        assert not np.isnan(post).any(), (code, name)
        if fc.is_i8(name):
            # an 8-bit decoder of the reference keeps no state for a frame that passes the pre-check: none does here, so
            # every posterior is compared
            assert (its != 0).all(), (code, name)


@pytest.mark.parametrize("code", fc.CODES)
def test_rounding_to_float_first_changes_the_result(oracle, code):
    """f64 rules: on at least 24 of the 32 main frames; 8-bit rules: on frames 28 and 29 (the quantiser's ties + and - one
    f64 ulp, which a float cannot tell from the tie); f32 rules: on none -- `as f32` of an f64 is the same rounding"""
    for name in NAMES:
        changed = _changed(oracle, code, name)
        if fc.is_f64(name):
            assert len([f for f in changed if f < fc.MAIN]) >= 24, (code, name, changed)
        elif fc.is_i8(name):
            assert 28 in changed and 29 in changed, (code, name, changed)
        else:
            assert changed == [], (code, name, changed)
