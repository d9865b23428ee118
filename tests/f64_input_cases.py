"""Codes, frames and references of the f64-input tests (test_f64_input_host.py, test_f64_input_gpu.py): channel LLRs that are
TRUE doubles -- computed and kept in f64; 0.7 % of the plain AWGN values are representable as a float -- for every decode
entry that takes f64.  The reference defines its input conversions on f64 (c_api/decoder.rs widens f32 to f64; the arithmetic narrows
once, by `as f32` or by its 8-bit quantiser), so a kernel that narrows early -- quantises an i8 rule from a float, truncates
instead of rounding to nearest even, flushes a float subnormal -- is wrong exactly on such values.

Codes (row_weight_cases, with that module's noise levels):
  "regular"    regular_code(8):   n = 96, 52 rows, 320 edges, sigma 0.76
  "staircase"  staircase_code(8): n = 328, 120 rows, 869 edges, sigma 0.68 -- degree-1/2 variables: row records, L-free path

Frames: the all-zero codeword, llr = 2 (1 + sigma z) / sigma^2 in f64, seeded; frame by frame

   0-5    plain f64 AWGN
   6-11   every position scaled by 2^e, e uniform in -80..8
  12-15   the whole frame scaled by 2^-60, 2^-40, 2^-28, 2^5
  16-19   5 % of the positions replaced by 1e300, 1.7e308, 1e39, 700 (one value per frame)
  20-23   5 % of the positions replaced by 5e-324, -0.0, -3e-310, +inf
  24      every position the exact midpoint of the two floats around it: a tie of the conversion to float
  25, 26  those midpoints + and - one f64 ulp
  27      (floor(8 llr) + 0.5) / 8: a tie of the 8-bit quantiser (round(8 llr), saturating)
  28, 29  those ties + and - one f64 ulp
  30      5 % of the positions at 3.4028235677973366e38, the smallest double that rounds to float infinity
  31      5 % of the positions at the double just below it (rounds to FLT_MAX)
  32, 33  the whole frame scaled by 2^-140 and 2^-150: the float-subnormal range

"5 % of the positions" are drawn so that no check row holds two of them.  Drawn freely, two infinite inputs (in f32 also
1e300, 1.7e308, 1e39 and the threshold of frame 30) met in one row, the row formed inf - inf, and the reference's A-Min*
rule panics on a NaN message: [HL]Aminstarf32 on frames 17, 18, 23 and 30, [HL]Aminstarf64 on frame 23 of the staircase
code.  With one such value per row at most, no name panics on any frame (test_f64_input_host.py).

The reference is oracle_binding.Decoder(graph, name).decode(frame, 20), the oracle's one-codeword f64 entry, frame by frame.
Everything is computed once and handed out read-only."""
import functools

import numpy as np

import row_weight_cases as rc

CODES = ("regular", "staircase")
WEIGHT = 8
FRAMES = 34
MAIN = 32                  # the frames the premises of test_f64_input_host.py count over
ITERATIONS = 20
SEED = 6464
FLOAT_INF_THRESHOLD = 3.4028235677973366e38     # FLT_MAX + half an ulp of FLT_MAX, exactly: a tie that rounds to the even +inf
SCALAR_FRAMES = (0, 6, 16, 24, 28)


def alist(code):
    return rc.code(code, WEIGHT)[1]


def _midpoints(llr):
    """the midpoint of the two adjacent floats around each value (exact in f64), and those two floats"""
    f = llr.astype(np.float32)
    below = f.astype(np.float64) <= llr
    lo = np.where(below, f, np.nextafter(f, np.float32(-np.inf)))
    hi = np.where(below, np.nextafter(f, np.float32(np.inf)), f)
    return 0.5 * (lo.astype(np.float64) + hi.astype(np.float64))


def _some(rng, code):
    """5 % of the positions (three at least), no two of them in one check row: a row that met two infinite inputs would
    form inf - inf, and the reference's A-Min* rule panics on a NaN message (arithmetic.rs:942-999)"""
    rows = rc.code(code, WEIGHT)[0]
    n = rc.columns(code, WEIGHT)
    count = max(3, round(0.05 * n))
    chosen, blocked = [], set()
    for v in rng.permutation(n).tolist():
        if v not in blocked:
            chosen.append(v)
            for r in rows:
                if v in r:
                    blocked.update(r)
        if len(chosen) == count:
            break
    assert len(chosen) == count
    return np.array(chosen)


@functools.lru_cache(maxsize=None)
def frames(code):
    """[FRAMES][n] f64"""
    n = rc.columns(code, WEIGHT)
    sigma = rc.SIGMA[code][WEIGHT]
    rng = np.random.default_rng([SEED, CODES.index(code)])
    out = 2.0 * (1.0 + sigma * rng.standard_normal((FRAMES, n))) / sigma ** 2
    out[6:12] *= np.exp2(rng.integers(-80, 9, size=(6, n)).astype(np.float64))
    for f, e in zip(range(12, 16), (-60, -40, -28, 5)):
        out[f] *= 2.0 ** e
    for f, v in zip(range(16, 24), (1e300, 1.7e308, 1e39, 700.0, 5e-324, -0.0, -3e-310, np.inf)):
        out[f, _some(rng, code)] = v
    out[24] = _midpoints(out[24])
    out[25] = np.nextafter(out[24], np.inf)
    out[26] = np.nextafter(out[24], -np.inf)
    out[27] = (np.floor(8.0 * out[27]) + 0.5) / 8.0
    out[28] = np.nextafter(out[27], np.inf)
    out[29] = np.nextafter(out[27], -np.inf)
    out[30, _some(rng, code)] = FLOAT_INF_THRESHOLD
    out[31, _some(rng, code)] = np.nextafter(FLOAT_INF_THRESHOLD, 0.0)
    out[32] *= 2.0 ** -140
    out[33] *= 2.0 ** -150
    out.setflags(write=False)
    return out


def is_f64(name):
    return name.endswith("f64")


def is_i8(name):
    return "i8" in name


def decode_reference(oracle, code, name, llrs, iterations=ITERATIONS, panics=None):
    """(bits [B][n] u8, iterations [B] i32 with -1 = failed, posterior [B][n] f64) of the oracle's one-codeword f64 entry,
    one decoder through the frames in order.  A frame on which the reference would panic raises -- or, given a list
    `panics`, is noted there and left zero (its iteration count -2), and a fresh decoder takes the next frame."""
    graph = oracle.Graph(alist(code))
    dec = oracle.Decoder(graph, name)
    bits = np.zeros(llrs.shape, dtype=np.uint8)
    its = np.zeros(len(llrs), dtype=np.int32)
    post = np.zeros(llrs.shape, dtype=np.float64)
    for f, frame in enumerate(llrs):
        try:
            ok, bits[f], it, post[f] = dec.decode(frame, iterations)
        except RuntimeError:
            if panics is None:
                raise
            panics.append(f)
            its[f] = -2
            dec = oracle.Decoder(graph, name)
            continue
        its[f] = it if ok else -1
    return bits, its, post


@functools.lru_cache(maxsize=None)
def reference(oracle, code, name, iterations=ITERATIONS):
    """of all frames of `code`, read-only"""
    want = decode_reference(oracle, code, name, frames(code), iterations)
    for a in want:
        a.setflags(write=False)
    return want
