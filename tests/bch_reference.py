"""A numpy / pure-Python restatement of the binary BCH codes of include/ldpc_toolbox.h, PART 5.  It shares nothing with
the library: the field by repeated multiplication with x, g as a product over cyclotomic cosets, the encoder by
polynomial division on Python integers, a syndrome-table decoder that implements the bounded-distance definition
literally (small codes), and an algebraic decoder (full Berlekamp-Massey with inversions over all 2t syndromes, then
the locator evaluated at every position) for the DVB-S2 sizes.

Polynomials over GF(2) are Python integers, bit i = coefficient of x^i.  A row of n bytes holds one bit per byte, byte i
the coefficient of x^(n-1-i); on input a byte equal to 1 is a one and anything else a zero."""
import itertools

import numpy as np

DVBS2 = {  # name: (n, k, t), EN 302 307-1 Tables 5a / 5b
    "R1_4": (16200, 16008, 12), "R1_3": (21600, 21408, 12), "R2_5": (25920, 25728, 12), "R1_2": (32400, 32208, 12),
    "R3_5": (38880, 38688, 12), "R2_3": (43200, 43040, 10), "R3_4": (48600, 48408, 12), "R4_5": (51840, 51648, 12),
    "R5_6": (54000, 53840, 10), "R8_9": (57600, 57472, 8), "R9_10": (58320, 58192, 8),
    "R1_4short": (3240, 3072, 12), "R1_3short": (5400, 5232, 12), "R2_5short": (6480, 6312, 12),
    "R1_2short": (7200, 7032, 12), "R3_5short": (9720, 9552, 12), "R2_3short": (10800, 10632, 12),
    "R3_4short": (11880, 11712, 12), "R4_5short": (12600, 12432, 12), "R5_6short": (13320, 13152, 12),
    "R8_9short": (14400, 14232, 12),
}
P_NORMAL, P_SHORT = 0x1002D, 0x402B


class Field:
    def __init__(self, m, poly):
        self.m, self.poly, self.order = m, poly, (1 << m) - 1
        self.exp = np.zeros(self.order, dtype=np.int64)
        self.log = np.full(1 << m, -1, dtype=np.int64)
        v = 1
        for e in range(self.order):
            assert self.log[v] < 0, "x is not primitive"
            self.exp[e], self.log[v] = v, e
            v <<= 1
            if v >> m:
                v ^= poly
        assert v == 1, "x is not primitive"

    def mul(self, a, b):
        return 0 if a == 0 or b == 0 else int(self.exp[(self.log[a] + self.log[b]) % self.order])

    def inv(self, a):
        return int(self.exp[(self.order - self.log[a]) % self.order])

    def minimal_polynomial(self, e):
        """of alpha^e: the product of (x + alpha^c) over the cyclotomic coset of e"""
        coset, c = [], e % self.order
        while c not in coset:
            coset.append(c)
            c = 2 * c % self.order
        p = [1]
        for c in coset:
            root, nxt = int(self.exp[c]), [0] * (len(p) + 1)
            for i, a in enumerate(p):
                nxt[i + 1] ^= a
                nxt[i] ^= self.mul(a, root)
            p = nxt
        assert all(a in (0, 1) for a in p)
        return sum(a << i for i, a in enumerate(p))


def poly_mul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a <<= 1
        b >>= 1
    return r


def poly_mod(a, g):
    dg = g.bit_length() - 1
    while a.bit_length() - 1 >= dg:
        a ^= g << (a.bit_length() - 1 - dg)
    return a


_FIELDS = {}


def field(m, poly):
    """the field of (m, P), built once"""
    if (m, poly) not in _FIELDS:
        _FIELDS[m, poly] = Field(m, poly)
    return _FIELDS[m, poly]


class Code:
    def __init__(self, m, poly, t, n):
        self.field = field(m, poly)
        self.m, self.t, self.n = m, t, n
        self.minimal = []
        for j in range(t):
            mp = self.field.minimal_polynomial(2 * j + 1)
            if mp not in self.minimal:
                self.minimal.append(mp)
        g = 1
        for mp in self.minimal:
            g = poly_mul(g, mp)
        self.g = g
        self.parity = g.bit_length() - 1
        self.k = n - self.parity
        assert n <= self.field.order and self.k >= 1
        self._table = None
        self._bytes = None

    @classmethod
    def from_spec(cls, spec):
        if spec.startswith("dvbs2:"):
            name = spec[6:]
            n, _, t = DVBS2[name]
            return cls(14, P_SHORT, t, n) if name.endswith("short") else cls(16, P_NORMAL, t, n)
        _, m, p, t, n = spec.split(":")
        return cls(int(m), int(p, 16), int(t), int(n))

    # ---- rows <-> integers ------------------------------------------------------------------------------------------
    @staticmethod
    def to_int(row):
        bits = (np.asarray(row, dtype=np.uint8) == 1).astype(np.uint8)
        pad = (-len(bits)) % 8
        return int.from_bytes(np.packbits(np.concatenate([np.zeros(pad, np.uint8), bits])).tobytes(), "big")

    @staticmethod
    def to_row(value, length):
        raw = np.frombuffer(value.to_bytes((length + 7) // 8, "big"), dtype=np.uint8)
        return np.unpackbits(raw)[-length:].copy() if length else np.zeros(0, np.uint8)

    def remainder_shifted(self, value):
        """(value * x^parity) mod g -- eight bits of the value at a time when g has at least eight"""
        if self.parity < 8 or value.bit_length() < 256:
            return poly_mod(value << self.parity, self.g)
        if self._bytes is None:
            self._bytes = [poly_mod(b << self.parity, self.g) for b in range(256)]
        mask, r = (1 << self.parity) - 1, 0
        for byte in value.to_bytes((value.bit_length() + 7) // 8, "big"):
            r = ((r << 8) & mask) ^ self._bytes[(r >> (self.parity - 8)) ^ byte]
        return r

    # ---- encoder ----------------------------------------------------------------------------------------------------
    def encode(self, msgs):
        msgs = np.asarray(msgs, dtype=np.uint8)
        out = np.zeros((len(msgs), self.n), dtype=np.uint8)
        for f, row in enumerate(msgs):
            v = self.to_int(row)
            out[f] = self.to_row((v << self.parity) | self.remainder_shifted(v), self.n)
        return out

    def is_codeword(self, row):
        return self.remainder_shifted(self.to_int(row)) == 0  # x is invertible mod g

    # ---- the definition, literally (small codes) -----------------------------------------------------------------------
    def table(self):
        """remainder mod g of every pattern of weight <= t -> the pattern"""
        if self._table is None:
            single = [poly_mod(1 << p, self.g) for p in range(self.n)]
            tab = {0: 0}
            for w in range(1, self.t + 1):
                for pos in itertools.combinations(range(self.n), w):
                    r = pat = 0
                    for p in pos:
                        r ^= single[p]
                        pat |= 1 << p
                    assert r not in tab, "two patterns of weight <= t share a syndrome"
                    tab[r] = pat
            self._table = tab
        return self._table

    def decode_table(self, rows):
        rows = (np.asarray(rows, dtype=np.uint8) == 1).astype(np.uint8)
        out, errors = rows.copy(), np.full(len(rows), -1, dtype=np.int32)
        tab = self.table()
        for f, row in enumerate(rows):
            v = self.to_int(row)
            pat = tab.get(poly_mod(v, self.g))
            if pat is not None:
                out[f] = self.to_row(v ^ pat, self.n)
                errors[f] = bin(pat).count("1")
        return out, errors

    # ---- algebraic decoder ---------------------------------------------------------------------------------------------
    def syndromes(self, row):
        """S_1 .. S_2t of a 0/1 row"""
        F = self.field
        powers = (self.n - 1 - np.flatnonzero(row)).astype(np.int64)
        return [int(np.bitwise_xor.reduce(F.exp[(j * powers) % F.order])) if len(powers) else 0 for j in range(1, 2 * self.t + 1)]

    def decode_one(self, row):
        F, t, n = self.field, self.t, self.n
        S = self.syndromes(row)
        if not any(S):
            return row.copy(), 0
        # Massey's algorithm over all 2t syndromes
        C, B, L, shift, b = [1], [1], 0, 1, 1
        for i in range(2 * t):
            d = S[i]
            for j in range(1, L + 1):
                if j < len(C):
                    d ^= F.mul(C[j], S[i - j])
            if d == 0:
                shift += 1
                continue
            T = list(C)
            coef = F.mul(d, F.inv(b))
            C = C + [0] * (len(B) + shift - len(C))
            for j, a in enumerate(B):
                C[j + shift] ^= F.mul(coef, a)
            if 2 * L <= i:
                L, B, b, shift = i + 1 - L, T, d, 1
            else:
                shift += 1
        if L > t:
            return row.copy(), -1
        # roots among the n positions of the shortened word: lambda(alpha^-p) for p in [0, n)
        p = np.arange(n, dtype=np.int64)
        value = np.zeros(n, dtype=np.int64)
        for j, a in enumerate(C):
            if a:
                value ^= F.exp[(int(F.log[a]) - j * p) % F.order]
        roots = np.flatnonzero(value == 0)
        if len(roots) != L:
            return row.copy(), -1
        out = row.copy()
        out[n - 1 - roots] ^= 1
        return out, L

    def decode(self, rows):
        rows = (np.asarray(rows, dtype=np.uint8) == 1).astype(np.uint8)
        out, errors = rows.copy(), np.zeros(len(rows), dtype=np.int32)
        for f, row in enumerate(rows):
            out[f], errors[f] = self.decode_one(row)
        return out, errors


def patterns(n, weights):
    """every error pattern of the given weights on n positions, as [count][n] uint8"""
    rows = []
    for w in weights:
        for pos in itertools.combinations(range(n), w):
            r = np.zeros(n, dtype=np.uint8)
            r[list(pos)] = 1
            rows.append(r)
    return np.array(rows, dtype=np.uint8)
