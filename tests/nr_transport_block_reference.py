"""A numpy restatement of the 5G NR transport block processing around the LDPC code, literally as TS 38.212 states it:
bit-serial long division for the CRCs (5.1), the loops of code block segmentation (5.2.2), the E_r of 5.4.2.1 and the
concatenation loop of 5.5.  Code block rows are block-major, as in include/ldpc_toolbox.h (PART 7): row r * batch + b is
block r of transport block b.  It shares nothing with the library: no tables of powers, no partial remainders."""
import numpy as np

# generator polynomials with their leading term, and their degree (5.1)
CRC24A = (0x1864CFB, 24)
CRC24B = (0x1800063, 24)
CRC16 = (0x11021, 16)

LIFTING_SIZES = sorted(a << j for a in (2, 3, 5, 7, 9, 11, 13, 15) for j in range(8) if a << j <= 384)   # Table 5.3.2-1
MAX_A = 1277992


def remainder(bits, poly) -> int:
    """the remainder of bits[0] x^(len-1) + ... + bits[len-1] divided by the polynomial, one bit at a time"""
    g, length = poly
    top = 1 << length
    s = 0
    for u in np.ascontiguousarray(bits, dtype=np.uint8).tobytes():
        s = (s << 1) | u
        if s & top:
            s ^= g
    return s


def parity_bits(bits, poly):
    """p_0 .. p_(L-1) of 5.1: the remainder of bits(x) x^L, p_0 the coefficient of the highest power"""
    length = poly[1]
    s = remainder(np.concatenate([np.asarray(bits, dtype=np.uint8), np.zeros(length, dtype=np.uint8)]), poly)
    return np.array([(s >> (length - 1 - i)) & 1 for i in range(length)], dtype=np.uint8)


def base_graph(a: int, rate: float) -> int:
    """7.2.2"""
    if a <= 292 or (a <= 3824 and rate <= 0.67) or rate <= 0.25:
        return 2
    return 1


class Config:
    """raises ValueError for what the library refuses"""

    def __init__(self, bg: int, a: int):
        if bg not in (1, 2) or not 1 <= a <= MAX_A:
            raise ValueError("no configuration")
        self.bg, self.a = bg, a
        self.tb_poly = CRC24A if a > 3824 else CRC16
        self.l_tb = self.tb_poly[1]
        self.b = a + self.l_tb
        kcb = 8448 if bg == 1 else 3840
        if self.b <= kcb:
            self.l_cb, self.c, b_prime = 0, 1, self.b
        else:
            self.l_cb = 24
            self.c = -(-self.b // (kcb - 24))
            b_prime = self.b + self.c * 24
        if b_prime % self.c != 0:
            raise ValueError("C does not divide B'")
        self.k_prime = b_prime // self.c
        if bg == 1:
            self.kb = 22
        elif self.b > 640:
            self.kb = 10
        elif self.b > 560:
            self.kb = 9
        elif self.b > 192:
            self.kb = 8
        else:
            self.kb = 6
        self.zc = min(z for z in LIFTING_SIZES if self.kb * z >= self.k_prime)
        self.k = (22 if bg == 1 else 10) * self.zc
        self.fillers = self.k - self.k_prime
        self.n = (68 if bg == 1 else 52) * self.zc

    @property
    def spec(self):
        return f"nr5g-tb:{self.bg}:{self.a}"

    def row(self):
        return (self.c, self.k_prime, self.kb, self.zc, self.k, self.fillers)

    def segment(self, payload):
        """payload [B][A] bytes (1 = one, anything else zero) -> rows [C * B][K] bytes 0 / 1 (filler bits as zeros)"""
        payload = (np.asarray(payload) == 1).astype(np.uint8)
        batch = payload.shape[0]
        rows = np.zeros((self.c * batch, self.k), dtype=np.uint8)
        take = self.k_prime - self.l_cb
        for t in range(batch):
            seq = np.concatenate([payload[t], parity_bits(payload[t], self.tb_poly)])      # b_0 .. b_(B-1)
            s = 0
            for r in range(self.c):
                block = rows[r * batch + t]
                block[:take] = seq[s:s + take]
                s += take
                if self.c > 1:
                    block[take:self.k_prime] = parity_bits(block[:take], CRC24B)
            assert s == self.b
        return rows

    def desegment(self, rows):
        """rows [C * B][K] -> payload [B][A], tb_ok [B], cb_ok [B][C]"""
        rows = (np.asarray(rows) == 1).astype(np.uint8)
        batch = rows.shape[0] // self.c
        payload = np.zeros((batch, self.a), dtype=np.uint8)
        tb_ok = np.zeros(batch, dtype=np.uint8)
        cb_ok = np.zeros((batch, self.c), dtype=np.uint8)
        take = self.k_prime - self.l_cb
        for t in range(batch):
            seq = np.concatenate([rows[r * batch + t, :take] for r in range(self.c)])
            payload[t] = seq[:self.a]
            tb_ok[t] = remainder(seq, self.tb_poly) == 0
            for r in range(self.c):
                cb_ok[t, r] = remainder(rows[r * batch + t, :self.k_prime], CRC24B) == 0 if self.c > 1 else tb_ok[t]
        return payload, tb_ok, cb_ok

    def block_lengths(self, g: int, q: int):
        """E_r, r < C (5.4.2.1 with C' = C)"""
        assert g % q == 0 and g // q >= self.c
        e = []
        for r in range(self.c):
            if r <= self.c - (g // q) % self.c - 1:
                e.append(q * (g // (q * self.c)))
            else:
                e.append(q * -(-g // (q * self.c)))
        return e

    def pack(self, blocks):
        """blocks[r]: [B][E_r] -> the flat packed array: the rows block-major, block 0's first"""
        return np.concatenate([np.asarray(x).reshape(-1) for x in blocks])

    def unpack(self, packed, batch: int, g: int, q: int):
        e, out, at = self.block_lengths(g, q), [], 0
        for r in range(self.c):
            out.append(np.asarray(packed)[at:at + batch * e[r]].reshape(batch, e[r]))
            at += batch * e[r]
        return out

    def concatenate(self, packed, batch: int, g: int, q: int):
        """5.5: the f_rk of block 0, then of block 1, ... -> [B][G] bytes 0 / 1"""
        blocks = self.unpack(packed, batch, g, q)
        out = np.zeros((batch, g), dtype=np.uint8)
        for t in range(batch):
            k = 0
            for r in range(self.c):
                e_r = blocks[r].shape[1]
                out[t, k:k + e_r] = blocks[r][t] == 1
                k += e_r
        return out

    def split(self, rx, q: int):
        """[B][G] values -> the flat packed array of the same type"""
        rx = np.asarray(rx)
        batch, g = rx.shape
        e = self.block_lengths(g, q)
        starts = np.concatenate([[0], np.cumsum(e)])
        return self.pack([rx[:, starts[r]:starts[r + 1]] for r in range(self.c)])
