"""A numpy restatement of 5G NR rate matching and rate recovery for one LDPC code block, literally as TS 38.212 5.4.2 and
include/ldpc_toolbox.h (PART 6) state it: a NULL-marked circular buffer, the `while` loop of bit selection and the double
loop of the bit interleaver.  Recovery is a per-column left-to-right sum in the array's dtype.  It shares nothing with the
library: no closed forms, no ranks."""
import numpy as np

NULL = -1
_K0_A = {1: (0, 17, 33, 56), 2: (0, 13, 25, 43)}       # TS 38.212 Table 5.4.2.1-2


class Config:
    def __init__(self, bg: int, zc: int, fillers: int = 0, ncb=None):
        assert bg in (1, 2)
        self.bg, self.zc, self.fillers = bg, zc, fillers
        self.n = (68 if bg == 1 else 52) * zc
        self.k = (22 if bg == 1 else 10) * zc
        self.N = self.n - 2 * zc
        self.ncb = self.N if ncb is None else ncb
        assert 0 <= fillers <= self.k - 2 * zc and 1 <= self.ncb <= self.N
        # the buffer: entry d holds the codeword column it carries, or NULL
        self.buffer = np.arange(2 * zc, self.n, dtype=np.int64)
        self.buffer[self.k - 2 * zc - fillers:self.k - 2 * zc] = NULL
        self.L = int((self.buffer[:self.ncb] != NULL).sum())
        assert self.L >= 1

    @property
    def spec(self):
        return f"nr5g:{self.bg}:{self.zc}:{self.fillers}:{self.ncb}"

    def k0(self, rv: int) -> int:
        return (_K0_A[self.bg][rv] * self.ncb // self.N) * self.zc

    def selection(self, e: int, rv: int):
        """e[k], k < E: the codeword column of selection index k"""
        out = np.zeros(e, dtype=np.int64)
        k0 = self.k0(rv)
        k = j = 0
        while k < e:
            d = (k0 + j) % self.ncb
            if self.buffer[d] != NULL:
                out[k] = self.buffer[d]
                k += 1
            j += 1
        return out

    def transmitted(self, e: int, rv: int, qm: int):
        """f[p], p < E: the codeword column at transmitted position p"""
        assert 1 <= qm <= 8 and e % qm == 0
        sel = self.selection(e, rv)
        f = np.zeros(e, dtype=np.int64)
        for i in range(qm):
            for q in range(e // qm):
                f[i + q * qm] = sel[i * (e // qm) + q]
        return f

    def match(self, codewords, e: int, rv: int, qm: int):
        """codewords [B][n] bytes (1 = one, anything else zero) -> [B][E] bytes 0 / 1"""
        return (np.asarray(codewords)[:, self.transmitted(e, rv, qm)] == 1).astype(np.uint8)

    def recover(self, rx, rv: int, qm: int, filler_llr, old=None):
        """rx [B][E] -> [B][n] in rx's dtype; old: the soft buffer to combine into (a new array is returned)"""
        rx = np.asarray(rx)
        B, e = rx.shape
        dtype = rx.dtype.type
        sel = self.selection(e, rv)
        # where selection index k lies after the interleaver
        pos = np.zeros(e, dtype=np.int64)
        for i in range(qm):
            for q in range(e // qm):
                pos[i * (e // qm) + q] = i + q * qm
        out = np.zeros((B, self.n), dtype=rx.dtype) if old is None else np.array(old, dtype=rx.dtype, copy=True)
        filler_columns = range(self.k - self.fillers, self.k)
        carried_by = [[] for _ in range(self.n)]                      # per column, ascending selection index
        for k in range(e):
            carried_by[sel[k]].append(k)
        with np.errstate(invalid="ignore", over="ignore"):
            for c in range(self.n):
                if c in filler_columns:
                    out[:, c] = dtype(filler_llr)
                    continue
                carriers = carried_by[c]
                if not carriers:
                    continue
                s = rx[:, pos[carriers[0]]].copy()
                for k in carriers[1:]:
                    s = (s + rx[:, pos[k]]).astype(rx.dtype)
                out[:, c] = s if old is None else (out[:, c] + s).astype(rx.dtype)
        return out

    def repeats(self, e: int, rv: int):
        """how many selection indices carry each column"""
        return np.bincount(self.selection(e, rv), minlength=self.n)
