"""What the NR link tests share, made on the CPU from the restatements of TS 38.212 / 38.211 alone: the symbols of a
transmission (segmentation, the scalar encoder, rate matching, concatenation, scrambling and mapping) and a seeded noise.
The GPU tests hand these symbols to the link handle and to the chain of stage handles alike, so the case -- and which of
its code blocks decode -- does not depend on the code under test."""
import functools

import numpy as np

import ldpc_toolbox_amd as lt
import nr_qam_reference as nq
import nr_rate_match_reference as rr
import nr_transport_block_reference as tr
from ldpc_toolbox_amd import simulation as sim


def parse(spec):
    """"nr5g-link:BG:A:G:QM" -> (bg, a, g, qm)"""
    fields = spec.split(":")
    assert fields[0] == "nr5g-link" and len(fields) == 5
    return tuple(int(x) for x in fields[1:])


def sigma_of(spec, ebn0_db):
    bg, a, g, qm = parse(spec)
    return sim.noise_sigma(a / g, ebn0_db, qm)


@functools.lru_cache(maxsize=None)
def codewords(spec, batch, payload_seed):
    """(payload [batch][A], codewords [C * batch][n] block-major), read-only"""
    bg, a, g, qm = parse(spec)
    ref = tr.Config(bg, a)
    payload = np.random.default_rng(payload_seed).integers(0, 2, (batch, a), dtype=np.uint8)
    enc = lt.Encoder(lt.code_alist(f"nr5g:{bg}:{ref.zc}"))
    cws = np.stack([enc.encode(row, ref.n) for row in ref.segment(payload)])
    payload.setflags(write=False)
    cws.setflags(write=False)
    return payload, cws


@functools.lru_cache(maxsize=None)
def transmission(spec, batch, payload_seed, rv, c_init=-1):
    """symbols [batch][G / QM] complex64 of the restatements, read-only"""
    bg, a, g, qm = parse(spec)
    ref = tr.Config(bg, a)
    rm = rr.Config(bg, ref.zc, ref.fillers)
    payload, cws = codewords(spec, batch, payload_seed)
    e = ref.block_lengths(g, qm)
    packed = ref.pack([rm.match(cws[r * batch:(r + 1) * batch], e[r], rv, qm) for r in range(ref.c)])
    symbols = nq.modulate(ref.concatenate(packed, batch, g, qm), qm, c_init, real=np.float32)
    symbols.setflags(write=False)
    return symbols


def received(spec, batch, payload_seed, rv, ebn0_db, noise_seed, c_init=-1):
    """the transmission behind an AWGN channel: complex64, each coordinate symbol + float32(sigma * normal)"""
    symbols = transmission(spec, batch, payload_seed, rv, c_init)
    rng = np.random.default_rng(noise_seed)
    noise = (sigma_of(spec, ebn0_db) * rng.standard_normal(symbols.shape + (2,))).astype(np.float32)
    out = symbols.copy()
    out.real += noise[..., 0]
    out.imag += noise[..., 1]
    return out
