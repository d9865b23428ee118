"""Constellations and the restatement chain shared by tests/test_modulator_gpu.py and tests/test_sim_constellation_gpu.py
-- TEST INFRASTRUCTURE ONLY.  Every table has unit mean energy (the simulator asks for it); the 2-, 16- and 32-point tables
have points of unequal energy, so their demapper needs the energy term."""
import numpy as np

import channel_restatement as cr
import demod_restatement as dr


def _unit(pts):
    return pts / np.sqrt(np.mean(pts.real * pts.real + pts.imag * pts.imag))


def two_points():
    return _unit(np.array([0.6 + 0.2j, -1.1 - 0.3j]))


def rings16():
    k = np.arange(8)
    return _unit(np.concatenate([np.exp(2j * np.pi * k / 8), 2.7 * np.exp(2j * np.pi * (k + 0.5) / 8)]))


def rings32():
    pts = np.concatenate([1.0 * np.exp(2j * np.pi * (np.arange(4) + 0.5) / 4), 2.0 * np.exp(2j * np.pi * np.arange(12) / 12),
                          3.3 * np.exp(2j * np.pi * (np.arange(16) + 0.25) / 16)])
    return _unit(pts[np.random.default_rng(32).permutation(32)])      # labels: a fixed random permutation


# name -> (points, energy term)
TABLES = {
    "two": (two_points(), True),
    "QPSK": (dr.QPSK, False),
    "8PSK": (dr.PSK8, False),
    "rings16": (rings16(), True),
    "rings32": (rings32(), True),
}


def bits_of(name):
    return len(TABLES[name][0]).bit_length() - 1


def make_demodulator(lt, name, device=0):
    pts, energy = TABLES[name]
    if name in ("QPSK", "8PSK"):
        return lt.Demodulator(name, device=device)
    return lt.Demodulator(pts, energy_term=energy, device=device)


def chain_llrs(tx_rows, name, max_log, interleaving, sigma, seed, first_frame):
    """the defined result of the simulator's generator: modulate -> AWGN -> demap, all in f64, each LLR rounded once"""
    pts, energy = TABLES[name]
    rx = cr.awgn(cr.modulate(tx_rows, pts, interleaving), sigma, seed, first_frame)
    return dr.demodulate(rx, sigma, pts, energy, max_log, interleaving).astype(np.float32)
