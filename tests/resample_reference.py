"""fp64 reference of the windowed-sinc resampler (utils.sinc_resample_bank / aed_resample_sinc), independent of the
product's evaluation: the bank from the closed form per (p, k) in numpy float64 (no torch op order), and a plain fp64 FIR.
Shared by tests/test_resample_cpu.py and tests/test_gpu_resample.py."""
import math

import numpy as np

# the rate pairs of the issue, with the bank shape [n, taps] and width each must give
RATE_PAIRS = [(44100, 16000, (160, 475), 17), (16000, 44100, (441, 174), 7), (48000, 44100, (147, 174), 7),
              (22050, 16000, (320, 459), 9), (48000, 16000, (1, 41), 19), (8000, 16000, (2, 15), 7)]
PAIR_IDS = [f"{a}->{b}" for a, b, _, _ in RATE_PAIRS]


def reduced(orig, new):
    """(o, n, base, width) of a rate pair: reduced rates, base = min(o, n)*0.99, width = ceil(6*o/base)."""
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * 0.99
    return o, n, base, math.ceil(6 * o / base)


def bank_fp64(orig, new):
    """K[p, k] = sinc(pi t) * cos^2(pi t / 12) * base/o,  t = clamp((-p/n + (k - width)/o) * base, -6, 6),  in float64."""
    o, n, base, width = reduced(orig, new)
    p = np.arange(n, dtype=np.float64)[:, None]
    k = np.arange(2 * width + o, dtype=np.float64)[None, :]
    t = np.clip((-p / n + (k - width) / o) * base, -6.0, 6.0)
    return np.sinc(t) * np.cos(np.pi * t / 12.0) ** 2 * (base / o)           # np.sinc(t) = sin(pi t)/(pi t), 1 at 0


def out_length(orig, new, length):
    o, n, _, _ = reduced(orig, new)
    return -(-n * length // o)


def fir_fp64(x, bank, o, width, with_bound=False):
    """y[c, q*n + p] = sum_k bank[p, k] * x[c, q*o + k - width] in float64, x = 0 outside [0, L), cut to ceil(n*L/o).
    `with_bound`: also sum_k |bank||x| per output, the scale of the fp32 dot-product bound."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    bank = np.asarray(bank, dtype=np.float64)
    n, taps = bank.shape
    assert taps == 2 * width + o
    C, L = x.shape
    out_len = -(-n * L // o)
    frames = -(-out_len // n)
    xp = np.zeros((C, (frames - 1) * o + taps))
    m = min(L, xp.shape[1] - width)
    xp[:, width:width + m] = x[:, :m]
    win = np.lib.stride_tricks.sliding_window_view(xp, taps, axis=1)[:, ::o][:, :frames]       # [C, frames, taps]
    y = np.einsum("cqk,pk->cqp", win, bank).reshape(C, -1)[:, :out_len]
    if not with_bound:
        return y
    mag = np.einsum("cqk,pk->cqp", np.abs(win), np.abs(bank)).reshape(C, -1)[:, :out_len]
    return y, mag


def gamma(taps):
    """The standard bound of an fp32 dot product of `taps` terms in any summation order: |fl(s) - s| <= gamma * sum|a||b|."""
    u = 2.0 ** -24
    return taps * u / (1.0 - taps * u)


def tone_plus_noise(sr, seconds=1.0, seed=0):
    """A 440 Hz tone plus noise, peak about 0.6."""
    rng = np.random.default_rng(seed)
    n = int(sr * seconds)
    return (0.5 * np.sin(2 * np.pi * 440.0 * np.arange(n) / sr) + 0.03 * rng.standard_normal(n)).astype(np.float32)
