"""Test infrastructure: a numpy float64 restatement of the STOI / ESTOI definition that csrc/stoi.hip implements (the algorithm of
pystoi.stoi(x, y, fs_sig, extended) as evaluation.py:28-36 calls it; parity unpinned vs pystoi, which is not installed).  No scipy: the
resampler is zero-stuffing plus np.convolve.  x is the clean signal, y the processed one."""
import math

import numpy as np

FS = 10000
N_FRAME = 256
HOP = 128
NFFT = 512
NUMBAND = 15
MINFREQ = 150
N = 30
BETA = -15.0
DYN_RANGE = 40.0
EPS = 2.0 ** -52
TOO_SHORT = 1e-5


def rate(fs):
    g = math.gcd(FS, fs)
    return FS // g, fs // g


def taps(p, q):
    """(g, L): Octave's resample filter, scaled to sum p"""
    fc = 1.0 / (2 * max(p, q))
    L = int(math.ceil((60 - 8) / (28.714 * fc / 10)))
    t = np.arange(-L, L + 1, dtype=np.float64)
    h = np.kaiser(2 * L + 1, 0.1102 * (60 - 8.7)) * 2 * p * fc * np.sinc(2 * fc * t)
    return p * h / h.sum(), L


def n10_of(length, p, q):
    return 0 if length <= 0 else -((-length * p) // q)


def frames_of(n):
    return 0 if n < N_FRAME else (n - N_FRAME) // HOP + 1


def resample(x, p, q):
    """y[n] = sum_m x[m] g[n q - m p + L], n < ceil(len p / q)"""
    x = np.asarray(x, dtype=np.float64)
    if p == q:
        return x.copy()
    n10 = n10_of(len(x), p, q)
    if n10 == 0:
        return np.zeros(0)
    g, L = taps(p, q)
    up = np.zeros(len(x) * p)
    up[::p] = x
    full = np.convolve(up, g)
    return full[np.arange(n10) * q + L]


def window():
    return np.hanning(N_FRAME + 2)[1:-1]


def band_edges():
    f = np.arange(NFFT // 2 + 1) * FS / NFFT
    k = np.arange(NUMBAND, dtype=np.float64)
    lo = [int(np.argmin((f - MINFREQ * 2.0 ** ((2 * b - 1) / 6)) ** 2)) for b in k]
    hi = [int(np.argmin((f - MINFREQ * 2.0 ** ((2 * b + 1) / 6)) ** 2)) for b in k]
    return lo, hi


def frame_energies(x10):
    """e_i in dB of the windowed frames of the (resampled) clean signal"""
    w = window()
    F = frames_of(len(x10))
    fr = np.stack([w * x10[i * HOP:i * HOP + N_FRAME] for i in range(F)]) if F else np.zeros((0, N_FRAME))
    return 20 * np.log10(np.sqrt((fr ** 2).sum(axis=1)) + EPS), fr


def _compact(frames_kept):
    K = len(frames_kept)
    out = np.zeros((K - 1) * HOP + N_FRAME)
    for k in range(K):
        out[k * HOP:k * HOP + N_FRAME] += frames_kept[k]
    return out


def _tob(sig, lo, hi):
    w = window()
    F = frames_of(len(sig))
    fr = np.stack([w * sig[i * HOP:i * HOP + N_FRAME] for i in range(F)])
    spec = np.fft.rfft(fr, n=NFFT, axis=1)
    p = np.abs(spec) ** 2
    return np.stack([np.sqrt(p[:, lo[b]:hi[b]].sum(axis=1)) for b in range(NUMBAND)])       # (15, K)


def stoi_full(x, y, fs, extended=False):
    """-> dict(score, K, X, Y (15, K envelopes), margin (dB), mask (kept per frame), frames)"""
    p, q = rate(fs)
    x10, y10 = resample(x, p, q), resample(y, p, q)
    e, xf = frame_energies(x10)
    F = len(e)
    if F == 0:
        return dict(score=TOO_SHORT, K=0, X=np.zeros((NUMBAND, 0)), Y=np.zeros((NUMBAND, 0)), margin=np.inf, mask=np.zeros(0, bool), frames=0)
    thr = e.max() - DYN_RANGE
    mask = e > thr
    margin = float(np.abs(e - thr).min())
    K = int(mask.sum())
    w = window()
    yf = np.stack([w * y10[i * HOP:i * HOP + N_FRAME] for i in range(F)])
    lo, hi = band_edges()
    X = _tob(_compact(xf[mask]), lo, hi)
    Y = _tob(_compact(yf[mask]), lo, hi)
    assert X.shape == (NUMBAND, K)
    out = dict(K=K, X=X, Y=Y, margin=margin, mask=mask, frames=F)
    if K < N:
        out['score'] = TOO_SHORT
        return out
    J = K - N + 1
    xs = np.stack([X[:, m - N:m] for m in range(N, K + 1)])          # (J, 15, 30)
    ys = np.stack([Y[:, m - N:m] for m in range(N, K + 1)])
    if not extended:
        c = np.linalg.norm(xs, axis=2, keepdims=True) / (np.linalg.norm(ys, axis=2, keepdims=True) + EPS)
        yp = np.minimum(c * ys, xs * (1 + 10 ** (-BETA / 20)))
        yp = yp - yp.mean(axis=2, keepdims=True)
        xc = xs - xs.mean(axis=2, keepdims=True)
        yp = yp / (np.linalg.norm(yp, axis=2, keepdims=True) + EPS)
        xc = xc / (np.linalg.norm(xc, axis=2, keepdims=True) + EPS)
        out['score'] = float((yp * xc).sum() / (J * NUMBAND))
    else:
        def unit(a, axis):
            a = a - a.mean(axis=axis, keepdims=True)
            s = (a ** 2).sum(axis=axis, keepdims=True)
            return a * np.where(s > 0, 1.0 / np.sqrt(np.where(s > 0, s, 1.0)), 0.0)
        xn = unit(unit(xs, 2), 1)
        yn = unit(unit(ys, 2), 1)
        out['score'] = float((xn * yn).sum() / (N * J))
    return out


def stoi(x, y, fs, extended=False):
    return stoi_full(x, y, fs, extended)['score']


# ---- seeded test signals shared by test_stoi_host.py and test_gpu_stoi.py
def speechlike(seed, n, fs, gaps=(), gap_db=-65.0):
    """low-passed noise (one pole: energy in every band) under a 4 Hz envelope, with the stretches `gaps` = [(start, stop), ...] (samples)
    turned down by gap_db, so that silent-frame removal really drops frames"""
    rng = np.random.RandomState(seed)
    white = rng.randn(n + 63)
    a = 0.6
    x = np.convolve(white, (1 - a) * a ** np.arange(64), mode='valid')[:n]
    t = np.arange(n) / fs
    x = x * (0.55 + 0.45 * np.sin(2 * np.pi * 4.0 * t + rng.uniform(0, 2 * np.pi)))
    for g0, g1 in gaps:
        x[g0:g1] *= 10.0 ** (gap_db / 20)
    return 0.1 * x


def add_noise(x, snr_db, seed):
    rng = np.random.RandomState(seed)
    v = rng.randn(len(x))
    v *= np.sqrt((x ** 2).sum() / ((v ** 2).sum() * 10.0 ** (snr_db / 10)))
    return x + v
