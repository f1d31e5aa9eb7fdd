"""CPU: the specification of the STOI / ESTOI gradient, pinned before any kernel is compared with it (as tests/test_decode_grad_host.py does for
the decode).  Parity unpinned vs asteroid / torch_stoi, which are not installed.

(a) tests/stoi_grad_ref.py, the differentiable torch float64 restatement, scores what tests/stoi_ref.py scores (1e-12) and its autograd
    gradient matches central differences along seeded directions (1e-6 relative);
(b) the hand-written adjoints that csrc/stoi_bwd.hip implements -- resampler adjoint, compaction / double-window gather, one-sided DFT adjoint,
    band rule -- written out in numpy here, agree with autograd to 1e-9 of the maximum, and the linear part satisfies the adjoint identity to
    1e-12;
(c) the gradient is exactly 0 past the length and for fewer than 30 kept frames;
(d) the host surface: objective.stoi / estoi exist, ask the training step for the waveform, refuse host tensors; se_stoi_grad_f32 refuses a null
    plan and an undersized workspace before it touches a device."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import stoi_ref as R      # noqa: E402
import stoi_grad_ref as G      # noqa: E402

TOL = 1e-9


def _relmax(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def _pair(seed, n, fs, gaps, snr=5.0):
    x = R.speechlike(seed, n, fs, gaps)
    return x, R.add_noise(x, snr, 100 + seed)


# ---- (a)
@pytest.mark.parametrize('fs,n,gaps', [(16000, 12000, [(4000, 6000)]), (10000, 8000, [(2000, 3200)])])
@pytest.mark.parametrize('extended', [False, True])
def test_restatement_scores_what_stoi_ref_scores(fs, n, gaps, extended):
    x, y = _pair(3, n, fs, gaps)
    r = G.stoi_full(x, torch.from_numpy(y), fs, extended)
    ref = R.stoi_full(x, y, fs, extended)
    assert r['K'] == ref['K'] >= 30 and r['K'] < ref['frames']          # frames really are dropped
    assert abs(float(r['score']) - ref['score']) < 1e-12
    if not extended:
        assert 0 <= r['clipped'] < 1 and r['clip_margin'] > 0


@pytest.mark.parametrize('fs,n,gaps', [(16000, 10000, [(3000, 4500)]), (10000, 6400, [(1500, 2500)])])
@pytest.mark.parametrize('extended', [False, True])
def test_autograd_matches_central_differences(fs, n, gaps, extended):
    """directional derivatives along seeded directions; the step is 1e-5 of the signal's scale: the truncation error is of relative order
    1e-10, the rounding error 1e-16 / step"""
    x, y = _pair(5, n, fs, gaps)
    yt = torch.tensor(y, requires_grad=True)
    G.stoi_full(x, yt, fs, extended)['score'].backward()
    g = yt.grad.numpy()
    f = lambda v: float(G.stoi_full(x, torch.from_numpy(v), fs, extended)['score'])      # noqa: E731
    h = 1e-4
    for seed in (1, 2, 3):
        d = 0.01 * np.random.RandomState(seed).randn(n)
        num = (f(y + h * d) - f(y - h * d)) / (2 * h)
        ana = float(g @ d)
        assert abs(num - ana) < 1e-6 * abs(ana), (seed, num, ana)


# ---- (b) the adjoints the kernels implement, in numpy
def resample_adjoint(gy10, n, p, q):
    """gy[m] = sum_k gy10[k] g[k q - m p + L], m < n"""
    g, L = R.taps(p, q)
    gy = np.zeros(n)
    k = np.arange(len(gy10))
    for m in range(n):
        j = k * q - m * p + L
        ok = (j >= 0) & (j <= 2 * L)
        gy[m] = (gy10[ok] * g[j[ok]]).sum()
    return gy


def gather_adjoint(gv, mask, n10):
    """gv (K, 256) = the gradient in the windowed frames of the compacted signal -> gy10 (n10,): window, overlap-add, gather back through the
    inverse of the kept-index list, window again, the at most two source frames that cover a sample"""
    w = R.window()
    idx = np.nonzero(mask)[0]
    K = len(idx)
    inv = -np.ones(len(mask), dtype=int)
    inv[idx] = np.arange(K)
    gt = w * gv
    gy10 = np.zeros(n10)
    for n in range(n10):
        for i in (n // R.HOP - 1, n // R.HOP):
            if i < 0 or i >= len(mask) or inv[i] < 0:
                continue
            k, t = inv[i], n - i * R.HOP
            gc = gt[k, t]
            if t < R.HOP:
                gc += gt[k - 1, t + R.HOP] if k > 0 else 0.0
            else:
                gc += gt[k + 1, t - R.HOP] if k + 1 < K else 0.0
            gy10[n] += w[t] * gc
    return gy10


def dft_adjoint(Gc):
    """Gc (K, 257) complex -> gv[n] = Re sum_k G_k e^{+2 pi i k n / 512}, n < 256: no doubling of the one-sided bins"""
    n = np.arange(R.N_FRAME)
    k = np.arange(R.NFFT // 2 + 1)
    return (Gc[:, :, None] * np.exp(2j * np.pi * k[None, :, None] * n[None, None, :] / R.NFFT)).real.sum(axis=1)


def band_rule(gE, Y):
    """gE (15, K), Y (K, 257) complex -> G = (gE / E) Y on the band's bins, 0 where E == 0 and outside the bands"""
    lo, hi = R.band_edges()
    out = np.zeros_like(Y)
    for b in range(R.NUMBAND):
        E = np.sqrt((np.abs(Y[:, lo[b]:hi[b]]) ** 2).sum(axis=1))
        c = np.where(E > 0, gE[b] / np.where(E > 0, E, 1.0), 0.0)
        out[:, lo[b]:hi[b]] = c[:, None] * Y[:, lo[b]:hi[b]]
    return out


def _mask_case(fs=16000, n=9000, seed=7):
    x, y = _pair(seed, n, fs, [(3000, 4600)])
    r = R.stoi_full(x, y, fs)
    assert 30 <= r['K'] < r['frames']
    idx = np.nonzero(r['mask'])[0]
    assert (np.diff(idx) > 1).any() and r['mask'][0] and r['mask'][-1]          # compacted neighbours that are no neighbours in the source
    return y, r['mask']


def test_resampler_adjoint():
    rng = np.random.RandomState(1)
    for n in (1, 37, 1000):
        y = torch.tensor(rng.randn(n), requires_grad=True)
        y10 = G.resample(y, 5, 8)
        g10 = rng.randn(len(y10))
        (y10 * torch.from_numpy(g10)).sum().backward()
        assert _relmax(resample_adjoint(g10, n, 5, 8), y.grad.numpy()) < TOL
    y = torch.randn(5, dtype=torch.float64)
    assert G.resample(y, 1, 1) is y          # the identity at 10 kHz


def test_compaction_double_window_gather():
    y, mask = _mask_case()
    y10 = torch.tensor(R.resample(y, 5, 8), requires_grad=True)
    idx = torch.from_numpy(np.nonzero(mask)[0])
    K = len(idx)
    v = G.frames(G.compact(G.frames(y10, len(mask))[idx]), K)          # (K, 256) windowed frames of the compacted signal
    gv = np.random.RandomState(2).randn(K, R.N_FRAME)
    (v * torch.from_numpy(gv)).sum().backward()
    got = gather_adjoint(gv, mask, len(y10))
    assert _relmax(got, y10.grad.numpy()) < TOL
    dropped_only = np.ones(len(y10), bool)
    for i in np.nonzero(mask)[0]:
        dropped_only[i * R.HOP:i * R.HOP + R.N_FRAME] = False
    assert dropped_only.any() and (got[dropped_only] == 0).all() and (y10.grad.numpy()[dropped_only] == 0).all()


def test_one_sided_dft_adjoint():
    rng = np.random.RandomState(3)
    v = torch.tensor(rng.randn(4, R.N_FRAME), requires_grad=True)
    Y = torch.fft.rfft(v, n=R.NFFT, dim=1)
    Gc = rng.randn(4, 257) + 1j * rng.randn(4, 257)
    (Y.real * torch.from_numpy(Gc.real) + Y.imag * torch.from_numpy(Gc.imag)).sum().backward()
    assert _relmax(dft_adjoint(Gc), v.grad.numpy()) < TOL


def test_band_rule():
    rng = np.random.RandomState(4)
    Yn = rng.randn(5, 257) + 1j * rng.randn(5, 257)
    Yn[2] = 0.0                                                     # a frame with E == 0 in every band
    Yn[3, 7:9] = 0.0                                                # and one band of another
    Yr, Yi = torch.tensor(Yn.real, requires_grad=True), torch.tensor(Yn.imag, requires_grad=True)
    E = G.bands(torch.complex(Yr, Yi))
    gE = rng.randn(R.NUMBAND, 5)
    (E * torch.from_numpy(gE)).sum().backward()
    got = band_rule(gE, Yn)
    assert torch.isfinite(Yr.grad).all() and torch.isfinite(Yi.grad).all()
    assert _relmax(got.real, Yr.grad.numpy()) < TOL and _relmax(got.imag, Yi.grad.numpy()) < TOL
    assert (got[2] == 0).all() and (got[3, 7:9] == 0).all() and (got[:, :7] == 0).all() and (got[:, 219:] == 0).all()
    assert (Yr.grad.numpy()[2] == 0).all() and (Yi.grad.numpy()[3, 7:9] == 0).all()


def test_adjoint_identity_of_the_linear_part():
    """A: processed signal -> spectrum of the compacted frames; |<A u, G> - <u, A^T G>| against sqrt(<Au,Au><G,G>), A^T from the numpy adjoints"""
    y, mask = _mask_case()
    idx = torch.from_numpy(np.nonzero(mask)[0])
    K = len(idx)
    rng = np.random.RandomState(5)
    u = rng.randn(len(y))
    u10 = G.resample(torch.from_numpy(u), 5, 8)
    Au = G.spectrum(G.compact(G.frames(u10, len(mask))[idx]), K).numpy()
    Gc = rng.randn(K, 257) + 1j * rng.randn(K, 257)
    ATg = resample_adjoint(gather_adjoint(dft_adjoint(Gc), mask, len(u10)), len(y), 5, 8)
    lhs = (Au.real * Gc.real + Au.imag * Gc.imag).sum()
    rhs = (u * ATg).sum()
    scale = np.sqrt((np.abs(Au) ** 2).sum() * (np.abs(Gc) ** 2).sum())
    assert abs(lhs - rhs) < 1e-12 * scale, (lhs, rhs, scale)


def test_whole_chain_from_the_numpy_adjoints():
    """autograd's envelope gradient pushed through band rule, DFT adjoint, gather and resampler adjoint = autograd's gradient in y"""
    y, mask = _mask_case()
    for fs in (16000, 10000):
        p, q = R.rate(fs)
        m = mask[:R.frames_of(R.n10_of(len(y), p, q))] if fs == 10000 else mask
        yt = torch.tensor(y, requires_grad=True)
        E = G.envelopes(yt, m, fs)
        gE = np.random.RandomState(6).randn(*E.shape)
        (E * torch.from_numpy(gE)).sum().backward()
        y10 = R.resample(y, p, q)
        idx = torch.from_numpy(np.nonzero(m)[0])
        Y = G.spectrum(G.compact(G.frames(torch.from_numpy(y10), len(m))[idx]), len(idx)).numpy()
        g10 = gather_adjoint(dft_adjoint(band_rule(gE, Y)), m, len(y10))
        got = g10 if p == q else resample_adjoint(g10, len(y), p, q)
        assert _relmax(got, yt.grad.numpy()) < TOL


# ---- (c)
@pytest.mark.parametrize('extended', [False, True])
def test_zero_past_the_length_and_for_fewer_than_30_frames(extended):
    x, y = _pair(9, 12000, 16000, [(4000, 6000)])
    clean, proc = np.stack([x, x, x, x]), np.stack([y, y, y, y])
    scores, grad, infos = G.batch(clean, proc, [12000, 9001, 4800, 0], 16000, extended)
    assert [r['K'] >= 30 for r in infos] == [True, True, False, False] and infos[2]['frames'] == 22
    assert scores[2] == 1e-5 and scores[3] == 1e-5
    assert (grad[2] == 0).all() and (grad[3] == 0).all()
    assert (grad[1, 9001:] == 0).all() and grad[1, :9001].abs().max() > 0 and grad[0].abs().max() > 0


# ---- (d)
def test_criteria_surface():
    from speech_enhancement_by_s3prl_amd import _lib, objective
    for cls, ext in ((objective.stoi, False), (objective.estoi, True)):
        crit = cls()
        assert crit.wants_wav is True and crit.sr == 16000 and crit.extended is ext and crit.reduce_fn is None
        assert cls(sr=10000).sr == 10000
        with pytest.raises(_lib.SEError):
            crit(wav_predicted=torch.randn(2, 8000), wav_tar=torch.randn(2, 8000), lengths=torch.tensor([8000, 7000]))
        with pytest.raises(_lib.SEError):
            crit(wav_predicted=torch.randn(2, 8000), wav_tar=torch.randn(2, 8000), length_masks=torch.ones(2, 8000))


def test_grad_entry_refuses_bad_arguments_without_a_device():
    from speech_enhancement_by_s3prl_amd import _lib
    lib = _lib.load()
    assert lib.se_stoi_grad_workspace_bytes(None, 2, 16000) == 0
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    rc = lib.se_stoi_grad_f32(None, p, p, 16, None, 1, 16, 0, 1.0, p, p, p, 256, None)
    assert rc != 0 and 'se_stoi_grad_f32: null argument' in lib.se_last_error().decode()
    plan = ctypes.c_void_p()
    if lib.se_stoi_plan_create(16000, plan) == 0:                       # a device is present: the size check comes before any launch
        need = lib.se_stoi_grad_workspace_bytes(plan, 2, 16000)
        assert need > lib.se_stoi_workspace_bytes(plan, 2, 16000) > 0
        rc = lib.se_stoi_grad_f32(plan, p, p, 16000, None, 2, 16000, 0, 1.0, p, p, p, need - 1, None)
        msg = lib.se_last_error().decode()
        assert rc != 0 and 'workspace of' in msg and 'se_stoi_grad_workspace_bytes' in msg, msg
        lib.se_stoi_plan_destroy(plan)
