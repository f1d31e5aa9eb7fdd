"""Host-side pins for training through the analysis transform (no GPU): the closed forms of tests/stft_grad_ref.py -- what csrc/stftg_bwd.hip
and csrc/specdist.hip implement -- agree with float64 autograd through oracle.preprocessor.stft to 1e-9 of the maximum, the adjoint satisfies
the adjoint identity to 1e-12, the criterion's loss matches central differences to 1e-6; and the host surface exists and refuses host tensors."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import stft_grad_ref as S      # noqa: E402

TOL = 1e-9

# name: (n_fft, hop, win, T)
GEOMS = {
    '400': (400, 160, 400, 5 * 160),
    '400_ragged_T': (400, 160, 400, 5 * 160 + 77),                # T no multiple of the hop
    '512': (512, 128, 512, 7 * 128 + 5),
    'short_window': (60, 20, 50, 9 * 20 + 3),                     # win < n_fft
    'T_m_plus_1': (400, 160, 400, 201),                           # both folds overlap on every interior sample
    'T_2m': (60, 20, 50, 60),
    '512_T_m_plus_1': (512, 128, 512, 257),
}


def _relmax(got, ref):
    return (got - ref).abs().max().item() / ref.abs().max().item()


def _case(name, B=2):
    n_fft, hop, win, T = GEOMS[name]
    g = S.geometry(n_fft, hop, win)
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    F, K = T // hop + 1, n_fft // 2 + 1
    x = torch.randn(B, T, generator=gen, dtype=torch.float64)
    G = torch.complex(torch.randn(B, F, K, generator=gen, dtype=torch.float64), torch.randn(B, F, K, generator=gen, dtype=torch.float64))
    gp = torch.randn(B, F, K, generator=gen, dtype=torch.float64)
    return g, T, x, G, gp


@pytest.mark.parametrize('name', list(GEOMS))
def test_adjoint_closed_form_vs_autograd(name):
    """an arbitrary complex G on (re, im), a gradient on the power, and both together"""
    g, T, x, G, gp = _case(name)
    for use_c, use_p in ((True, False), (False, True), (True, True)):
        xr = x.clone().requires_grad_(True)
        X = S.spectrum(xr, g)
        loss = 0
        if use_c:
            loss = loss + (X.real * G.real + X.imag * G.imag).sum()
        if use_p:
            loss = loss + ((X.real ** 2 + X.imag ** 2) * gp).sum()
        loss.backward()
        got = S.stft_bwd_closed(S.spectral_gradient(gp if use_p else None, G if use_c else None, X.detach()), T, g)
        assert _relmax(got, xr.grad) < TOL, (name, use_c, use_p, _relmax(got, xr.grad))


@pytest.mark.parametrize('name', list(GEOMS))
def test_adjoint_identity(name):
    g, T, x, G, _ = _case(name)
    Au = S.spectrum(x, g)
    ATG = S.stft_bwd_closed(G, T, g)
    lhs = (Au.real * G.real + Au.imag * G.imag).sum().item()
    rhs = (x * ATG).sum().item()
    scale = ((Au.abs() ** 2).sum() * (G.abs() ** 2).sum()).sqrt().item()
    assert abs(lhs - rhs) <= 1e-12 * scale, (lhs, rhs, scale)


def _criterion_case():
    gen = torch.Generator().manual_seed(7)
    B, F, K, hop = 4, 12, 33, 16
    p_tar = torch.rand(B, F, K, generator=gen, dtype=torch.float64) + 1e-3
    p_pred = p_tar * (0.5 + torch.rand(B, F, K, generator=gen, dtype=torch.float64))
    p_pred[0, 2, 3:9] = 0.0                   # under the clamp: gradient exactly 0
    p_pred[1, 1] = S.CLAMP                    # at the clamp: still 0
    p_pred[1, 4, 5] = p_tar[1, 4, 5]          # sign(0) = 0 in the log term
    p_pred[2] = p_tar[2]                      # a == 0: the sc term has no gradient
    lengths = [hop * (F - 1), hop * 7 + 3, hop * 4, 0]
    return p_pred, p_tar, lengths, hop


def test_criterion_coefficients_vs_autograd():
    p_pred, p_tar, lengths, hop = _criterion_case()
    for b in range(p_pred.shape[0]):
        pr = p_pred.clone().requires_grad_(True)
        lb = S.specdist_loss_b(pr, p_tar, lengths, hop)
        lb[b].backward()
        ref = pr.grad
        got = S.specdist_grad_closed(p_pred, p_tar, lengths, hop)
        assert torch.isfinite(ref).all() and torch.isfinite(got).all()
        other = [i for i in range(p_pred.shape[0]) if i != b]
        assert (ref[other] == 0).all()
        if ref[b].abs().max() == 0:
            assert (got[b] == 0).all()
        else:
            assert _relmax(got[b], ref[b]) < TOL
    got = S.specdist_grad_closed(p_pred, p_tar, lengths, hop)
    counts = S.frame_counts(lengths, hop, p_pred.shape[1])
    assert counts == [12, 8, 5, 0]
    for b, nf in enumerate(counts):
        assert (got[b, nf:] == 0).all()
    assert (got[0, 2, 3:9] == 0).all() and (got[1, 1] == 0).all() and (got[3] == 0).all()
    lb = S.specdist_loss_b(p_pred, p_tar, lengths, hop)
    assert lb[3].item() == 0.0 and lb[2].item() == 0.0 and lb[0].item() > 0


def test_loss_matches_central_differences():
    """the whole restatement (mask, three small resolutions, per-utterance distance, means) along seeded directions"""
    res = ((64, 16, 64), (128, 32, 96), (60, 20, 50))
    T = 700
    tar, pred = S.noisy_pair(3, T, 16000, seed=3)
    lengths = [T, 431, 0]
    f = lambda w: S.multires_loss(w, tar, lengths, resolutions=res)      # noqa: E731
    w = pred.clone().requires_grad_(True)
    f(w).backward()
    g = w.grad
    assert (g[1, 431:] == 0).all() and (g[2] == 0).all()
    h = 1e-6
    for seed in (1, 2, 3):
        d = torch.randn(3, T, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * pred.std()
        num = (f(pred + h * d) - f(pred - h * d)).item() / (2 * h)
        ana = (g * d).sum().item()
        assert abs(num - ana) < 1e-6 * abs(ana), (seed, num, ana)


def test_restatement_composes_the_closed_forms():
    """d loss / d wav through autograd = the closed-form criterion gradient pushed through the closed-form adjoint, then masked"""
    n_fft, hop, win = 128, 32, 96
    T = 500
    tar, pred = S.noisy_pair(3, T, 16000, seed=5)
    lengths = [T, 333, 150]
    g = S.geometry(n_fft, hop, win)
    w = pred.clone().requires_grad_(True)
    S.multires_loss(w, tar, lengths, resolutions=((n_fft, hop, win),)).backward()
    wp, wt = S.mask_wav(pred, lengths), S.mask_wav(tar, lengths)
    X = S.spectrum(wp, g)
    gp = S.specdist_grad_closed(X.real ** 2 + X.imag ** 2, S.power_of(wt, g), lengths, hop) / 3
    got = S.mask_wav(S.stft_bwd_closed(S.spectral_gradient(gp, None, X), T, g), lengths)
    assert _relmax(got, w.grad) < TOL


def test_surface():
    """objective.MultiResSTFT and preprocessor.stft_for_loss exist, ask the training step for the waveform, and take device tensors only"""
    from speech_enhancement_by_s3prl_amd import _lib, objective, preprocessor
    crit = objective.MultiResSTFT()
    assert crit.wants_wav and crit.resolutions == S.RESOLUTIONS and crit.clamp == S.CLAMP and crit.reduce_fn is None
    assert list(crit.state_dict()) == []
    with pytest.raises(_lib.SEError):
        crit(wav_predicted=torch.zeros(1, 2000), wav_tar=torch.zeros(1, 2000), lengths=torch.tensor([2000]))
    with pytest.raises(_lib.SEError):
        preprocessor.stft_for_loss(preprocessor.StftPlan(256, 64, 256), torch.zeros(1, 2000))


def test_entry_points_refuse_bad_arguments_without_a_device():
    from speech_enhancement_by_s3prl_amd import _lib
    lib = _lib.load()
    assert lib.se_stft_bwd_chunk(None) == -1 and lib.se_stft_bwd_workspace_bytes(None, 2, 1000) == 0
    assert lib.se_stft_bwd_f32(None, None, None, None, 1, 5, 800, None, 800, None, 0, None) == -1
    assert b'se_stft_bwd_f32' in lib.se_last_error()
    assert lib.se_specdist_scratch_doubles(4, 76, 129) >= 4 * 3 + 8
    assert lib.se_specdist_loss_f32(None, None, None, 64, 4, 76, 129, ctypes.c_float(1e-7), None, None, None) == -1
    assert b'se_specdist_loss_f32' in lib.se_last_error()
