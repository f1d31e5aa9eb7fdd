"""CPU: the specification of the gradients through the decode, pinned before any kernel is compared with it.  The closed forms of
tests/decode_grad_ref.py (what csrc/istftg_bwd.hip, se_dbnorm_bwd_f32 and se_sisdr_grad_f32 implement) agree with float64 autograd through the
oracle's istft / masked_normalize_decibel / sisdr_eval to 1e-9 relative to the maximum; and the host surface of the waveform criterion exists
and refuses host tensors."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import decode_grad_ref as R      # noqa: E402
from oracle import objective as oobj      # noqa: E402
from oracle import preprocessor as opre      # noqa: E402

TOL = 1e-9


def _relmax(got, ref):
    return ((got - ref).abs().max() / ref.abs().max()).item()


GEOMS = {
    'default': dict(sample_rate=16000, win_ms=25, hop_ms=10, n_freq=201),       # 400 / 400 / 160
    'short_window': dict(sample_rate=1000, win_ms=50, hop_ms=20, n_freq=31),    # n_fft 60, win 50, hop 20
}


@pytest.mark.parametrize('name', list(GEOMS))
def test_istft_adjoint_closed_form(name):
    """formula 1 on F = 5 frames: every output sample is within n_fft of a signal edge, so the edge rule of the envelope matters throughout"""
    geom = opre.Geometry(**GEOMS[name])
    gen = torch.Generator().manual_seed(3)
    B, F, K = 2, 5, geom.n_freq
    power = torch.rand(B, F, K, generator=gen, dtype=torch.float64) + 0.05
    power[0, 2, 3:9] = 0.0                    # the P <= 0 convention: exactly 0 there in both
    power[1, 4] = 0.0
    phase = (torch.rand(B, F, K, generator=gen, dtype=torch.float64) - 0.5) * 6.2
    n_out = geom.hop * (F - 1)
    g = torch.randn(B, n_out + 13, generator=gen, dtype=torch.float64)          # wav_stride > n_out: the tail multiplies the zero fill
    p = power.clone().requires_grad_(True)
    wav = R.pad_to(R.istft_chain(p, phase, geom), n_out + 13)
    (wav * g).sum().backward()
    got = R.istft_bwd_closed(g, power, phase, geom)
    assert torch.isfinite(p.grad).all()
    assert _relmax(got, p.grad) < TOL
    assert (got[power <= 0] == 0).all() and (p.grad[power <= 0] == 0).all()


@pytest.mark.parametrize('form', ['fixed_db', 'reference_audio'])
def test_dbnorm_backward_closed_form(form):
    """formula 2 with lengths {T, ragged, 0}"""
    gen = torch.Generator().manual_seed(5)
    B, T = 3, 257
    wav = torch.randn(B, T, generator=gen, dtype=torch.float64) * 0.05
    g = torch.randn(B, T, generator=gen, dtype=torch.float64)
    lengths = torch.tensor([T, T - 37, 0])
    target = -25 if form == 'fixed_db' else torch.randn(B, T, generator=gen, dtype=torch.float64) * 0.2
    ref, dead = R.dbnorm_grad_ref(wav, g, target, lengths)
    got = R.dbnorm_bwd_closed(wav, g, target, lengths)
    assert dead.tolist() == [False, False, form == 'reference_audio']          # scale = 0: torch's nan, the convention's 0
    assert _relmax(got, ref) < TOL
    assert (got[dead] == 0).all()


def test_sisdr_coefficients():
    """formula 3: (p_b, q_b) against autograd of evaluation.py:5-10, and that expression against the oracle's value"""
    gen = torch.Generator().manual_seed(7)
    for n, gain in ((300, 0.7), (17, 1.3), (4000, 1.0)):      # the estimate a few dB off the target: Q is not near zero
        tar = torch.randn(n, generator=gen, dtype=torch.float64) * 0.1
        src = (gain * tar + 0.05 * torch.randn(n, generator=gen, dtype=torch.float64)).requires_grad_(True)
        val = R.sisdr_expr(src, tar)
        assert abs(val.item() - oobj.sisdr_eval(src.detach(), tar)) < 1e-12 * max(1.0, abs(val.item()))
        val.backward()
        s = src.detach()
        p, q = R.sisdr_coeffs((s * tar).sum(), (tar * tar).sum(), (s * s).sum())
        assert _relmax(p * tar + q * s, src.grad) < TOL
    # an empty utterance: both coefficients vanish (the score is 10 log10(eps))
    z = torch.zeros((), dtype=torch.float64)
    p, q = R.sisdr_coeffs(z, z, z)
    assert p.item() == 0.0 and q.item() == 0.0


def test_decode_chain_is_the_oracle_decode():
    """the differentiable chain computes what oracle.decode.decode_wav computes (where P > 0 the safe magnitude is the plain one)"""
    from oracle import decode as odec
    geom = opre.Geometry()
    gen = torch.Generator().manual_seed(9)
    B, F = 2, 6
    power = torch.rand(B, F, geom.n_freq, generator=gen, dtype=torch.float64) + 0.01
    phase = (torch.rand(B, F, geom.n_freq, generator=gen, dtype=torch.float64) - 0.5) * 6.0
    lengths = torch.tensor([geom.hop * (F - 1) + 50, 500])
    tar = torch.randn(B, int(lengths.max()), generator=gen, dtype=torch.float64)
    for target in (-25, tar):
        assert _relmax(R.decode_chain(power, phase, lengths, geom, target), odec.decode_wav(power, phase, lengths, geom, target)) < 1e-12


def test_encoded_phase_word_round_trip():
    """the host restatement of the encoded phase word gives back the unit phasor: (+-(1 - t^2), 2 t) / (1 + t^2)"""
    ph = torch.linspace(-3.14, 3.14, 1001, dtype=torch.float64)
    w = R.encode_phase(ph)
    t = (w & ~1).view(torch.float32).double()
    c = (1 - t * t) / (1 + t * t) * torch.where((w & 1) == 1, -1.0, 1.0)
    s = 2 * t / (1 + t * t)
    assert (c - ph.cos()).abs().max().item() < 1e-6 and (s - ph.sin()).abs().max().item() < 1e-6


def test_wav_sisdr_surface():
    """objective.WavSISDR exists, asks the training step for the waveform, and takes device tensors only"""
    from speech_enhancement_by_s3prl_amd import _lib
    from speech_enhancement_by_s3prl_amd.objective import WavSISDR
    crit = WavSISDR()
    assert crit.wants_wav is True and crit.eps == 1e-10 and crit.reduce_fn is None
    with pytest.raises(_lib.SEError):
        crit(wav_predicted=torch.randn(2, 100), wav_tar=torch.randn(2, 100), lengths=torch.tensor([100, 50]))
