"""GPU: training through the decode.  se_istft_bwd_f32 (csrc/istftg_bwd.hip), se_dbnorm_bwd_f32, se_sisdr_grad_f32 and their autograd glue
(preprocessor._IstftFn, decode._DbNormFn, objective.WavSISDR, pipeline.HeadFinetuneStep with a `wants_wav` criterion) against the float64
chain of tests/decode_grad_ref.py (itself pinned by tests/test_decode_grad_host.py).

Bound of every gradient comparison: max |got - ref| < 1e-4 max |ref| per utterance (rows whose reference is all zero must be exactly zero) --
the bound of the transforms and criterion gradients (tests/test_gpu_objectives.py, tests/test_gpu_preprocessor.py); loss values 1e-4 relative.
The measured maxima are printed and logged (conftest.bounded)."""
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import decode_grad_ref as R      # noqa: E402
from conftest import bounded      # noqa: E402
from oracle import heads as oheads      # noqa: E402
from oracle import preprocessor as opre      # noqa: E402

pytestmark = pytest.mark.gpu

BOUND = 1e-4
DEV = torch.device('cuda:0')

# case: (sample_rate, win_ms, hop_ms, n_freq, n_mels, general plan)
CASES = {
    'fixed400': (16000, 25, 10, 201, 40, False),       # 400 / 400 / 160 through se_plan_create: the general tables built beside the 400-point ones
    'any400': (16000, 25, 10, 201, 40, True),          # the same geometry through se_plan_create_any
    'n512': (16000, 32, 8, 257, 40, True),             # 512 / 512 / 128
    'n200_8k': (8000, 25, 10, 101, 40, True),          # 200 / 200 / 80 at 8 kHz
    'short_window': (1000, 50, 20, 31, 10, True),      # n_fft 60, win 50, hop 20: win < n_fft
}
B = 3


def _geom(case):
    sr, win_ms, hop_ms, n_freq, n_mels, _ = CASES[case]
    return opre.Geometry(sample_rate=sr, win_ms=win_ms, hop_ms=hop_ms, n_freq=n_freq, n_mels=n_mels)


@functools.lru_cache(maxsize=None)
def _P(case):
    from speech_enhancement_by_s3prl_amd.preprocessor import OnlinePreprocessor
    sr, win_ms, hop_ms, n_freq, n_mels, general = CASES[case]
    p = OnlinePreprocessor(sample_rate=sr, win_ms=win_ms, hop_ms=hop_ms, n_freq=n_freq, n_mels=n_mels, n_mfcc=13)
    p.general_plan = general
    return p.to(DEV)


def _lib():
    from speech_enhancement_by_s3prl_amd import _lib as L
    return L, L.load()


def _err(got, ref):
    """max over the utterances of max |got - ref| / max |ref|; an utterance whose reference is all zero must be exactly zero"""
    got, ref = got.detach().double().cpu().flatten(1), ref.detach().double().cpu().flatten(1)
    worst = 0.0
    for gr, rr in zip(got, ref):
        top = rr.abs().max().item()
        if top == 0.0:
            assert (gr == 0).all()
            continue
        worst = max(worst, (gr - rr).abs().max().item() / top)
    return worst


def _check(name, got, ref):
    e = _err(got, ref)
    print(f'{name}: {e:.3e}')
    bounded('decode_grad/' + name, e, BOUND)


@functools.lru_cache(maxsize=None)
def _data(case):
    """one seeded case, shared and left unchanged: F = 2 chunk + 3 frames (a workgroup border and a partial last workgroup), wav_stride = T > n_out"""
    L, lib = _lib()
    g = _geom(case)
    chunk = lib.se_istft_bwd_chunk_frames(_P(case)._plan(DEV))
    assert chunk >= 1
    F = 2 * chunk + 3
    T = (F - 1) * g.hop + g.hop // 2
    x = R.harmonic_batch(B, T, g.sample_rate, seed=sum(map(ord, case)))
    spec = opre.stft(x, g).transpose(-1, -2)                      # (B, F, K) complex128
    assert spec.shape == (B, F, g.n_freq)
    power = spec.real ** 2 + spec.imag ** 2
    power = power + 1e-3 * power.max()
    phase = torch.atan2(spec.imag, spec.real)
    grad = torch.randn(B, T, generator=torch.Generator().manual_seed(11), dtype=torch.float64)
    return {'F': F, 'T': T, 'power': power, 'phase': phase, 'g': grad, 'ref': _chain_grad(power, phase, grad, g)}


def _chain_grad(power, phase, grad, geom):
    p = power.clone().requires_grad_(True)
    wav = R.pad_to(R.istft_chain(p, phase, geom), grad.shape[1])
    (wav * grad).sum().backward()
    return p.grad


def _bwd(case, grad, power, phase=None, tphase=None):
    L, lib = _lib()
    g32, p32 = grad.float().to(DEV).contiguous(), power.float().to(DEV).contiguous()
    ph = None if phase is None else phase.float().to(DEV).contiguous()
    tp = None if tphase is None else tphase.to(DEV).contiguous()
    out = torch.full_like(p32, float('nan'))                      # fully written, no accumulate
    Bn, F, K = p32.shape
    L.check(lib.se_istft_bwd_f32(_P(case)._plan(DEV), L.ptr(g32), g32.shape[1], L.ptr(p32), L.ptr(ph), L.ptr(tp), Bn, F, L.ptr(out), L.stream()),
            'se_istft_bwd_f32')
    return out


@pytest.mark.parametrize('case', list(CASES))
def test_adjoint_kernel_vs_chain(gpu, case):
    """1: phase and encoded-phase forms against the float64 chain, every element compared, and against each other"""
    d = _data(case)
    got_ph = _bwd(case, d['g'], d['power'], phase=d['phase'])
    got_tp = _bwd(case, d['g'], d['power'], tphase=R.encode_phase(d['phase']))
    assert torch.isfinite(got_ph).all() and torch.isfinite(got_tp).all()
    _check(f'1/{case}/phase', got_ph, d['ref'])
    _check(f'1/{case}/tphase', got_tp, d['ref'])
    _check(f'1/{case}/phase_vs_tphase', got_ph, got_tp.double())


@pytest.mark.parametrize('case', list(CASES))
def test_zero_power_convention(gpu, case):
    """2: a block of bins and one whole frame at P = 0: the gradient is exactly 0.0 there and within the bound elsewhere"""
    d = _data(case)
    power = d['power'].clone()
    power[0, 1:4, 2:11] = 0.0
    power[1, d['F'] // 2] = 0.0
    ref = _chain_grad(power, d['phase'], d['g'], _geom(case))
    for form, kw in (('phase', {'phase': d['phase']}), ('tphase', {'tphase': R.encode_phase(d['phase'])})):
        got = _bwd(case, d['g'], power, **kw)
        assert (got.cpu()[power == 0] == 0).all()
        _check(f'2/{case}/{form}', got, ref)


@pytest.mark.parametrize('case', list(CASES))
def test_adjoint_identity(gpu, case):
    """3: <A u, g> = <u, A^T g> with A the forward kernel (magnitude -> waveform at a fixed phase) and A^T g = grad_power 2 sqrt(P): no oracle"""
    L, lib = _lib()
    d = _data(case)
    F, T = d['F'], d['T']
    u = (0.2 + torch.rand(B, F, _geom(case).n_freq, generator=torch.Generator().manual_seed(5))).to(DEV)
    P = (u * u).contiguous()
    ph = d['phase'].float().to(DEV).contiguous()
    g = d['g'].float().to(DEV).contiguous()
    wav = torch.empty(B, T, device=DEV)
    L.check(lib.se_istft_f32(_P(case)._plan(DEV), L.ptr(P), L.ptr(ph), B, F, 2.0, L.ptr(wav), T, None, None, L.stream()), 'se_istft_f32')
    ATg = _bwd(case, g, P, phase=ph).double().cpu() * 2 * P.double().cpu().sqrt()
    Au, g64, u64 = wav.double().cpu(), g.double().cpu(), P.double().cpu().sqrt()
    lhs, rhs = (Au * g64).sum().item(), (u64 * ATg).sum().item()
    scale = ((Au * Au).sum() * (g64 * g64).sum()).sqrt().item()
    print(f'3/{case}: |<Au,g> - <u,ATg>| / sqrt(<Au,Au><g,g>) = {abs(lhs - rhs) / scale:.3e}')
    bounded(f'decode_grad/3/{case}', abs(lhs - rhs) / scale, BOUND)


@pytest.mark.parametrize('form', ['fixed_db', 'reference_audio'])
def test_dbnorm_backward(gpu, form):
    """4: lengths {T, T - 37, T / 2, 0}; grad_wav aliased with grad_out and not; and through the autograd node"""
    from speech_enhancement_by_s3prl_amd import decode
    L, lib = _lib()
    gen = torch.Generator().manual_seed(21)
    Bn, T = 4, 2 * 4096 + 301
    wav = torch.randn(Bn, T, generator=gen) * 0.05
    g = torch.randn(Bn, T, generator=gen)
    lengths = torch.tensor([T, T - 37, T // 2, 0])
    tar = torch.randn(Bn, T, generator=gen) * 0.2
    ref, _ = R.dbnorm_grad_ref(wav.double(), g.double(), -25 if form == 'fixed_db' else tar.double(), lengths)
    wav_d, g_d, len_d, tar_d = wav.to(DEV), g.to(DEV), lengths.to(DEV), tar.to(DEV)
    target = -25 if form == 'fixed_db' else tar_d
    wav_sumsq = decode.masked_sumsq(wav_d, len_d)
    ref_sumsq = None if form == 'fixed_db' else decode.masked_sumsq(tar_d, len_d)
    sums = {'audio_sumsq': wav_sumsq, 'ref_sumsq': ref_sumsq}      # handed over: summed once (the summing launch's atomics may round differently per run)
    with torch.no_grad():
        y = decode.masked_normalize_decibel(wav_d, target, len_d, **sums)
    scratch = torch.empty(Bn, device=DEV, dtype=torch.float64)
    for alias in (False, True):
        gin = g_d.clone()
        out = gin if alias else torch.full_like(gin, float('nan'))
        L.check(lib.se_dbnorm_bwd_f32(L.ptr(y), L.ptr(gin), Bn, T, T, L.ptr(len_d), L.ptr(wav_sumsq), L.ptr(ref_sumsq), -25.0, 1e-8, L.ptr(scratch),
                                      L.ptr(out), L.stream()), 'se_dbnorm_bwd_f32')
        _check(f'4/{form}/alias{int(alias)}', out, ref)
    w = wav_d.clone().requires_grad_(True)
    y2 = decode.masked_normalize_decibel(w, target, len_d, **sums)
    assert torch.equal(y2.detach(), y)
    (y2 * g_d).sum().backward()
    _check(f'4/{form}/autograd', w.grad, ref)


def test_wav_sisdr_loss_and_gradient(gpu):
    """5: ragged lengths with an empty utterance, the estimate a few dB off the target"""
    from speech_enhancement_by_s3prl_amd import evaluation
    from speech_enhancement_by_s3prl_amd.objective import WavSISDR
    gen = torch.Generator().manual_seed(31)
    Bn, ld = 4, 5000
    tar = torch.randn(Bn, ld, generator=gen) * 0.1
    src = torch.tensor([0.7, 1.3, 1.0, 0.9])[:, None] * tar + 0.05 * torch.randn(Bn, ld, generator=gen)
    lengths = torch.tensor([ld, ld - 1234, 1201, 0])
    s64 = src.double().requires_grad_(True)
    rloss = R.wav_sisdr_loss(s64, tar.double(), lengths)
    rloss.backward()
    s = src.to(DEV).requires_grad_(True)
    loss, extra = WavSISDR()(wav_predicted=s, wav_tar=tar.to(DEV), lengths=lengths.to(DEV))
    assert extra == {}
    loss.backward()
    scores = evaluation.sisdr_batch(src.to(DEV), tar.to(DEV), lengths.to(DEV))
    print(f'5/loss: {abs(loss.item() - rloss.item()) / abs(rloss.item()):.3e}')
    assert abs(loss.item() + scores.double().mean().item()) < 1e-6 * abs(loss.item())
    bounded('decode_grad/5/loss', abs(loss.item() - rloss.item()) / abs(rloss.item()), BOUND)
    _check('5/grad', s.grad, s64.grad)
    for b in range(Bn):
        assert (s.grad[b, int(lengths[b]):] == 0).all()


@functools.lru_cache(maxsize=None)
def _e2e():
    """a ragged 3-utterance batch of about 0.3 s with its preprocessor, head state and float64 chain result"""
    from speech_enhancement_by_s3prl_amd import pipeline
    from speech_enhancement_by_s3prl_amd.heads import LinearResidual
    T = 4850
    gen = torch.Generator().manual_seed(41)
    clean = R.harmonic_batch(B, T, 16000, seed=43).float()
    wavs = torch.stack([clean + 0.02 * torch.randn(B, T, generator=gen), clean], dim=1).contiguous()       # (B, 2, T): noisy, clean
    lengths = torch.tensor([T, T - 333, T // 2 + 1])
    pre = pipeline.build_preprocessor(pipeline.make_config(), DEV, upstream='baseline')
    torch.manual_seed(0)
    head = LinearResidual(input_size=120, output_size=201, activation='Sigmoid', cmvn=True)
    state = {k: v.detach().clone() for k, v in head.state_dict().items()}
    g = opre.Geometry()
    fl = [dict(pipeline.BASELINE_FEAT, channel=0), opre.get_feat_config('linear', 0), opre.get_feat_config('phase', 0)]
    rfeats, rlin, rph = opre.forward(wavs.double(), fl, g)
    w = state['linear.weight'].double().requires_grad_(True)
    b = state['linear.bias'].double().requires_grad_(True)
    rpred, _ = oheads.linear_residual(rfeats, rlin, w, b, activation='Sigmoid')
    rwav = R.decode_chain(rpred, rph, lengths, g, wavs[:, 1].double())
    rloss = R.wav_sisdr_loss(rwav, wavs[:, 1].double(), lengths)
    rloss.backward()
    return {'wavs': wavs, 'lengths': lengths, 'pre': pre, 'state': state, 'rloss': rloss.item(), 'gw': w.grad, 'gb': b.grad}


def _head(state):
    from speech_enhancement_by_s3prl_amd.heads import LinearResidual
    head = LinearResidual(input_size=120, output_size=201, activation='Sigmoid', cmvn=True)
    head.load_state_dict(state)
    return head.to(DEV)


def test_end_to_end_head_gradient(gpu):
    """6: features -> LinearResidual -> decode_wav(..., wav_tar) -> WavSISDR -> backward, and the same through pipeline.HeadFinetuneStep"""
    from speech_enhancement_by_s3prl_amd import decode, pipeline
    from speech_enhancement_by_s3prl_amd.objective import WavSISDR
    from speech_enhancement_by_s3prl_amd.solver import get_optimizer
    e = _e2e()
    pre, wavs, lengths = e['pre'], e['wavs'].to(DEV), e['lengths'].to(DEV)
    head = _head(e['state'])
    with torch.no_grad():
        feats_up, feats_down, lin_inp, ph_inp, lin_tar, ph_tar = pre(wavs)
    predicted, _ = head(features=feats_down, linears=lin_inp)
    wav_tar = wavs[:, 1, :]
    wav = decode.decode_wav(pre, predicted, ph_inp, lengths, wav_tar)
    loss, _ = WavSISDR()(wav_predicted=wav, wav_tar=wav_tar, lengths=lengths)
    loss.backward()
    print(f'6/loss: {abs(loss.item() - e["rloss"]) / abs(e["rloss"]):.3e}')
    bounded('decode_grad/6/loss', abs(loss.item() - e['rloss']) / abs(e['rloss']), BOUND)
    _check('6/weight', head.linear.weight.grad[None], e['gw'][None])
    _check('6/bias', head.linear.bias.grad[None], e['gb'][None])
    head2 = _head(e['state'])
    opt = get_optimizer(list(head2.named_parameters()), lr=1e-4, warmup_proportion=0.1, training_steps=100)
    step = pipeline.HeadFinetuneStep(pre, head2, opt, criterion=WavSISDR())
    loss2, grad_norm, skipped = step(wavs, lengths)
    assert not skipped and grad_norm > 0
    assert abs(loss2.item() - loss.item()) <= 1e-6 * abs(loss.item())
    loss3, grad_norm3, skipped3 = step(wavs, lengths)              # a second step runs on the same objects (the learning rate warms up from 0)
    assert not skipped3 and grad_norm3 > 0 and torch.isfinite(loss3)


def test_no_behaviour_change_and_repeatability(gpu):
    """7: decode_wav with and without autograd returns the same bits; two backward launches return the same bits"""
    from speech_enhancement_by_s3prl_amd import decode
    e = _e2e()
    pre, wavs, lengths = e['pre'], e['wavs'].to(DEV), e['lengths'].to(DEV)
    head = _head(e['state'])
    with torch.no_grad():
        feats_up, feats_down, lin_inp, ph_inp, lin_tar, ph_tar = pre(wavs)
        predicted, _ = head(features=feats_down, linears=lin_inp)
    for target in (-25, wavs[:, 1, :]):
        with torch.no_grad():
            plain = decode.decode_wav(pre, predicted, ph_inp, lengths, target)
        tracked = decode.decode_wav(pre, predicted.clone().requires_grad_(True), ph_inp, lengths, target)
        assert plain.grad_fn is None and tracked.grad_fn is not None
        assert torch.equal(plain, tracked.detach())
    d = _data('fixed400')
    a = _bwd('fixed400', d['g'], d['power'], phase=d['phase'])
    b = _bwd('fixed400', d['g'], d['power'], phase=d['phase'])
    assert torch.equal(a, b)
    from speech_enhancement_by_s3prl_amd.preprocessor import OnlinePreprocessor
    with pytest.raises(NotImplementedError):
        OnlinePreprocessor.istft(_P('fixed400'), d['power'].float().to(DEV).requires_grad_(True), d['phase'].float().to(DEV), linear_power=1)
