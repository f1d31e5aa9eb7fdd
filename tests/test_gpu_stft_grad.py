"""GPU: training through the analysis.  se_stft_bwd_f32 (csrc/stftg_bwd.hip), the spectral criterion's kernels (csrc/specdist.hip) and their
autograd glue (preprocessor.stft_for_loss, objective.MultiResSTFT, pipeline.HeadFinetuneStep with that criterion) against the float64 closed
forms and restatement of tests/stft_grad_ref.py (themselves pinned by tests/test_stft_grad_host.py).

Bound of every gradient comparison: max |got - ref| < 1e-4 max |ref| per utterance (rows whose reference is all zero must be exactly zero) --
the fp32-path bar of DESIGN.md section 2, as tests/test_gpu_decode_grad.py; loss values 1e-4 relative; head gradients 1e-4 normwise; the
adjoint identity 1e-5.  The measured maxima are printed and logged (conftest.bounded)."""
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import decode_grad_ref as R      # noqa: E402
import stft_grad_ref as S      # noqa: E402
from conftest import bounded      # noqa: E402
from oracle import heads as oheads      # noqa: E402
from oracle import preprocessor as opre      # noqa: E402

pytestmark = pytest.mark.gpu

BOUND = 1e-4
DEV = torch.device('cuda:0')

# case: (sample_rate, win_ms, hop_ms, n_freq, n_mels, general plan)
CASES = {
    'fixed400': (16000, 25, 10, 201, 40, False),       # 400 / 160 / 201 through se_plan_create: the general tables built beside the 400-point ones
    'any400': (16000, 25, 10, 201, 40, True),          # the same geometry through se_plan_create_any
    'n512': (16000, 32, 8, 257, 40, True),             # 512 / 128 / 257
    'n200_8k': (8000, 25, 10, 101, 40, True),          # 200 / 80 / 101 at 8 kHz
    'short_window': (1000, 50, 20, 31, 10, True),      # n_fft 60, win 50, hop 20: win < n_fft
}
SIZES = ('border', 'ragged', 'short')
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


def _check(name, got, ref, bound=BOUND):
    e = _err(got, ref)
    print(f'{name}: {e:.3e}')
    bounded('stft_grad/' + name, e, bound)


def _T(case, size):
    """border: 2 chunk + 3 hops (two workgroup borders and a partial last workgroup); ragged: 2 chunk + 3 samples (no multiple of the hop);
    short: m + 1 (both folds on every interior sample)"""
    L, lib = _lib()
    g = _geom(case)
    chunk = lib.se_stft_bwd_chunk(_P(case)._plan(DEV))
    assert chunk >= g.hop and chunk % g.hop == 0
    return {'border': 2 * chunk + 3 * g.hop, 'ragged': 2 * chunk + 3, 'short': g.n_fft // 2 + 1}[size]


def _stft(case, wav):
    """se_stft_f32 on a (B, T) float32 device waveform -> power (B, F, K), complx (B, F, K, 2)"""
    from speech_enhancement_by_s3prl_amd.preprocessor import stft_for_loss
    return stft_for_loss(_P(case), wav, want_complx=True)


def _bwd(case, T, grad_power=None, grad_complx=None, complx=None, stride=None, fill=float('nan')):
    L, lib = _lib()
    plan = _P(case)._plan(DEV)
    g = _geom(case)
    F = T // g.hop + 1
    stride = T if stride is None else stride
    out = torch.full((B, stride), fill, device=DEV, dtype=torch.float32)
    nbytes = lib.se_stft_bwd_workspace_bytes(plan, B, T)
    ws = torch.full((max(1, nbytes),), 0xff, device=DEV, dtype=torch.uint8)       # NaN words: nothing may be read before it is written
    L.check(lib.se_stft_bwd_f32(plan, L.ptr(grad_power), L.ptr(grad_complx), L.ptr(complx), B, F, T, L.ptr(out), stride, L.ptr(ws), nbytes, L.stream()),
            'se_stft_bwd_f32')
    return out


@functools.lru_cache(maxsize=None)
def _data(case, size):
    """one seeded case, shared and left unchanged"""
    g = _geom(case)
    T = _T(case, size)
    F, K = T // g.hop + 1, g.n_freq
    gen = torch.Generator().manual_seed(sum(map(ord, case + size)))
    x = R.harmonic_batch(B, T, g.sample_rate, seed=sum(map(ord, case))).float() + 0.01 * torch.randn(B, T, generator=gen)
    G = torch.randn(B, F, K, 2, generator=gen)
    gp = torch.randn(B, F, K, generator=gen)
    return {'T': T, 'F': F, 'x': x, 'G': G, 'gp': gp}


@pytest.mark.parametrize('size', SIZES)
@pytest.mark.parametrize('case', list(CASES))
def test_adjoint_kernel_vs_closed_form(gpu, case, size):
    """1: grad_complx alone with an arbitrary G, and grad_power + complx with X from se_stft_f32 itself; every element compared"""
    d = _data(case, size)
    g, T = _geom(case), d['T']
    got = _bwd(case, T, grad_complx=d['G'].to(DEV))
    assert torch.isfinite(got).all()
    _check(f'1/{case}/{size}/complx', got, S.stft_bwd_closed(torch.view_as_complex(d['G'].double()), T, g))
    power, complx = _stft(case, d['x'].to(DEV))
    assert complx.shape == (B, d['F'], g.n_freq, 2)
    got = _bwd(case, T, grad_power=d['gp'].to(DEV), complx=complx)
    assert torch.isfinite(got).all()
    X = torch.view_as_complex(complx.double().cpu())
    _check(f'1/{case}/{size}/power', got, S.stft_bwd_closed(S.spectral_gradient(d['gp'].double(), None, X), T, g))
    both = _bwd(case, T, grad_power=d['gp'].to(DEV), grad_complx=d['G'].to(DEV), complx=complx)
    _check(f'1/{case}/{size}/both', both,
           S.stft_bwd_closed(S.spectral_gradient(d['gp'].double(), torch.view_as_complex(d['G'].double()), X), T, g))


@pytest.mark.parametrize('case', list(CASES))
def test_adjoint_identity(gpu, case):
    """2: <A u, G> = <u, A^T G> with A u the complx output of se_stft_f32 and A^T G from the new kernel: no oracle"""
    d = _data(case, 'ragged')
    u = d['x'].to(DEV)
    _, Au = _stft(case, u)
    ATG = _bwd(case, d['T'], grad_complx=d['G'].to(DEV))
    Au64, G64, u64, ATG64 = Au.double().cpu(), d['G'].double(), u.double().cpu(), ATG.double().cpu()
    lhs, rhs = (Au64 * G64).sum().item(), (u64 * ATG64).sum().item()
    scale = ((Au64 * Au64).sum() * (G64 * G64).sum()).sqrt().item()
    print(f'2/{case}: |<Au,G> - <u,ATG>| / sqrt(<Au,Au><G,G>) = {abs(lhs - rhs) / scale:.3e}')
    bounded(f'stft_grad/2/{case}', abs(lhs - rhs) / scale, 1e-5)


@pytest.mark.parametrize('case', list(CASES))
def test_exactness(gpu, case):
    """3: zero fill past T, bit-identical repeats, and a zeroed block of frames changes nothing outside the samples those frames cover"""
    d = _data(case, 'border')
    g, T, F = _geom(case), d['T'], d['F']
    m = g.n_fft // 2
    G = d['G'].to(DEV)
    a = _bwd(case, T, grad_complx=G, stride=T + 37)
    b = _bwd(case, T, grad_complx=G, stride=T + 37, fill=1.0)
    assert (a[:, T:] == 0).all() and torch.equal(a, b)
    assert torch.equal(a[:, :T], _bwd(case, T, grad_complx=G))
    f1, f2 = F // 2 - 2, F // 2 + 2                         # interior frames: their samples [hop f1 - m, hop (f2 - 1) + m) touch neither fold
    lo, hi = g.hop * f1 - m, g.hop * (f2 - 1) + m
    assert lo > m and hi < T - 1 - m
    G2 = G.clone()
    G2[:, f1:f2] = 0
    c = _bwd(case, T, grad_complx=G2)
    assert torch.equal(c[:, :lo], a[:, :lo]) and torch.equal(c[:, hi:], a[:, hi:T])
    assert not torch.equal(c[:, lo:hi], a[:, lo:hi])


# ---- the criterion ------------------------------------------------------------------------------------------------------------------------
T_MR = 4800
LENGTHS_MR = (4800, 3001, 1300, 0)
# harmonic_batch plus white noise at 5 dB, times 8: at harmonic_batch's own level (0.1) no seed of 6000 kept every counted bin of both signals
# 100 x above the clamp (the best floor was 8e-7); the criterion does not depend on a common gain except through the clamp
SEED_MR, GAIN_MR = 5380, 8.0


@functools.lru_cache(maxsize=None)
def _mr():
    tar, pred = S.noisy_pair(4, T_MR, 16000, SEED_MR, gain=GAIN_MR)
    tar, pred = tar.float(), pred.float()
    # the clamp branch cannot hide a mismatch: every counted bin of both signals is 100 x above the clamp in the float64 restatement
    floor = S.counted_power_floor(pred.double(), tar.double(), LENGTHS_MR)
    assert floor >= 100 * S.CLAMP, floor
    w = pred.double().requires_grad_(True)
    loss = S.multires_loss(w, tar.double(), LENGTHS_MR)
    loss.backward()
    return {'tar': tar, 'pred': pred, 'loss': loss.item(), 'grad': w.grad}


def test_multires_loss_and_gradient(gpu):
    """4: ragged batch with an empty utterance at the default three resolutions"""
    from speech_enhancement_by_s3prl_amd.objective import MultiResSTFT
    d = _mr()
    lengths = torch.tensor(LENGTHS_MR)
    s = d['pred'].to(DEV).requires_grad_(True)
    loss, extra = MultiResSTFT()(wav_predicted=s, wav_tar=d['tar'].to(DEV), lengths=lengths.to(DEV))
    assert extra == {}
    loss.backward()
    print(f'4/loss: {abs(loss.item() - d["loss"]) / abs(d["loss"]):.3e}')
    bounded('stft_grad/4/loss', abs(loss.item() - d['loss']) / abs(d['loss']), BOUND)
    _check('4/grad', s.grad, d['grad'])
    for b, n in enumerate(LENGTHS_MR):
        assert (s.grad[b, n:] == 0).all()
    assert (s.grad[3] == 0).all()
    loss2, _ = MultiResSTFT()(wav_predicted=d['pred'].to(DEV), wav_tar=d['tar'].to(DEV), length_masks=(torch.arange(T_MR)[None] < lengths[:, None]).to(DEV))
    assert loss2.grad_fn is None and torch.equal(loss2, loss.detach())      # the plain forward, and the reference's mask signature


def test_multires_silent_interval(gpu):
    """5: wav_predicted exactly 0 over [1500, 3600), which holds whole frames at every resolution: finite everywhere, and exactly 0 on the
    samples that only such frames cover ([2560, 2816): the 1024-point frames 9 .. 12 span [1792, 3584))"""
    from speech_enhancement_by_s3prl_amd.objective import MultiResSTFT
    d = _mr()
    pred = d['pred'].clone()
    pred[:, 1500:3600] = 0.0
    s = pred.to(DEV).requires_grad_(True)
    loss, _ = MultiResSTFT()(wav_predicted=s, wav_tar=d['tar'].to(DEV), lengths=torch.tensor(LENGTHS_MR).to(DEV))
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(s.grad).all()
    assert (s.grad[:, 2560:2816] == 0).all()
    assert s.grad[0].abs().max() > 0 and s.grad[1].abs().max() > 0
    for b, n in enumerate(LENGTHS_MR):
        assert (s.grad[b, n:] == 0).all()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _e2e():
    """a ragged 3-utterance batch of about 0.3 s with its preprocessor, head state and float64 chain result"""
    from speech_enhancement_by_s3prl_amd import pipeline
    from speech_enhancement_by_s3prl_amd.heads import LinearResidual
    T = 4850
    gen = torch.Generator().manual_seed(41)
    clean = R.harmonic_batch(B, T, 16000, seed=43).float()
    wavs = torch.stack([clean + 0.02 * torch.randn(B, T, generator=gen), clean + 0.01 * torch.randn(B, T, generator=gen)], dim=1).contiguous()
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
    rloss = S.multires_loss(rwav, wavs[:, 1].double(), lengths.tolist())
    rloss.backward()
    return {'wavs': wavs, 'lengths': lengths, 'pre': pre, 'state': state, 'rloss': rloss.item(), 'gw': w.grad, 'gb': b.grad}


def _head(state):
    from speech_enhancement_by_s3prl_amd.heads import LinearResidual
    head = LinearResidual(input_size=120, output_size=201, activation='Sigmoid', cmvn=True)
    head.load_state_dict(state)
    return head.to(DEV)


def _normwise(got, ref):
    got, ref = got.detach().double().cpu(), ref.double()
    return ((got - ref).norm() / ref.norm()).item()


def test_end_to_end_head_gradient(gpu):
    """6: pipeline.HeadFinetuneStep with criterion = MultiResSTFT(): features -> LinearResidual -> decode_wav -> the three transforms -> loss"""
    from speech_enhancement_by_s3prl_amd import decode, pipeline
    from speech_enhancement_by_s3prl_amd.objective import MultiResSTFT
    from speech_enhancement_by_s3prl_amd.solver import get_optimizer
    e = _e2e()
    pre, wavs, lengths = e['pre'], e['wavs'].to(DEV), e['lengths'].to(DEV)
    head = _head(e['state'])
    with torch.no_grad():
        feats_up, feats_down, lin_inp, ph_inp, lin_tar, ph_tar = pre(wavs)
    predicted, _ = head(features=feats_down, linears=lin_inp)
    wav_tar = wavs[:, 1, :]
    wav = decode.decode_wav(pre, predicted, ph_inp, lengths, wav_tar)
    loss, _ = MultiResSTFT()(wav_predicted=wav, wav_tar=wav_tar, lengths=lengths)
    loss.backward()
    e_loss = abs(loss.item() - e['rloss']) / abs(e['rloss'])
    e_w, e_b = _normwise(head.linear.weight.grad, e['gw']), _normwise(head.linear.bias.grad, e['gb'])
    print(f'6/loss: {e_loss:.3e}  6/weight: {e_w:.3e}  6/bias: {e_b:.3e}')
    bounded('stft_grad/6/loss', e_loss, BOUND)
    bounded('stft_grad/6/weight', e_w, BOUND)
    bounded('stft_grad/6/bias', e_b, BOUND)
    head2 = _head(e['state'])
    opt = get_optimizer(list(head2.named_parameters()), lr=1e-4, warmup_proportion=0.1, training_steps=100)
    step = pipeline.HeadFinetuneStep(pre, head2, opt, criterion=MultiResSTFT())
    loss2, grad_norm, skipped = step(wavs, lengths)
    assert not skipped and grad_norm > 0
    assert abs(loss2.item() - loss.item()) <= 1e-6 * abs(loss.item())
    loss3, grad_norm3, skipped3 = step(wavs, lengths)              # a second step runs on the same objects (the learning rate warms up from 0)
    assert not skipped3 and grad_norm3 > 0 and torch.isfinite(loss3)
