"""GPU parity of the GENERAL STFT / iSTFT path (se_plan_create_any: csrc/stftg.hip, csrc/istftg.hip) over seven geometries, against the CPU
oracle (oracle/preprocessor.py, geometry-general) and a float64 framed DFT.  Tolerances are those of the 400-point path
(tests/test_gpu_preprocessor.py): _relmax < 1e-4 on power, complex spectra and waveforms, 2e-3 absolute on log-mel with deltas, 5e-3 on
CMVN'd features, 1e-5 against the float64 DFT.

Each geometry runs at two lengths: T = 3 n_fft + 7 (every frame touches the reflect padding, T is no multiple of the hop) and a T that gives
2 FR + 3 frames for that plan's frames-per-workgroup FR (interior workgroups, a partial last one, the iSTFT halo)."""
import functools

import numpy as np
import pytest
import torch

from oracle import decode as odec
from oracle import heads as oheads
from oracle import objective as oobj
from oracle import preprocessor as opre

pytestmark = pytest.mark.gpu

# case: (sample_rate, win_ms, hop_ms, n_freq, n_mels) -- millisecond values that give exact sample counts.  n_mels is 40 where every one of 40
# HTK filters has a bin under it; the two toy geometries take as many filters as their 17 / 31 bins fill (an empty filter is a constant
# log(eps) column, whose CMVN is 0 / 0 in the oracle and in the kernels alike)
CASES = {
    'a': (1000, 32, 8, 17, 6),          # 32 / 32 / 8: smallest m, radix 4 only
    'b': (1000, 50, 20, 31, 10),        # 60 / 50 / 20: radices 2 3 5, zero-padded centred window
    'c': (8000, 25, 10, 101, 40),       # 200 / 200 / 80: the 8 kHz config
    'd': (16000, 20, 10, 161, 40),      # 320 / 320 / 160
    'e': (16000, 25, 10, 201, 40),      # 400 / 400 / 160: the general path at the default geometry
    'f': (16000, 32, 8, 257, 40),       # 512 / 512 / 128: wide mel triangles (up to 33 bins, past the specialised plan's 32)
    'g': (16000, 64, 16, 513, 40),      # 1024 / 1024 / 256: LDS ceiling (triangles up to 65 bins)
}
B, C = 3, 2


def _relmax(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().flatten(1).max(dim=1).values / b.abs().flatten(1).max(dim=1).values).max().item()


def _geom(case):
    sr, win_ms, hop_ms, n_freq, n_mels = CASES[case]
    return opre.Geometry(sample_rate=sr, win_ms=win_ms, hop_ms=hop_ms, n_freq=n_freq, n_mels=n_mels)


@functools.lru_cache(maxsize=None)
def _P(case):
    from speech_enhancement_by_s3prl_amd.preprocessor import OnlinePreprocessor
    sr, win_ms, hop_ms, n_freq, n_mels = CASES[case]
    p = OnlinePreprocessor(sample_rate=sr, win_ms=win_ms, hop_ms=hop_ms, n_freq=n_freq, n_mels=n_mels, n_mfcc=13)
    p.general_plan = True                 # case e: the general kernels, not the specialised 400-point ones
    return p.to(torch.device('cuda:0'))


def _lengths(case):
    """(T touching the padding everywhere, T giving 2 FR + 3 frames)"""
    from speech_enhancement_by_s3prl_amd import _lib
    P, g = _P(case), _geom(case)
    fr = _lib.load().se_plan_chunk_frames(P._plan(torch.device('cuda:0')), 0)
    assert fr >= 1
    t2 = (2 * fr + 2) * g.hop + g.hop // 2
    assert t2 // g.hop + 1 == 2 * fr + 3 and t2 <= 40000 and t2 > g.n_fft // 2
    return 3 * g.n_fft + 7, t2


@functools.lru_cache(maxsize=None)
def _data(case, which):
    """one batch per (case, length) with its oracle spectra, shared by the tests and left unchanged"""
    g = _geom(case)
    T = _lengths(case)[which]
    gen = torch.Generator().manual_seed(1000 * ord(case) + which)
    wavs = torch.randn(B, C, T, generator=gen) * 0.1
    fl = [opre.get_feat_config('linear', 0), opre.get_feat_config('phase', 0), opre.get_feat_config('linear', 1), opre.get_feat_config('phase', 1)]
    ref = opre.forward(wavs, fl, g)
    return wavs, ref


ALL = [(c, w) for c in CASES for w in (0, 1)]


def _feat_list():
    return [
        {'feat_type': 'mel', 'channel': 0, 'log': True, 'delta': 2, 'cmvn': True},
        {'feat_type': 'mel', 'channel': 1, 'log': True, 'delta': 2, 'cmvn': False},
        {'feat_type': 'mel', 'channel': 0, 'log': False, 'delta': 0, 'cmvn': False},
        opre.get_feat_config('linear', 0), opre.get_feat_config('phase', 0),
        opre.get_feat_config('linear', 1), opre.get_feat_config('phase', 1),
        opre.get_feat_config('complx', 1),
        opre.get_feat_config('mfcc', 0), opre.get_feat_config('mfcc', 1, delta=2, cmvn=True),
    ]


@pytest.mark.parametrize('case,which', ALL)
def test_features_vs_oracle(gpu, case, which):
    """1: every feature type through OnlinePreprocessor.forward (complx in the list: the eager atan2 path, se_stft2_f32)"""
    P, g = _P(case), _geom(case)
    wavs, _ = _data(case, which)
    fl = _feat_list()
    feats = P(wavs.to(gpu), fl)
    ref = opre.forward(wavs, fl, g)
    F = wavs.shape[-1] // g.hop + 1
    assert [tuple(f.shape) for f in feats] == [tuple(r.shape) for r in ref]
    assert feats[3].shape == (B, F, g.n_freq)
    assert _relmax(feats[3], ref[3]) < 1e-4 and _relmax(feats[5], ref[5]) < 1e-4
    for lin, ph, rlin, rph in ((feats[3], feats[4], ref[3], ref[4]), (feats[5], feats[6], ref[5], ref[6])):
        z = torch.polar(lin.cpu().double().sqrt(), ph.cpu().double())          # phase through the phasor, not per-bin angles
        rz = torch.polar(rlin.double().sqrt(), rph.double())
        assert ((z - rz).abs().flatten(1).max(dim=1).values / rz.abs().flatten(1).max(dim=1).values).max().item() < 1e-4
    assert _relmax(feats[7], ref[7]) < 1e-4                                     # complx (B, F, 2 K)
    assert _relmax(feats[2], ref[2]) < 1e-4                                     # raw mel
    assert (feats[1].cpu() - ref[1]).abs().max().item() < 2e-3                  # log-mel + deltas
    assert (feats[0].cpu() - ref[0]).abs().max().item() < 5e-3                  # CMVN'd
    assert torch.isfinite(feats[0]).all()
    scale = ref[8].abs().max().item()
    assert (feats[8].cpu() - ref[8]).abs().max().item() < 2e-4 * scale          # raw cepstra (test_mfcc_vs_oracle's bound)
    assert (feats[9].cpu() - ref[9]).abs().max().item() < 5e-3


def _dft64_power(x, g):
    """float64 framed DFT built here: reflect padding, periodic Hann of length win centred in n_fft, one-sided power (F, K)"""
    x = np.asarray(x, dtype=np.float64)
    xp = np.pad(x, g.n_fft // 2, mode='reflect')
    n = np.arange(g.win)
    w = np.zeros(g.n_fft)
    left = (g.n_fft - g.win) // 2
    w[left:left + g.win] = 0.5 - 0.5 * np.cos(2 * np.pi * n / g.win)
    F = len(x) // g.hop + 1
    frames = np.stack([xp[f * g.hop:f * g.hop + g.n_fft] * w for f in range(F)])
    t = np.arange(g.n_fft)
    D = np.exp(-2j * np.pi * np.outer(t, np.arange(g.n_freq)) / g.n_fft)
    return np.abs(frames @ D) ** 2


@pytest.mark.parametrize('case', list(CASES))
def test_power_vs_float64_dft(gpu, case):
    """2: noise and a pure tone on a bin centre against the float64 DFT"""
    P, g = _P(case), _geom(case)
    wavs, _ = _data(case, 1)
    lin, = P(wavs.to(gpu), [P.get_feat_config('linear', 0)])
    ref = torch.from_numpy(_dft64_power(wavs[0, 0].numpy(), g))
    assert _relmax(lin.cpu()[0:1], ref[None]) < 1e-5
    k = g.n_freq // 3
    T = 8 * g.n_fft                                           # long enough for frames clear of the reflect padding at every hop
    tone = torch.cos(2 * np.pi * k * torch.arange(T, dtype=torch.float64) / g.n_fft).float().view(1, 1, -1)
    lin, = P(tone.to(gpu), [P.get_feat_config('linear', 0)])
    ref = torch.from_numpy(_dft64_power(tone[0, 0].numpy(), g))
    assert _relmax(lin.cpu(), ref[None]) < 1e-5
    lo, hi = g.n_fft // g.hop + 1, lin.shape[1] - g.n_fft // g.hop - 1            # frames clear of the padding
    mid = lin[0, lo:hi].cpu()
    assert mid.shape[0] >= 1 and (mid.argmax(dim=-1) == k).all()
    if g.win == g.n_fft:        # periodic Hann: |X[k]| = sum(w) / 2 = n_fft / 4
        assert torch.allclose(mid[:, k], torch.full_like(mid[:, k], (g.n_fft / 4.0) ** 2), rtol=1e-4)


def _decode_words(word):
    t = word.view(torch.float32).double()
    sgn = 1.0 - 2.0 * (word & 1).double()
    return t, torch.view_as_complex(torch.stack([sgn * (1 - t * t) / (1 + t * t), 2 * t / (1 + t * t)], dim=-1).contiguous())


@pytest.mark.parametrize('case,which', ALL)
def test_encoded_phase_and_round_trip(gpu, case, which):
    """3 + 4: se_stft_tphase_f32 (|t| <= 1, decoded phasor vs the oracle) and iSTFT(STFT(x)) = x through both inverse entries"""
    from speech_enhancement_by_s3prl_amd.preprocessor import LazyPhase
    P, g = _P(case), _geom(case)
    wavs, ref = _data(case, which)
    fl = [P.get_feat_config('linear', 0), P.get_feat_config('phase', 0), P.get_feat_config('linear', 1), P.get_feat_config('phase', 1)]
    P.channel_inp = 0
    f = P(wavs.to(gpu), fl)
    assert type(f[1]) is LazyPhase and f[1]._tphase is not None
    assert _relmax(f[0], ref[0]) < 1e-4 and _relmax(f[2], ref[2]) < 1e-4
    t, ph = _decode_words(f[1]._tphase.cpu())
    assert t.abs().max().item() <= 1.0 + 1e-6
    z = ph * f[0].cpu().double().sqrt()
    rz = torch.polar(ref[0].double().sqrt(), ref[1].double())
    assert ((z - rz).abs().flatten(1).max(dim=1).values / rz.abs().flatten(1).max(dim=1).values).max().item() < 1e-4
    n_out = g.hop * (wavs.shape[-1] // g.hop)
    wav = P.istft(f[0], f[1])                                   # the encoded-phase entry
    assert f[1]._value is None and wav.shape == (B, n_out)
    assert _relmax(wav.cpu(), wavs[:, 0, :n_out]) < 1e-4
    wav2 = P.istft(f[2], f[3] + 0)                              # the atan2 entry (a plain tensor), other channel
    assert _relmax(wav2.cpu(), wavs[:, 1, :n_out]) < 1e-4


@pytest.mark.parametrize('case,which', ALL)
def test_istft_masked_vs_oracle(gpu, case, which):
    """5: a masked spectrum through se_istft_f32, se_istft_tphase_f32 and its log_input form, with the fused masked square sum, a padded
    output row and ragged lengths.  The oracle call (torch.istft) raises on a NOLA violation: the geometry is legal."""
    P, g = _P(case), _geom(case)
    wavs, ref = _data(case, which)
    T = wavs.shape[-1]
    gen = torch.Generator().manual_seed(7)
    pred = ref[0] * torch.rand(ref[0].shape, generator=gen)
    rwav = opre.istft(pred, ref[1], g)
    n_out = g.hop * (T // g.hop)
    assert rwav.shape == (B, n_out)
    lengths = torch.tensor([T, T // 2 + 1, n_out - 1])
    mask = (torch.arange(n_out)[None] < lengths[:, None]).double()
    rs = (rwav.double().pow(2) * mask).sum(dim=1)
    P.channel_inp = 0
    fl = [P.get_feat_config('linear', 0), P.get_feat_config('phase', 0)]
    f = P(wavs.to(gpu), fl)
    eager = f[1] + 0
    # atan2-phase entry
    wav, ss = P.istft_with_sumsq(pred.to(gpu), eager, lengths=lengths.to(gpu), out_len=T)
    assert wav.shape == (B, T) and _relmax(wav[:, :n_out], rwav) < 1e-4 and (wav[:, n_out:] == 0).all()
    assert ((ss.cpu().double() - rs).abs() / rs).max().item() < 1e-4
    # encoded-phase entry, with the reference's square sum in the same launch
    tgt = wavs[:, 1].to(gpu).contiguous()
    wav, ss, rss = P._istft_tphase(pred.to(gpu), f[1]._tphase, lengths.to(gpu), T, ref=tgt)
    assert _relmax(wav[:, :n_out], rwav) < 1e-4 and (wav[:, n_out:] == 0).all()
    assert ((ss.cpu().double() - rs).abs() / rs).max().item() < 1e-4
    full = (torch.arange(T)[None] < lengths[:, None]).double()
    rr = (wavs[:, 1].double().pow(2) * full).sum(dim=1)
    assert rss is not None and ((rss.cpu().double() - rr).abs() / rr).max().item() < 1e-4
    # log_input = 1: the plane holds log(predicted)
    logp = (pred + 1e-20).log()
    wav, ss = P._istft_tphase(logp.to(gpu), f[1]._tphase, lengths.to(gpu), T, log_input=True)
    assert _relmax(wav[:, :n_out], rwav) < 1e-4
    assert ((ss.cpu().double() - rs).abs() / rs).max().item() < 1e-4
    # linear_power != 2
    rw3 = opre.istft(pred, ref[1], g, linear_power=3)
    assert _relmax(P.istft(pred.to(gpu), eager, linear_power=3), rw3) < 1e-4


@pytest.mark.parametrize('which', [0, 1])
def test_general_vs_specialised_kernels(gpu, which):
    """6: case e, the two kernel families on the same input: different summation orders of the same transform"""
    from speech_enhancement_by_s3prl_amd.preprocessor import OnlinePreprocessor
    G = _P('e')
    S = OnlinePreprocessor().to(gpu)
    wavs, _ = _data('e', which)
    fl = [G.get_feat_config('linear', 0), G.get_feat_config('phase', 0)]
    G.channel_inp = S.channel_inp = 0
    fg, fs = G(wavs.to(gpu), fl), S(wavs.to(gpu), fl)
    assert _relmax(fg[0], fs[0]) < 1e-4
    mask = torch.rand(fg[0].shape, generator=torch.Generator().manual_seed(3)).to(gpu)
    assert _relmax(G.istft(fs[0] * mask, fg[1]), S.istft(fs[0] * mask, fs[1])) < 1e-4
    assert _relmax(G.istft(fs[0] * mask, fg[1] + 0), S.istft(fs[0] * mask, fs[1] + 0)) < 1e-4


def test_evaluate_pass_8khz(gpu):
    """7, case c: features -> LinearResidual(D, 101, 'Sigmoid') -> mask x noisy power -> decode_wav (iSTFT + dB normalisation), ragged"""
    from speech_enhancement_by_s3prl_amd.decode import decode_wav
    from speech_enhancement_by_s3prl_amd.heads import LinearResidual
    P, g = _P('c'), _geom('c')
    wavs, _ = _data('c', 1)
    T = wavs.shape[-1]
    lengths = torch.tensor([T, T - 333, T // 2])
    fl = [{'feat_type': 'mel', 'channel': 0, 'log': True, 'delta': 2, 'cmvn': False}, P.get_feat_config('linear', 0), P.get_feat_config('phase', 0)]
    P.channel_inp = 0
    feats, lin, ph = P(wavs.to(gpu), fl)
    rfeats, rlin, rph = opre.forward(wavs, fl, g)
    torch.manual_seed(0)
    head = LinearResidual(input_size=120, output_size=101, activation='Sigmoid', cmvn=True)
    rpred, _ = oheads.linear_residual(rfeats, rlin, head.linear.weight.detach(), head.linear.bias.detach())
    head = head.to(gpu)
    with torch.no_grad():
        pred, _ = head(features=feats, linears=lin)
    assert ((pred.cpu() - rpred).abs().max() / rpred.abs().max()).item() < 1e-4
    for target, rtarget in ((-25, -25), (wavs[:, 1].to(gpu), wavs[:, 1])):
        got = decode_wav(P, pred, ph, lengths.to(gpu), target)
        rdec = odec.decode_wav(rpred, rph, lengths, g, rtarget)
        assert got.shape == rdec.shape
        assert ((got.cpu() - rdec).abs().max() / rdec.abs().max()).item() < 1e-4


def test_criteria_257_bins_and_the_mask_head_limit(gpu):
    """7, case f: the preprocessor and the L1 / SISDR criteria at 257 bins; LinearResidual (N <= 256) refuses loudly"""
    from speech_enhancement_by_s3prl_amd import _lib
    from speech_enhancement_by_s3prl_amd.decode import get_length_masks
    from speech_enhancement_by_s3prl_amd.heads import LinearResidual
    from speech_enhancement_by_s3prl_amd.objective import L1, SISDR
    P, g = _P('f'), _geom('f')
    wavs, ref = _data('f', 1)
    fl = [P.get_feat_config('linear', 0), P.get_feat_config('linear', 1)]
    lin, tar = P(wavs.to(gpu), fl)
    assert lin.shape[-1] == 257 and _relmax(tar, ref[2]) < 1e-4
    F = lin.shape[1]
    frames = torch.tensor([F, F - 2, F // 2])
    masks = get_length_masks(frames.to(gpu), F)
    rmasks = odec.get_length_masks(frames, F)
    lp = (lin * 0.5 + 1e-3).log()
    rlp = (ref[0] * 0.5 + 1e-3).log()
    loss, _ = L1()(log_predicted=lp, linear_tar=tar, stft_length_masks=masks)
    rloss = oobj.l1(rlp, ref[2], rmasks)
    assert abs(loss.item() - rloss.item()) < 1e-4 * abs(rloss.item())
    noise = 0.5 + torch.rand(ref[2].shape, generator=torch.Generator().manual_seed(4))           # an estimate some dB off the target
    with torch.no_grad():
        sloss, _ = SISDR()(predicted=tar * noise.to(gpu), linear_tar=tar, stft_length_masks=masks)
    rsloss = oobj.sisdr_objective(ref[2] * noise, ref[2], rmasks)
    assert abs(rsloss.item()) > 1.0 and abs(sloss.item() - rsloss.item()) < 1e-4 * abs(rsloss.item())
    with pytest.raises(_lib.SEError):
        LinearResidual(input_size=257, output_size=257).to(gpu)(features=lin, linears=lin)


def test_unsupported_geometry_names_the_rule(gpu):
    """8"""
    from speech_enhancement_by_s3prl_amd import _lib
    from speech_enhancement_by_s3prl_amd.preprocessor import OnlinePreprocessor
    for n_freq, frag in ((8, 'factor 7'), (36, 'factor 7')):
        p = OnlinePreprocessor(sample_rate=1000, win_ms=2 * (n_freq - 1), hop_ms=(n_freq - 1) // 2, n_freq=n_freq).to(gpu)
        with pytest.raises(_lib.SEError, match=frag):
            p(torch.randn(1, 1, 500, device=gpu), [p.get_feat_config('linear', 0)])


def test_zero_arg_probe_and_stft_attr(gpu):
    """the dimension probe and the sampler's _stft surface at another geometry"""
    P, g = _P('f'), _geom('f')
    feats = P(None, [P.get_feat_config('linear', 0), {'feat_type': 'mel', 'channel': 0, 'log': True, 'delta': 2, 'cmvn': True},
                     P.get_feat_config('mfcc', 0, delta=1)])
    assert [f.shape[-1] for f in feats] == [257, 120, 26] and feats[0].shape[:2] == (1, 16000 // 128 + 1)
    wav = torch.randn(2, 3000, generator=torch.Generator().manual_seed(2))
    c = P._stft(wav.to(gpu))
    assert c.shape == (2, 257, 3000 // 128 + 1, 2)
    rc = opre.stft(wav, g)
    assert _relmax(torch.view_as_complex(c.cpu().contiguous()).abs().transpose(1, 2), rc.abs().transpose(1, 2)) < 1e-4
