"""Runs STFT + iSTFT a few times at batch B (for rocprofv3 --pmc passes):   python tools/one_stft.py B

With a geometry it measures instead:   python tools/one_stft.py B --n-fft 512 --hop 128 [--win 512] [--general] [--seconds 10] [--out FILE]
time per launch (HIP events around `--repeats` back-to-back launches, after `--warmup` launches, median of `--rounds` rounds) and the fraction
of 8 TB/s that the launch's algorithmic bytes amount to, for the forward transform (one channel: power + phase planes) and the inverse one
(power + phase -> waveform).  --general forces the general kernels at 400 / 160 (the specialised ones are the default there)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speech_enhancement_by_s3prl_amd.preprocessor import OnlinePreprocessor  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('B', nargs='?', type=int, default=256)
ap.add_argument('--n-fft', type=int, default=None)
ap.add_argument('--hop', type=int, default=None)
ap.add_argument('--win', type=int, default=None)
ap.add_argument('--sample-rate', type=int, default=16000)
ap.add_argument('--seconds', type=float, default=10.0)
ap.add_argument('--general', action='store_true')
ap.add_argument('--warmup', type=int, default=10)
ap.add_argument('--repeats', type=int, default=20)
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--out', default=None)
a = ap.parse_args()
dev = torch.device('cuda:0')

if a.n_fft is None:
    P = OnlinePreprocessor().to(dev)
    wavs = torch.randn(a.B, 2, 160000, device=dev) * 0.1
    fl = [P.get_feat_config('linear', 0), P.get_feat_config('phase', 0)]
    for _ in range(4):
        lin, ph = P(wavs, fl)
        wav = P.istft(lin, ph)
    torch.cuda.synchronize()
    sys.exit(0)

sr = a.sample_rate
hop = a.hop or a.n_fft // 4
win = a.win or a.n_fft
P = OnlinePreprocessor(sample_rate=sr, win_ms=1000.0 * win / sr, hop_ms=1000.0 * hop / sr, n_freq=a.n_fft // 2 + 1).to(dev)
P.general_plan = a.general
P.lazy_phase = False
assert P._win_args == {'n_fft': a.n_fft, 'hop_length': hop, 'win_length': win}, P._win_args
T = int(a.seconds * sr)
wavs = torch.randn(a.B, 1, T, device=dev) * 0.1
fl = [P.get_feat_config('linear', 0), P.get_feat_config('phase', 0)]
lin, ph = P(wavs, fl)
F, K = lin.shape[1:]


def timed(fn):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.repeats):
            fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1000.0 / a.repeats)
    return statistics.median(us), min(us), max(us)


fwd = timed(lambda: P(wavs, fl))
inv = timed(lambda: P.istft(lin, ph))
fwd_bytes = a.B * (4.0 * T + 8.0 * F * K)
inv_bytes = a.B * (8.0 * F * K + 4.0 * hop * (F - 1))
res = {'geometry': {'n_fft': a.n_fft, 'win': win, 'hop': hop, 'n_freq': K}, 'kernels': 'general' if (a.general or not (K == 201 and hop == 160)) else 'specialised',
       'B': a.B, 'T': T, 'frames': F, 'method': f'HIP events around {a.repeats} launches, {a.warmup} warm-up, median of {a.rounds} rounds (min, max beside it); '
       'includes the output allocations of the Python wrapper',
       'stft_us': [round(v, 1) for v in fwd], 'stft_frac_of_8TBs': round(fwd_bytes / (fwd[0] * 1e-6) / 8e12, 4),
       'istft_us': [round(v, 1) for v in inv], 'istft_frac_of_8TBs': round(inv_bytes / (inv[0] * 1e-6) / 8e12, 4)}
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'a') as fh:
        fh.write(line + '\n')
