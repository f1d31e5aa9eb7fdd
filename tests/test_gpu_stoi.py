"""GPU: se_stoi_f32 (csrc/stoi.hip) through evaluation.stoi_batch / stoi_eval / estoi_eval / MetricStage against the numpy float64 restatement
of the same definition (tests/stoi_ref.py).  Parity unpinned vs pystoi, which is not installed.

Signals: seeded speech-like noise (low-passed noise under a 4 Hz envelope) with one or two stretches 65 dB down, so that frames really are
dropped; processed = clean + white noise at 5 dB SNR.  Both are rounded to fp32 first: the restatement sees exactly what the kernels see.
Before any GPU compare the restatement alone must show, per utterance, a margin of at least 0.05 dB between every frame energy and the keep
threshold (a rounding flip could otherwise hide or fake an error) and, where a stretch was turned down, at least one dropped frame with kept
frames on both sides.

Partitions the shapes straddle (constants of csrc/stoi.hip): resampler 256 outputs per workgroup, energy kernel 16 frames per workgroup, mask
kernel scan chunks of 256 frames, band kernel 4 compacted frames per workgroup, score kernel 4 segments per workgroup.  The straddle case has
311 frames (two scan chunks, frames dropped in both, 311 % 16 != 0), a kept count and a segment count that are no multiples of 4.

Bounds (`bounded`, ~2x the values measured on an MI355X; none may exceed the project's 1e-4):
  envelopes, relative to the utterance's envelope maximum   measured 6.9e-8 ... 1.29e-7   bound 3e-7
  score, absolute (STOI and ESTOI, and |score - 1| on       measured 0 ... 2.74e-8       bound 6e-8
  identical signals)
The score is float64 arithmetic on the fp32 envelopes, written as an fp32 in [0.5, 1): half an ulp is 3e-8, which is what is measured."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import stoi_ref as R      # noqa: E402
from conftest import bounded      # noqa: E402

pytestmark = pytest.mark.gpu

TOB_BOUND = 3e-7
SCORE_BOUND = 6e-8
MIN_MARGIN_DB = 0.05
SCAN_CHUNK, BAND_FRAMES, SCORE_SEGMENTS, ENERGY_FRAMES = 256, 4, 4, 16

# name -> (sr, T, lengths or None, per utterance (seed, gaps in input samples))
CASES = {
    'ragged': (16000, 16000, [16000, 9001, 4800], [(11, [(6000, 9000)]), (12, [(2500, 4200)]), (13, [(1500, 2500)])]),
    'straddle': (16000, 64000, [64000], [(21, [(9000, 13000), (56000, 59500)])]),
    'same_rate': (10000, 12000, [12000, 7777], [(31, [(4000, 6000)]), (32, [(1000, 2200), (5000, 6000)])]),
    'no_lengths': (16000, 16000, None, [(41, [(3000, 5500)]), (42, [(10000, 12500)])]),
    'empty': (16000, 16000, [16000, 0, -5], [(51, [(7000, 9500)]), (52, []), (53, [])]),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (clean (B, T) fp32, processed (B, T) fp32, lengths, sr, refs[b][extended]) computed once and shared; the CPU-side conditions hold"""
    sr, T, lengths, utts = CASES[name]
    clean = np.stack([R.speechlike(seed, T, sr, gaps) for seed, gaps in utts]).astype(np.float32)
    proc = np.stack([R.add_noise(c.astype(np.float64), 5.0, 1000 + seed) for c, (seed, _) in zip(clean, utts)]).astype(np.float32)
    refs = []
    for b, (seed, gaps) in enumerate(utts):
        n = T if lengths is None else min(max(lengths[b], 0), T)
        r = [R.stoi_full(clean[b, :n].astype(np.float64), proc[b, :n].astype(np.float64), sr, ext) for ext in (False, True)]
        if r[0]['frames']:
            assert r[0]['margin'] >= MIN_MARGIN_DB, (name, b, r[0]['margin'])
            mask = r[0]['mask']
            if gaps:
                dropped = np.nonzero(~mask)[0]
                assert len(dropped) >= 1 and mask[:dropped[0]].any() and mask[dropped[-1] + 1:].any(), (name, b, mask)
        refs.append(r)
    return torch.from_numpy(clean), torch.from_numpy(proc), lengths, sr, refs


def test_case_shapes_are_the_ones_the_partitions_need():
    _, _, _, _, refs = case('ragged')
    assert [r[0]['frames'] for r in refs] == [77, 42, 22] and refs[2][0]['score'] == 1e-5
    r = case('straddle')[4][0][0]
    assert r['frames'] == 311 > SCAN_CHUNK and r['frames'] % ENERGY_FRAMES != 0
    assert (~r['mask'][:SCAN_CHUNK]).any() and (~r['mask'][SCAN_CHUNK:]).any()          # drops in both scan chunks: the second chunk's base is not its index
    assert r['K'] % BAND_FRAMES != 0 and (r['K'] - 29) % SCORE_SEGMENTS != 0
    assert R.n10_of(64000, 5, 8) % 256 != 0                                              # the resampler's last workgroup is partial
    assert [r[0]['frames'] for r in case('empty')[4]] == [77, 0, 0]


@pytest.mark.parametrize('name', sorted(CASES))
def test_stoi_vs_float64_restatement(gpu, name):
    from speech_enhancement_by_s3prl_amd.evaluation import stoi_batch
    clean, proc, lengths, sr, refs = case(name)
    ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int64)
    c, p = clean.to(gpu), proc.to(gpu)
    for ext in (False, True):
        score, kept, tob = stoi_batch(p, c, ln, sr, ext, return_aux=True)
        score, kept, tob = score.cpu().numpy(), kept.cpu().numpy(), tob.cpu().numpy().astype(np.float64)
        tag = f'stoi_{name}_{"estoi" if ext else "stoi"}'
        assert kept.tolist() == [r[ext]['K'] for r in refs], (kept, [r[ext]['K'] for r in refs])
        for b, r in enumerate(refs):
            r = r[ext]
            K = r['K']
            assert (tob[:, b, :, K:] == 0).all()
            if K:
                for s, E in ((0, r['X']), (1, r['Y'])):
                    bounded(f'{tag}_tob{s}_b{b}', float(np.abs(tob[s, b, :, :K] - E).max() / E.max()), TOB_BOUND)
            if K < 30:
                assert score[b] == np.float32(1e-5), (b, score[b])
            else:
                bounded(f'{tag}_score_b{b}', abs(float(score[b]) - r['score']), SCORE_BOUND)


def test_identical_signals_score_one(gpu):
    from speech_enhancement_by_s3prl_amd.evaluation import stoi_batch
    clean, _, lengths, sr, _ = case('ragged')
    c = clean.to(gpu)
    ln = torch.tensor(lengths, dtype=torch.int64)
    for ext in (False, True):
        s = stoi_batch(c, c, ln, sr, ext).cpu().numpy()
        for b in (0, 1):
            bounded(f'stoi_identical_{int(ext)}_b{b}', abs(float(s[b]) - 1.0), SCORE_BOUND)
        assert s[2] == np.float32(1e-5)


def test_repeated_calls_are_bit_identical(gpu):
    """fixed summation order: no atomics anywhere in the chain"""
    from speech_enhancement_by_s3prl_amd.evaluation import stoi_batch
    clean, proc, _, sr, _ = case('straddle')
    c, p = clean.to(gpu), proc.to(gpu)
    a = [stoi_batch(p, c, None, sr, ext) for ext in (False, True)]
    b = [stoi_batch(p, c, None, sr, ext) for ext in (False, True)]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_metric_stage_keeps_the_device_metrics_on_the_device(gpu):
    from speech_enhancement_by_s3prl_amd.evaluation import MetricStage, sisdr_batch, stoi_batch
    stage = MetricStage(['stoi', 'estoi', 'sisdr'], gpu)
    assert stage.pool is None and stage.copy_stream is None                 # no worker, no D2H path
    want = np.zeros(3)
    for name in ('ragged', 'no_lengths'):
        clean, proc, lengths, sr, _ = case(name)
        c, p = clean.to(gpu), proc.to(gpu)
        ln = torch.tensor(lengths if lengths is not None else [clean.shape[1]] * clean.shape[0], dtype=torch.int64)
        stage.submit(p, c, ln)
        direct = [stoi_batch(p, c, ln, sr, False), stoi_batch(p, c, ln, sr, True), sisdr_batch(p, c, ln)]
        want += [float(d.double().mean()) for d in direct]
    assert len(stage._batches) == 2
    assert all(torch.is_tensor(v) and v.is_cuda for per in stage._batches for v in per)
    got = stage.average().numpy()
    assert np.allclose(got, (want / 2).astype(np.float32), rtol=1e-6, atol=0), (got, want / 2)
    stage.close()


def test_eval_drop_ins_agree_with_the_batch_call(gpu):
    from speech_enhancement_by_s3prl_amd.evaluation import estoi_eval, stoi_batch, stoi_eval
    clean, proc, _, sr, refs = case('no_lengths')
    c, p = clean[0].to(gpu), proc[0].to(gpu)
    s, e = stoi_eval(p, c, sr), estoi_eval(p, c, sr)
    assert isinstance(s, float) and isinstance(e, float)
    assert s == float(stoi_batch(p[None], c[None], None, sr, False)[0]) and e == float(stoi_batch(p[None], c[None], None, sr, True)[0])
    bounded('stoi_eval_score', abs(s - refs[0][0]['score']), SCORE_BOUND)
    bounded('estoi_eval_score', abs(e - refs[0][1]['score']), SCORE_BOUND)


def test_other_strings_and_rates_still_raise(gpu):
    from speech_enhancement_by_s3prl_amd import _lib
    from speech_enhancement_by_s3prl_amd.evaluation import MetricStage, stoi_batch
    clean, proc, _, _, _ = case('no_lengths')
    c, p = clean.to(gpu), proc.to(gpu)
    stage = MetricStage(['pesq_nb'], gpu)
    with pytest.raises(ValueError, match="'sisdr', 'stoi' and 'estoi'"):
        stage.submit(p, c, torch.tensor([16000, 16000]))
    stage.close()
    with pytest.raises(_lib.SEError, match='unsupported sample rate 8000'):
        stoi_batch(p, c, None, sr=8000)
    with pytest.raises(_lib.SEError):
        stoi_batch(proc, clean)                                              # host tensors
