"""GPU: se_stoi_grad_f32 (csrc/stoi_bwd.hip) and the criteria objective.stoi / objective.estoi against float64 autograd through the
differentiable restatement tests/stoi_grad_ref.py (itself pinned by tests/test_stoi_grad_host.py).  Parity unpinned vs asteroid / torch_stoi.

Signals: stoi_ref.speechlike with stretches 65 dB down (frames really are dropped: compacted neighbours are no neighbours in the source),
processed = clean + white noise at 5 or 0 dB SNR, both rounded to fp32 first.  Before any GPU compare the restatement alone must show, for every
scored utterance, a keep-mask margin >= 0.05 dB and a clip margin >= 1e-4, and for STOI a clipped share strictly between 0 and 1 in at least
one utterance per case: an fp32 / fp64 branch flip is then not read as an error (asserted in `case`, also by a test that needs no GPU; never
used to skip an utterance).

Bound: max |g - g_ref| <= 1e-4 max |g_ref| per utterance, the project's fp32-path bar, against the float64 autograd
gradient; the end-to-end head gradients 1e-4 normwise, losses 1e-4 relative.  Measured on an MI355X (conftest.bounded logs every value):
  kernel gradient          STOI 2.8e-7 ... 1.1e-6      ESTOI 2.7e-7 ... 5.8e-7
  criteria                 gradient as the kernel's; loss 2.3e-8 ... 7.5e-8
  end to end               loss 1.4e-8, weight.grad 4.7e-7, bias.grad 4.8e-7 (normwise)"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import stoi_ref as R      # noqa: E402
import stoi_grad_ref as G      # noqa: E402
from conftest import bounded      # noqa: E402

BOUND = 1e-4
MIN_MARGIN_DB = 0.05
MIN_CLIP_MARGIN = 1e-4
BAND_FRAMES = 4

# name -> (sr, T, lengths, per utterance (seed, gaps in input samples, SNR in dB))
CASES = {
    'ragged16k': (16000, 16000, [16000, 13001, 4800, 0],
                  [(61, [(6000, 9300)], 5.0), (62, [(2500, 4500)], 0.0), (63, [], 5.0), (64, [], 0.0)]),
    'straddle16k': (16000, 64000, [64000], [(75, [(9000, 13000), (56000, 59500)], 0.0)]),
    'same_rate10k': (10000, 10000, [10000, 7777], [(81, [(4000, 6000)], 0.0), (82, [(1000, 2200)], 5.0)]),
}


def check_conditions(name, infos):
    """the restatement's own distance from every branch, per scored utterance and form; infos[b][extended]"""
    scored = [r for r in infos if r[0]['K'] >= 30]
    assert scored, name
    for r in scored:
        assert r[0]['margin'] >= MIN_MARGIN_DB, (name, r[0]['margin'])
        assert r[0]['clip_margin'] >= MIN_CLIP_MARGIN, (name, r[0]['clip_margin'])
    assert any(0 < r[0]['clipped'] < 1 for r in scored), (name, [r[0]['clipped'] for r in scored])


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(clean, proc (B, T) fp32 tensors, lengths, sr, score[ext] (B,), grad[ext] (B, T) float64, infos[b][ext]); computed once, shared,
    left unchanged"""
    sr, T, lengths, utts = CASES[name]
    clean = np.stack([R.speechlike(seed, T, sr, gaps) for seed, gaps, _ in utts]).astype(np.float32)
    proc = np.stack([R.add_noise(c.astype(np.float64), snr, 1000 + seed) for c, (seed, _, snr) in zip(clean, utts)]).astype(np.float32)
    out = {'clean': torch.from_numpy(clean), 'proc': torch.from_numpy(proc), 'lengths': lengths, 'sr': sr, 'score': {}, 'grad': {}}
    per = {}
    for ext in (False, True):
        out['score'][ext], out['grad'][ext], per[ext] = G.batch(clean, proc, lengths, sr, ext)
    out['infos'] = [(per[False][b], per[True][b]) for b in range(len(utts))]
    check_conditions(name, out['infos'])
    return out


def test_cases_keep_clear_of_every_branch_and_cover_the_partitions():
    """needs no GPU: the conditions on the restatement (asserted in `case`) and the shapes the kernels' partitions need"""
    c = case('ragged16k')
    info = [r[0] for r in c['infos']]
    assert [r['frames'] for r in info] == [77, 62, 22, 0] and [r['K'] >= 30 for r in info] == [True, True, False, False]
    assert all(r['K'] < r['frames'] and r['K'] % BAND_FRAMES != 0 for r in info[:2])          # frames dropped; a partial last band workgroup
    assert (c['grad'][False][2:] == 0).all() and (c['grad'][False][1, 13001:] == 0).all()
    r = case('straddle16k')['infos'][0][0]
    assert r['frames'] == 311 and 30 <= r['K'] < 311 and r['K'] % BAND_FRAMES != 0 and R.n10_of(64000, 5, 8) % 256 != 0
    info = [r[0] for r in case('same_rate10k')['infos']]
    assert all(30 <= r['K'] < r['frames'] for r in info)


def _lib():
    from speech_enhancement_by_s3prl_amd import _lib as L
    return L, L.load()


def _call(dev, proc, clean, lengths, sr, ext, scale=1.0, short_by=0):
    """se_stoi_grad_f32 on device copies -> (stoi_out, grad); the outputs start as NaN: every element is written"""
    from speech_enhancement_by_s3prl_amd.evaluation import _stoi_plan
    L, lib = _lib()
    p, c = proc.to(dev).contiguous(), clean.to(dev).contiguous()
    B, T = p.shape
    ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int64, device=dev)
    plan = _stoi_plan(dev, sr)
    nbytes = lib.se_stoi_grad_workspace_bytes(plan, B, T)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    score = torch.full((B,), float('nan'), device=dev)
    grad = torch.full((B, T), float('nan'), device=dev)
    L.check(lib.se_stoi_grad_f32(plan, L.ptr(c), L.ptr(p), T, L.ptr(ln), B, T, int(ext), float(scale), L.ptr(score), L.ptr(grad), L.ptr(ws),
                                 nbytes - short_by, L.stream()), 'se_stoi_grad_f32')
    return score, grad


def _err(tag, got, ref):
    """per utterance max |got - ref| / max |ref| through `bounded`; a row whose reference is all zero must be exactly zero"""
    got, ref = got.detach().double().cpu(), ref.double()
    for b, (gr, rr) in enumerate(zip(got, ref)):
        top = rr.abs().max().item()
        if top == 0.0:
            assert (gr == 0).all(), (tag, b)
            continue
        e = (gr - rr).abs().max().item() / top
        print(f'{tag}_b{b}: {e:.3e}')
        bounded(f'stoi_grad/{tag}_b{b}', e, BOUND)


@pytest.mark.gpu
@pytest.mark.parametrize('ext', [False, True], ids=['stoi', 'estoi'])
@pytest.mark.parametrize('name', sorted(CASES))
def test_gradient_vs_float64_autograd(gpu, name, ext):
    from speech_enhancement_by_s3prl_amd.evaluation import stoi_batch
    c = case(name)
    lengths, sr = c['lengths'], c['sr']
    score, grad = _call(gpu, c['proc'], c['clean'], lengths, sr, ext)
    assert torch.isfinite(grad).all()
    fwd = stoi_batch(c['proc'].to(gpu), c['clean'].to(gpu), torch.tensor(lengths), sr, ext)
    assert torch.equal(score, fwd)                                              # bit-identical to se_stoi_f32
    _err(f'{name}_{"estoi" if ext else "stoi"}', grad, c['grad'][ext])
    g = grad.cpu()
    for b, n in enumerate(lengths):
        assert (g[b, n:] == 0).all()
        if c['infos'][b][ext]['K'] < 30:
            assert (g[b] == 0).all() and score[b].item() == np.float32(1e-5)
        else:
            assert g[b].abs().max() > 0
    score2, grad2 = _call(gpu, c['proc'], c['clean'], lengths, sr, ext)
    assert torch.equal(grad, grad2) and torch.equal(score, score2)             # fixed order everywhere: no atomics
    for scale in (-1.0, 0.5):
        s3, g3 = _call(gpu, c['proc'], c['clean'], lengths, sr, ext, scale=scale)
        assert torch.equal(g3, grad * scale) and torch.equal(s3, score)


@pytest.mark.gpu
def test_no_lengths_and_undersized_workspace(gpu):
    c = case('same_rate10k')
    T = c['proc'].shape[1]
    full, gfull = _call(gpu, c['proc'][:1], c['clean'][:1], None, c['sr'], False)
    same, gsame = _call(gpu, c['proc'][:1], c['clean'][:1], [T], c['sr'], False)
    assert torch.equal(full, same) and torch.equal(gfull, gsame)
    L, _ = _lib()
    with pytest.raises(L.SEError, match='se_stoi_grad_f32: workspace of .* needed'):
        _call(gpu, c['proc'], c['clean'], c['lengths'], c['sr'], False, short_by=1)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['ragged16k', 'same_rate10k'])
def test_criteria_loss_and_gradient(gpu, name):
    """objective.stoi / estoi: -mean_b score_b and its gradient through autograd, lengths given or taken from the mask's row sums"""
    from speech_enhancement_by_s3prl_amd import objective
    c = case(name)
    B, T = c['proc'].shape
    lengths = torch.tensor(c['lengths'])
    for cls, ext in ((objective.stoi, False), (objective.estoi, True)):
        crit = cls(sr=c['sr'])
        rloss = -c['score'][ext].mean().item()
        rgrad = -c['grad'][ext] / B
        for form in ('lengths', 'length_masks'):
            s = c['proc'].to(gpu).requires_grad_(True)
            kw = {'lengths': lengths.to(gpu)} if form == 'lengths' else {'length_masks': (torch.arange(T)[None, :] < lengths[:, None]).float().to(gpu)}
            loss, extra = crit(wav_predicted=s, wav_tar=c['clean'].to(gpu), **kw)
            assert extra == {}
            loss.backward()
            tag = f'crit_{name}_{cls.__name__}_{form}'
            print(f'{tag}_loss: {abs(loss.item() - rloss) / abs(rloss):.3e}')
            bounded(f'stoi_grad/{tag}_loss', abs(loss.item() - rloss) / abs(rloss), BOUND)
            _err(tag, s.grad, rgrad)
        with torch.no_grad():
            plain, _ = crit(wav_predicted=c['proc'].to(gpu), wav_tar=c['clean'].to(gpu), lengths=lengths.to(gpu))
        assert torch.equal(plain, loss.detach())                               # the score does not depend on whether a gradient is asked for


# ---- end to end: HeadFinetuneStep(criterion=objective.stoi()) against decode_grad_ref's float64 decode followed by stoi_grad_ref
E2E_LENGTHS = [12800, 10007, 8000]          # 0.5 - 0.8 s, each >= 6554 samples (the shortest that yields 30 frames)


@functools.lru_cache(maxsize=None)
def _e2e_ref():
    """host only: batch, head state and the float64 chain's loss and head gradients; the branch conditions hold for the decoded waveforms"""
    import decode_grad_ref as D
    from oracle import heads as oheads
    from oracle import preprocessor as opre
    T = E2E_LENGTHS[0]
    clean = torch.from_numpy(np.stack([R.speechlike(91 + b, T, 16000) for b in range(3)])).float()
    noisy = torch.from_numpy(np.stack([R.add_noise(clean[b].double().numpy(), 5.0, 95 + b) for b in range(3)])).float()
    wavs = torch.stack([noisy, clean], dim=1).contiguous()                     # (B, 2, T): noisy, clean
    lengths = torch.tensor(E2E_LENGTHS)
    assert min(E2E_LENGTHS) >= 6554
    from speech_enhancement_by_s3prl_amd import pipeline
    from speech_enhancement_by_s3prl_amd.heads import LinearResidual
    torch.manual_seed(0)
    head = LinearResidual(input_size=120, output_size=201, activation='Sigmoid', cmvn=True)
    state = {k: v.detach().clone() for k, v in head.state_dict().items()}
    g = opre.Geometry()
    fl = [dict(pipeline.BASELINE_FEAT, channel=0), opre.get_feat_config('linear', 0), opre.get_feat_config('phase', 0)]
    rfeats, rlin, rph = opre.forward(wavs.double(), fl, g)
    w = state['linear.weight'].double().requires_grad_(True)
    b = state['linear.bias'].double().requires_grad_(True)
    rpred, _ = oheads.linear_residual(rfeats, rlin, w, b, activation='Sigmoid')
    rwav = D.decode_chain(rpred, rph, lengths, g, wavs[:, 1].double())
    infos = [G.stoi_full(wavs[i, 1, :n].double().numpy(), rwav[i, :n], 16000, False) for i, n in enumerate(E2E_LENGTHS)]
    assert all(r['K'] >= 30 for r in infos)
    check_conditions('e2e', [(r, r) for r in infos])
    rloss = -torch.stack([r['score'] for r in infos]).mean()
    rloss.backward()
    return {'wavs': wavs, 'lengths': lengths, 'state': state, 'rloss': rloss.item(), 'gw': w.grad, 'gb': b.grad}


def test_end_to_end_reference_keeps_clear_of_every_branch():
    """needs no GPU"""
    e = _e2e_ref()
    assert e['gw'].abs().max() > 0 and e['gb'].abs().max() > 0 and torch.isfinite(e['gw']).all()


@pytest.mark.gpu
def test_end_to_end_head_finetune_step(gpu):
    from speech_enhancement_by_s3prl_amd import objective, pipeline
    from speech_enhancement_by_s3prl_amd.heads import LinearResidual
    from speech_enhancement_by_s3prl_amd.solver import get_optimizer
    e = _e2e_ref()
    pre = pipeline.build_preprocessor(pipeline.make_config(), gpu, upstream='baseline')
    head = LinearResidual(input_size=120, output_size=201, activation='Sigmoid', cmvn=True)
    head.load_state_dict(e['state'])
    head = head.to(gpu)
    opt = get_optimizer(list(head.named_parameters()), lr=1e-4, warmup_proportion=0.1, training_steps=100)
    step = pipeline.HeadFinetuneStep(pre, head, opt, criterion=objective.stoi())
    seen = {}                                                                  # the step clears .grad after the update: keep what its backward produced
    head.linear.weight.register_hook(lambda g: seen.__setitem__('weight', g.detach().clone()))
    head.linear.bias.register_hook(lambda g: seen.__setitem__('bias', g.detach().clone()))
    loss, grad_norm, skipped = step(e['wavs'].to(gpu), e['lengths'].to(gpu))
    assert not skipped and grad_norm > 0 and set(seen) == {'weight', 'bias'}
    print(f'e2e loss: {abs(loss.item() - e["rloss"]) / abs(e["rloss"]):.3e}')
    bounded('stoi_grad/e2e_loss', abs(loss.item() - e['rloss']) / abs(e['rloss']), BOUND)
    for nm, got, ref in (('weight', seen['weight'], e['gw']), ('bias', seen['bias'], e['gb'])):
        err = ((got.double().cpu() - ref).norm() / ref.norm()).item()
        print(f'e2e {nm}: {err:.3e}')
        bounded(f'stoi_grad/e2e_{nm}', err, BOUND)
