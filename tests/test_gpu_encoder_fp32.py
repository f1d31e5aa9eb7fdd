"""GPU: the exact-fp32 parity mode of the encoder (TRANSFORMER.set_precision('fp32'), csrc/fp32path.hip) -- BASELINE.json configs 2 / 3 at the
tolerance north_star states: enhanced magnitudes within 1e-4 relative of the reference's fp32 CPU path (here: the oracle restating it), at
the reference geometry (6 x 768 x 12 x 3072, T' = 1001, 10 s utterances), through the whole evaluate()-style pass of runner.py:556-575.
The bf16 path stays the bench default (BASELINE.json names bf16); its bounds live in test_gpu_encoder_pipeline.py."""
import os

import pytest
import torch

from oracle import decode as odec
from oracle import encoder as oenc
from oracle import heads as oheads
from oracle import objective as oobj
from oracle import preprocessor as opre

pytestmark = pytest.mark.gpu

from conftest import bounded  # noqa: E402


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm()).item()


def test_gemm_f32_vs_fp64(gpu):
    """se_gemm_f32 in all its addressing forms against fp64: nn.Linear layout with bias / gelu / residual-by-row-modulo, the batched
    two-level-strided Q K^T form and the (K, N) row-major P V form; ragged sizes off the 64-tiles."""
    from speech_enhancement_by_s3prl_amd import _lib as L
    lib = L.load()
    torch.manual_seed(0)
    M, N, K = 131, 201, 77
    A, W, b = torch.randn(M, K, device=gpu), torch.randn(N, K, device=gpu), torch.randn(N, device=gpu)
    R = torch.randn(17, N, device=gpu)
    C = torch.empty(M, N, device=gpu)
    L.check(lib.se_gemm_f32(L.ptr(A), K, L.ptr(W), K, 0, L.ptr(b), L.ptr(R), 17, M, N, K, L.SE_ACT['GELU'], 1.0, L.ptr(C), N, 1, 1, 0, 0, 0, 0, 0, 0, L.stream()), 'gemm')
    ref = torch.nn.functional.gelu(A.double() @ W.double().T + b.double()) + R.double()[torch.arange(M, device=gpu) % 17]
    assert (C.double() - ref).abs().max().item() < 2e-5 * ref.abs().max().item()
    # batched attention forms
    B, heads, T = 2, 3, 70
    H = heads * 64
    q, k, v = (torch.randn(B * T, H, device=gpu) for _ in range(3))
    S = torch.empty(B, heads, T, T, device=gpu)
    L.check(lib.se_gemm_f32(L.ptr(q), H, L.ptr(k), H, 0, None, None, 0, T, T, 64, 0, 0.125, L.ptr(S), T, B, heads, T * H, 64, T * H, 64, heads * T * T, T * T,
                            L.stream()), 'qk')
    qh = q.double().view(B, T, heads, 64).permute(0, 2, 1, 3)
    kh = k.double().view(B, T, heads, 64).permute(0, 2, 1, 3)
    vh = v.double().view(B, T, heads, 64).permute(0, 2, 1, 3)
    Sref = qh @ kh.transpose(-1, -2) / 8.0
    assert (S.double() - Sref).abs().max().item() < 1e-5 * Sref.abs().max().item()
    lengths = torch.tensor([T, 33], device=gpu, dtype=torch.int32)
    L.check(lib.se_softmax_rows_f32(L.ptr(S), L.ptr(lengths), B, heads, T, L.stream()), 'softmax')
    mask = (torch.arange(T, device=gpu)[None, :] >= lengths[:, None].long()).double() * -10000.0
    Pref = torch.softmax(Sref + mask[:, None, None, :], dim=-1)
    assert (S.double() - Pref).abs().max().item() < 2e-6
    ctx = torch.empty(B * T, H, device=gpu)
    L.check(lib.se_gemm_f32(L.ptr(S), T, L.ptr(v), H, 1, None, None, 0, T, 64, T, 0, 1.0, L.ptr(ctx), H, B, heads, heads * T * T, T * T, T * H, 64, T * H, 64,
                            L.stream()), 'pv')
    cref = (Pref @ vh).permute(0, 2, 1, 3).reshape(B * T, H)
    assert (ctx.double() - cref).abs().max().item() < 1e-5 * cref.abs().max().item()


_ORACLE = {}


def _oracle_pass(cfg, ckpt, pre, wavs, lengths):
    """the CPU oracle's evaluate()-style pass at the reference geometry, computed once for both parity modes"""
    if 'r' not in _ORACLE:
        geom = opre.Geometry()
        f = opre.forward(wavs, pre.feat_list, geom)
        ocfg = oenc.Config(cfg)
        hid = oenc.encoder_forward(f[0], ckpt['Transformer'], ocfg)
        rpred, rres = oheads.spec_head(hid, ckpt['SpecHead'], ocfg, log=True)
        rwav = odec.decode_wav(rpred, f[3], lengths, geom, wavs[:, 1])
        rloss = oobj.l1(rres['log_predicted'], f[4], odec.get_length_masks(lengths // 160 + 1))
        _ORACLE['r'] = (hid, rpred, rwav, rloss)
    return _ORACLE['r']


@pytest.mark.parametrize('precision,hid_l2', [('fp32', 2e-5), ('bf16x3', 3e-5), ('bf16x3:rowln', 3e-5)])
def test_fp32_mode_meets_1e4_at_the_reference_geometry(gpu, precision, hid_l2, monkeypatch):
    """both parity modes of the encoder against the oracle: 'fp32' (fp32 operands on the fp32 matrix instruction) and 'bf16x3' (every nn.Linear
    as one bf16 GEMM over three-term splits of both operands, attention core in exact fp32) -- the same bounds, north_star's 1e-4 on enhanced
    magnitudes among them"""
    from speech_enhancement_by_s3prl_amd import pipeline, synth
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    if precision.endswith(':rowln'):
        # the form the three-term mode takes from B = 21 on (transformer.encode_x3): the two N = 768 projections of a layer as ONE row-complete
        # projection + residual + LayerNorm launch that also writes the next operand's split (se_gemm_res_ln_x3_bf16) -- forced on at this batch of 2
        monkeypatch.setenv('SE_AMD_X3_ROWLN', '7')
        precision = 'bf16x3'
    elif precision == 'bf16x3':
        monkeypatch.setenv('SE_AMD_X3_ROWLN', '0')
    cfg = pipeline.make_config()                                   # 6 x 768 x 12 x 3072 (config/pretrain_sample.yaml)
    ckpt = pipeline.synthetic_checkpoint(cfg, seed=0)
    up = pipeline.build_upstream(ckpt, gpu).set_precision(precision)
    pre = pipeline.build_preprocessor(cfg, gpu)
    step = pipeline.UpstreamEnhanceStep(pre, up)
    lengths, wavs = synth.synth_batch(2, 160000)                   # two 10 s utterances ...
    lengths[1] = 100000                                            # ... the second one cut to 6.25 s and zero padded as collate_fn does
    wavs[1, :, 100000:] = 0.0                                      # (dataset.py:169-179): padded frames / masked keys
    wav_pred, loss, predicted = step(wavs.to(gpu), lengths.to(gpu))
    with torch.no_grad():
        hidden = up(pre(wavs.to(gpu))[0])
    hid, rpred, rwav, rloss = _oracle_pass(cfg, ckpt, pre, wavs, lengths)
    assert hidden.shape == hid.shape == (2, 1001, 768)
    tag = f'{precision} mode'
    bounded(f'{tag}: hidden rel-L2 (6 layers, T=1001)', rel_l2(hidden, hid), hid_l2)
    bounded(f'{tag}: hidden max-norm', (hidden.cpu() - hid).abs().max().item() / hid.abs().max().item(), 1e-4)
    mag, rmag = predicted.cpu().double().sqrt(), rpred.double().sqrt()
    per_utt = ((mag - rmag).abs().flatten(1).max(dim=1).values / rmag.flatten(1).max(dim=1).values).max().item()
    bounded(f'{tag}: enhanced magnitudes, max-norm per utterance (north_star: 1e-4)', per_utt, 1e-4)
    bounded(f'{tag}: enhanced magnitudes rel-L2', rel_l2(mag, rmag), 1e-4)
    bounded(f'{tag}: enhanced waveform max-norm', ((wav_pred.cpu() - rwav).abs().max() / rwav.abs().max()).item(), 1e-4)
    bounded(f'{tag}: L1 loss', abs(loss.item() - rloss.item()) / abs(rloss.item()), 1e-5 if precision == 'fp32' else 2e-5)
    for i in range(2):
        n = int(lengths[i])
        a = oobj.sisdr_eval(wav_pred[i, :n].cpu(), wavs[i, 1, :n])
        r = oobj.sisdr_eval(rwav[i, :n], wavs[i, 1, :n])
        bounded(f'{tag}: SI-SDR delta utterance {i} (dB)', abs(a - r), 1e-3)
    # and the mode is a switch: back to bf16 gives the bench path again
    up.set_precision('bf16')
    with torch.no_grad():
        h16 = up(pre(wavs.to(gpu))[0])
    assert 1e-4 < rel_l2(h16, hid) < 6e-3


def test_split3_terms_reconstruct_the_operand(gpu):
    """se_split3_bf16: x1 + x2 reproduces x to 2^-16 relative, slices in the activation / weight order, zero padding up to Kp"""
    from speech_enhancement_by_s3prl_amd import _lib as L
    lib = L.load()
    torch.manual_seed(3)
    rows, cols, Kp = 37, 80, 128
    x = torch.randn(rows, cols, device=gpu) * torch.logspace(-3, 3, cols, device=gpu)
    for which in (0, 1):
        out = torch.full((rows, 3 * Kp), 7.0, device=gpu, dtype=torch.bfloat16)
        L.check(lib.se_split3_bf16(L.ptr(x), cols, rows, cols, Kp, which, L.ptr(out), L.stream()), 'split3')
        s0, s1, s2 = out[:, :Kp].float(), out[:, Kp:2 * Kp].float(), out[:, 2 * Kp:].float()
        hi, mid = (s0, s2) if which == 0 else (s0, s1)
        assert torch.equal(hi, x.bfloat16().float().pad if False else torch.nn.functional.pad(x.bfloat16().float(), (0, Kp - cols)))
        assert torch.equal(s1 if which == 0 else s2, hi)
        assert (out[:, cols:Kp] == 0).all() and (out[:, Kp + cols:2 * Kp] == 0).all() and (out[:, 2 * Kp + cols:] == 0).all()
        err = ((hi + mid)[:, :cols].double() - x.double()).abs() / x.double().abs()
        assert err.max().item() < 2.0 ** -16


@pytest.mark.parametrize('B,T,heads,lens', [(2, 333, 3, [333, 130]), (1, 1001, 2, None), (3, 64, 1, [64, 1, 33]), (1, 129, 12, [77]),
                                            (3, 130, 2, [130, 0, 65])])      # a silent utterance: the -10000 on every key cancels, full attention
def test_mhsa_x3_vs_fp64(gpu, B, T, heads, lens):
    """se_mhsa_fwd_x3_f32 (two-term operand splits, three products each, exact online softmax) against fp64 attention with the reference's
    additive -10000 on padded keys: 3e-5 of the largest context value (the split drops 2^-18-relative product terms)"""
    from speech_enhancement_by_s3prl_amd import _lib as L
    lib = L.load()
    torch.manual_seed(T + heads)
    H = 64 * heads
    qkv = torch.randn(B * T, 3 * H, device=gpu) * 1.7
    lengths = torch.tensor(lens if lens else [T] * B, device=gpu, dtype=torch.int32)
    ctx = torch.full((B * T, H), float('nan'), device=gpu)
    L.check(lib.se_mhsa_fwd_x3_f32(L.ptr(qkv), L.ptr(lengths), B, T, heads, L.ptr(ctx), L.stream()), 'mhsa_x3')
    x = qkv.double().reshape(B, T, 3, heads, 64)
    q, k, v = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)
    s = q @ k.transpose(-1, -2) / 8.0
    pad = (torch.arange(T, device=gpu)[None, :] >= lengths[:, None]).double() * -10000.0
    p = torch.softmax(s + pad[:, None, None, :], dim=-1)
    ref = (p @ v).transpose(1, 2).reshape(B * T, H)
    assert torch.isfinite(ctx).all()
    err = (ctx.double() - ref).abs().max().item() / ref.abs().max().item()
    bounded(f'mhsa_x3[{B},{T},{heads}] context max-norm', err, 3e-5)


@pytest.mark.parametrize('M,K', [(300, 2304), (128, 768), (1001, 9216)])
def test_gemm_res_ln_x3_equals_the_two_launches(gpu, M, K):
    """se_gemm_res_ln_x3_bf16 (row-complete projection + residual + LayerNorm + the split of its rows, one launch) against se_gemm_res_ln_bf16
    followed by se_split3_bf16: the fp32 rows and all three slices bit for bit (ragged last row tile at M = 300 / 1001)"""
    from speech_enhancement_by_s3prl_amd import _lib as L
    lib = L.load()
    torch.manual_seed(M + K)
    N = 768
    A = torch.randn(M, K, device=gpu).bfloat16()
    W = (torch.randn(N, K, device=gpu) * 0.03).bfloat16()
    bias, res = torch.randn(N, device=gpu), torch.randn(M, N, device=gpu)
    lw, lb = torch.rand(N, device=gpu) + 0.5, torch.randn(N, device=gpu)
    o_ref = torch.empty(M, N, device=gpu)
    L.check(lib.se_gemm_res_ln_bf16(L.ptr(A), K, L.ptr(W), K, L.ptr(bias), L.ptr(res), L.ptr(lw), L.ptr(lb), 1e-12, M, N, K, L.ptr(o_ref), None, L.stream()), 'ref')
    s_ref = torch.empty(M, 3 * N, device=gpu, dtype=torch.bfloat16)
    L.check(lib.se_split3_bf16(L.ptr(o_ref), N, M, N, N, 0, L.ptr(s_ref), L.stream()), 'split')
    o = torch.empty(M, N, device=gpu)
    s3 = torch.full((M, 3 * N), float('nan'), device=gpu, dtype=torch.bfloat16)
    L.check(lib.se_gemm_res_ln_x3_bf16(L.ptr(A), K, L.ptr(W), K, L.ptr(bias), L.ptr(res), L.ptr(lw), L.ptr(lb), 1e-12, M, N, K, L.ptr(o), L.ptr(s3), L.stream()), 'x3')
    assert torch.equal(o, o_ref)
    assert torch.equal(s3.view(torch.int16), s_ref.view(torch.int16))
    # and the three slices reconstruct the fp32 rows to 2^-17
    y = s3[:, :N].float() + s3[:, 2 * N:].float()
    assert (y - o).abs().max().item() <= 2.0 ** -16 * o.abs().max().item()


def test_x3_position_table_follows_the_sequence_length(gpu):
    """the three-term mode cached its positional table TILED to (B T, H) and keyed on that shape, so (B, T) = (2, 2 T') followed by
    (4, T') -- same B T -- reused the positions of the other T.  The same engine run at both shapes must agree with the fp32 mode each time."""
    from speech_enhancement_by_s3prl_amd import pipeline
    cfg = pipeline.make_config(layers=1)
    ckpt = pipeline.synthetic_checkpoint(cfg, seed=3)
    up = pipeline.build_upstream(ckpt, gpu)
    torch.manual_seed(0)
    for B, T in ((2, 96), (4, 48), (1, 192)):
        feats = torch.randn(B, T, 80, device=gpu)
        with torch.no_grad():
            h3 = up.set_precision('bf16x3')(feats)
            h32 = up.set_precision('fp32')(feats)
        assert rel_l2(h3, h32.cpu()) < 3e-5, (B, T, rel_l2(h3, h32.cpu()))
    up.set_precision('bf16')
