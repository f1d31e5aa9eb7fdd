"""Host checks of tests/encoder_stage_ref.py (no GPU): the staged float64 reference IS oracle.encoder when its roundings are off, differs from
it by a bf16-sized amount when they are on, its test weights make sublayer and attention errors visible, and its per-row metric sees every
planted error of the kinds a wrong kernel would make -- with the bounds tests/test_gpu_encoder_stages.py uses.

Planted errors at (B, T) = (3, 101), hidden 768 (every instance of each kind must exceed its bound), and what the OLD whole-tensor bound (relative L2
< 6e-3 on top of the 3.1e-3 the kernels measure, added in quadrature) would have said at the bench shape, 32 032 x 768 random fp32 rows
(values printed by test_planted_errors_are_seen; `old` = the whole-tensor figure the planted error alone produces):
    kind                                              smallest per-row figure          old figure   old bound (6e-3)
    (i)   one row replaced by its neighbour           8.7e-2                           7.6e-3       caught for independent rows (5.6e-3 x sqrt 2); a neighbour
                                                                                                    correlated as these hidden states are (8.7e-2 of a row): 4.8e-4, PASSED
    (ii)  one row with another frame's position row   1.5e-1 (t + 1), 6.5e-1 (row % 128)  8.5e-4    PASSED
    (iii) a tile's ragged tail left stale             1.07                             4.5e-2       caught (32 rows)
    (iv)  one element off by 2^-6 of the RMS row norm 1.56e-2 = 2^-6 exactly           8.7e-5       PASSED
    (v)   the residual's low byte dropped in one row  1.8e-3 = 2^-9.1 (max metric)     8.6e-6       PASSED
    (vi)  utterance b computed with b + 1's length    5.1e-1                           9.0e-2       caught when all 1001 rows of the utterance move
Kind (v) is below what bf16 operands leave in a layer's rows, so the row metric cannot own it: it is judged by the pass-through case, whose
2^-12 max-norm ceiling it exceeds in every row."""
import math

import pytest
import torch

import encoder_stage_ref as esr
from oracle import encoder as oenc
from oracle import heads as oheads


def _cfg(hidden=768, heads=12, inter=3072, layers=2):
    return oenc.Config({'transformer': {'hidden_size': hidden, 'num_attention_heads': heads, 'intermediate_size': inter, 'num_hidden_layers': layers}})


def _feats(B, T, D=80, seed=0, lens=None):
    f = torch.randn(B, T, D, generator=torch.Generator().manual_seed(seed))
    for b, n in enumerate(lens or []):
        f[b, n:] = 0.0
    return f


@pytest.fixture(scope='module')
def full():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cfg = _cfg()
    sd, head = esr.stage_weights(cfg, seed=11)
    return cfg, sd, head


@pytest.mark.parametrize('lens', [[37, 20, 5], [37, 1, 36], [37, 0, 12]], ids=['ragged', 'length-1', 'all-zero-utterance'])
def test_roundings_off_is_the_oracle(lens):
    cfg = _cfg(128, 2, 256, 2)
    sd, head = esr.stage_weights(cfg, inp_dim=24, spec_out=33, seed=3)
    sd64, head64 = {k: v.double() for k, v in sd.items()}, {k: v.double() for k, v in head.items()}
    feats = _feats(3, 37, 24, seed=5, lens=lens).double()
    lengths = oenc.valid_lengths(feats)
    assert lengths.tolist() == lens
    ref = esr.StageRef(sd64, head64, cfg, rounded=False)
    mine = ref.encoder(feats, lengths)
    theirs = oenc.encoder_forward(feats, sd64, cfg, all_layers=True)
    for i, (a, b) in enumerate(zip(mine[1:], theirs)):
        assert (a - b).abs().max().item() < 1e-10, ('layer', i)
    p, pred, logp = ref.spec_head(mine[-1], log_target=True, act='ReLU')
    op, _ = oenc.spec_head_forward(theirs[-1], head64, cfg)
    assert (p - op).abs().max().item() < 1e-10
    for log in (True, False):
        for act in ('ReLU', 'Sigmoid', 'Identity'):
            _, pred, logp = ref.spec_head(mine[-1], log_target=log, act=act, eps=1e-6)
            opred, ores = oheads.spec_head(theirs[-1], head64, cfg, log=log, activation=act, eps=1e-6)
            # log(p + eps) has the derivative 1 / (p + eps): a 1e-14 difference of p reads 1e-10 at p + eps = 1e-4, so it is compared where
            # p > 1e-2 (log_target: everywhere, log_predicted is p itself)
            ok = torch.isfinite(ores['log_predicted']) & (log | (op > 1e-2))
            assert (pred - opred).abs().max().item() < 1e-10 * max(1.0, opred.abs().max().item())
            assert (logp[ok] - ores['log_predicted'][ok]).abs().max().item() < 1e-10


def test_roundings_on_differ_by_a_bf16_sized_amount(full):
    """the share of the old whole-tensor figure that is operand rounding, not kernel error: printed, and held to the bf16 scale (2^-9 = 2e-3 per
    rounding; a few of them per layer add in quadrature and the LayerNorms carry them on)"""
    cfg, sd, head = full
    feats = _feats(3, 101, seed=7, lens=[101, 50, 1])
    lengths = oenc.valid_lengths(feats)
    on = esr.StageRef(sd, head, cfg, rounded=True).encoder(feats, lengths)
    off = esr.StageRef(sd, head, cfg, rounded=False).encoder(feats, lengths)
    for i, (a, b) in enumerate(zip(on, off)):
        e = esr.rel_l2(a, b)
        print(f'stage {i}: rounded vs unrounded reference rel-L2 {e:.3e}, worst row {esr.row_err(a, b)[0].max().item():.3e}')
        assert 1e-5 < e < 2e-2, (i, e)


def test_the_test_weights_make_errors_visible(full):
    cfg, sd, head = full
    ref = esr.StageRef(sd, head, cfg, rounded=False)
    feats = _feats(2, 130, seed=9)
    lengths = torch.tensor([130, 130])
    x = ref.input_stage(feats)
    for i in range(cfg.num_hidden_layers):
        parts = ref.layer_parts(x, lengths, i)
        ra, ro = esr.rms(parts['a']) / esr.rms(x), esr.rms(parts['o']) / esr.rms(parts['x1'])
        peak = parts['probs'].max(dim=-1).values.mean().item()
        print(f'layer {i}: attention-output / residual RMS {ra:.2f}, FFN-output / residual RMS {ro:.2f}, mean largest probability {peak:.3f}')
        assert 0.5 <= ra <= 2.0 and 0.5 <= ro <= 2.0, (i, ra, ro)
        assert peak > 0.2, (i, peak)
        x = parts['x2']
    # the plain N(0, 0.02) weights do NOT meet them: that is why they are not used
    sd0, head0 = oenc.init_weights(cfg, 80, seed=11, spec_out=201)
    ref0 = esr.StageRef(sd0, head0, cfg, rounded=False)
    x0 = ref0.input_stage(feats)
    parts0 = ref0.layer_parts(x0, lengths, 0)
    assert esr.rms(parts0['a']) / esr.rms(x0) < 0.5 and parts0['probs'].max(dim=-1).values.mean().item() < 0.2


def _whole_tensor(rel_rows, n_rows, M=32032):
    """the whole-tensor relative L2 when n_rows of M equal-norm rows carry a per-row relative error rel_rows"""
    return rel_rows * math.sqrt(n_rows / M)


def test_planted_errors_are_seen(full):
    cfg, sd, head = full
    B, T, H = 3, 101, 768
    lens = [101, 50, 1]
    feats = _feats(B, T, seed=7, lens=lens)
    lengths = torch.tensor(lens)
    ref = esr.StageRef(sd, head, cfg, rounded=True)
    x0 = ref.input_stage(feats)
    x1 = ref.layer(x0, lengths, 0)
    x2 = ref.layer(x1, lengths, 1)
    layer_bound = max(esr.ROW_BOUND[k] for k in esr.ROW_BOUND if k.startswith('layer/'))
    input_bound = max(esr.ROW_BOUND[k] for k in esr.ROW_BOUND if k.startswith('input/'))
    report, missed = {}, []

    def all_exceed(name, errs, bound):      # every instance, none left out; the misses are collected so that the whole table prints before the assert
        errs = torch.as_tensor(errs, dtype=torch.float64).flatten()
        report[name] = errs.min().item()
        if not (errs > bound).all():
            missed.append((name, errs.min().item(), bound, f'{int((errs <= bound).sum())} of {errs.numel()} instances at or under the bound'))

    flat = x2.reshape(B * T, H)
    # (i) a stale row: row m carries row m - 1, every m (across utterance boundaries too)
    got = flat.clone()
    got[1:] = flat[:-1]
    all_exceed('(i) stale row', esr.row_err(got.view(B, T, H), x2)[0].flatten()[1:], layer_bound)
    # (ii) another frame's positional row in the input stage: t + 1 instead of t, every row (adjacent rows differ least)
    pre = ref.pre_layernorm(feats)
    pe = oenc.position_encoding(T + 1, H, torch.float64)
    wrong = ref._ln(pre - pe[None, :T] + pe[None, 1:], 'input_representations.LayerNorm')
    all_exceed('(ii) wrong positional row', esr.row_err(wrong, x0)[0], input_bound)
    #      ... and the row-index-modulo-T mistake of a tile that straddles utterances: position (b T + t) % 128 in place of t
    m = torch.arange(B * T)
    pe_big = oenc.position_encoding(128, H, torch.float64)
    wrong = ref._ln(pre - pe[None, :T] + pe_big[m % 128].view(B, T, H), 'input_representations.LayerNorm')
    e = esr.row_err(wrong, x0)[0].flatten()
    all_exceed('(ii) position = row % 128', e[(m % 128) != (m % T)], input_bound)
    # (iii) the ragged tail of the third 128-row tile (rows 256 .. 302) left at its previous value: the in-place stream still holds x1 there
    got = x2.reshape(B * T, H).clone()
    got[256:] = x1.reshape(B * T, H)[256:]
    all_exceed('(iii) stale ragged tail', esr.row_err(got.view(B, T, H), x2)[0].flatten()[256:], layer_bound)
    # (iv) one element off by 2^-6 of the RMS row norm: every row, first / last / a middle column
    den = x2.pow(2).sum(-1).mean(dim=1).sqrt()                       # (B,)
    errs = []
    for col in (0, 383, 767):
        got = x2.clone()
        got[:, :, col] += (2.0 ** -6) * den[:, None]
        errs.append(esr.row_err(got, x2)[0])
    all_exceed('(iv) one element 2^-6', torch.stack(errs), layer_bound)
    # (vi) utterance b computed with utterance b + 1's length
    wrong = ref.layer(x1, torch.roll(lengths, -1), 1)
    all_exceed('(vi) neighbour length', esr.row_err(wrong, x2)[0].max(dim=1).values, layer_bound)
    # (v) the residual's low byte dropped (the stream read as its bf16 half only), every row: below the bf16 noise of a layer's rows, so it is the
    #     pass-through case that owns it -- zeroed sublayers, LayerNorms at weight 1 / bias 0, the stream must come back as the input stage's rows
    sdz = dict(sd)
    for i in range(2):
        p = f'encoder.layer.{i}.'
        for n in ('attention.output.dense', 'output.dense'):
            sdz[p + n + '.weight'], sdz[p + n + '.bias'] = torch.zeros_like(sd[p + n + '.weight']), torch.zeros_like(sd[p + n + '.bias'])
        for n in ('attention.output.LayerNorm', 'output.LayerNorm'):
            sdz[p + n + '.weight'], sdz[p + n + '.bias'] = torch.ones(H), torch.zeros(H)
    sdz['input_representations.LayerNorm.weight'], sdz['input_representations.LayerNorm.bias'] = torch.ones(H), torch.zeros(H)
    refz = esr.StageRef(sdz, head, cfg, rounded=True)
    z0 = refz.input_stage(feats)
    assert (refz.layer(refz.layer(z0, lengths, 0), lengths, 1) - z0).abs().max().item() < 1e-9       # the reference passes the stream through
    lost = refz._ln(esr.bf16(z0), 'encoder.layer.0.output.LayerNorm')
    m_err = (lost - z0).abs().max(dim=-1).values / z0.abs().max(dim=-1).values
    all_exceed('(v) low byte dropped, pass-through metric', m_err, esr.PASS_THROUGH)
    report['(v) under the row metric'] = esr.row_err(lost, z0)[0].min().item()
    # ---- what the old whole-tensor bound would have said at 32 032 x 768
    M = 32032
    big = torch.randn(M, H, generator=torch.Generator().manual_seed(1))
    got = big.clone()
    got[1000] = big[999]
    old = {'(i) stale row (independent rows)': esr.rel_l2(got, big)}
    got = big.clone()
    got[M - M % 128:] = big[M - M % 128 - 32:M - M % 128 - 32 + M % 128]
    old['(iii) stale ragged tail (32 rows)'] = esr.rel_l2(got, big)
    got = big.clone()
    got[1000, 5] += (2.0 ** -6) * big.norm(dim=1).pow(2).mean().sqrt()
    old['(iv) one element 2^-6'] = esr.rel_l2(got, big)
    old['(ii) wrong positional row'] = _whole_tensor(report['(ii) wrong positional row'], 1)
    old['(v) low byte dropped'] = _whole_tensor(report['(v) under the row metric'], 1)
    old['(vi) neighbour length (all 1001 rows at the smallest per-utterance worst row)'] = _whole_tensor(report['(vi) neighbour length'], 1001)
    base = 3.1e-3
    for k, v in report.items():
        print(f'planted {k}: smallest figure {v:.3e}')
    for k, v in old.items():
        verdict = 'PASSED (unseen)' if math.hypot(base, v) < 6e-3 else 'caught'
        print(f'old whole-tensor rel-L2 for {k}: {v:.3e} -> {verdict}')
    assert not missed, missed
    assert math.hypot(base, old['(iv) one element 2^-6']) < 6e-3 and math.hypot(base, old['(v) low byte dropped']) < 6e-3


def test_spec_heads_refuse_activations_their_epilogue_does_not_build():
    """SpecHead / Mockingjay hand their activation to se_spechead_fwd2_bf16, whose epilogue builds Identity / ReLU / Sigmoid: the other names that the
    linear heads accept (GELU, Exp) used to come out as Identity there"""
    from speech_enhancement_by_s3prl_amd import heads, pipeline
    ckpt = pipeline.synthetic_checkpoint(pipeline.make_config(layers=1, hidden=64, heads=1, intermediate=64))
    for act in ('ReLU', 'Sigmoid', 'Identity'):
        assert heads.SpecHead(201, ckpt, activation=act).activation == act
    for act in ('GELU', 'Exp', 'Tanh'):
        with pytest.raises(NotImplementedError):
            heads.SpecHead(201, ckpt, activation=act)
    assert heads._act_id('GELU') == 3 and heads._act_id('Exp') == 4          # still ids of the linear heads


def test_row_err_names_the_place():
    ref = torch.randn(2, 7, 16, generator=torch.Generator().manual_seed(0)).double()
    got = ref.clone()
    got[1, 4, 9] += 0.5
    err, worst = esr.row_err(got, ref)
    assert worst == (1, 4, 9) and err[1, 4] == err.max() and (err.flatten().sort().values[:-1] == 0).all()
    assert 'utterance 1, frame 4, column 9' in esr.where('layer 1', 'row-complete', worst)
    got[0, 0, 0] = float('nan')
    assert esr.row_err(got, ref)[1] == (0, 0, 0) and math.isinf(esr.row_err(got, ref)[0].max().item())
