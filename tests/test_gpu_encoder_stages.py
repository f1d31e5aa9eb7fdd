"""Per-row, per-stage parity of the inference encoder (se_encoder_fwd2_bf16) and spec head (se_spechead_fwd2_bf16) against the staged float64
reference of tests/encoder_stage_ref.py, on both dispatch paths: the GEMM + LayerNorm pairs (`unfused`) and the row-complete kernels on the
24-bit residual stream (`row-complete`, forced with fused_ln_min_rows = 1; 1 << 30 forbids it).

A stage is reached without a C entry of its own by building encoders of depth 1, 2, ... from the same weights; stage l + 1 is judged teacher-forced
from what the depth-l encoder returned (encoder_stage_ref's docstring says what that rests on; the bit-identical rerun is asserted here).  Layer 0
is judged from the reference's own input stage: the input stage has no bf16 rounding that the reference does not restate, and the input cases
below hold it to the reference on its own.  The input stage is read through a depth-1 encoder whose sublayers add nothing (zero output
matrices, LayerNorms at weight 1 / bias 0, a fixed vector c as the attention-output bias): hidden = LN(LN(x0 + c)), and the reference applies the
same to its x0.  The input LayerNorm keeps its own non-trivial weights; c makes the read-out move with a scale error of a whole row, which two
plain LayerNorms would forget (_with_offset).  An offset common to all columns of a row stays invisible there, as it is to every LayerNorm of the model.

Every case fills its outputs with NaN first and must get finite values back; every assertion names stage, path, utterance, frame and column.
Bounds: encoder_stage_ref.ROW_BOUND (2x the measured worst value per group, never above 2e-2), every value logged through conftest.bounded.

Measured on the MI355X (worst row_err.max per group -> bound):
    input stage, GEMM + LayerNorm pair          1.47e-7  -> 2.9e-7        input stage, row-complete (24-bit hops restated)   3.54e-6 -> 7.1e-6
    layer, split-K FFN2 (<= 3072 rows)          3.55e-3  -> 7.1e-3        layer, plain FFN2 (I = 192, 3073 rows)             3.82e-3 -> 7.6e-3
    layer, hidden 256                           3.47e-3  -> 6.9e-3        layer, row-complete                                3.53e-3 -> 7.1e-3
    spec head p                                 5.99e-4  -> 1.2e-3        predicted / log_predicted, elementwise             1.27e-3 -> 2.5e-3
    spec head `predicted` with negative p (log_target 0, unshifted), per row over the norm of p: 5.99e-4 under the bound of p.
    position only: 9.3e-8 / 1.2e-7 (pair, T = 101 / 5008), 2.6e-6 / 2.8e-6 (row-complete) against 1e-5; one-hot input stage 1.2e-7 / 4.7e-6 against 1e-5;
    pass-through 3.75e-5 = 2^-14.7 against 2^-12.
The silent-utterance case read 0.88 in the silent utterance's rows before the attention kernels' length rule was changed from "at least 1" to
"0 or less masks nothing" (csrc/mhsa.hip, mhsa8.hip, mhsa_bwd.hip, mhsa_x3.hip; include/se_amd.h states the contract)."""
import functools
import math

import pytest
import torch

import encoder_stage_ref as esr
from oracle import encoder as oenc

pytestmark = pytest.mark.gpu

from conftest import bounded  # noqa: E402

PATHS = {'unfused': 1 << 30, 'row-complete': 1}
K_SPLITK_ROWS = 3072


def takes_splitk(M, H, I):
    """the documented rule of the small-batch FFN2 (csrc/encoder.hip): split-K + ln_reduce_kernel, else the plain GEMM + LayerNorm"""
    return M <= K_SPLITK_ROWS and H == 768 and I % 256 == 0 and I // 4 >= 128


def _threads():
    import os
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))


def _ocfg(hidden, heads, inter, layers):
    return oenc.Config({'transformer': {'hidden_size': hidden, 'num_attention_heads': heads, 'intermediate_size': inter, 'num_hidden_layers': layers}})


@functools.lru_cache(maxsize=None)
def _weights(hidden, heads, inter, layers):
    _threads()
    return esr.stage_weights(_ocfg(hidden, heads, inter, layers), seed=11)


def _zero_sublayers(sd, layers, H, in_ln_identity):
    sd = dict(sd)
    for i in range(layers):
        p = f'encoder.layer.{i}.'
        for n in ('attention.output.dense', 'output.dense'):
            sd[p + n + '.weight'], sd[p + n + '.bias'] = torch.zeros_like(sd[p + n + '.weight']), torch.zeros_like(sd[p + n + '.bias'])
        for n in ('attention.output.LayerNorm', 'output.LayerNorm'):
            sd[p + n + '.weight'], sd[p + n + '.bias'] = torch.ones(H), torch.zeros(H)
    if in_ln_identity:
        sd['input_representations.LayerNorm.weight'], sd['input_representations.LayerNorm.bias'] = torch.ones(H), torch.zeros(H)
    return sd


def _upstream(gpu, sd, head, hidden, heads, inter, layers, path):
    from speech_enhancement_by_s3prl_amd import pipeline
    cfg = pipeline.make_config(layers=layers, hidden=hidden, heads=heads, intermediate=inter)
    ckpt = pipeline.synthetic_checkpoint(cfg)
    ckpt['Transformer'], ckpt['SpecHead'] = esr.truncate(sd, layers), head
    up = pipeline.build_upstream(ckpt, gpu)
    up._engine.fused_ln_min_rows = PATHS[path]
    up.SpecHead.spechead._engine.fused_ln_min_rows = PATHS[path]
    return up


def _encode(up, feats, lengths):
    """se_encoder_fwd2_bf16 into a NaN-filled output -> (status, hidden, workspace, workspace bytes)"""
    from speech_enhancement_by_s3prl_amd import _lib
    lib = _lib.load()
    B, T, _ = feats.shape
    eng = up._engine
    h = eng._ensure(up.model, None, feats.device)
    ws, n = eng._workspace(h, B, T, feats.device)
    H = up.model.config.hidden_size
    hidden = torch.full((B, T, H), float('nan'), device=feats.device, dtype=torch.float32)
    rc = lib.se_encoder_fwd2_bf16(h, _lib.ptr(feats), None, _lib.ptr(lengths), B, T, _lib.ptr(hidden), _lib.ptr(ws), n, _lib.stream())
    torch.cuda.synchronize()
    return rc, hidden, ws, n


def _run(gpu, sd, head, spec, layers, path, feats, lengths):
    """hidden (B, T, H) on the CPU of the depth-`layers` encoder; the rerun must be bit-identical and everything finite"""
    hidden_, heads, inter = spec
    up = _upstream(gpu, sd, head, hidden_, heads, inter, layers, path)
    f, n = feats.to(gpu).contiguous(), lengths.to(gpu).int().contiguous()
    rc, h1, _, _ = _encode(up, f, n)
    assert rc == 0, (path, layers, rc)
    rc, h2, _, _ = _encode(up, f, n)
    assert rc == 0 and torch.equal(h1, h2), f'depth {layers} [{path}]: a rerun of the same encoder is not bit-identical'
    h1 = h1.cpu()
    assert torch.isfinite(h1).all(), f'depth {layers} [{path}]: non-finite hidden states (NaN-filled output not overwritten?)'
    return h1


def _read_through(ref, x0, path):
    """what a depth-1 encoder with zeroed sublayer matrices returns for the input-stage rows x0: LN(LN(x0 + c)) with two weight-1 / bias-0 LayerNorms
    and c = the attention-output bias (zero, or the fixed vector of _with_offset); on the row-complete path the stream takes its 24-bit form in
    front of each LayerNorm (after the input stage and after the attention-output launch)"""
    q = esr.q24 if path == 'row-complete' else (lambda t: t)
    x = ref._ln(q(x0) + ref.sd['encoder.layer.0.attention.output.dense.bias'], 'encoder.layer.0.attention.output.LayerNorm')
    return ref._ln(q(x) + ref.sd['encoder.layer.0.output.dense.bias'], 'encoder.layer.0.output.LayerNorm')


def _with_offset(sdz, H):
    """A LayerNorm forgets a scale common to its whole input row, so LN(LN(x0)) alone would not see an input stage whose rows are off by a factor
    (a wrong eps, a lost rstd).  With a fixed vector c ~ N(0, 1) added in front of the first LayerNorm (the attention-output bias; its matrix stays
    zero) the read-out is LN(x0 + c), which moves with the scale of x0.  What stays invisible is an offset common to all columns of a row: every
    LayerNorm downstream removes it, in the read-out and in the model alike."""
    sdz = dict(sdz)
    sdz['encoder.layer.0.attention.output.dense.bias'] = torch.randn(H, generator=torch.Generator().manual_seed(77))
    return sdz


def _feats(B, T, lens, seed, D=80):
    f = torch.randn(B, T, D, generator=torch.Generator().manual_seed(seed))
    for b, n in enumerate(lens):
        f[b, n:] = 0.0
    return f


def _judge(name, group, path, got, ref):
    err, worst = esr.row_err(got, ref)
    v = err.max().item()
    print(f'{name} [{path}] {group}: worst row {v:.3e}  ({esr.where(name, path, worst)})')
    try:
        bounded(f'encoder_stages {name} [{path}] row_err.max', v, esr.ROW_BOUND[group])
    except AssertionError as e:
        raise AssertionError(f'{esr.where(name, path, worst)}: {v:.3e} >= {esr.ROW_BOUND[group]:.1e}') from e
    return v


def _layer_group(path, M, H, I):
    if path == 'row-complete':
        return 'layer/row-complete'
    if H != 768:
        return 'layer/unfused-256'
    return 'layer/unfused-splitk' if takes_splitk(M, H, I) else 'layer/unfused-plain'


def _check_layers(gpu, tag, path, spec, layers, feats, lengths):
    _threads()
    H, heads, I = spec
    sd, head = _weights(H, heads, I, layers)
    ref = esr.StageRef(sd, head, _ocfg(H, heads, I, layers), rounded=True)
    B, T, _ = feats.shape
    prev = ref.input_stage(feats)
    outs = []
    for depth in range(1, layers + 1):
        got = _run(gpu, sd, head, spec, depth, path, feats, lengths)
        want = ref.layer(prev, lengths, depth - 1)
        _judge(f'{tag} layer {depth - 1}', _layer_group(path, B * T, H, I), path, got, want)
        prev = got.double()
        outs.append(got)
    return outs


LAYER_CASES = [
    # id, path, (hidden, heads, I), layers, B, T, lengths
    ('U-a', 'unfused', (768, 12, 3072), 2, 2, 130, [130, 77]),
    ('U-a+len1', 'unfused', (768, 12, 3072), 2, 3, 130, [130, 77, 1]),       # two utterances cannot carry T, an interior length and 1: a third one does
    ('U-b', 'unfused', (768, 12, 192), 2, 3, 130, [130, 77, 1]),
    ('U-c-3072', 'unfused', (768, 12, 512), 1, 24, 128, [128, 77, 1] * 8),
    ('U-c-3073', 'unfused', (768, 12, 512), 1, 7, 439, [439, 200, 1, 439, 64, 65, 128]),
    ('U-d', 'unfused', (256, 4, 512), 2, 3, 65, [65, 64, 1]),
    ('F-a', 'row-complete', (768, 12, 3072), 2, 3, 101, [101, 50, 1]),
    ('F-b', 'row-complete', (768, 12, 192), 2, 1, 17, [17]),
    ('F-b+len1', 'row-complete', (768, 12, 192), 2, 3, 17, [17, 9, 1]),
    ('F-c', 'row-complete', (768, 12, 3072), 1, 2, 128, [128, 1]),
]


@pytest.mark.parametrize('case', LAYER_CASES, ids=[f'{c[0]}-{c[1]}' for c in LAYER_CASES])
def test_layers_per_row(gpu, case):
    tag, path, spec, layers, B, T, lens = case
    H, heads, I = spec
    if tag.startswith('U-c'):
        # the documented rule, not a guess at which kernel ran: 3072 rows take the split-K FFN2, 3073 the plain one, same reference for both
        assert takes_splitk(B * T, H, I) == (B * T <= K_SPLITK_ROWS) and B * T in (3072, 3073)
    if tag.startswith('U-a'):
        assert takes_splitk(B * T, H, I)
    if tag.startswith('U-b'):
        assert not takes_splitk(B * T, H, I) and (I // 64) == 3
    _check_layers(gpu, tag, path, spec, layers, _feats(B, T, lens, seed=B * 1000 + T), torch.tensor(lens))


INPUT_CASES = [('unfused', 2, 130, [130, 77]), ('unfused', 3, 101, [101, 50, 1]), ('row-complete', 3, 101, [101, 50, 1]), ('row-complete', 1, 17, [17]),
               ('row-complete', 2, 128, [128, 1])]


@pytest.mark.parametrize('path,B,T,lens', INPUT_CASES, ids=[f'{c[0]}-{c[1]}x{c[2]}' for c in INPUT_CASES])
def test_input_stage_per_row(gpu, path, B, T, lens):
    _threads()
    spec = (768, 12, 192)
    sd, head = _weights(768, 12, 192, 1)
    sdz = _with_offset(_zero_sublayers(sd, 1, 768, in_ln_identity=False), 768)      # the input LayerNorm keeps its own weights (1 + 0.1 N, 0.1 N)
    feats = _feats(B, T, lens, seed=T)
    got = _run(gpu, sdz, head, spec, 1, path, feats, torch.tensor(lens))
    ref = esr.StageRef(sdz, head, _ocfg(768, 12, 192, 1), rounded=True)
    want = _read_through(ref, ref.input_stage(feats), path)
    _judge('input stage', 'input/' + path, path, got, want)


@pytest.mark.parametrize('path', ['unfused'])
def test_input_stage_256_per_row(gpu, path):
    """hidden 256: layernorm_kernel<1> with the table, the width that can never take the row-complete kernels"""
    _threads()
    spec = (256, 4, 512)
    sd, head = _weights(256, 4, 512, 1)
    sdz = _with_offset(_zero_sublayers(sd, 1, 256, in_ln_identity=False), 256)
    lens = [65, 64, 1]
    feats = _feats(3, 65, lens, seed=65)
    got = _run(gpu, sdz, head, spec, 1, path, feats, torch.tensor(lens))
    ref = esr.StageRef(sdz, head, _ocfg(256, 4, 512, 1), rounded=True)
    want = _read_through(ref, ref.input_stage(feats), path)
    _judge('input stage (hidden 256)', 'input/unfused', path, got, want)


# ---- the spec head ---------------------------------------------------------------------------------------------------------------------------------
HEAD_ACTS = ('ReLU', 'Sigmoid', 'Identity')      # every activation the head accepts; the other ids of se_act are refused (test_spec_head_refuses_unbuilt_activations)


def _place(i, T, N):
    return f'utterance {i // (T * N)}, frame {(i // N) % T}, column {i % N}'


@pytest.mark.parametrize('path', list(PATHS))
def test_spec_head_per_row(gpu, path):
    """p per row; predicted (and log_predicted) elementwise, relative: raw given (N = 201, unpadded rows) and raw NULL (the padded internal buffer:
    204 columns, ld 208), log_target 1 and 0, the three activations the head accepts, x_bf_valid 1 (the bf16 copy the encoder's last launch left in
    the workspace) and 0 (the cast pass).  For log_target = 0 the output bias is shifted so that the reference's smallest p is 1.5 (log(p + eps),
    and a relative judgement of `predicted`); p is judged with the shift taken off again, it would only inflate the row norms.  With every p positive
    ReLU never clamps, so log_target = 0 also runs UNSHIFTED with log_predicted = NULL (log of a negative p is NaN by the formula): about half of
    the p are negative there, ReLU must give exact zeros for them, and `predicted` is judged per row by its absolute error over the RMS row
    norm of p under the bound of p (ReLU, Sigmoid and Identity are 1-Lipschitz: they cannot enlarge the error of p)."""
    from speech_enhancement_by_s3prl_amd import _lib
    _threads()
    lib = _lib.load()
    spec = (768, 12, 3072)
    H, heads, I = spec
    B, T, lens, N = 3, 101, [101, 50, 1], 201
    sd, head0 = _weights(H, heads, I, 2)
    ocfg = _ocfg(H, heads, I, 2)
    feats = _feats(B, T, lens, seed=B * 1000 + T)
    chain = esr.StageRef(sd, head0, ocfg, rounded=True)
    p0 = chain.spec_head(chain.encoder(feats, torch.tensor(lens))[-1])[0]
    shift = float(1.5 - p0.min().item())
    shifted = dict(head0)
    shifted['output.bias'] = head0['output.bias'] + shift
    up = _upstream(gpu, sd, head0, H, heads, I, 2, path)
    f, n = feats.to(gpu).contiguous(), torch.tensor(lens, device=gpu, dtype=torch.int32)
    rc, hidden, ws, nws = _encode(up, f, n)
    assert rc == 0 and torch.isfinite(hidden).all()
    hidden_cpu = hidden.cpu()
    sh = up.SpecHead.spechead
    up_s = _upstream(gpu, sd, shifted, H, heads, I, 2, path)          # only its head is used: the same trunk, the shifted output bias
    sh_s = up_s.SpecHead.spechead
    handles = {0.0: (sh._engine._ensure(None, sh, gpu), esr.StageRef(sd, head0, ocfg, rounded=True)),
               shift: (sh_s._engine._ensure(None, sh_s, gpu), esr.StageRef(sd, shifted, ocfg, rounded=True))}
    worst_p = worst_e = 0.0
    first = {}

    def call(hh, log_target, act, valid, with_raw, with_logp):
        pred = torch.full((B, T, N), float('nan'), device=gpu)
        logp = torch.full((B, T, N), float('nan'), device=gpu) if with_logp else None
        raw = torch.full((B, T, N), float('nan'), device=gpu) if with_raw else None
        rc = lib.se_spechead_fwd2_bf16(hh, _lib.ptr(hidden), B, T, log_target, _lib.SE_ACT[act], 1e-6, _lib.ptr(pred), _lib.ptr(logp), _lib.ptr(raw),
                                       _lib.ptr(ws), nws, valid, _lib.stream())
        torch.cuda.synchronize()
        return rc, pred.cpu(), None if logp is None else logp.cpu(), None if raw is None else raw.cpu()

    for valid in (1, 0):                                     # x_bf_valid = 0 rewrites the workspace's bf16 copy with the same values
        for log_target, off in ((1, 0.0), (0, shift)):
            hh, ref = handles[off]
            assert lib.se_encoder_workspace_bytes(hh, B, T) <= nws
            for act in HEAD_ACTS:
                p_ref, pred_ref, logp_ref = ref.spec_head(hidden_cpu, log_target=bool(log_target), act=act, eps=1e-6)
                if not log_target:
                    assert p_ref.min().item() > 0.5, 'the shifted bias must keep the reference p positive'
                for with_raw in (True, False):
                    name = f'spec head [{path}] x_bf_valid={valid} log_target={log_target} act={act} raw={"given" if with_raw else "NULL"}'
                    rc, pred, logp, raw = call(hh, log_target, act, valid, with_raw, True)
                    assert rc == 0, name
                    assert torch.isfinite(pred).all() and torch.isfinite(logp).all(), name + ': non-finite output'
                    if with_raw:
                        assert torch.isfinite(raw).all(), name + ': non-finite raw'
                        err, worst = esr.row_err(raw.double() - off, p_ref - off)
                        assert err.max().item() < esr.ROW_BOUND['head/p'], (esr.where(name + ' p', path, worst), err.max().item())
                        worst_p = max(worst_p, err.max().item())
                    if log_target:                           # log_predicted IS p: the padded buffer's rows judged per row through it
                        err, worst = esr.row_err(logp, p_ref)
                        assert err.max().item() < esr.ROW_BOUND['head/p'], (esr.where(name + ' log_predicted', path, worst), err.max().item())
                        worst_p = max(worst_p, err.max().item())
                        if with_raw:
                            assert torch.equal(logp, raw), name + ': log_predicted is not the raw output'
                    else:
                        e = (logp.double() - logp_ref).abs()
                        assert e.max().item() < esr.ROW_BOUND['head/predicted'], (name + ' log_predicted: ' + _place(int(e.argmax()), T, N), e.max().item())
                        worst_e = max(worst_e, e.max().item())
                    e = (pred.double() - pred_ref).abs() / pred_ref.abs()
                    assert e.max().item() < esr.ROW_BOUND['head/predicted'], (name + ' predicted: ' + _place(int(e.argmax()), T, N), e.max().item())
                    worst_e = max(worst_e, e.max().item())
                    key = (log_target, act, with_raw)        # x_bf_valid 1 / 0: the same arithmetic on the same bf16 rows
                    if key in first:
                        assert torch.equal(pred, first[key][0]) and torch.equal(logp, first[key][1]), name + ': x_bf_valid = 0 differs from x_bf_valid = 1'
                    else:
                        first[key] = (pred, logp)
    # log_target = 0 unshifted: negative p, log_predicted = NULL
    hh, ref = handles[0.0]
    worst_c = 0.0
    for act in HEAD_ACTS:
        p_ref, pred_ref, _ = ref.spec_head(hidden_cpu, log_target=False, act=act, eps=1e-6)
        neg = p_ref < -1e-2                                  # far enough below 0 that the kernel's p is negative too (its error is ~1e-3 of the row)
        assert neg.float().mean().item() > 0.25, 'the unshifted head must give negative p'
        for with_raw in (True, False):
            name = f'spec head [{path}] unshifted log_target=0 act={act} raw={"given" if with_raw else "NULL"} log_predicted=NULL'
            rc, pred, _, raw = call(hh, 0, act, 0, with_raw, False)
            assert rc == 0 and torch.isfinite(pred).all(), name
            if act == 'ReLU':
                assert (pred[neg] == 0).all() and (pred >= 0).all(), name + ': ReLU does not clamp'
            if act == 'Identity':
                assert (pred[neg] < 0).all(), name
                if with_raw:
                    assert torch.equal(pred, raw), name + ': predicted is not the raw output'
            err, worst = esr.row_err(pred.double() - pred_ref + p_ref, p_ref)      # |pred - pred_ref| per row over the RMS row norm of p
            assert err.max().item() < esr.ROW_BOUND['head/p'], (esr.where(name + ' predicted', path, worst), err.max().item())
            worst_c = max(worst_c, err.max().item())
    bounded(f'encoder_stages spec head [{path}] p row_err.max', worst_p, esr.ROW_BOUND['head/p'])
    bounded(f'encoder_stages spec head [{path}] predicted elementwise', worst_e, esr.ROW_BOUND['head/predicted'])
    bounded(f'encoder_stages spec head [{path}] predicted with negative p, per row over the norm of p', worst_c, esr.ROW_BOUND['head/p'])


@pytest.mark.parametrize('path', list(PATHS))
def test_spec_head_refuses_unbuilt_activations(gpu, path):
    """the epilogue kernels build Identity / ReLU / Sigmoid; se_act also lists GELU and Exp (the linear heads' ids).  They used to come out as Identity
    with status 0: now the C entries return an error before anything is written, and SpecHead / Mockingjay refuse them at construction
    (tests/test_encoder_stage_ref_host.py)."""
    from speech_enhancement_by_s3prl_amd import _lib
    lib = _lib.load()
    H, heads, I = 768, 12, 192
    B, T, N = 1, 17, 201
    sd, head = _weights(H, heads, I, 1)
    up = _upstream(gpu, sd, head, H, heads, I, 1, path)
    rc, hidden, ws, nws = _encode(up, _feats(B, T, [T], seed=1).to(gpu), torch.tensor([T], device=gpu, dtype=torch.int32))
    assert rc == 0
    sh = up.SpecHead.spechead
    hh = sh._engine._ensure(None, sh, gpu)
    for act in sorted(set(_lib.SE_ACT) - set(HEAD_ACTS)) + [7, -1]:
        a = _lib.SE_ACT[act] if isinstance(act, str) else act
        pred = torch.full((B, T, N), float('nan'), device=gpu)
        rc = lib.se_spechead_fwd2_bf16(hh, _lib.ptr(hidden), B, T, 1, a, 1e-6, _lib.ptr(pred), None, None, _lib.ptr(ws), nws, 0, _lib.stream())
        torch.cuda.synchronize()
        assert rc != 0 and torch.isnan(pred).all(), f'[{path}] activation {act} must be refused'
        p = torch.ones(8, device=gpu)
        out = torch.full((8,), float('nan'), device=gpu)
        rc = lib.se_spec_epilogue_f32(_lib.ptr(p), 8, 1, a, 1e-6, _lib.ptr(out), None, _lib.stream())
        torch.cuda.synchronize()
        assert rc != 0 and torch.isnan(out).all(), f'se_spec_epilogue_f32: activation {act} must be refused'


# ---- exact cases -----------------------------------------------------------------------------------------------------------------------------------
def _position_only_weights(H, heads, I, layers):
    sd, head = _weights(H, heads, I, layers)
    sd = _zero_sublayers(sd, layers, H, in_ln_identity=True)
    sd['input_representations.spec_transform.bias'] = torch.zeros(H)
    return sd, head


@pytest.mark.parametrize('path', list(PATHS))
@pytest.mark.parametrize('B,T', [(3, 101), (2, 5008)], ids=['3x101', '2x5008-kMaxPos'])
def test_position_only(gpu, path, B, T):
    """feats = 0 with explicit lengths = T, in_b = 0, every LayerNorm at weight 1 / bias 0, every sublayer output matrix 0: hidden[b, t] = LN(pe[t]) for every
    b whatever attention does.  Derived bound: fp32 accuracy (1e-5) on both paths -- what is left is the fp32 LayerNorms; on the row-complete path
    the reference restates the two 24-bit forms the stream takes on the way out (as the one-hot case; 8.7e-6 without).  T = 5008 = kMaxPos uses
    the last table row."""
    H, heads, I = 768, 12, 192
    sd, head = _position_only_weights(H, heads, I, 1)
    feats = torch.zeros(B, T, 80)
    got = _run(gpu, sd, head, (H, heads, I), 1, path, feats, torch.full((B,), T))
    pe = oenc.position_encoding(T, H, torch.float64)
    x0 = oenc.layer_norm(pe, torch.ones(H, dtype=torch.float64), torch.zeros(H, dtype=torch.float64), 1e-12)[None].expand(B, T, H)
    want = _read_through(esr.StageRef(sd, head, _ocfg(H, heads, I, 1), rounded=True), x0, path)
    err, worst = esr.row_err(got, want)
    bound = esr.EXACT_INPUT
    print(f'position only [{path}] ({B}, {T}): worst row {err.max().item():.3e}')
    bounded(f'encoder_stages position only [{path}] ({B},{T}) ' + esr.where('', path, worst), err.max().item(), bound)


@pytest.mark.parametrize('path', list(PATHS))
def test_T_above_kMaxPos_is_an_error(gpu, path):
    H, heads, I = 768, 12, 192
    sd, head = _position_only_weights(H, heads, I, 1)
    up = _upstream(gpu, sd, head, H, heads, I, 1, path)
    rc, hidden, _, _ = _encode(up, torch.zeros(1, 5009, 80, device=gpu), torch.full((1,), 5009, device=gpu, dtype=torch.int32))
    assert rc != 0 and torch.isnan(hidden).all(), f'[{path}] T = 5009 > kMaxPos must be refused before anything is written'


@pytest.mark.parametrize('path', ['row-complete'])
def test_pass_through_24bit_stream(gpu, path):
    """random features, zeroed sublayers, L = 2, forced row-complete: the stream crosses the 24-bit form 2L - 1 = 3 times and must come back as the
    input stage's rows.  Ceiling: 2^-17 per hop + fp32 LayerNorm noise -> 2^-12 of the row's largest magnitude; a stream that lost its low bytes
    reads >= 2^-9 (tests/test_encoder_stage_ref_host.py plants exactly that)."""
    _threads()
    H, heads, I = 768, 12, 3072
    B, T, lens = 3, 101, [101, 50, 1]
    sd, head = _weights(H, heads, I, 2)
    sdz = _zero_sublayers(sd, 2, H, in_ln_identity=True)
    feats = _feats(B, T, lens, seed=3101)
    got = _run(gpu, sdz, head, (H, heads, I), 2, path, feats, torch.tensor(lens)).double()
    want = esr.StageRef(sdz, head, _ocfg(H, heads, I, 2), rounded=True).input_stage(feats)
    e = (got - want).abs().max(dim=-1).values / want.abs().max(dim=-1).values
    i = int(e.argmax())
    col = int((got - want).abs()[i // T, i % T].argmax())
    print(f'pass-through: worst row {e.max().item():.3e} = 2^{math.log2(e.max().item()):.1f}')
    bounded('encoder_stages pass-through ' + esr.where('', path, (i // T, i % T, col)), e.max().item(), esr.PASS_THROUGH)


@pytest.mark.parametrize('path', list(PATHS))
def test_one_hot_features_input_stage_is_exact(gpu, path):
    """feature row m = the unit vector at column m % D, in_w / in_b small integers: the projection is exact in bf16 x bf16 -> fp32, so the input stage
    is judged at fp32 accuracy (1e-5) on both paths (read through two weight-1 / bias-0 LayerNorms, as the other input cases; on the row-complete
    path the reference restates the 24-bit form the stream takes on the way: without that the two hops alone read 1.003e-5)."""
    H, heads, I, D = 768, 12, 192, 80
    B, T = 3, 101
    sd, head = _weights(H, heads, I, 1)
    sd = _zero_sublayers(sd, 1, H, in_ln_identity=False)
    g = torch.Generator().manual_seed(5)
    sd['input_representations.spec_transform.weight'] = torch.randint(-2, 3, (H, D), generator=g).float()
    sd['input_representations.spec_transform.bias'] = torch.randint(-1, 2, (H,), generator=g).float()
    m = torch.arange(B * T)
    feats = torch.zeros(B * T, D)
    feats[m, m % D] = 1.0
    feats = feats.view(B, T, D)
    got = _run(gpu, sd, head, (H, heads, I), 1, path, feats, torch.full((B,), T))
    ref = esr.StageRef(sd, head, _ocfg(H, heads, I, 1), rounded=True)
    assert torch.equal(ref.pre_layernorm(feats), esr.StageRef(sd, head, _ocfg(H, heads, I, 1), rounded=False).pre_layernorm(feats))    # nothing to round
    want = _read_through(ref, ref.input_stage(feats), path)
    err, worst = esr.row_err(got, want)
    print(f'one-hot input stage [{path}]: worst row {err.max().item():.3e}')
    bounded(f'encoder_stages one-hot input stage [{path}] ' + esr.where('', path, worst), err.max().item(), esr.EXACT_INPUT)


@pytest.mark.parametrize('path', list(PATHS))
def test_silent_utterance_attends_to_all_keys(gpu, path):
    """utterance 1 is all zeros: se_valid_lengths_i32 gives it the length 0, the reference then adds -10000 to EVERY score of it, which cancels in
    the softmax: full attention over the T keys (as oracle/encoder.py and the fp32 mode do).  The other utterances' rows must not notice it."""
    from speech_enhancement_by_s3prl_amd import _lib
    lib = _lib.load()
    spec = (768, 12, 3072)
    B, T, lens = 3, 130, [130, 0, 70]
    feats = _feats(B, T, lens, seed=130)
    n = torch.empty(B, device=gpu, dtype=torch.int32)
    f = feats.to(gpu).contiguous()
    _lib.check(lib.se_valid_lengths_i32(_lib.ptr(f), B, T, 80, _lib.ptr(n), _lib.stream()), 'se_valid_lengths_i32')
    assert n.tolist() == lens
    outs = _check_layers(gpu, 'silent utterance', path, spec, 2, feats, n.cpu())
    sd, head = _weights(*spec, 2)
    without = _run(gpu, sd, head, spec, 2, path, feats[[0, 2]].contiguous(), torch.tensor([130, 70]))
    assert torch.equal(outs[-1][[0, 2]], without), f'[{path}] the rows of the other utterances change with a silent utterance in the batch'
