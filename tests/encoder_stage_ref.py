"""Float64 reference of the inference encoder and spec head ONE STAGE AT A TIME, and the per-row metric of their parity tests.  Test
infrastructure only: no autograd, no project code beyond oracle/encoder.py's position_encoding, gelu and layer_norm.

    input_stage(feats)              B1: projection + sinusoid table + LayerNorm
    layer(x_prev, lengths, i)       B2 + B3 of layer i from the previous hidden states
    spec_head(hidden, ...)          B4 + the exp / log / activation epilogue

With `rounded=True` the reference rounds to bf16 exactly where se_encoder_fwd2_bf16 / se_spechead_fwd2_bf16 do:
  * every weight matrix (biases, LayerNorm parameters and the sinusoid table stay fp32 there, float64 here);
  * the query rows of the fused QKV weight and bias the way se_encoder_create makes `qkv_w_inf` / `qkv_b_inf`: scaled by log2(e) / 8 in fp32
    FIRST, then the weight rounded to bf16 (the bias stays fp32); the softmax is then taken in base 2 with no further scale;
  * the GEMM operands: x_bf (the bf16 copy of the stream that QKV, FFN1 and the head's dense read), qkv, ctx, h;
  * the spec head's normalised rows (the output GEMM's operand);
  * the input rows (cast_pad_kernel: bf16, zero-padded to 128 columns -- zeros add nothing to a dot product, so the padding has no arithmetic).
What is left between it and the kernels: the accumulation order of the fp32 MFMA sums, the attention kernel's bf16 probabilities (P is rounded
before P V), and the fp32 LayerNorm / GELU / exp.  `rounded=False` switches every rounding off: the chain is then oracle.encoder in float64
(tests/test_encoder_stage_ref_host.py holds it to 1e-10).

Masking: keys at or beyond the valid length are excluded; a length of 0 (or less) means all T keys, as in the reference, whose -10000 on every
score of such an utterance cancels in the softmax.

How the GPU test reaches a stage without a C entry per stage (tests/test_gpu_encoder_stages.py): encoders of depth 1, 2, ... are built from the SAME
weights (a checkpoint truncated to its first l layers).  Stage l + 1 is judged TEACHER-FORCED: the hidden states the depth-l encoder returned go
through `layer(., ., l)` here and are compared with what the depth-(l + 1) encoder returned.  This rests on two things:
  * layers 1..l of both encoders run the same kernels on the same data: the kernels take no atomics-ordered sums on this path, and the test asserts
    that a rerun of the same encoder is bit-identical, so this is shown, not supposed;
  * the depth-l encoder returns fp32, while the depth-(l + 1) encoder's internal stream is fp32 (GEMM + LayerNorm pair: identical) or, on the
    row-complete path, the 24-bit form of the same value (bf16 + int8, csrc/gemm4.hip): a 2^-17 relative difference, far below every bound here.
"""
import math

import torch

from oracle import encoder as oenc

Q_SCALE_F32 = torch.tensor(0.125, dtype=torch.float32) * torch.tensor(1.44269504088896340736, dtype=torch.float32)     # encoder_impl.h: kQScale

# ---- per-row bounds (row_err.max()) of tests/test_gpu_encoder_stages.py, shared with the planted-error test --------------------------------------
# 2x the worst value measured on the MI355X against THIS reference over the cases of the group (the convention of conftest.bounded), never above
# CEILING = 2e-2, the max-norm bound test_encoder_small_vs_oracle already applies to the whole tensor: above it the per-row metric would be no
# sharper than what the suite had.  Measured values: see ROW_MEASURED.
CEILING = 2e-2
ROW_MEASURED = {                                   # worst row_err.max() over the cases of the group (the log that conftest.bounded keeps)
    'input/unfused': 1.467e-7,                     # hidden 256; 1.29e-7 at 768.  fp32 accumulation order and the fp32 LayerNorms: nothing else is left
    'input/row-complete': 3.539e-6,                # read through two 24-bit hops that the reference restates (q24); 1.05e-5 without restating them
    'layer/unfused-splitk': 3.552e-3,              # U-c at 3072 rows; U-a 3.28e-3, the silent-utterance batch 3.36e-3
    'layer/unfused-plain': 3.817e-3,               # U-b; U-c at 3073 rows 3.59e-3
    'layer/unfused-256': 3.468e-3,                 # U-d
    'layer/row-complete': 3.533e-3,                # F-c; F-a 3.36e-3, F-b 3.52e-3
    'head/p': 5.990e-4,                            # GEMM + LayerNorm pair; the row-complete dense -> GELU -> LayerNorm kernel 1.340e-4
    'head/predicted': 1.267e-3,                    # elementwise relative, GEMM + LayerNorm pair; row-complete 2.26e-4
}
ROW_BOUND = {k: min(CEILING, float(f'{2.0 * v:.1e}')) for k, v in ROW_MEASURED.items()}
EXACT_INPUT = 1e-5            # one-hot features, integer weights: the pre-LayerNorm row is exact, what is left is the fp32 LayerNorm
PASS_THROUGH = 2.0 ** -12     # 2L - 1 hops through the 24-bit form at 2^-17 each + fp32 LayerNorm noise; a stream that lost its low bytes reads >= 2^-9


def bf16(t):
    """round to nearest even through fp32, as the kernels' f2bf / pack_bf16x2 do, back in float64"""
    return t.float().bfloat16().double()


def q24(t):
    """the 24-bit form in which the row-complete path keeps its residual stream between launches (csrc/gemm4.hip): hi = the round-to-nearest bf16 of
    the fp32 value y, lo = min((bits(y) - (hi << 16) + 128) >> 8, 127) as a signed byte, decoded as the bit pattern (hi << 16) + (lo << 8).  The
    layer bounds ignore its 2^-17; the cases that hold the row-complete input stage to fp32 accuracy cannot, since they read it through a depth-1
    encoder whose stream takes this form twice on the way out."""
    y = t.float().contiguous()
    bits = y.view(torch.int32).long() & 0xffffffff
    hi = ((bits + 0x7fff + ((bits >> 16) & 1)) >> 16) & 0xffff
    d = (bits - (hi << 16)) & 0xffffffff
    d = torch.where(d >= 0x80000000, d - 0x100000000, d)                   # the signed 32-bit difference
    lo = torch.clamp((d + 128) >> 8, max=127)
    out = ((hi << 16) + (lo << 8)) & 0xffffffff
    out = torch.where(out >= 0x80000000, out - 0x100000000, out).to(torch.int32)
    return out.view(torch.float32).double().reshape(t.shape)


def _ident(t):
    return t.double()


def valid_keys(lengths, B, T):
    """(B, T) bool: key t of utterance b takes part.  0 or less: all T keys; above T: T."""
    n = torch.as_tensor(lengths).long().reshape(B)
    n = torch.where(n <= 0, torch.full_like(n, T), n.clamp(max=T))
    return torch.arange(T)[None, :] < n[:, None]


class StageRef:
    """sd / head: state dicts with S3PRL's key names (oracle/encoder.py), cfg: oracle.encoder.Config."""

    def __init__(self, sd, head, cfg, rounded=True):
        self.sd = {k: v.double() for k, v in sd.items()}
        self.head = None if head is None else {k: v.double() for k, v in head.items()}
        self.cfg = cfg
        self.rounded = rounded
        self.r = bf16 if rounded else _ident

    def _lin(self, x, name, sd=None):
        sd = self.sd if sd is None else sd
        return x @ self.r(sd[name + '.weight']).t() + sd[name + '.bias']

    def _ln(self, x, name, sd=None):
        sd = self.sd if sd is None else sd
        return oenc.layer_norm(x, sd[name + '.weight'], sd[name + '.bias'], self.cfg.layer_norm_eps)

    def pre_layernorm(self, feats):
        """the input projection + the positional row, before the LayerNorm (B, T, H)"""
        B, T, _ = feats.shape
        x = self._lin(self.r(feats.double()), 'input_representations.spec_transform')
        return x + oenc.position_encoding(T, self.cfg.hidden_size, torch.float64)[None]

    def input_stage(self, feats):
        return self._ln(self.pre_layernorm(feats), 'input_representations.LayerNorm')

    def attention(self, x_prev, lengths, i, want_probs=False):
        """ctx (B, T, H) of layer i (rounded as the kernel's output), optionally the probabilities (B, heads, T, T)"""
        B, T, H = x_prev.shape
        nh = self.cfg.num_attention_heads
        dh = H // nh
        p = f'encoder.layer.{i}.attention.self.'
        sd = self.sd
        xb = self.r(x_prev.double())
        if self.rounded:
            wq = (sd[p + 'query.weight'].float() * Q_SCALE_F32).bfloat16().double()
            bq = (sd[p + 'query.bias'].float() * Q_SCALE_F32).double()
        else:
            wq = sd[p + 'query.weight'] * (math.log2(math.e) / 8.0)
            bq = sd[p + 'query.bias'] * (math.log2(math.e) / 8.0)
        q = self.r(xb @ wq.t() + bq)
        k = self.r(self._lin(xb, p + 'key'))
        v = self.r(self._lin(xb, p + 'value'))
        q = q.view(B, T, nh, dh).permute(0, 2, 1, 3)
        k = k.view(B, T, nh, dh).permute(0, 2, 1, 3)
        v = v.view(B, T, nh, dh).permute(0, 2, 1, 3)
        s2 = q @ k.transpose(-1, -2)                                     # base-2 scores: log2(e) / 8 rides the queries
        s2 = s2.masked_fill(~valid_keys(lengths, B, T)[:, None, None, :], float('-inf'))
        pr = torch.exp2(s2 - s2.max(dim=-1, keepdim=True).values)
        pr = pr / pr.sum(-1, keepdim=True)
        ctx = self.r((pr @ v).permute(0, 2, 1, 3).reshape(B, T, H))
        return (ctx, pr) if want_probs else ctx

    def layer_parts(self, x_prev, lengths, i):
        """every intermediate of layer i: a = attention-output dense (before the residual add), x1, o = FFN-output dense (before the add), x2"""
        p = f'encoder.layer.{i}.'
        x_prev = x_prev.double()
        ctx, pr = self.attention(x_prev, lengths, i, want_probs=True)
        a = self._lin(ctx, p + 'attention.output.dense')
        x1 = self._ln(a + x_prev, p + 'attention.output.LayerNorm')
        h = self.r(oenc.gelu(self._lin(self.r(x1), p + 'intermediate.dense')))
        o = self._lin(h, p + 'output.dense')
        x2 = self._ln(o + x1, p + 'output.LayerNorm')
        return dict(probs=pr, ctx=ctx, a=a, x1=x1, h=h, o=o, x2=x2)

    def layer(self, x_prev, lengths, i):
        return self.layer_parts(x_prev, lengths, i)['x2']

    def encoder(self, feats, lengths):
        """the chained reference: [input stage, layer 0, layer 1, ...]"""
        outs = [self.input_stage(feats)]
        for i in range(self.cfg.num_hidden_layers):
            outs.append(self.layer(outs[-1], lengths, i))
        return outs

    def spec_head(self, hidden, log_target=True, act='ReLU', eps=1e-6):
        """-> p (the raw linear output), predicted, log_predicted, each (B, T, N)"""
        hd = self.head
        d = oenc.gelu(self._lin(self.r(hidden.double()), 'dense', hd))
        n = self.r(self._ln(d, 'LayerNorm', hd))
        p = self._lin(n, 'output', hd)
        if log_target:
            pred, logp = p.exp(), p
        else:
            pred, logp = p, (p + eps).log()
        pred = {'ReLU': torch.relu, 'Sigmoid': torch.sigmoid, 'Identity': lambda t: t}[act](pred)
        return p, pred, logp


# ---- test weights that make errors visible -------------------------------------------------------------------------------------------------------
# oracle.encoder.init_weights' N(0, 0.02) matrices make every sublayer a small correction to the residual (a wrong attention output would move the
# hidden states by a fraction of it) and the softmax nearly uniform (a wrong mask or a stale key tile would barely move the context).  The weights
# are therefore scaled, layer by layer, on a fixed probe batch in float64: W_q, W_k so that the base-e scores have standard deviation SCORE_STD, the
# attention-output and FFN-output matrices so that the RMS of what they add equals the RMS of the residual it is added to, the input projection so
# that it matches the RMS of the positional table, the head's dense to unit pre-activations.  tests/test_encoder_stage_ref_host.py checks the result.
SCORE_STD = 4.0
PROBE = (2, 130)


def rms(t):
    return t.double().pow(2).mean().sqrt().item()


def probe_feats(inp_dim, B=PROBE[0], T=PROBE[1], seed=1234):
    return torch.randn(B, T, inp_dim, generator=torch.Generator().manual_seed(seed))


def stage_weights(cfg, inp_dim=80, spec_out=201, seed=0):
    """(sd, head) fp32 state dicts: oracle.encoder.init_weights(seed) scaled as described above.  Layer l's scales depend on layers < l only, so a
    shallower encoder's weights are the first layers of a deeper one's."""
    sd, head = oenc.init_weights(cfg, inp_dim, seed=seed, spec_out=spec_out)
    sd = {k: v.double() for k, v in sd.items()}
    head = {k: v.double() for k, v in head.items()}
    ref = StageRef(sd, head, cfg, rounded=False)
    sd = ref.sd                                             # scale in place what the reference reads
    feats = probe_feats(inp_dim)
    B, T, _ = feats.shape
    lengths = torch.full((B,), T)
    H, nh = cfg.hidden_size, cfg.num_attention_heads

    def scale(name, s):
        sd[name + '.weight'] *= s
        sd[name + '.bias'] *= s
    proj = ref._lin(feats.double(), 'input_representations.spec_transform')
    scale('input_representations.spec_transform', math.sqrt(0.5) / rms(proj))
    x = ref.input_stage(feats)
    for i in range(cfg.num_hidden_layers):
        p = f'encoder.layer.{i}.'
        q = ref._lin(x, p + 'attention.self.query').view(B, T, nh, H // nh).permute(0, 2, 1, 3)
        k = ref._lin(x, p + 'attention.self.key').view(B, T, nh, H // nh).permute(0, 2, 1, 3)
        s = math.sqrt(SCORE_STD / (q @ k.transpose(-1, -2) / 8.0).std().item())
        scale(p + 'attention.self.query', s)
        scale(p + 'attention.self.key', s)
        parts = ref.layer_parts(x, lengths, i)
        scale(p + 'attention.output.dense', rms(x) / rms(parts['a']))
        parts = ref.layer_parts(x, lengths, i)
        scale(p + 'output.dense', rms(parts['x1']) / rms(parts['o']))
        x = ref.layer(x, lengths, i)
    pre = x @ head['dense.weight'].t() + head['dense.bias']
    head['dense.weight'] *= 1.0 / rms(pre)
    head['dense.bias'] *= 1.0 / rms(pre)
    return {k: v.float() for k, v in sd.items()}, {k: v.float() for k, v in head.items()}


def truncate(sd, layers):
    """the state dict of the first `layers` layers"""
    keep = {}
    for k, v in sd.items():
        if k.startswith('encoder.layer.') and int(k.split('.')[2]) >= layers:
            continue
        keep[k] = v
    return keep


# ---- the metric ------------------------------------------------------------------------------------------------------------------------------------
def row_err(got, ref):
    """got, ref (B, T, H).  Per row: |got - ref|_2 over the RMS of the row norms of `ref` in that utterance (as tests/mhsa_grad_ref.py does per
    (utterance, head)): not over the row's own norm, so a row with a small true value does not dominate.  Returns (err (B, T), (b, t, col)): the
    worst (utterance, frame) and the column of that row's largest element error.  A NaN anywhere reads as inf."""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape and got.dim() == 3, (got.shape, ref.shape)
    B, T, _ = ref.shape
    diff = (got - ref).norm(dim=-1)
    den = ref.pow(2).sum(-1).mean(dim=1, keepdim=True).sqrt()                 # (B, 1)
    err = torch.where(diff > 0, diff / den, torch.zeros_like(diff))          # 0 / 0 (an all-zero reference met exactly) is no error
    err = torch.where(torch.isfinite(diff), err, torch.full_like(err, float('inf')))
    i = int(err.argmax())
    b, t = i // T, i % T
    col = int(torch.nan_to_num((got[b, t] - ref[b, t]).abs(), nan=float('inf')).argmax())
    return err, (b, t, col)


def where(stage, path, worst):
    """the text every assertion of the stage tests carries"""
    return f'{stage} [{path}] worst row: utterance {worst[0]}, frame {worst[1]}, column {worst[2]}'


def rel_l2(got, ref):
    return ((got.double() - ref.double()).norm() / ref.double().norm()).item()
