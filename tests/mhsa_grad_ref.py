"""Float64 reference for the training attention (se_mhsa_fwd_lse_bf16 -> se_mhsa_bwd_bf16) as CLOSED FORMS, no autograd, and the per-row
error metric of its parity tests.  Test infrastructure only.

With S = Q K^T / 8 (keys >= lengths[b] excluded), P = softmax(S), m = keep / (1 - p) the dropout factor (1 without dropout), dO = d(ctx):
    ctx = (P m) V      lse2 = logsumexp(S) / ln 2      D = rowsum(dO . ctx)      dP = dO V^T      dS = P (m dP - D)
    dV = (P m)^T dO    dK = dS^T Q / 8                 dQ = dS K / 8
which is what csrc/mhsa.hip and csrc/mhsa_bwd.hip implement tile by tile.  Queries >= lengths[b] are ordinary rows: they attend to the valid
keys, get a dQ and contribute to dK / dV.  tests/test_mhsa_grad_ref_host.py holds these forms to torch.autograd and to finite differences, and
shows that row_err sees planted single-row errors; tests/test_gpu_mhsa_train.py compares the kernels with them."""
import math

import torch

from oracle import encoder as oenc

HD = 64

# ---- per-row bounds (row_err.max()) of tests/test_gpu_mhsa_train.py, shared with the planted-error test ------------------------------------
# ~2x the worst value measured on the MI355X over the cases of the respective family (the convention of conftest.bounded), never above CEILING:
# P, dS and the outputs are each rounded to bf16 (2^-9 relative), so a per-row figure above 2e-2 would be a finding, not a bound to adopt.
CEILING = 2e-2
# random scores (shape cases a-f at drop 0 / 0.1 / 0.5, uniform attention).  Measured worst: ctx 1.04e-2 (e, drop 0.1), dQ 1.28e-2 (f, drop 0.1),
# dK 1.16e-2 (d, drop 0), dV 1.07e-2 (d, drop 0.5): 2x is 2.1e-2 .. 2.6e-2, so all four sit at the ceiling (1.6x .. 1.9x the measurement)
ROW_BOUND = {'ctx': CEILING, 'dQ': CEILING, 'dK': CEILING, 'dV': CEILING}
# rising maxima and scores far from zero, gradient rows over max(RMS, grad_floors).  Measured worst: ctx 3.01e-3 (rising maxima), dQ 6.80e-3
# (rising maxima), dK 3.02e-3 (level -60), dV 9.5e-4 (level +50)
ROW_BOUND_PEAKED = {'ctx': 6e-3, 'dQ': 1.4e-2, 'dK': 6e-3, 'dV': 2e-3}
TENSOR_BOUND = 6.5e-3          # whole-tensor relative L2 of test_mhsa_backward_vs_autograd, kept as a second assert

# row_err never divides by less than TINY x the RMS row norm of the whole reference tensor: an utterance of length 1 has dS = 0 exactly (one key,
# P = 1, dP = D), so its reference dQ / dK are zero while the kernel leaves the fp32 residue of dP - D, ~1e-6 of the tensor's scale
TINY = 1e-3
# Peaked families only.  A dQ row is sum_j dS_ij k_j / 8.  Where the keys are nearly parallel the sum cancels to a few percent of its terms,
# but the bf16 rounding of each dS_ij does not: the absolute error is up to 2^-9 of the UN-cancelled magnitude sum_j |dS_ij| |k_j| / 8.  The same
# holds for dK (sum_i |dS_ij| |q_i| / 8) and dV (sum_i |P m|_ij |dO_i|), and there a second thing happens: one key can carry most of the
# probability of EVERY query (identical query rows), so its row is several times the RMS of its (b, head) and its plain rounding error, taken
# over that RMS, is several times 2^-9.  grad_floors returns CANCEL x the un-cancelled magnitude per row as an absolute floor of the row's
# divisor: a row whose un-cancelled size exceeds 1 / CANCEL = 4x the RMS is judged against a quarter of that size (the bf16 rounding of the
# MFMA operand alone then reads at most 4 x 2^-9 = 7.8e-3, under CEILING), every other row against the RMS of its (b, head)
CANCEL = 0.25


CASE_D = (8, 130, 1, (1, 63, 64, 65, 127, 128, 129, 130))     # every key-tile (64) and workgroup (128) boundary falls on a length


def random_operands(B, T, heads, seed):
    """the random bf16 operands of the shape cases: qkv ~ 1.5 N(0, 1) (B T, 3 H), d_o ~ N(0, 1) (B T, H), on the CPU from a seeded generator"""
    gen = torch.Generator().manual_seed(seed)
    H = heads * HD
    return (torch.randn(B * T, 3 * H, generator=gen) * 1.5).bfloat16(), torch.randn(B * T, H, generator=gen).bfloat16()


def _split(qkv, B, T, heads):
    x = qkv.double().reshape(B, T, 3, heads, HD)
    return x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)      # (B, heads, T, 64) each


def _rows(t, B, T, heads):
    """(B * T, heads * 64) -> (B, heads, T, 64)"""
    return t.double().reshape(B, T, heads, HD).transpose(1, 2)


def _flat(t, B, T, heads):
    """(B, heads, T, 64) -> (B * T, heads * 64)"""
    return t.transpose(1, 2).reshape(B * T, heads * HD)


def effective_lengths(lengths, T):
    """the kernels' rule (include/se_amd.h): a length of 0 or less masks nothing (the reference's -10000 on every key cancels in the softmax), a
    length above T counts as T"""
    return None if lengths is None else [T if int(n) <= 0 else min(int(n), T) for n in lengths]


def _core(qkv, d_o, lengths, B, T, heads, drop, seed, site, ctx_for_D, keep):
    q, k, v = _split(qkv, B, T, heads)
    g = _rows(d_o, B, T, heads)
    n = torch.full((B,), T, dtype=torch.long) if lengths is None else torch.as_tensor(effective_lengths(lengths, T))
    s = q @ k.transpose(-1, -2) / 8.0
    s = s.masked_fill((torch.arange(T)[None, :] >= n[:, None])[:, None, None, :], float('-inf'))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    if drop > 0:
        if keep is None:
            keep = oenc.keep_mask(seed, site, B * heads * T, T, drop)
        m = keep.reshape(B, heads, T, T).double() / (1.0 - drop)
    else:
        m = torch.ones_like(p)
    pm = p * m
    ctx = pm @ v
    d_own = (g * ctx).sum(-1)
    D = d_own if ctx_for_D is None else (g * _rows(ctx_for_D, B, T, heads)).sum(-1)
    dp = g @ v.transpose(-1, -2)
    ds = p * (m * dp - D[..., None])
    return dict(q=q, k=k, v=v, g=g, p=p, pm=pm, ctx=ctx, lse2=lse / math.log(2.0), D=D, ds=ds,
                dQ=ds @ k / 8.0, dK=ds.transpose(-1, -2) @ q / 8.0, dV=pm.transpose(-1, -2) @ g)


def mhsa_train_ref(qkv, d_o, lengths, B, T, heads, drop=0.0, seed=0, site=0, ctx_for_D=None, keep=None):
    """qkv (B T, 3 heads 64), d_o (B T, heads 64): the bf16-valued operands (any dtype; used in float64).  lengths: None or B ints.
    Returns ctx (B T, H), lse2 (B, heads, T; log2 domain as the kernel stores it), D (B, heads, T), dQ, dK, dV (B T, H each), float64.
    D = rowsum(d_o . ctx) of the reference's own ctx, or of `ctx_for_D` when given (the kernel's contract is D from ITS bf16-rounded ctx); the
    gradients use that D.  The dropout keep mask is oracle.encoder.keep_mask(seed, site, B heads T, T, drop) unless `keep` overrides it."""
    c = _core(qkv, d_o, lengths, B, T, heads, drop, seed, site, ctx_for_D, keep)
    return (_flat(c['ctx'], B, T, heads), c['lse2'], c['D'], _flat(c['dQ'], B, T, heads), _flat(c['dK'], B, T, heads), _flat(c['dV'], B, T, heads))


def d_abs_sum(d_o, ctx, B, T, heads):
    """sum |d_o . ctx| per (b, head, row): the scale of D's rounding error"""
    return (_rows(d_o, B, T, heads) * _rows(ctx, B, T, heads)).abs().sum(-1)


def d_of(d_o, ctx, B, T, heads):
    """D = rowsum(d_o . ctx) (B, heads, T) in float64 from any ctx (the kernel's own, for its fp32 dot product)"""
    return (_rows(d_o, B, T, heads) * _rows(ctx, B, T, heads)).sum(-1)


def grad_floors(qkv, d_o, lengths, B, T, heads, drop=0.0, seed=0, site=0):
    """{'dQ', 'dK', 'dV'} -> (B, heads, T) absolute floors for row_err, per row: CANCEL x the un-cancelled magnitude of the row's sum (see CANCEL)"""
    c = _core(qkv, d_o, lengths, B, T, heads, drop, seed, site, None, None)
    ds = c['ds'].abs()
    return {'dQ': CANCEL * (ds @ c['k'].norm(dim=-1, keepdim=True)).squeeze(-1) / 8.0,
            'dK': CANCEL * (ds.transpose(-1, -2) @ c['q'].norm(dim=-1, keepdim=True)).squeeze(-1) / 8.0,
            'dV': CANCEL * (c['pm'].abs().transpose(-1, -2) @ c['g'].norm(dim=-1, keepdim=True)).squeeze(-1)}


def row_err(got, ref, B, T, heads, floor=None, rows=None):
    """got, ref (B T, heads 64).  For each (b, head, row): |got - ref|_2 of the 64-vector over the RMS of the row norms of `ref` in that
    (b, head) -- not over the row's own norm, so rows with a tiny true gradient do not dominate.  `rows` (B ints, for dK / dV: the lengths) limits
    the RMS to the first rows[b] rows of utterance b: the rows of padded keys are zero by construction (and asserted to be exactly zero apart from
    this), and averaging over them would only scale the figure by sqrt(T / length) -- 14x for the one live row of an utterance of length 1 in
    T = 200, whose plain 2^-9 output rounding would then read 2.6e-2.  The error itself is taken on all T rows.  The divisor is never below `floor`
    (a float, a (B, heads) or a (B, heads, T) tensor) nor below TINY x the RMS row norm of the whole tensor.  Returns the (B, heads, T) tensor and its argmax
    (b, head, row)."""
    r = _rows(ref, B, T, heads)
    diff = (_rows(got, B, T, heads) - r).norm(dim=-1)                     # (B, heads, T)
    sq = (r * r).sum(-1)
    n = torch.full((B,), T, dtype=torch.long) if rows is None else torch.as_tensor(rows).long().clamp(1, T)
    live = (torch.arange(T)[None, :] < n[:, None])[:, None, :].to(sq.dtype)       # (B, 1, T)
    rms_all = ((sq * live).sum() / (live.sum() * heads)).sqrt().item()
    den = ((sq * live).sum(-1) / n[:, None].to(sq.dtype)).sqrt().clamp(min=TINY * rms_all)      # (B, heads)
    den = den[..., None].expand_as(diff)
    if floor is not None:
        f = torch.as_tensor(floor, dtype=den.dtype)
        den = torch.maximum(den, (f[..., None] if f.dim() == 2 else f).expand_as(diff))
    err = torch.where(diff > 0, diff / den, torch.zeros_like(diff))      # 0 / 0 (an all-zero reference met exactly) is no error
    i = int(err.argmax())
    return err, (i // (heads * T), (i // T) % heads, i % T)


def rel_l2(got, ref):
    return ((got.double() - ref.double()).norm() / ref.double().norm()).item()
