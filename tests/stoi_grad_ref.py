"""Test infrastructure: a torch float64 restatement of stoi_ref.stoi_full that is differentiable in the processed signal y -- the reference of
se_stoi_grad_f32 (csrc/stoi_bwd.hip) and of objective.stoi / objective.estoi.  Parity unpinned vs asteroid / torch_stoi, which are not
installed: the criterion is the negative of the project's own score.

The keep mask and the kept indices come from stoi_ref (numpy, no grad) on the clean signal x: constants of the differentiation.  The band
envelopes use a square root whose gradient is 0 at 0 (the stated convention: d E / d Y = 0 where E == 0).  Besides the score, three figures
per utterance say how far the float64 evaluation is from a branch that an fp32 evaluation could take differently:
  margin        dB between the nearest frame energy and the keep threshold (as stoi_ref)
  clip_margin   min |c y - x clip| / (x clip) over all segment elements (STOI only; inf for ESTOI)
  clipped       the share of clipped elements (STOI only)"""
import numpy as np
import torch
import torch.nn.functional as F

import stoi_ref as R

CLIP = 1 + 10 ** (-R.BETA / 20)


class _SafeSqrt(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p):
        r = p.clamp(min=0).sqrt()
        ctx.save_for_backward(p, r)
        return r

    @staticmethod
    def backward(ctx, g):
        p, r = ctx.saved_tensors
        return torch.where(p > 0, g / (2 * r.clamp(min=1e-300)), torch.zeros_like(g))


safe_sqrt = _SafeSqrt.apply


def window():
    return torch.from_numpy(R.window())


def resample(y, p, q):
    """y[n] = sum_m x[m] g[n q - m p + L], n < ceil(len p / q): zero stuffing and a full convolution, as stoi_ref.resample"""
    if p == q:
        return y
    n10 = R.n10_of(len(y), p, q)
    if n10 == 0:
        return y[:0]
    g, L = R.taps(p, q)
    up = y.new_zeros(len(y) * p)
    up[::p] = y
    full = F.conv1d(up[None, None], torch.from_numpy(g[::-1].copy())[None, None], padding=2 * L)[0, 0]
    return full[torch.arange(n10) * q + L]


def frames(sig, count):
    """(count, 256): the windowed frames at hop 128"""
    return sig.unfold(0, R.N_FRAME, R.HOP)[:count] * window()


def compact(kept_frames):
    """overlap-add of the kept windowed frames in kept order -> (K - 1) 128 + 256 samples"""
    K = kept_frames.shape[0]
    z = kept_frames.new_zeros(1, R.HOP)
    return (torch.cat([kept_frames[:, :R.HOP], z]) + torch.cat([z, kept_frames[:, R.HOP:]])).reshape((K + 1) * R.HOP)


def spectrum(c, K):
    """(K, 257) complex: the zero-padded one-sided transform of the windowed frames of the compacted signal"""
    return torch.fft.rfft(frames(c, K), n=R.NFFT, dim=1)


def bands(spec):
    """(15, K): sqrt of the band sums of |Y|^2, gradient 0 where the sum is 0"""
    lo, hi = R.band_edges()
    pw = spec.real ** 2 + spec.imag ** 2
    return torch.stack([safe_sqrt(pw[:, lo[b]:hi[b]].sum(dim=1)) for b in range(R.NUMBAND)])


def envelopes(y, mask, fs):
    """processed signal -> (15, K) envelopes through the constant keep mask"""
    p, q = R.rate(fs)
    y10 = resample(y, p, q)
    idx = torch.from_numpy(np.nonzero(mask)[0])
    yf = frames(y10, len(mask))[idx]
    return bands(spectrum(compact(yf), len(idx)))


def _unit(a, dim):
    a = a - a.mean(dim=dim, keepdim=True)
    s = (a ** 2).sum(dim=dim, keepdim=True)
    ok = s > 0
    return a * torch.where(ok, 1.0 / torch.sqrt(torch.where(ok, s, torch.ones_like(s))), torch.zeros_like(s))


def score_of(X, Y, extended):
    """X, Y (15, K >= 30) -> (score, clip_margin, clipped share)"""
    J = X.shape[1] - R.N + 1
    xs = X.unfold(1, R.N, 1).permute(1, 0, 2)          # (J, 15, 30)
    ys = Y.unfold(1, R.N, 1).permute(1, 0, 2)
    if extended:
        xn = _unit(_unit(xs, 2), 1)
        yn = _unit(_unit(ys, 2), 1)
        return (xn * yn).sum() / (R.N * J), float('inf'), 0.0
    c = torch.linalg.vector_norm(xs, dim=2, keepdim=True) / (torch.linalg.vector_norm(ys, dim=2, keepdim=True) + R.EPS)
    a, cl = c * ys, xs * CLIP
    with torch.no_grad():
        clip_margin = float(((a - cl).abs() / cl).min())
        clipped = float((a > cl).double().mean())
    yp = torch.minimum(a, cl)
    yp = yp - yp.mean(dim=2, keepdim=True)
    xc = xs - xs.mean(dim=2, keepdim=True)
    yp = yp / (torch.linalg.vector_norm(yp, dim=2, keepdim=True) + R.EPS)
    xc = xc / (torch.linalg.vector_norm(xc, dim=2, keepdim=True) + R.EPS)
    return (yp * xc).sum() / (J * R.NUMBAND), clip_margin, clipped


def stoi_full(x, y, fs, extended=False):
    """x: clean (numpy or tensor, no grad), y: processed float64 tensor, both 1-D of one length ->
    dict(score (0-d tensor, differentiable in y), K, margin, clip_margin, clipped, frames)"""
    x = np.asarray(x.detach() if torch.is_tensor(x) else x, dtype=np.float64)
    r = R.stoi_full(x, np.zeros_like(x), fs, extended)      # the clean side: mask, margin, X
    out = dict(K=r['K'], margin=r['margin'], frames=r['frames'], clip_margin=float('inf'), clipped=0.0)
    if r['K'] < R.N:
        out['score'] = y.sum() * 0 + R.TOO_SHORT               # the constant: a zero gradient
        return out
    Y = envelopes(y, r['mask'], fs)
    out['score'], out['clip_margin'], out['clipped'] = score_of(torch.from_numpy(r['X']), Y, extended)
    return out


def batch(clean, proc, lengths, fs, extended):
    """clean, proc (B, T) arrays (the fp32 values the kernels see), lengths or None ->
    (scores (B,) float64 tensor, grad (B, T) float64 = d score_b / d proc[b] with zeros past each length, list of the per-utterance dicts)"""
    B, T = clean.shape
    scores, grads, infos = [], [], []
    for b in range(B):
        n = T if lengths is None else min(max(int(lengths[b]), 0), T)
        y = torch.tensor(np.asarray(proc[b, :n], dtype=np.float64), requires_grad=True)
        r = stoi_full(np.asarray(clean[b, :n], dtype=np.float64), y, fs, extended)
        r['score'].backward()
        g = torch.zeros(T, dtype=torch.float64)
        g[:n] = y.grad
        scores.append(r['score'].detach())
        grads.append(g)
        infos.append(r)
    return torch.stack(scores), torch.stack(grads), infos
