"""Float64 references for the gradients through the decode (iSTFT with a fixed phase -> right pad -> masked dB normalisation -> waveform
SI-SDR).  Test infrastructure only.

(a) the CHAIN: torch autograd through oracle.preprocessor.istft, oracle.decode.masked_normalize_decibel and the expression of
    oracle.objective.sisdr_eval, with the magnitudes from `safe_sqrt` (gradient 0 at P <= 0: the stated subgradient convention; torch's
    pow(0.5) gives inf / nan there);
(b) CLOSED FORMS of the three backward passes as plain tensor arithmetic -- what the kernels implement.
tests/test_decode_grad_host.py holds (b) to (a); the GPU tests compare the kernels with (a)."""
import math

import torch

from oracle import decode as odec
from oracle import preprocessor as opre


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


# ---- (a) the chain -------------------------------------------------------------------------------------------------------------
def istft_chain(power, phase, geom):
    """(B, F, K) power, phase -> (B, hop (F - 1)) through the oracle's istft (linear_power = 1 on the safe magnitudes)"""
    return opre.istft(safe_sqrt(power), phase, geom, linear_power=1)


def pad_to(wav, n):
    return torch.cat([wav, wav.new_zeros(wav.size(0), n - wav.size(1))], dim=1) if n > wav.size(1) else wav


def dbnorm_chain(wav, target, lengths):
    return odec.masked_normalize_decibel(wav, target, odec.get_length_masks(lengths, wav.size(1)))


def sisdr_expr(src, tar, eps=1e-10):
    """oracle.objective.sisdr_eval (evaluation.py:5-10) without its .item()"""
    alpha = (src * tar).sum() / ((tar * tar).sum() + eps)
    ay = alpha * tar
    norm = ((ay - src) * (ay - src)).sum() + eps
    return 10 * ((ay * ay).sum() / norm + eps).log10()


def wav_sisdr_loss(wav, tar, lengths, eps=1e-10):
    """-mean_b sisdr_b over the first lengths[b] samples"""
    return -torch.stack([sisdr_expr(wav[b, :int(lengths[b])], tar[b, :int(lengths[b])], eps) for b in range(wav.size(0))]).mean()


def decode_chain(power, phase, lengths, geom, target, out_len=None):
    """Runner._decode_wav (runner.py:266-270) on the safe magnitudes"""
    wav = istft_chain(power, phase, geom)
    return dbnorm_chain(pad_to(wav, int(max(lengths)) if out_len is None else out_len), target, lengths)


def dbnorm_grad_ref(wav, g, target, lengths):
    """autograd of the normalisation; a row whose scale is 0 (reference-audio form, nothing under the mask) is nan in torch (pow(0.5) at 0) and
    0 by the convention of the closed form: d scale / d wav = 0 there"""
    w = wav.detach().clone().requires_grad_(True)
    y = dbnorm_chain(w, target, lengths)
    (y * g).sum().backward()
    dead = torch.isnan(w.grad).any(dim=1)
    return torch.where(dead[:, None], torch.zeros_like(w.grad), w.grad), dead


# ---- (b) closed forms ------------------------------------------------------------------------------------------------------------
def window_full(geom, dtype=torch.float64):
    """periodic Hann of length win centred in n_fft"""
    w = torch.zeros(geom.n_fft, dtype=dtype)
    left = (geom.n_fft - geom.win) // 2
    w[left:left + geom.win] = torch.hann_window(geom.win, dtype=dtype)
    return w


def envelope(geom, F, dtype=torch.float64):
    """env[p] = sum over the frames f in [0, F) that contain p of w^2[p - hop f], p < hop (F - 1) + n_fft"""
    w2 = window_full(geom, dtype) ** 2
    env = torch.zeros(geom.hop * (F - 1) + geom.n_fft, dtype=dtype)
    for f in range(F):
        env[f * geom.hop:f * geom.hop + geom.n_fft] += w2
    return env


def istft_bwd_closed(g, power, phase, geom):
    """g (B, >= hop (F - 1)) = d loss / d wav -> d loss / d power (B, F, K): formula 1 of the decode-gradient specification"""
    B, F, K = power.shape
    N, m, hop = geom.n_fft, geom.n_fft // 2, geom.hop
    n_out = hop * (F - 1)
    env = envelope(geom, F, g.dtype)
    gy = g.new_zeros(B, n_out + N)
    gy[:, m:m + n_out] = g[:, :n_out] / env[m:m + n_out]
    frames = gy.unfold(-1, N, hop)                                   # (B, F, N), zero padded
    G = torch.fft.rfft(frames * window_full(geom, g.dtype), dim=-1)
    ck = torch.full((K,), 2.0, dtype=g.dtype)
    ck[0] = ck[m] = 1.0
    d_re = ck / N * G.real
    d_im = ck / N * G.imag
    d_im[..., 0] = 0
    d_im[..., m] = 0
    num = d_re * phase.cos() + d_im * phase.sin()
    return torch.where(power > 0, num / (2 * power.clamp(min=1e-300).sqrt()), torch.zeros_like(num))


def dbnorm_bwd_closed(wav, g, target, lengths, eps=1e-8):
    """formula 2.  With y = scale wav:  d wav[n] = scale g[n] - [n < len] y[n] (sum g y) / (scale M (len + eps));  scale = 0 -> scale g"""
    B, T = wav.shape
    mask = (torch.arange(T)[None, :] < lengths[:, None]).to(wav.dtype)
    cnt = mask.sum(dim=1) + eps
    M = (wav * wav * mask).sum(dim=1) / cnt + eps
    if isinstance(target, (int, float)):
        R = torch.full((B,), 10.0 ** (target / 10.0), dtype=wav.dtype)
    else:
        R = (target[:, :T] ** 2 * mask).sum(dim=1) / cnt
    scale = (R / M).sqrt()
    y = wav * scale[:, None]
    dot = (g * y).sum(dim=1)
    coef = torch.where(scale > 0, dot / (scale.clamp(min=1e-300) * M * cnt), torch.zeros_like(dot))
    return scale[:, None] * g - mask * y * coef[:, None]


def sisdr_coeffs(a, b, c, eps=1e-10):
    """formula 3: d sisdr / d s[n] = p t[n] + q s[n] from a = <s,t>, b = <t,t>, c = <s,s>"""
    alpha = a / (b + eps)
    E = alpha * alpha * b
    Q = E - 2 * alpha * a + c + eps
    k = 10.0 / (math.log(10.0) * (E / Q + eps))
    e1 = 2 * alpha * b / (b + eps)
    r1 = (2 * alpha * b - 2 * a) / (b + eps)
    return k * (e1 / Q - E * (r1 - 2 * alpha) / Q ** 2), k * (-2 * E / Q ** 2)


def encode_phase(phase):
    """the encoded phase word of se_stft_tphase_f32 from an angle: fp32 t = tan(half the angle of (|cos|, sin)) with bit 0 = (cos < 0), as int32"""
    c, s = phase.double().cos(), phase.double().sin()
    t = (s / (1.0 + c.abs())).float().contiguous()
    bits = t.view(torch.int32)
    return (bits & ~1) | (c < 0).to(torch.int32)


def harmonic_batch(B, T, sample_rate, seed):
    """seeded harmonic signals (B, T): a few partials of a per-utterance fundamental with random amplitudes and phases"""
    gen = torch.Generator().manual_seed(seed)
    t = torch.arange(T, dtype=torch.float64) / sample_rate
    out = []
    for _ in range(B):
        f0 = (0.01 + 0.02 * torch.rand((), generator=gen).item()) * sample_rate
        x = torch.zeros(T, dtype=torch.float64)
        for h in range(1, 9):
            if h * f0 < 0.45 * sample_rate:
                amp = torch.rand((), generator=gen).item() / h
                x += amp * torch.sin(2 * math.pi * h * f0 * t + 6.28 * torch.rand((), generator=gen).item())
        out.append(0.1 * x)
    return torch.stack(out)
