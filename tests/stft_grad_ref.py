"""Float64 references for the gradients through the analysis transform and the multi-resolution STFT criterion.  Test infrastructure only.

(a) the RESTATEMENT: torch autograd through oracle.preprocessor.stft, with the clamp, the masking, the per-utterance sums and the loss of
    objective.MultiResSTFT written out;
(b) CLOSED FORMS without autograd -- what csrc/stftg_bwd.hip and csrc/specdist.hip implement: the adjoint of reflect padding + framing +
    window + one-sided real transform, and the criterion's per-utterance coefficients.
tests/test_stft_grad_host.py holds (b) to (a); the GPU tests compare the kernels with (b) and the criterion with (a)."""
import torch

from oracle import preprocessor as opre

CLAMP = 1e-7
SC_EPS = 1e-12
RESOLUTIONS = ((256, 64, 256), (512, 128, 512), (1024, 256, 1024))


def geometry(n_fft, hop, win, sample_rate=16000):
    """the oracle's Geometry for a resolution given in samples"""
    g = opre.Geometry(sample_rate=sample_rate, n_freq=n_fft // 2 + 1)
    g.win, g.hop = int(win), int(hop)
    return g


def window_full(geom, dtype=torch.float64):
    """periodic Hann of length win centred in n_fft"""
    w = torch.zeros(geom.n_fft, dtype=dtype)
    left = (geom.n_fft - geom.win) // 2
    w[left:left + geom.win] = torch.hann_window(geom.win, dtype=dtype)
    return w


# ---- (a) the restatement ---------------------------------------------------------------------------------------------------------
def spectrum(wav, geom):
    """(B, T) -> complex (B, F, K): the analysis through the oracle, time-major as se_stft_f32 writes it"""
    return opre.stft(wav, geom).transpose(-1, -2)


def power_of(wav, geom):
    X = spectrum(wav, geom)
    return X.real ** 2 + X.imag ** 2


def mask_wav(wav, lengths):
    """zero at and past lengths[b] (the reference's wav * length_masks)"""
    keep = torch.arange(wav.shape[1])[None, :] < torch.as_tensor(lengths)[:, None]
    return torch.where(keep, wav, torch.zeros((), dtype=wav.dtype))


def frame_counts(lengths, hop, F):
    """frames f < lengths[b] / hop + 1 (runner.py:455), none for an empty utterance"""
    return [min(F, int(L) // hop + 1) if int(L) > 0 else 0 for L in lengths]


def magnitudes(power, clamp=CLAMP):
    """sqrt(max(P, clamp)) with gradient exactly 0 where P <= clamp"""
    return torch.where(power > clamp, power, torch.full_like(power, clamp)).sqrt()


def specdist_sums(p_pred, p_tar, lengths, hop, clamp=CLAMP):
    """per utterance (a, c, l, n) over the counted frames"""
    B, F, K = p_pred.shape
    X, Y = magnitudes(p_pred, clamp), magnitudes(p_tar, clamp)
    out = []
    for b, nf in enumerate(frame_counts(lengths, hop, F)):
        x, y = X[b, :nf], Y[b, :nf]
        out.append((((y - x) ** 2).sum(), (y * y).sum(), (y.log() - x.log()).abs().sum(), nf * K))
    return out


def specdist_loss_b(p_pred, p_tar, lengths, hop, clamp=CLAMP):
    """(B): sqrt(a) / (sqrt(c) + 1e-12) + l / max(n, 1); the sc term has gradient 0 at a == 0"""
    rows = []
    for a, c, l, n in specdist_sums(p_pred, p_tar, lengths, hop, clamp):
        ra = torch.where(a > 0, a, torch.ones_like(a)).sqrt() * (a > 0)
        rows.append(ra / (c.sqrt() + SC_EPS) + l / max(n, 1))
    return torch.stack(rows)


def multires_loss_b(wav_pred, wav_tar, lengths, resolutions=RESOLUTIONS, sample_rate=16000, clamp=CLAMP):
    """(B): mean over the resolutions of the per-utterance distance of the masked waveforms"""
    wp, wt = mask_wav(wav_pred, lengths), mask_wav(wav_tar, lengths)
    per = []
    for n_fft, hop, win in resolutions:
        g = geometry(n_fft, hop, win, sample_rate)
        per.append(specdist_loss_b(power_of(wp, g), power_of(wt, g), lengths, hop, clamp))
    return torch.stack(per).mean(dim=0)


def multires_loss(wav_pred, wav_tar, lengths, **kw):
    return multires_loss_b(wav_pred, wav_tar, lengths, **kw).mean()


def counted_power_floor(wav_pred, wav_tar, lengths, resolutions=RESOLUTIONS, sample_rate=16000):
    """the smallest power of either masked signal over every counted bin of every resolution"""
    wp, wt = mask_wav(wav_pred, lengths), mask_wav(wav_tar, lengths)
    low = float('inf')
    for n_fft, hop, win in resolutions:
        g = geometry(n_fft, hop, win, sample_rate)
        for P in (power_of(wp, g), power_of(wt, g)):
            for b, nf in enumerate(frame_counts(lengths, hop, P.shape[1])):
                if nf:
                    low = min(low, P[b, :nf].min().item())
    return low


# ---- (b) closed forms ------------------------------------------------------------------------------------------------------------
def spectral_gradient(grad_power, grad_complx, X):
    """G = grad_complx + 2 grad_power X (complex (B, F, K)); either gradient may be None"""
    G = torch.zeros_like(X)
    if grad_complx is not None:
        G = G + grad_complx
    if grad_power is not None:
        G = G + 2 * grad_power * X
    return G


def stft_bwd_closed(G, T, geom):
    """complex G (B, F, K) = d loss / d (re, im) -> d loss / d wav (B, T):
       gy_f[n] = Re sum_{k <= m} G_{f,k} e^{+2 pi i k n / N};  gpad = overlap-add of w gy_f (no envelope);  fold of the reflect padding"""
    B, F, K = G.shape
    N, m, hop = geom.n_fft, geom.n_fft // 2, geom.hop
    assert K == m + 1 and F == T // hop + 1 and T > m
    ck = torch.full((K,), 2.0, dtype=torch.float64)
    ck[0] = ck[m] = 1.0
    gy = torch.fft.irfft(G / ck, n=N, dim=-1) * N          # c2r: the imaginary parts at k = 0 and k = m contribute nothing
    gy = gy * window_full(geom)
    gpad = torch.zeros(B, T + 2 * m, dtype=torch.float64)
    for f in range(F):
        gpad[:, f * hop:f * hop + N] += gy[:, f]
    grad = gpad[:, m:m + T].clone()
    n = torch.arange(1, m + 1)
    grad[:, n] += gpad[:, m - n]
    n = torch.arange(T - 1 - m, T - 1)
    grad[:, n] += gpad[:, 2 * (T - 1) + m - n]
    return grad


def specdist_grad_closed(p_pred, p_tar, lengths, hop, clamp=CLAMP):
    """d loss_b / d p_pred (B, F, K) from the per-utterance sums:
       [ (|X| - |Y|) / (sqrt(a) (sqrt(c) + 1e-12)) - sign(log|Y| - log|X|) / (n |X|) ] / (2 |X|) on the counted frames where P > clamp"""
    B, F, K = p_pred.shape
    X, Y = magnitudes(p_pred, clamp), magnitudes(p_tar, clamp)
    grad = torch.zeros_like(p_pred)
    sums = specdist_sums(p_pred, p_tar, lengths, hop, clamp)
    for b, nf in enumerate(frame_counts(lengths, hop, F)):
        a, c, _, n = sums[b]
        csc = 1.0 / (a.sqrt() * (c.sqrt() + SC_EPS)) if a > 0 else 0.0
        x, y = X[b, :nf], Y[b, :nf]
        d = ((x - y) * csc - torch.sign(y.log() - x.log()) / (max(n, 1) * x)) / (2 * x)
        grad[b, :nf] = torch.where(p_pred[b, :nf] > clamp, d, torch.zeros_like(d))
    return grad


def noisy_pair(B, T, sample_rate, seed, snr_db=5.0, gain=1.0):
    """(target, predicted): the same seeded harmonic signals, each plus white noise of its own at snr_db, times `gain` (the criterion does not
    depend on a common gain except through the clamp)"""
    import decode_grad_ref as D
    clean = D.harmonic_batch(B, T, sample_rate, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    out = []
    for _ in range(2):
        noise = torch.randn(B, T, generator=gen, dtype=torch.float64)
        scale = (clean.pow(2).mean(dim=1) / noise.pow(2).mean(dim=1) / 10 ** (snr_db / 10)).sqrt()
        out.append(gain * (clean + scale[:, None] * noise))
    return out[0], out[1]
