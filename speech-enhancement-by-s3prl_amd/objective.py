"""Row E1: the L1 objective of the reference (objective.py:103-117) on the gfx950 kernel, with autograd.

Criterion contract kept: forward(**all_runner_locals, **model_results) -> (loss, dict); arguments are bound
by local-variable name and the rest swallowed by **kwargs (runner.py:458,575).  Under data parallelism the
un-normalised sum and the element count are all-reduced BEFORE dividing (a global masked mean, not a mean of
per-rank means); see dist.py."""
import torch
import torch.nn as nn

from . import _lib


_L1_SCRATCH = {}      # (device, stream) -> persistent scratch of se_l1_masked_loss_f32: {ticket, -, per-workgroup partial sums}; the ticket is self-cleaning


def _l1_scratch(dev, B):
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(dev).cuda_stream)      # one per stream: calls on two streams may overlap
    n = int(_lib.load().se_l1_scratch_doubles(int(B)))
    t = _L1_SCRATCH.get(key)
    if t is None or t.numel() < n:
        t = _L1_SCRATCH[key] = torch.zeros(max(n, 1024), device=dev, dtype=torch.float64)
    return t


class _L1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, log_predicted, linear_tar, lengths, len_div, eps, reduce_fn):
        """lengths: frame counts (len_div == 0) or waveform lengths (frames = lengths // len_div + 1, runner.py:455)"""
        lib = _lib.load()
        lp = log_predicted.contiguous().float()
        tar = linear_tar.contiguous().float()
        B, F, K = lp.shape
        lens = lengths.to(device=lp.device, dtype=torch.int64).contiguous()
        sums = torch.empty(2, device=lp.device, dtype=torch.float64)
        need_grad = log_predicted.requires_grad
        grad = torch.empty_like(lp) if need_grad else None
        if reduce_fn is None:
            # one launch: sums, count AND the loss come out of the kernel (last-arriving workgroup), no zeroing launch, no division kernels
            loss = torch.empty((), device=lp.device, dtype=torch.float32)
            rc = lib.se_l1_masked_loss_f32(_lib.ptr(lp), _lib.ptr(tar), _lib.ptr(lens), int(len_div), B, F, K, float(eps), _lib.ptr(_l1_scratch(lp.device, B)),
                                           _lib.ptr(sums), _lib.ptr(loss), _lib.ptr(grad), _lib.stream())
            if rc != 0:
                # the arrival ticket is reset by the launch's LAST workgroup: after a launch that did not run to completion it may be anything, and a
                # stale ticket would leave `loss` unwritten on every later call -- start the next call from a fresh zeroed scratch
                _L1_SCRATCH.clear()
            _lib.check(rc, 'se_l1_masked_loss_f32')
            ctx.save_for_backward(grad if grad is not None else torch.empty(0), sums)
            return loss
        if len_div:
            lens = lens // int(len_div) + 1
        _lib.check(lib.se_l1_masked_f32(_lib.ptr(lp), _lib.ptr(tar), _lib.ptr(lens), B, F, K, float(eps), _lib.ptr(sums),
                                        _lib.ptr(grad), _lib.stream()), 'se_l1_masked_f32')
        if reduce_fn is not None:
            sums = reduce_fn(sums)          # all-reduce(sum) of (sum |.|, count) across ranks
        ctx.save_for_backward(grad if grad is not None else torch.empty(0), sums)
        return (sums[0] / sums[1]).float()

    @staticmethod
    def backward(ctx, g):
        sign, sums = ctx.saved_tensors
        return sign * (g / sums[1].float()), None, None, None, None, None


class L1(nn.Module):
    """objective.py:103-117.  `stft_length_masks` (B, T') is what the runner passes; the kernel takes the equivalent per-utterance frame
    counts, so either `stft_lengths` (no extra pass), the mask, or -- cheapest, nothing to compute in front -- the waveform `wav_lengths`
    with `hop` (frames = wav_lengths // hop + 1, runner.py:455)."""

    def __init__(self, eps=1e-10, **kwargs):
        super().__init__()
        self.eps = eps
        self.reduce_fn = None   # set by dist.DataParallelStep for the global masked mean

    def forward(self, log_predicted, linear_tar, stft_length_masks=None, stft_lengths=None, wav_lengths=None, hop=None, **kwargs):
        if wav_lengths is not None and hop:
            loss = _L1Fn.apply(log_predicted, linear_tar, wav_lengths, int(hop), self.eps, self.reduce_fn)
            return loss, {}
        if stft_lengths is None:
            stft_lengths = stft_length_masks.sum(dim=-1)
        loss = _L1Fn.apply(log_predicted, linear_tar, stft_lengths, 0, self.eps, self.reduce_fn)
        return loss, {}


def _frame_lengths(stft_length_masks, stft_lengths, device):
    if stft_lengths is None:
        stft_lengths = stft_length_masks.sum(dim=-1)
    return stft_lengths.to(device=device, dtype=torch.int64).contiguous()


def sisdr_loss_inference(predicted, linear_tar, lengths, len_div, eps):
    """objective.py:81-100 without autograd (evaluate(), runner.py:575): two launches -- partial sums, then loss_b and their mean -- with the
    frame counts derived inside (`lengths` = waveform lengths when len_div = hop, runner.py:455).  Returns (loss, loss_b)."""
    lib = _lib.load()
    p, t = predicted.contiguous().float(), linear_tar.contiguous().float()
    B, F, N = p.shape
    lens = lengths.to(device=p.device, dtype=torch.int64).contiguous()
    scratch = torch.empty(int(lib.se_sisdr_spec_loss_scratch_doubles(B, F, N)) + 2, device=p.device, dtype=torch.float64)
    loss_b = torch.empty(B, device=p.device, dtype=torch.float32)
    loss = torch.empty((), device=p.device, dtype=torch.float32)
    _lib.check(lib.se_sisdr_spec_loss_f32(_lib.ptr(p), _lib.ptr(t), _lib.ptr(lens), int(len_div), B, F, N, float(eps), scratch[2:].data_ptr(), _lib.ptr(loss_b),
                                          scratch.data_ptr(), _lib.ptr(loss), _lib.stream()), 'se_sisdr_spec_loss_f32')
    return loss, loss_b


class _SISDRFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, predicted, linear_tar, lens, eps, reduce_fn):
        lib = _lib.load()
        p, t = predicted.contiguous().float(), linear_tar.contiguous().float()
        B, F, N = p.shape
        scratch = torch.empty(5 * B, device=p.device, dtype=torch.float64)
        loss_b = torch.empty(B, device=p.device, dtype=torch.float32)
        grad = torch.empty_like(p) if predicted.requires_grad else None
        _lib.check(lib.se_sisdr_spec_f32(_lib.ptr(p), _lib.ptr(t), _lib.ptr(lens), B, F, N, float(eps), 1.0, _lib.ptr(scratch), _lib.ptr(loss_b),
                                         _lib.ptr(grad), _lib.stream()), 'se_sisdr_spec_f32')
        sums = torch.stack([loss_b.double().sum(), torch.full((), float(B), device=p.device, dtype=torch.float64)])      # a fill kernel: capturable in a hipGraph (torch.tensor() is a host copy)
        if reduce_fn is not None:
            sums = reduce_fn(sums)          # (sum of per-utterance losses, utterance count) across ranks: a global mean over utterances
        ctx.save_for_backward(grad if grad is not None else torch.empty(0), sums)
        return (sums[0] / sums[1]).float()

    @staticmethod
    def backward(ctx, g):
        grad, sums = ctx.saved_tensors
        return grad * (g / sums[1].float()), None, None, None, None


class SISDR(nn.Module):
    """objective.py:81-100: scale-invariant SDR between sqrt-power spectrograms, mean over the utterances of the batch."""

    def __init__(self, eps=1e-10, **kwargs):
        super().__init__()
        self.eps = eps
        self.reduce_fn = None

    def forward(self, predicted, linear_tar, stft_length_masks=None, stft_lengths=None, wav_lengths=None, hop=None, **kwargs):
        no_grad = not (torch.is_grad_enabled() and predicted.requires_grad)
        if no_grad and self.reduce_fn is None and predicted.is_cuda:
            # evaluate(): nothing differentiates the criterion and no other rank contributes -- loss and mean from two launches
            side = getattr(predicted, '_se_sisdr', None)        # heads.LinearResidual.enhance: the sums came out of the head's own launch
            if side is not None and side[1] == predicted._version and side[2] is linear_tar and side[3] == float(self.eps):
                return side[0], {}
            if wav_lengths is not None and hop:
                return sisdr_loss_inference(predicted, linear_tar, wav_lengths, int(hop), self.eps)[0], {}
            return sisdr_loss_inference(predicted, linear_tar, _frame_lengths(stft_length_masks, stft_lengths, predicted.device), 0, self.eps)[0], {}
        if stft_lengths is None and stft_length_masks is None and wav_lengths is not None and hop:
            stft_lengths = wav_lengths // int(hop) + 1
        lens = _frame_lengths(stft_length_masks, stft_lengths, predicted.device)
        return _SISDRFn.apply(predicted, linear_tar, lens, self.eps, self.reduce_fn), {}


class _WSDFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, linear_inp, offset, linear_tar, lens, alpha, db_interval, eps, reduce_fn, max_reduce_fn):
        lib = _lib.load()
        inp, off, tar = linear_inp.contiguous().float(), offset.contiguous().float(), linear_tar.contiguous().float()
        B, F, N = off.shape
        dev = off.device
        energy = torch.empty(B * F, device=dev, dtype=torch.float32)
        emax = torch.empty(1, device=dev, dtype=torch.float32)
        _lib.check(lib.se_wsd_energy_f32(_lib.ptr(tar), B, F, N, _lib.ptr(energy), _lib.ptr(emax), _lib.stream()), 'se_wsd_energy_f32')
        if max_reduce_fn is not None:
            emax = max_reduce_fn(emax)      # the reference's threshold is relative to the loudest frame of the WHOLE batch
        sums = torch.empty(3, device=dev, dtype=torch.float64)
        grad = torch.empty_like(off) if offset.requires_grad else None
        _lib.check(lib.se_wsd_f32(_lib.ptr(inp), _lib.ptr(off), _lib.ptr(tar), _lib.ptr(lens), _lib.ptr(energy), _lib.ptr(emax), B, F, N, float(alpha),
                                  float(db_interval), float(eps), 1.0, _lib.ptr(sums), _lib.ptr(grad), _lib.stream()), 'se_wsd_f32')
        tot = torch.stack([alpha * sums[0] + (1.0 - alpha) * sums[1], torch.full((), float(B), device=dev, dtype=torch.float64)])
        if reduce_fn is not None:
            tot = reduce_fn(tot)
        ctx.save_for_backward(grad if grad is not None else torch.empty(0), tot)
        return (tot[0] / tot[1]).float()

    @staticmethod
    def backward(ctx, g):
        grad, tot = ctx.saved_tensors
        return None, grad * (g / tot[1].float()), None, None, None, None, None, None, None


class WSD(nn.Module):
    """objective.py:119-153: weighted speech-distortion loss on the mask (`offset`), without the TensorBoard logger."""

    def __init__(self, alpha=0.5, db_interval=30, eps=1e-10, **kwargs):
        super().__init__()
        self.alpha, self.db_interval, self.eps = alpha, db_interval, eps
        self.reduce_fn = None
        self.max_reduce_fn = None

    def forward(self, linear_inp, offset, linear_tar, stft_length_masks=None, stft_lengths=None, **kwargs):
        lens = _frame_lengths(stft_length_masks, stft_lengths, offset.device)
        loss = _WSDFn.apply(linear_inp, offset, linear_tar, lens, self.alpha, self.db_interval, self.eps, self.reduce_fn, self.max_reduce_fn)
        return loss, {}


class _WavSISDRFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, wav_predicted, wav_tar, lens, eps, reduce_fn):
        lib = _lib.load()
        s, t = wav_predicted.contiguous().float(), wav_tar.contiguous().float()
        B, ld = s.shape
        sums = torch.empty(3 * B, device=s.device, dtype=torch.float64)
        sisdr = torch.empty(B, device=s.device, dtype=torch.float32)
        _lib.check(lib.se_sisdr_f32(_lib.ptr(s), _lib.ptr(t), ld, _lib.ptr(lens), B, float(eps), _lib.ptr(sums), _lib.ptr(sisdr), _lib.stream()), 'se_sisdr_f32')
        grad = None
        if wav_predicted.requires_grad:      # d (-sisdr_b) / d wav_predicted, zeros past each length
            grad = torch.empty_like(s)
            _lib.check(lib.se_sisdr_grad_f32(_lib.ptr(s), _lib.ptr(t), ld, _lib.ptr(lens), B, float(eps), _lib.ptr(sums), -1.0, _lib.ptr(grad),
                                             _lib.stream()), 'se_sisdr_grad_f32')
        tot = torch.stack([-sisdr.double().sum(), torch.full((), float(B), device=s.device, dtype=torch.float64)])
        if reduce_fn is not None:
            tot = reduce_fn(tot)            # (sum of per-utterance losses, utterance count) across ranks: a global mean over utterances
        ctx.save_for_backward(grad if grad is not None else torch.empty(0), tot)
        return (tot[0] / tot[1]).float()

    @staticmethod
    def backward(ctx, g):
        grad, tot = ctx.saved_tensors
        return grad * (g / tot[1].float()), None, None, None, None


class WavSISDR(nn.Module):
    """The waveform criterion the reference declares on `wav_predicted` / `wav_tar` (objective.py:16-45) with the score of evaluation.py:5-10:
    -mean_b sisdr_b over the first lengths[b] samples of each utterance.  `wants_wav` tells a training step to decode the waveform for it
    (pipeline.HeadFinetuneStep); the gradient reaches the head through decode.decode_wav."""

    wants_wav = True

    def __init__(self, eps=1e-10, **kwargs):
        super().__init__()
        self.eps = eps
        self.reduce_fn = None   # set by dist.DataParallelStep: (sum, count) all-reduced before dividing

    def forward(self, wav_predicted, wav_tar, lengths, **kwargs):
        if not (wav_predicted.is_cuda and wav_tar.is_cuda):
            raise _lib.SEError('libse_amd kernels take device tensors only (got a CPU tensor); there is no CPU fallback')
        if wav_tar.shape[-1] < wav_predicted.shape[-1]:
            raise _lib.SEError('wav_tar is shorter than wav_predicted')
        wav_tar = wav_tar[..., :wav_predicted.shape[-1]]
        lens = lengths.to(device=wav_predicted.device, dtype=torch.int64).contiguous()
        return _WavSISDRFn.apply(wav_predicted, wav_tar, lens, self.eps, self.reduce_fn), {}


class _StoiFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, wav_predicted, wav_tar, lens, sr, extended, reduce_fn):
        from .evaluation import _stoi_plan
        lib = _lib.load()
        s, t = wav_predicted.contiguous().float(), wav_tar.contiguous().float()
        B, ld = s.shape
        plan = _stoi_plan(s.device, sr)
        score = torch.empty(B, device=s.device, dtype=torch.float32)
        grad = None
        with torch.cuda.device(s.device):
            if wav_predicted.requires_grad:      # d (-stoi_b) / d wav_predicted, zeros past each length: the forward's launches, then the backward's
                nbytes = lib.se_stoi_grad_workspace_bytes(plan, B, ld)
                ws = torch.empty(max(1, nbytes), device=s.device, dtype=torch.uint8)
                grad = torch.empty_like(s)
                _lib.check(lib.se_stoi_grad_f32(plan, _lib.ptr(t), _lib.ptr(s), ld, _lib.ptr(lens), B, ld, int(extended), -1.0, _lib.ptr(score),
                                                _lib.ptr(grad), _lib.ptr(ws), nbytes, _lib.stream()), 'se_stoi_grad_f32')
            else:
                nbytes = lib.se_stoi_workspace_bytes(plan, B, ld)
                ws = torch.empty(max(1, nbytes), device=s.device, dtype=torch.uint8)
                _lib.check(lib.se_stoi_f32(plan, _lib.ptr(t), _lib.ptr(s), ld, _lib.ptr(lens), B, ld, int(extended), _lib.ptr(score), None, None,
                                           _lib.ptr(ws), nbytes, _lib.stream()), 'se_stoi_f32')
        tot = torch.stack([-score.double().sum(), torch.full((), float(B), device=s.device, dtype=torch.float64)])
        if reduce_fn is not None:
            tot = reduce_fn(tot)            # (sum of per-utterance losses, utterance count) across ranks: a global mean over utterances
        ctx.save_for_backward(grad if grad is not None else torch.empty(0), tot)
        return (tot[0] / tot[1]).float()

    @staticmethod
    def backward(ctx, g):
        grad, tot = ctx.saved_tensors
        return grad * (g / tot[1].float()), None, None, None, None, None


class stoi(nn.Module):
    """objective.py:16-29 (asteroid's NegSTOILoss on wav_predicted / wav_tar) as the negative of the project's own device score:
    -mean_b stoi_b over the first lengths[b] samples of each utterance, stoi_b what evaluation.stoi_batch returns (csrc/stoi.hip) and its
    gradient that of csrc/stoi_bwd.hip.  Parity unpinned vs asteroid / torch_stoi.  An utterance with fewer than 30 kept frames scores the
    constant 1e-5 and has a zero gradient.  `wants_wav` as WavSISDR: pipeline.HeadFinetuneStep decodes the waveform for it."""

    wants_wav = True
    extended = False

    def __init__(self, sr=16000, **kwargs):
        super().__init__()
        self.sr = sr
        self.reduce_fn = None   # set by dist.DataParallelStep: (sum, count) all-reduced before dividing

    def forward(self, wav_predicted, wav_tar, lengths=None, length_masks=None, **kwargs):
        if not (wav_predicted.is_cuda and wav_tar.is_cuda):
            raise _lib.SEError('libse_amd kernels take device tensors only (got a CPU tensor); there is no CPU fallback')
        if wav_tar.shape[-1] < wav_predicted.shape[-1]:
            raise _lib.SEError('wav_tar is shorter than wav_predicted')
        wav_tar = wav_tar[..., :wav_predicted.shape[-1]]
        if lengths is None:      # the reference's signature passes the (B, T) mask
            lengths = length_masks.sum(dim=-1)
        lens = lengths.to(device=wav_predicted.device, dtype=torch.int64).contiguous()
        return _StoiFn.apply(wav_predicted, wav_tar, lens, self.sr, self.extended, self.reduce_fn), {}


class estoi(stoi):
    """objective.py:32-45: the extended form (row- and column-normalised segments), otherwise as `stoi`."""

    extended = True


class _SpecDistFn(torch.autograd.Function):
    """One resolution of MultiResSTFT on two power planes: (B) per-utterance losses; backward = the gradient plane the forward's launches wrote
    (csrc/specdist.hip), scaled per utterance."""

    @staticmethod
    def forward(ctx, power_pred, power_tar, lens, hop, clamp):
        lib = _lib.load()
        p, t = power_pred.contiguous().float(), power_tar.contiguous().float()
        B, F, K = p.shape
        scratch = torch.empty(int(lib.se_specdist_scratch_doubles(B, F, K)), device=p.device, dtype=torch.float64)
        loss_b = torch.empty(B, device=p.device, dtype=torch.float32)
        _lib.check(lib.se_specdist_loss_f32(_lib.ptr(p), _lib.ptr(t), _lib.ptr(lens), int(hop), B, F, K, float(clamp), _lib.ptr(scratch),
                                            _lib.ptr(loss_b), _lib.stream()), 'se_specdist_loss_f32')
        grad = None
        if power_pred.requires_grad:
            grad = torch.empty_like(p)
            _lib.check(lib.se_specdist_grad_f32(_lib.ptr(p), _lib.ptr(t), _lib.ptr(lens), int(hop), B, F, K, float(clamp), _lib.ptr(scratch), 1.0,
                                                _lib.ptr(grad), _lib.stream()), 'se_specdist_grad_f32')
        ctx.save_for_backward(grad if grad is not None else torch.empty(0))
        return loss_b

    @staticmethod
    def backward(ctx, g):
        grad, = ctx.saved_tensors
        return grad * g.float()[:, None, None], None, None, None, None


class _UtteranceMeanFn(torch.autograd.Function):
    """mean over the utterances of (B) per-utterance losses; under data parallelism (sum, count) are all-reduced before dividing"""

    @staticmethod
    def forward(ctx, loss_b, reduce_fn):
        tot = torch.stack([loss_b.double().sum(), torch.full((), float(loss_b.numel()), device=loss_b.device, dtype=torch.float64)])
        if reduce_fn is not None:
            tot = reduce_fn(tot)
        ctx.save_for_backward(tot)
        ctx.n = loss_b.numel()
        return (tot[0] / tot[1]).float()

    @staticmethod
    def backward(ctx, g):
        tot, = ctx.saved_tensors
        return (g / tot[1].float()).expand(ctx.n), None


class MultiResSTFT(nn.Module):
    """The multi-resolution STFT distance of Yamamoto et al. 2020 (Parallel WaveGAN) between `wav_predicted` and `wav_tar`: at each resolution
    (n_fft, hop, win) in samples, per utterance, spectral convergence plus the mean log-magnitude L1 over the frames f < lengths[b] // hop + 1,
    with |X| = sqrt(max(power, clamp)); the loss is the mean over the utterances of the mean over the resolutions.  Both waveforms are zeroed at
    and past lengths[b] first (the reference's `wav * length_masks`, objective.py:25-26), so the gradient is exactly 0 there.  The transforms
    run on the general STFT kernels (preprocessor.stft_for_loss; a resolution outside the supported set of se_plan_create_any raises with the
    plan's message on first use), the gradient flows through se_stft_bwd_f32 and composes with decode.decode_wav.  `wants_wav` as WavSISDR."""

    wants_wav = True

    def __init__(self, resolutions=((256, 64, 256), (512, 128, 512), (1024, 256, 1024)), sample_rate=16000, clamp=1e-7, **kwargs):
        super().__init__()
        from .preprocessor import StftPlan
        self.resolutions = tuple(tuple(int(v) for v in r) for r in resolutions)
        assert self.resolutions and all(len(r) == 3 for r in self.resolutions)
        self.sample_rate, self.clamp = sample_rate, float(clamp)
        self._stfts = [StftPlan(n_fft, hop, win, sample_rate) for n_fft, hop, win in self.resolutions]      # plans: lazily, per device
        self.reduce_fn = None   # set by dist.DataParallelStep: (sum, count) all-reduced before dividing

    def forward(self, wav_predicted, wav_tar, lengths=None, length_masks=None, **kwargs):
        from .preprocessor import stft_for_loss
        if not (wav_predicted.is_cuda and wav_tar.is_cuda):
            raise _lib.SEError('libse_amd kernels take device tensors only (got a CPU tensor); there is no CPU fallback')
        if wav_tar.shape[-1] < wav_predicted.shape[-1]:
            raise _lib.SEError('wav_tar is shorter than wav_predicted')
        T = wav_predicted.shape[-1]
        if lengths is None:      # the reference's signature passes the (B, T) mask
            lengths = length_masks.sum(dim=-1)
        lens = lengths.to(device=wav_predicted.device, dtype=torch.int64).contiguous()
        keep = torch.arange(T, device=lens.device)[None, :] < lens[:, None]
        zero = torch.zeros((), device=lens.device, dtype=wav_predicted.dtype)
        pred = torch.where(keep, wav_predicted, zero)
        tar = torch.where(keep, wav_tar[..., :T].to(wav_predicted.dtype), zero).detach()
        per_res = []
        for st in self._stfts:
            hop = st._win_args['hop_length']
            per_res.append(_SpecDistFn.apply(stft_for_loss(st, pred), stft_for_loss(st, tar), lens, hop, self.clamp))
        loss_b = torch.stack(per_res).mean(dim=0)
        return _UtteranceMeanFn.apply(loss_b, self.reduce_fn), {}
