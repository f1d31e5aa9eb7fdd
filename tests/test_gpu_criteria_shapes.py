"""GPU parity of the criteria (csrc/l1.hip, the SISDR and WSD kernels of csrc/objectives.hip) and of the decode reductions (masked_sumsq_kernel,
dbnorm_kernel, length_masks_kernel of csrc/istft.hip) against float64 references, at the shapes where their launch rules change.

References: oracle/objective.py on .double() inputs with float64 autograd, oracle/decode.py for the normalisation.  Losses and sums are held to
1e-4 relative, gradients and waveforms to max|a - b| <= 1e-4 max|b| per utterance.

Grid rules crossed by SHAPES (B, F, N): L1 launches min(max(1, min(64, 512 / B)), ceil(F N / 256)) workgroups per utterance; the SISDR / WSD
kernels max(1, min(64, ceil(F N / 8192))), the SISDR loss form additionally at most max(1, 2048 / B)."""
import functools
import math

import pytest
import torch

from conftest import bounded
from oracle import decode as odec
from oracle import objective as oobj

pytestmark = pytest.mark.gpu

SHAPES = [
    (1, 3, 33),          # F N below one workgroup
    (1, 1001, 201),      # 64 L1 workgroups with several trips each; 25 SISDR chunks
    (3, 50, 201),        # 40 L1 workgroups (by size), 2 SISDR chunks
    (5, 41, 257),        # 257 bins
    (70, 17, 201),       # 512 / B = 7 L1 workgroups per utterance
    (600, 2, 33),        # one L1 workgroup per utterance; 2048 / B = 3
]
EPS = 1e-10
HOP = 160


def _frame_sets(B, F):
    """frame-count vectors that together hold F, 1, 0 and interior values"""
    pool = [F, 1, 0] + sorted({F // 2, F - 1, 2} - {F, 1, 0, -1})
    pool = [v for i, v in enumerate(pool) if v not in pool[:i] and 0 <= v <= F]
    if B >= len(pool):
        return [torch.tensor([pool[i % len(pool)] for i in range(B)])]
    sets = []
    for s in range(0, len(pool), B):
        sets.append(torch.tensor([pool[(s + i) % len(pool)] for i in range(B)]))
    return sets


def _wav_lengths(frames, F):
    """waveform lengths whose frame counts (w // 160 + 1, capped at F) the reference mask is built from: remainders 0, 159 and 77, and lengths
    past the last frame where the count is F"""
    w = []
    for i, fr in enumerate(frames.tolist()):
        if fr >= F and i % 2 == 0:
            w.append(F * HOP + 5)
        else:
            w.append(max(fr - 1, 0) * HOP + (0, 159, 77)[i % 3])
    w = torch.tensor(w)
    return w, torch.clamp(w // HOP + 1, max=F)


def _masks(frames, F):
    return (torch.arange(F)[None] < frames[:, None]).long()


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def _rows_err(got, want):
    """max over utterances of max|a - b| / max|b|; an utterance whose reference is all zero must be exactly zero"""
    got, want = got.double().cpu().flatten(1), want.double().cpu().flatten(1)
    scale = want.abs().max(dim=1).values
    zero = scale == 0
    assert (got[zero] == 0).all()
    if zero.all():
        return 0.0
    return ((got - want).abs().max(dim=1).values[~zero] / scale[~zero]).max().item()


def _id(shape):
    return 'x'.join(str(v) for v in shape)


# ---------------------------------------------------------------------------------------------------------------------------- L1

@functools.lru_cache(maxsize=None)
def _l1_data(shape):
    """(log_pred, linear_tar, float64 difference): log_pred = log(tar + eps) +- (0.01 + U), so no element lies within 0.01 of the sign flip"""
    B, F, K = shape
    gen = torch.Generator().manual_seed(B * 1000003 + F * 1009 + K)
    tar = (torch.randn(shape, generator=gen, dtype=torch.float64) * 2.0).exp()
    tar[torch.rand(shape, generator=gen) < 0.02] = 0.0
    tar = tar.float()
    sign = torch.where(torch.rand(shape, generator=gen) < 0.5, -1.0, 1.0).double()
    lp = ((tar.double() + EPS).log() + sign * (0.01 + torch.rand(shape, generator=gen, dtype=torch.float64))).float()
    d = lp.double() - (tar.double() + EPS).log()
    assert d.abs().min().item() > 0.01 - 1e-5          # 1e-5: the rounding of log_pred to float32 (|log_pred| < 32: half an ulp is 1e-6)
    return lp, tar, d


def _l1_reference(shape, frames):
    lp, tar, d = _l1_data(shape)
    m = _masks(frames, shape[1])
    rsum, rcnt = oobj.l1_sums(lp.double(), tar.double(), m, EPS)
    rloss = oobj.l1(lp.double(), tar.double(), m, EPS) if rcnt.item() > 0 else torch.tensor(float('nan'))
    return rsum.item(), rcnt.item(), rloss.item(), (torch.sign(d) * m.unsqueeze(-1)).float()


def _l1_check(name, got_sum, got_cnt, got_loss, grad, ref):
    rsum, rcnt, rloss, rsign = ref
    assert got_cnt == rcnt, (name, got_cnt, rcnt)
    assert torch.equal(grad.cpu(), rsign), name            # the reference's sign on valid elements, exactly 0 elsewhere
    if rcnt == 0:
        assert got_sum == 0 and math.isnan(got_loss) and math.isnan(rloss), name        # an empty mask: 0 / 0 on both sides
        return
    bounded(f'{name} sum rel', _rel(got_sum, rsum), 1e-4)
    bounded(f'{name} loss rel', _rel(got_loss, rloss), 1e-4)


def _l1_two_step(gpu, shape, lens):
    from speech_enhancement_by_s3prl_amd import _lib
    lib = _lib.load()
    B, F, K = shape
    lp, tar, _ = _l1_data(shape)
    lp, tar = lp.to(gpu), tar.to(gpu)
    lens = lens.to(device=gpu, dtype=torch.int64)
    sums = torch.full((2,), float('nan'), device=gpu, dtype=torch.float64)
    grad = torch.full(shape, float('nan'), device=gpu)
    _lib.check(lib.se_l1_masked_f32(_lib.ptr(lp), _lib.ptr(tar), _lib.ptr(lens), B, F, K, EPS, _lib.ptr(sums), _lib.ptr(grad), _lib.stream()), 'se_l1_masked_f32')
    s = sums.cpu()
    return s[0].item(), s[1].item(), (s[0] / s[1]).item(), grad


def _l1_one_launch(gpu, shape, lens, len_div, scratch):
    from speech_enhancement_by_s3prl_amd import _lib
    lib = _lib.load()
    B, F, K = shape
    lp, tar, _ = _l1_data(shape)
    lp, tar = lp.to(gpu), tar.to(gpu)
    lens = lens.to(device=gpu, dtype=torch.int64)
    sums = torch.full((2,), float('nan'), device=gpu, dtype=torch.float64)
    loss = torch.full((), float('nan'), device=gpu)
    grad = torch.full(shape, float('nan'), device=gpu)
    _lib.check(lib.se_l1_masked_loss_f32(_lib.ptr(lp), _lib.ptr(tar), _lib.ptr(lens), int(len_div), B, F, K, EPS, _lib.ptr(scratch), _lib.ptr(sums),
                                         _lib.ptr(loss), _lib.ptr(grad), _lib.stream()), 'se_l1_masked_loss_f32')
    s = sums.cpu()
    assert scratch[:1].view(torch.int64).item() == 0          # the arrival ticket is back at zero
    return s[0].item(), s[1].item(), loss.item(), grad


def _l1_scratch(gpu, B):
    from speech_enhancement_by_s3prl_amd import _lib
    return torch.zeros(int(_lib.load().se_l1_scratch_doubles(B)), device=gpu, dtype=torch.float64)


@pytest.mark.parametrize('shape', SHAPES, ids=_id)
def test_l1_vs_float64(gpu, shape):
    """se_l1_masked_f32, and se_l1_masked_loss_f32 with frame counts (len_div = 0) and waveform lengths (len_div = 160); the one-launch form
    runs twice on the same scratch, so a ticket that did not return to zero leaves the second call's outputs unwritten (NaN)"""
    B, F, K = shape
    scratch = _l1_scratch(gpu, B)
    for si, frames in enumerate(_frame_sets(B, F)):
        name = f'l1 {_id(shape)} set{si}'
        ref = _l1_reference(shape, frames)
        _l1_check(name + ' two-step', *_l1_two_step(gpu, shape, frames), ref)
        for rep in range(2):
            _l1_check(f'{name} one-launch#{rep}', *_l1_one_launch(gpu, shape, frames, 0, scratch), ref)
        wl, wframes = _wav_lengths(frames, F)
        assert wframes.max().item() <= F and wframes.min().item() >= 1
        wref = _l1_reference(shape, wframes)
        for rep in range(2):
            _l1_check(f'{name} one-launch len_div=160#{rep}', *_l1_one_launch(gpu, shape, wl, HOP, scratch), wref)


def test_l1_negative_length_counts_as_zero(gpu):
    """a negative length is an empty utterance, as in the SISDR kernels (objectives.hip: frames_of): no valid frame with frame counts, the
    one frame of an empty waveform (0 // 160 + 1) with waveform lengths -- never a negative element count"""
    shape = (5, 41, 257)
    B, F, K = shape
    frames = torch.tensor([F, -1, -7, 3, -2 ** 40])
    ref = _l1_reference(shape, torch.clamp(frames, min=0))
    assert ref[1] == (F + 3) * K
    scratch = _l1_scratch(gpu, B)
    _l1_check('l1 negative two-step', *_l1_two_step(gpu, shape, frames), ref)
    _l1_check('l1 negative one-launch', *_l1_one_launch(gpu, shape, frames, 0, scratch), ref)
    wl = torch.tensor([F * HOP, -1, -161, 2 * HOP + 5, -2 ** 40])
    wref = _l1_reference(shape, torch.tensor([F, 1, 1, 3, 1]))
    _l1_check('l1 negative one-launch len_div=160', *_l1_one_launch(gpu, shape, wl, HOP, scratch), wref)


# ------------------------------------------------------------------------------------------------------------------------- SISDR

@functools.lru_cache(maxsize=None)
def _sisdr_data(shape):
    """predicted = target x U(0.5, 1.5) with 5 % negative values and 5 % exact zeros; the target has exact zeros too"""
    gen = torch.Generator().manual_seed(shape[0] * 7919 + shape[1] * 31 + shape[2] + 1)
    tar = torch.rand(shape, generator=gen).pow(2) * 4.0
    tar[torch.rand(shape, generator=gen) < 0.02] = 0.0
    pred = tar * (0.5 + torch.rand(shape, generator=gen))
    r = torch.rand(shape, generator=gen)
    pred = torch.where(r < 0.05, -torch.rand(shape, generator=gen), pred)
    pred = torch.where((r >= 0.05) & (r < 0.10), torch.zeros(()), pred)
    assert (pred < 0).any() and (pred == 0).any()
    return pred, tar


def _sisdr_reference(shape, frames):
    """(per-utterance losses, d loss_b / d predicted where float64 autograd is finite, its finite mask, the mask of elements that must be 0)"""
    pred, tar = _sisdr_data(shape)
    B, F, N = shape
    m = _masks(frames, F)
    p = pred.double().requires_grad_(True)
    loss_b = torch.stack([oobj.sisdr_objective(p[b:b + 1], tar[b:b + 1].double(), m[b:b + 1], EPS) for b in range(B)])
    assert abs(loss_b.mean().item() - oobj.sisdr_objective(p, tar.double(), m, EPS).item()) < 1e-9 * abs(loss_b.mean().item())
    loss_b.sum().backward()
    assert loss_b.detach().abs().min().item() >= 1.0          # every |loss_b| is at least 1 dB: the relative bound means something
    finite = torch.isfinite(p.grad)
    must_be_zero = (m.unsqueeze(-1) == 0) | (pred <= 0)
    assert (~finite <= (pred <= 0)).all()                      # autograd is non-finite only where sqrt(relu(.)) has no derivative
    return loss_b.detach(), torch.where(finite, p.grad, torch.zeros((), dtype=torch.float64)), finite, must_be_zero


def _sisdr_check_grad(name, grad, ref):
    _, rgrad, finite, must_be_zero = ref
    g = grad.cpu()
    assert torch.isfinite(g).all() and (g[must_be_zero] == 0).all(), name
    bounded(f'{name} grad relmax', _rows_err(torch.where(finite, g.double(), torch.zeros((), dtype=torch.float64)), rgrad), 1e-4)


@pytest.mark.parametrize('shape', SHAPES, ids=_id)
def test_sisdr_vs_float64(gpu, shape):
    """se_sisdr_spec_f32 (per-utterance losses, gradient) and se_sisdr_spec_loss_f32 (len_div = 0 and 160: losses, their mean, sums_out); a
    zero-length utterance gives the reference's -10 log10(eps) = 100 dB"""
    from speech_enhancement_by_s3prl_amd import _lib
    lib = _lib.load()
    B, F, N = shape
    pred, tar = _sisdr_data(shape)
    p, t = pred.to(gpu), tar.to(gpu)
    for si, frames in enumerate(_frame_sets(B, F)):
        name = f'sisdr {_id(shape)} set{si}'
        ref = _sisdr_reference(shape, frames)
        lens = frames.to(device=gpu, dtype=torch.int64)
        scratch = torch.full((5 * B,), float('nan'), device=gpu, dtype=torch.float64)
        loss_b = torch.full((B,), float('nan'), device=gpu)
        grad = torch.full(shape, float('nan'), device=gpu)
        _lib.check(lib.se_sisdr_spec_f32(_lib.ptr(p), _lib.ptr(t), _lib.ptr(lens), B, F, N, EPS, 1.0, _lib.ptr(scratch), _lib.ptr(loss_b), _lib.ptr(grad),
                                         _lib.stream()), 'se_sisdr_spec_f32')
        bounded(f'{name} loss_b rel', ((loss_b.cpu().double() - ref[0]).abs() / ref[0].abs()).max().item(), 1e-4)
        if (frames == 0).any():
            assert abs(ref[0][frames == 0] - 100.0).max().item() < 1e-6
        _sisdr_check_grad(name, grad, ref)
        wl, wframes = _wav_lengths(frames, F)
        for len_div, ll, r in ((0, frames, ref), (HOP, wl, _sisdr_reference(shape, wframes))):
            n = int(lib.se_sisdr_spec_loss_scratch_doubles(B, F, N))
            slab = torch.full((n,), float('nan'), device=gpu, dtype=torch.float64)
            loss_b = torch.full((B,), float('nan'), device=gpu)
            sums = torch.full((2,), float('nan'), device=gpu, dtype=torch.float64)
            loss = torch.full((), float('nan'), device=gpu)
            lens = ll.to(device=gpu, dtype=torch.int64)
            _lib.check(lib.se_sisdr_spec_loss_f32(_lib.ptr(p), _lib.ptr(t), _lib.ptr(lens), len_div, B, F, N, EPS, _lib.ptr(slab), _lib.ptr(loss_b),
                                                  _lib.ptr(sums), _lib.ptr(loss), _lib.stream()), 'se_sisdr_spec_loss_f32')
            bounded(f'{name} loss form len_div={len_div} loss_b rel', ((loss_b.cpu().double() - r[0]).abs() / r[0].abs()).max().item(), 1e-4)
            bounded(f'{name} loss form len_div={len_div} mean rel', _rel(loss.item(), r[0].mean().item()), 1e-4)
            s = sums.cpu()
            assert s[1].item() == B
            bounded(f'{name} loss form len_div={len_div} sums_out rel', _rel(s[0].item(), r[0].sum().item()), 1e-4)


def test_sisdr_negative_length_is_an_empty_utterance(gpu):
    """the behaviour the L1 kernel is aligned with: a negative frame count gives the zero-length loss and an all-zero gradient row"""
    from speech_enhancement_by_s3prl_amd import _lib
    lib = _lib.load()
    shape = (5, 41, 257)
    B, F, N = shape
    pred, tar = _sisdr_data(shape)
    frames = torch.tensor([F, -1, -7, 3, -2 ** 40])
    ref = _sisdr_reference(shape, torch.clamp(frames, min=0))
    p, t, lens = pred.to(gpu), tar.to(gpu), frames.to(device=gpu, dtype=torch.int64)
    scratch = torch.full((5 * B,), float('nan'), device=gpu, dtype=torch.float64)
    loss_b = torch.full((B,), float('nan'), device=gpu)
    grad = torch.full(shape, float('nan'), device=gpu)
    _lib.check(lib.se_sisdr_spec_f32(_lib.ptr(p), _lib.ptr(t), _lib.ptr(lens), B, F, N, EPS, 1.0, _lib.ptr(scratch), _lib.ptr(loss_b), _lib.ptr(grad),
                                     _lib.stream()), 'se_sisdr_spec_f32')
    bounded('sisdr negative loss_b rel', ((loss_b.cpu().double() - ref[0]).abs() / ref[0].abs()).max().item(), 1e-4)
    _sisdr_check_grad('sisdr negative', grad, ref)


# --------------------------------------------------------------------------------------------------------------------------- WSD

WSD_LADDER = [-6.0, -12.0, -20.0, -29.0, -31.0, -36.0, -45.0]      # frame energies in dB below the loudest frame; db_interval = 30: none within 0.5 dB of the threshold
DB_INTERVAL = 30.0


@functools.lru_cache(maxsize=None)
def _wsd_data(shape):
    """(linear_inp, offset, linear_tar): every frame's energy sits on WSD_LADDER below the batch's loudest frame (10.0), which is the LAST
    frame of utterance 0 -- a padded frame whenever that utterance is shorter than F; linear_inp is below linear_tar on about a third of the bins"""
    B, F, N = shape
    gen = torch.Generator().manual_seed(B * 104729 + F * 211 + N + 2)
    prof = torch.rand(shape, generator=gen, dtype=torch.float64) + 0.05
    prof = prof / prof.sum(dim=-1, keepdim=True)
    step = torch.randint(0, len(WSD_LADDER), (B, F), generator=gen)
    db = torch.tensor(WSD_LADDER, dtype=torch.float64)[step]
    db[0, F - 1] = 0.0
    tar = (prof * (10.0 * 10.0 ** (db / 10.0)).unsqueeze(-1)).float()
    inp = tar * (0.5 + 1.5 * torch.rand(shape, generator=gen))
    off = torch.rand(shape, generator=gen)
    assert (inp < tar).any() and (inp > tar).any()
    energy = tar.double().sum(dim=-1)
    thres = 10 * torch.log10(energy.max() + EPS) - DB_INTERVAL
    assert ((10 * torch.log10(energy + EPS) - thres).abs() > 0.5).all()          # the voice mask is the same in float32 and float64
    return inp, off, tar


def _wsd_frame_sets(B, F):
    """as _frame_sets, with utterance 0 -- whose last frame is the loudest of the batch -- shorter than F in at least one set"""
    sets = _frame_sets(B, F)
    if F > 1:
        short = sets[-1].clone()
        short[0] = F - 1
        sets.append(short)
    return sets


@pytest.mark.parametrize('shape', SHAPES, ids=_id)
def test_wsd_vs_float64(gpu, shape):
    """se_wsd_energy_f32 + se_wsd_f32 through objective.WSD (loss, gradient of the mask) and directly (both sums); the loudest frame of the
    batch is a padded one in the last length set: the threshold follows it, as the reference's maximum over ALL frames does"""
    from speech_enhancement_by_s3prl_amd import _lib
    from speech_enhancement_by_s3prl_amd.objective import WSD
    lib = _lib.load()
    B, F, N = shape
    inp, off, tar = _wsd_data(shape)
    ginp, gtar = inp.to(gpu), tar.to(gpu)
    sets = _wsd_frame_sets(B, F)
    assert F == 1 or sets[-1][0].item() == F - 1
    for si, frames in enumerate(sets):
        name = f'wsd {_id(shape)} set{si}'
        m = _masks(frames, F)
        roff = off.double().requires_grad_(True)
        rloss = oobj.wsd_objective(inp.double(), roff, tar.double(), m, 0.5, DB_INTERVAL, EPS)
        rloss.backward()
        rspeech = oobj.wsd_objective(inp.double(), off.double(), tar.double(), m, 1.0, DB_INTERVAL, EPS).item() * B
        rnoise = oobj.wsd_objective(inp.double(), off.double(), tar.double(), m, 0.0, DB_INTERVAL, EPS).item() * B
        lens = frames.to(device=gpu, dtype=torch.int64)
        goff = off.to(gpu).requires_grad_(True)
        loss, _ = WSD(alpha=0.5, db_interval=DB_INTERVAL, eps=EPS)(linear_inp=ginp, offset=goff, linear_tar=gtar, stft_lengths=lens)
        loss.backward()
        energy = torch.full((B * F,), float('nan'), device=gpu)
        emax = torch.full((1,), float('nan'), device=gpu)
        _lib.check(lib.se_wsd_energy_f32(_lib.ptr(gtar), B, F, N, _lib.ptr(energy), _lib.ptr(emax), _lib.stream()), 'se_wsd_energy_f32')
        sums = torch.full((3,), float('nan'), device=gpu, dtype=torch.float64)
        _lib.check(lib.se_wsd_f32(_lib.ptr(ginp), _lib.ptr(goff.detach()), _lib.ptr(gtar), _lib.ptr(lens), _lib.ptr(energy), _lib.ptr(emax), B, F, N, 0.5,
                                  DB_INTERVAL, EPS, 1.0, _lib.ptr(sums), None, _lib.stream()), 'se_wsd_f32')
        bounded(f'{name} energy relmax', _rows_err(energy.view(B, F), tar.double().sum(dim=-1)), 1e-4)
        bounded(f'{name} energy max rel', _rel(emax.item(), tar.double().sum(dim=-1).max().item()), 1e-4)
        s = sums.cpu()
        if frames.sum().item() == 0:
            assert s[0].item() == 0 and s[1].item() == 0 and loss.item() == 0 and rloss.item() == 0 and (goff.grad == 0).all()
            continue
        assert rnoise > 0
        if rspeech == 0:          # no valid frame above the threshold: the voice mask removes every term
            assert s[0].item() == 0
        else:
            bounded(f'{name} speech sum rel', _rel(s[0].item(), rspeech), 1e-4)
        bounded(f'{name} noise sum rel', _rel(s[1].item(), rnoise), 1e-4)
        bounded(f'{name} loss rel', _rel(loss.item(), rloss.item()), 1e-4)
        g = goff.grad.cpu()
        assert (g[m == 0] == 0).all()
        bounded(f'{name} grad relmax', _rows_err(g, roff.grad), 1e-4)


# ------------------------------------------------------------------------------------------------------------- decode reductions

def _sumsq_lengths(T):
    """0, 1, T, above T, a negative one, and interior lengths with len % 4 = 0 .. 3"""
    base = (T // 2) // 4 * 4
    inner = [min(base + r, T) for r in range(4)]
    return torch.tensor([T, 0, 1, T + 3, -3] + inner + [T - 1])


@pytest.mark.parametrize('T', [5, 2049, 70000])
@pytest.mark.parametrize('aligned', [True, False], ids=['aligned', 'unaligned'])
def test_masked_sumsq_vs_float64(gpu, T, aligned):
    """se_masked_sumsq_f32 on both paths: row stride a multiple of 4 floats (every row 16-byte aligned: float4 loads + the len & 3 tail on
    workgroup 0) and an odd row stride (rows 1, 2, 3 of every four take the scalar path); 1, 2 and 32 workgroups per row"""
    from speech_enhancement_by_s3prl_amd import _lib
    lib = _lib.load()
    lengths = _sumsq_lengths(T)
    if T >= 8:
        assert {int(v) % 4 for v in lengths[5:9]} == {0, 1, 2, 3}
    B = lengths.numel()
    stride = (T + 3) // 4 * 4 + (0 if aligned else 1)
    x = torch.randn(B, stride, generator=torch.Generator().manual_seed(T + stride)) * 0.1
    gx = x.to(gpu)
    assert gx.data_ptr() % 16 == 0
    sums = torch.full((B,), float('nan'), device=gpu)
    lens = lengths.to(device=gpu, dtype=torch.int64)
    _lib.check(lib.se_masked_sumsq_f32(_lib.ptr(gx), B, T, stride, _lib.ptr(lens), _lib.ptr(sums), _lib.stream()), 'se_masked_sumsq_f32')
    want = (x[:, :T].double().pow(2) * (torch.arange(T)[None] < lengths[:, None])).sum(dim=1)
    got, zero = sums.cpu().double(), want == 0
    assert zero.sum().item() >= 2 and (got[zero] == 0).all()          # lengths 0 and -3 (and the interior 0 at T = 5)
    bounded(f'masked_sumsq T={T} stride={stride} rel', ((got[~zero] - want[~zero]).abs() / want[~zero]).max().item(), 1e-4)
    if not aligned and T % 2 == 1:          # the Python entry on a contiguous (B, T) with odd T: the same unaligned rows
        from speech_enhancement_by_s3prl_amd.decode import masked_sumsq
        got = masked_sumsq(gx[:, :T], lens).cpu().double()
        assert (got[zero] == 0).all()
        bounded(f'masked_sumsq T={T} contiguous rel', ((got[~zero] - want[~zero]).abs() / want[~zero]).max().item(), 1e-4)


@pytest.mark.parametrize('T', [5, 2049, 70000])
def test_masked_normalize_decibel_vs_oracle(gpu, T):
    """masked_normalize_decibel in the fixed -25 dB form and in the reference-audio form (dbnorm_kernel with ref_sumsq: the target level is the
    masked power of channel 1 of a (B, 2, T) batch, read in place) against oracle/decode.py in float64; lengths 0, 1, T, above T, interior"""
    from speech_enhancement_by_s3prl_amd.decode import masked_normalize_decibel
    lengths = torch.tensor([T, 0, 1, T + 3, T // 2 + 1, T - 1])
    B = lengths.numel()
    gen = torch.Generator().manual_seed(T)
    audio = torch.randn(B, T, generator=gen) * 0.1
    wavs = torch.randn(B, 2, T, generator=gen) * 0.3
    m = (torch.arange(T)[None] < lengths[:, None]).long()
    for name, target, rtarget in (('fixed -25 dB', -25, -25), ('reference audio', wavs.to(gpu)[:, 1], wavs[:, 1].double())):
        want = odec.masked_normalize_decibel(audio.double(), rtarget, m)
        got = masked_normalize_decibel(audio.to(gpu), target, lengths.to(gpu))
        assert got.shape == (B, T) and torch.isfinite(got).all()
        bounded(f'dbnorm T={T} {name} relmax', _rows_err(got, want), 1e-4)
    assert (want[1] == 0).all() and want[0].abs().max() > 0          # reference-audio form: an empty mask has no level, the row goes to zero


@pytest.mark.parametrize('max_len', [1, 1000, 70000])
def test_length_masks_bit_exact(gpu, max_len):
    """get_length_masks against the reference's arange < lengths: 0, 1, max_len, above max_len, negative, interior; one and 256 workgroups"""
    from speech_enhancement_by_s3prl_amd.decode import get_length_masks
    lengths = torch.tensor([max_len, 0, 1, max_len + 5, -2, max_len // 2, max_len - 1])
    got = get_length_masks(lengths.to(gpu), max_len)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), odec.get_length_masks(lengths, max_len))
