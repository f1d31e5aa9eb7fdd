"""GPU parity of the log-input iSTFT: se_istft_tphase_f32(..., log_input = 1) on a plan of se_plan_create, the only way into
csrc/istft2.hip (istftp_kernel<1>: a persistent kernel that prefetches the next chunk's spectra while the current one is transformed).

Reference: oracle.preprocessor.istft (torch.istft) in float64 on pred = noisy power x U(0.25, 1.25); the kernel gets log(pred + 1e-20) and the
encoded phase words of P(wavs).  Bounds: the project's fp32 bar per utterance, max|a - b| <= 1e-4 max|b|, and 1e-4 relative
on the square sums against float64 sums of the oracle waveform.

The kernel's hop-blocks per chunk HB (20..27) follow pick_hop_blocks(F - 1, B, slots); `slots` is 3 x CUs unless SE_AMD_STFT_SLOTS is set,
which the library reads on every call: a small slot count makes one workgroup walk many chunks at tiny shapes.  The rule is restated here
ONLY to choose shapes, and the tests assert the HB they expect, so a change of the rule reports lost coverage instead of passing."""
import functools
import math

import pytest
import torch

from conftest import bounded
from oracle import preprocessor as opre

pytestmark = pytest.mark.gpu

GEOM = opre.Geometry()
HOP = 160
ENV = 'SE_AMD_STFT_SLOTS'


def _pick_hop_blocks(n_blocks, B, slots):
    """csrc/istft2.hip: pick_hop_blocks, restated to choose shapes"""
    best, best_cost = 27, 1e30
    for hb in range(27, 19, -1):
        chunks = B * ((n_blocks + hb - 1) // hb)
        rounds = (chunks + slots - 1) // slots
        cost = float(rounds * (hb + 3 + 4))
        if cost < best_cost - 1e-9:
            best_cost, best = cost, hb
    return best


def _geometry(F, B, slots):
    """(HB, chunks per utterance, workgroups launched)"""
    if slots is None:
        slots = 3 * torch.cuda.get_device_properties(0).multi_processor_count
    hb = _pick_hop_blocks(F - 1, B, slots)
    cpu = (F - 1 + hb - 1) // hb
    return hb, cpu, min(B * cpu, slots)


def _relmax(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().flatten(1).max(dim=1).values / b.abs().flatten(1).max(dim=1).values).max().item()


def _sum_err(got, want):
    """largest relative error of the rows whose float64 sum is not zero; a row whose sum is zero (length 0) must be exactly zero"""
    got, want = got.double().cpu(), want.double().cpu()
    zero = want == 0
    assert (got[zero] == 0).all(), (got, want)
    if zero.all():
        return 0.0
    return ((got[~zero] - want[~zero]).abs() / want[~zero]).max().item()


@pytest.fixture(scope='module')
def P(gpu):
    from speech_enhancement_by_s3prl_amd.preprocessor import OnlinePreprocessor
    p = OnlinePreprocessor().to(gpu)
    p.channel_inp = 0
    return p


@functools.lru_cache(maxsize=None)
def _case(B, T, whole_range=False):
    """one batch per shape, shared and left unchanged: (wavs, oracle phase, pred, the log plane the kernel gets, float64 oracle waveform)"""
    gen = torch.Generator().manual_seed(31 * T + B + (7 if whole_range else 0))
    wavs = torch.randn(B, 2, T, generator=gen) * 0.1
    lin, ph = opre.forward(wavs, [opre.get_feat_config('linear', 0), opre.get_feat_config('phase', 0)], GEOM)
    if whole_range:
        # log values over the whole range the plane can hold, log(1e-20) .. log(4): the fast exponential where its argument is large
        lo, hi = math.log(1e-20), math.log(4.0)
        logp = (lo + (hi - lo) * torch.rand(lin.shape, generator=gen, dtype=torch.float64)).float()
        pred = logp.double().exp()
    else:
        pred = (lin * (0.25 + torch.rand(lin.shape, generator=gen))).double()
        logp = (pred + 1e-20).log().float()
    rwav = opre.istft(pred, ph.double(), GEOM)
    assert rwav.dtype == torch.float64 and rwav.shape == (B, HOP * (T // HOP))
    return wavs, ph, pred, logp, rwav


def _length_pool(T):
    """T, n_out - 1, an odd value that splits a four-sample quad, 0, and a value above T"""
    n_out = HOP * (T // HOP)
    odd = (n_out // 2) // 4 * 4 + 3
    assert odd % 4 == 3 and 0 < odd < n_out
    return [T, n_out - 1, odd, 0, T + 9]


def _lengths(T, B, first):
    pool = _length_pool(T)
    return torch.tensor([pool[(first + i) % len(pool)] for i in range(B)])


def _tphase(P, gpu, wavs):
    from speech_enhancement_by_s3prl_amd.preprocessor import LazyPhase
    f = P(wavs.to(gpu), [P.get_feat_config('linear', 0), P.get_feat_config('phase', 0)])
    assert type(f[1]) is LazyPhase and f[1]._tphase is not None
    return f[1]._tphase.reshape(-1, f[1].shape[-2], f[1].shape[-1])


def _istft(P, gpu, plane, tph, lengths, out_len, log_input, ref=None):
    """se_istft_tphase_f32 through the C ABI into buffers pre-filled with NaN: every sample of a row, the right pad included, has to be
    written by the kernel.  Returns (wav (B, out_len), sumsq (B), ref_sumsq (B) or None)."""
    from speech_enhancement_by_s3prl_amd import _lib
    lib = _lib.load()
    plane = plane.float().contiguous().to(gpu)
    B, F, K = plane.shape
    assert tph.shape == (B, F, K) and tph.is_contiguous() and out_len >= HOP * (F - 1)
    wav = torch.full((B, out_len), float('nan'), device=gpu)
    ss = torch.full((B,), float('nan'), device=gpu)
    rss = torch.full((B,), float('nan'), device=gpu) if ref is not None else None
    lens = lengths.to(device=gpu, dtype=torch.int64).contiguous()
    if ref is not None:
        assert ref.is_cuda and ref.dtype == torch.float32 and ref.stride(1) == 1 and ref.shape == (B, out_len)
    _lib.check(lib.se_istft_tphase_f32(P._plan(gpu), _lib.ptr(plane), _lib.ptr(tph), B, F, int(log_input), _lib.ptr(wav), out_len, _lib.ptr(lens),
                                       _lib.ptr(ss), ref.data_ptr() if ref is not None else None, int(ref.stride(0)) if ref is not None else 0,
                                       _lib.ptr(rss), _lib.stream()), 'se_istft_tphase_f32')
    torch.cuda.synchronize()
    return wav, ss, rss


def _slots(monkeypatch, slots):
    if slots is None:
        monkeypatch.delenv(ENV, raising=False)
    else:
        monkeypatch.setenv(ENV, str(slots))


def _run_and_check(P, gpu, monkeypatch, name, B, T, slots, first_length, whole_range=False):
    """the log_input = 1 kernel on the shape's batch against the float64 oracle: waveform, right pad, masked square sums"""
    wavs, _, _, logp, rwav = _case(B, T, whole_range)
    n_out = HOP * (T // HOP)
    lengths = _lengths(T, B, first_length)
    tph = _tphase(P, gpu, wavs)             # the forward transform runs before the slot count is changed: only the inverse is under test
    _slots(monkeypatch, slots)
    wav, ss, _ = _istft(P, gpu, logp, tph, lengths, T, log_input=True)
    assert wav.shape == (B, T) and torch.isfinite(wav).all()
    bounded(f'istft_log {name} wav relmax', _relmax(wav[:, :n_out], rwav), 1e-4)
    assert (wav[:, n_out:] == 0).all()
    mask = (torch.arange(n_out)[None] < lengths[:, None]).double()
    bounded(f'istft_log {name} sumsq rel', _sum_err(ss, (rwav.pow(2) * mask).sum(dim=1)), 1e-4)
    return wav, ss


# slots = 1 and B = 1: the rule selects HB = 20 .. 27 at these frame counts, and one workgroup walks every chunk (the prefetch loop runs)
EVERY_HB = [(29, 20), (42, 21), (44, 22), (46, 23), (48, 24), (50, 25), (52, 26), (54, 27)]


def test_shapes_cover_every_hop_block_count():
    """the cases below are chosen with the restated rule: together they must reach every HB the kernel can be launched with"""
    got = {_pick_hop_blocks(F - 1, 1, 1) for F, _ in EVERY_HB}
    assert got == set(range(20, 28)), got
    for F, hb in EVERY_HB:
        assert _pick_hop_blocks(F - 1, 1, 1) == hb and (F - 1 + hb - 1) // hb >= 2, (F, hb)


@pytest.mark.parametrize('i', range(len(EVERY_HB)))
def test_every_hop_block_count_one_workgroup(P, gpu, monkeypatch, i):
    """HB = 20 + i with one resident workgroup: two chunks walked by the same workgroup, the second loaded while the first is transformed and
    shorter than the first; T = 160 (F - 1) + 77 (a right pad to fill) for even i, 160 (F - 1) for odd i; one of the five ragged lengths each"""
    F, hb = EVERY_HB[i]
    assert _geometry(F, 1, 1) == (hb, 2, 1)
    T = HOP * (F - 1) + (77 if i % 2 == 0 else 0)
    _run_and_check(P, gpu, monkeypatch, f'HB={hb} F={F} T={T} slots=1', 1, T, 1, i)


@pytest.mark.parametrize('slots,geom', [(2, (27, 2, 2)), (5, (20, 3, 5))])
def test_chunks_alternate_between_utterances(P, gpu, monkeypatch, slots, geom):
    """B = 3, F = 54 with 2 and with 5 resident workgroups: a workgroup's consecutive chunks belong to different utterances (its square sums
    must land in the right rows), and rows 1, 2 of the (3, T) output are not 16-byte aligned (T % 4 = 1): the scalar store path"""
    F = 54
    T = HOP * (F - 1) + 77
    assert T % 4 != 0 and _geometry(F, 3, slots) == geom
    _run_and_check(P, gpu, monkeypatch, f'B=3 F={F} T={T} slots={slots}', 3, T, slots, slots)


@pytest.mark.parametrize('B,T', [(3, 8123), (1, 201), (1, 321), (1, 160 * 20 + 1)])
def test_default_slots(P, gpu, monkeypatch, B, T):
    """the launch as the product makes it (no slot override, one chunk per workgroup): F = 51 at B = 3 (unaligned rows), the smallest
    transforms F = 2 and F = 3, and F - 1 = 20 hop-blocks = exactly one full chunk"""
    F = T // HOP + 1
    hb, cpu, _ = _geometry(F, B, None)
    assert hb == 20 and cpu == (3 if T == 8123 else 1)
    _run_and_check(P, gpu, monkeypatch, f'B={B} T={T} default slots', B, T, None, T % 5)


@pytest.mark.parametrize('F', [61, 62])
def test_chunk_tails(P, gpu, monkeypatch, F):
    """HB = 20 with two resident workgroups: F - 1 = 60 = 3 full chunks, and F - 1 = 61 whose fourth chunk holds ONE hop-block (three frames),
    reached by workgroup 1 inside its persistent loop"""
    hb, cpu, wgs = _geometry(F, 1, 2)
    assert (hb, wgs) == (20, 2) and cpu == (F - 1 + 19) // 20 and (F - 1) % 20 == F - 61
    _run_and_check(P, gpu, monkeypatch, f'tail F={F} slots=2', 1, HOP * (F - 1) + 77, 2, F)


def test_unaligned_rows_and_last_chunk_zero_fill(P, gpu, monkeypatch):
    """B = 2, out_len = T = 160 x 28 + 77 (T % 4 = 1) with one resident workgroup: row 1 starts 4 bytes past a 16-byte boundary, so its quads
    go out as scalar stores, and the 77 pad samples of each row are zero-filled by that row's LAST chunk only (the output starts as NaN)"""
    F, T = 29, HOP * 28 + 77
    assert T % 4 == 1 and _geometry(F, 2, 1) == (20, 2, 1)
    wav, _ = _run_and_check(P, gpu, monkeypatch, f'unaligned B=2 T={T} slots=1', 2, T, 1, 1)
    assert wav.data_ptr() % 16 == 0 and (wav.data_ptr() + 4 * T) % 16 != 0
    assert (wav[:, HOP * 28:] == 0).all() and wav[:, HOP * 28:].shape[1] == 77


def test_reference_sums_run_to_the_length(P, gpu, monkeypatch):
    """ref= with T % 160 != 0 and lengths in (n_out, T]: the reference waveform's square sum runs over n < min(length, T) -- past the
    n_out = 160 (F - 1) samples the transform returns -- as the default kernel's does (include/se_amd.h).  The reference rows are channel 1 of
    the (B, 2, T) batch read in place: row stride 2 T, odd T, so rows are unaligned for se_masked_sumsq_f32 as well."""
    B, T = 3, 8123
    wavs, _, pred, logp, _ = _case(B, T)
    n_out = HOP * (T // HOP)
    lengths = torch.tensor([T, n_out + 51, n_out - 40])
    assert T % HOP != 0 and n_out < lengths[1] < T
    tph = _tphase(P, gpu, wavs)
    ref = wavs.to(gpu)[:, 1]
    assert ref.stride(0) == 2 * T
    _slots(monkeypatch, None)
    want = (wavs[:, 1].double().pow(2) * (torch.arange(T)[None] < lengths[:, None])).sum(dim=1)
    wav1, ss1, rss1 = _istft(P, gpu, logp, tph, lengths, T, log_input=True, ref=ref)
    wav0, ss0, rss0 = _istft(P, gpu, pred, tph, lengths, T, log_input=False, ref=ref)
    bounded('istft_log ref_sumsq rel vs float64', _sum_err(rss1, want), 1e-4)
    bounded('istft default ref_sumsq rel vs float64', _sum_err(rss0, want), 1e-4)
    bounded('istft_log ref_sumsq rel vs the default kernel', _sum_err(rss1, rss0), 1e-4)
    # a sum over n < min(length, n_out) would miss this much of rows 0 and 1: the bound above can tell the two readings apart
    short = (wavs[:, 1, :n_out].double().pow(2) * (torch.arange(n_out)[None] < lengths[:, None])).sum(dim=1)
    assert ((want - short) / want)[:2].min().item() > 1e-3
    bounded('istft_log sumsq rel vs the default kernel', _sum_err(ss1, ss0), 1e-4)
    # the wrapper's own path (sums side by side, one clearing launch) gives the same three results
    wavw, ssw, rssw = P._istft_tphase(logp.to(gpu), tph, lengths.to(gpu), T, log_input=True, ref=ref)
    assert torch.equal(wavw, wav1) and rssw is not None
    bounded('istft_log wrapper ref_sumsq rel', _sum_err(rssw, want), 1e-4)
    bounded('istft_log wrapper sumsq rel', _sum_err(ssw, ss1), 1e-4)


def test_two_400_point_kernels_agree(P, gpu, monkeypatch):
    """log_input = 1 (exp(x / 2), persistent kernel) and log_input = 0 (sqrt, the default kernel) on the same pred: the same transform in the
    same order, so they agree far inside the oracle bound"""
    B, T = 3, 8123
    wavs, _, pred, logp, _ = _case(B, T)
    lengths = _lengths(T, B, 0)
    tph = _tphase(P, gpu, wavs)
    for slots in (None, 1):
        _slots(monkeypatch, slots)
        wav1, _, _ = _istft(P, gpu, logp, tph, lengths, T, log_input=True)
        _slots(monkeypatch, None)
        wav0, _, _ = _istft(P, gpu, pred, tph, lengths, T, log_input=False)
        bounded(f'istft_log vs default kernel relmax slots={slots}', _relmax(wav1, wav0), 1e-5)


def test_log_values_over_the_whole_range(P, gpu, monkeypatch):
    """log values drawn from log(1e-20) .. log(4), B = 2, F = 30 (HB = 20, two chunks per row in one workgroup); the oracle gets exp of the
    very float32 values the kernel reads"""
    F = 30
    assert _geometry(F, 2, 1) == (20, 2, 1)
    _run_and_check(P, gpu, monkeypatch, 'whole log range B=2 F=30 slots=1', 2, HOP * (F - 1) + 77, 1, 0, whole_range=True)
