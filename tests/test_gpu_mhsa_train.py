"""GPU parity of the training attention through the C ABI, row by row: se_mhsa_fwd_lse_bf16 followed by se_mhsa_bwd_bf16 (mhsa_bwd_dq_kernel: dQ and
D; mhsa_bwd_dkv_kernel: dK and dV) against the closed-form fp64 reference of tests/mhsa_grad_ref.py on the same bf16-valued operands.  Every
quantity is judged per (utterance, head, row) with row_err, so a failure names the row; every output is pre-filled with NaN and lives between
guard rows that must come back untouched.  Read from the shapes (grid = ceil(T / 128) workgroups x heads x B, pairs = heads B):
  (a) (1, 64, 1)    pairs 1: plain mapping, one workgroup, one key tile
  (b) (1, 65, 1)    pairs 1: plain mapping, one workgroup (the second tile holds one key, padded, and one query)
  (c) (2, 129, 1)   pairs 2: plain mapping, 2 workgroups per pair, the second one row deep; utterance 1 (length 65): dkv workgroup 1 exits early
  (d) (8, 130, 1)   pairs 8: XCD mapping, 2 workgroups per pair; lengths 1 .. 128: dkv workgroup 1 exits early (all its keys padded)
  (e) (2, 257, 4)   pairs 8: XCD mapping, 3 workgroups per pair; utterance 1 (length 120): dkv workgroups 1 and 2 exit early
  (f) (3, 200, 3)   pairs 9: plain mapping, 2 workgroups per pair; utterances 1 and 2 (lengths 77, 1): dkv workgroup 1 exits early
PARITY UNPINNED vs the original S3PRL (restatement-defined oracle, see oracle/__init__.py)."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import bounded  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mhsa_grad_ref as R      # noqa: E402

SEED, SITE = 0x1234567890abcdef % (1 << 63), 7
GUARD_ROWS, GUARD_FLOATS, SENTINEL = 8, 64, -12345.0


def _L():
    from speech_enhancement_by_s3prl_amd import _lib
    return _lib


class _Guarded:
    """an output of `rows` x `cols` pre-filled with NaN inside an allocation that carries `guard` rows of a sentinel on either side"""

    def __init__(self, gpu, rows, cols, guard, dtype):
        self.buf = torch.full((rows + 2 * guard, cols), SENTINEL, device=gpu, dtype=dtype)
        self.out = self.buf[guard:guard + rows]
        self.out.fill_(float('nan'))
        self.guard = guard
        assert self.out.is_contiguous() and self.out.data_ptr() % 16 == 0

    def untouched(self):
        g = self.guard
        return bool((self.buf[:g] == SENTINEL).all() and (self.buf[-g:] == SENTINEL).all())


class _Guarded1:
    """a float vector of n elements, NaN inside, GUARD_FLOATS sentinel floats on either side"""

    def __init__(self, gpu, n):
        self.buf = torch.full((n + 2 * GUARD_FLOATS,), SENTINEL, device=gpu, dtype=torch.float32)
        self.out = self.buf[GUARD_FLOATS:GUARD_FLOATS + n]
        self.out.fill_(float('nan'))

    def untouched(self):
        return bool((self.buf[:GUARD_FLOATS] == SENTINEL).all() and (self.buf[-GUARD_FLOATS:] == SENTINEL).all())


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _forward(gpu, qkv_g, len_g, B, T, heads, drop, site):
    L = _L()
    H = heads * 64
    ctx = _Guarded(gpu, B * T, H, GUARD_ROWS, torch.bfloat16)
    lse = _Guarded1(gpu, B * heads * T)
    L.check(L.load().se_mhsa_fwd_lse_bf16(L.ptr(qkv_g), L.ptr(len_g), B, T, heads, L.ptr(ctx.out), L.ptr(lse.out), drop, SEED, site, L.stream()), 'fwd')
    torch.cuda.synchronize()
    assert ctx.untouched() and lse.untouched(), 'forward wrote outside ctx / lse'
    return ctx, lse


def _backward(gpu, qkv_g, ctx, do_g, lse, len_g, B, T, heads, drop, site):
    L = _L()
    H = heads * 64
    dqkv = _Guarded(gpu, B * T, 3 * H, GUARD_ROWS, torch.bfloat16)
    dvec = _Guarded1(gpu, B * heads * T)
    L.check(L.load().se_mhsa_bwd_bf16(L.ptr(qkv_g), L.ptr(ctx.out), L.ptr(do_g), L.ptr(lse.out), L.ptr(len_g), B, T, heads, L.ptr(dqkv.out), L.ptr(dvec.out),
                                      drop, SEED, site, L.stream()), 'bwd')
    torch.cuda.synchronize()
    assert dqkv.untouched() and dvec.untouched(), 'backward wrote outside dqkv / dvec'
    return dqkv, dvec


def _run(gpu, qkv, d_o, lens, B, T, heads, drop):
    """forward + backward through the C ABI with guards, NaN pre-fill and the determinism checks; returns CPU tensors ctx, lse, dvec, dqkv"""
    qkv_g, do_g = qkv.to(gpu), d_o.to(gpu)
    len_g = torch.tensor(lens, dtype=torch.int32, device=gpu) if lens else None
    ctx, lse = _forward(gpu, qkv_g, len_g, B, T, heads, drop, SITE)
    dqkv, dvec = _backward(gpu, qkv_g, ctx, do_g, lse, len_g, B, T, heads, drop, SITE)
    for name, t in (('ctx', ctx), ('lse', lse), ('dqkv', dqkv), ('dvec', dvec)):
        assert torch.isfinite(t.out.float()).all(), f'{name}: an element was not written (NaN pre-fill) or is not finite'
    # no atomics, deterministic: a second backward is bit-identical
    dqkv2, dvec2 = _backward(gpu, qkv_g, ctx, do_g, lse, len_g, B, T, heads, drop, SITE)
    assert torch.equal(_bits(dqkv.out), _bits(dqkv2.out)) and torch.equal(_bits(dvec.out), _bits(dvec2.out))
    if drop > 0:                      # the same (seed, site) reproduces the mask bit for bit, another site draws another
        ctx2, lse2 = _forward(gpu, qkv_g, len_g, B, T, heads, drop, SITE)
        assert torch.equal(_bits(ctx.out), _bits(ctx2.out)) and torch.equal(_bits(lse.out), _bits(lse2.out))
        ctx3, _ = _forward(gpu, qkv_g, len_g, B, T, heads, drop, SITE + 1)
        assert not torch.equal(_bits(ctx.out), _bits(ctx3.out))
    return ctx.out.cpu(), lse.out.cpu().reshape(B, heads, T), dvec.out.cpu().reshape(B, heads, T), dqkv.out.cpu()


def _check(tag, out, qkv, d_o, lens, B, T, heads, drop, bounds, floor=None, lse_tol=1e-3):
    """the per-case assertions.  ctx, lse and D are held to the reference alone.  The gradients are held to the reference with D taken from the
    kernel's own (bf16-rounded) ctx, which is the kernel's contract: dS = P (m dP - D) is a difference, and the 2^-9 rounding of ctx in D does not
    shrink with it (one valid key: dS = 0 exactly, but D - m dP = the rounding of ctx)."""
    ctx, lse, dvec, dqkv = out
    rctx, rlse, rD = R.mhsa_train_ref(qkv, d_o, lens, B, T, heads, drop, SEED, SITE)[:3]
    rdQ, rdK, rdV = R.mhsa_train_ref(qkv, d_o, lens, B, T, heads, drop, SEED, SITE, ctx_for_D=ctx)[3:]
    H = heads * 64
    lens = R.effective_lengths(lens, T)         # a length of 0 masks nothing: no padded query or key rows in that utterance
    # forward, all q < T (padded queries are ordinary rows)
    e = (lse.double() - rlse).abs()
    assert e.max().item() < lse_tol, (tag, 'lse', e.max().item(), divmod(int(e.argmax()), T))
    e, where = R.row_err(ctx, rctx, B, T, heads)
    bounded(f'mhsa_train[{tag}] ctx row_err.max at (b, head, row) = {where}', e.max().item(), bounds['ctx'])
    # D: the kernel's contract is the fp32 dot product of ITS bf16 ctx with d_o; against the reference it is off by the rounding of ctx
    own = R.d_of(d_o, ctx, B, T, heads)
    e = (dvec.double() - own).abs()
    assert e.max().item() < 1e-5 * own.abs().max().item(), (tag, 'dvec vs its own ctx', e.max().item(), own.abs().max().item())
    slack = 2.0 ** -8 * R.d_abs_sum(d_o, rctx, B, T, heads)
    e = (dvec.double() - rD).abs() - slack
    assert e.max().item() <= 0, (tag, 'dvec vs reference', e.max().item(), divmod(int(e.argmax()), T))
    # gradients
    got = {'dQ': dqkv[:, :H], 'dK': dqkv[:, H:2 * H], 'dV': dqkv[:, 2 * H:]}
    for name, r in (('dQ', rdQ), ('dK', rdK), ('dV', rdV)):
        e, where = R.row_err(got[name], r, B, T, heads, floor=floor[name] if floor else None, rows=None if name == 'dQ' else lens)
        bounded(f'mhsa_train[{tag}] {name} row_err.max at (b, head, row) = {where}', e.max().item(), bounds[name])
        if floor is None:
            bounded(f'mhsa_train[{tag}] {name} rel-L2', R.rel_l2(got[name], r), R.TENSOR_BOUND)
        if name == 'dQ' and lens:               # padded queries still attend to the valid keys: a dQ of their own, under the same bound
            pad = torch.zeros(B, heads, T, dtype=torch.bool)
            for b, n in enumerate(lens):
                pad[b, :, n:] = True
            if pad.any():
                rows = got['dQ'].double().reshape(B, T, heads, 64).transpose(1, 2).abs().amax(dim=-1)
                for b, n in enumerate(lens):    # (one valid key: P = 1 and dS = dP - D = 0 for every query, so there dQ is 0 by the formula)
                    assert n == 1 or (rows[b, :, n:] > 0).all(), (tag, 'a padded query row has dQ = 0 in utterance', b)
                bounded(f'mhsa_train[{tag}] dQ row_err.max over padded queries', e[pad].max().item(), bounds['dQ'])
    if lens:                                    # padded keys: exact zeros, selected not multiplied
        for b, n in enumerate(lens):
            assert torch.count_nonzero(dqkv[b * T + n:(b + 1) * T, H:]) == 0, (tag, 'padded key rows of utterance', b)


SHAPES = {'a': (1, 64, 1, None), 'b': (1, 65, 1, [64]), 'c': (2, 129, 1, [129, 65]), 'd': (R.CASE_D[0], R.CASE_D[1], R.CASE_D[2], list(R.CASE_D[3])),
          'e': (2, 257, 4, [257, 120]), 'f': (3, 200, 3, [200, 77, 1]),
          'g': (3, 130, 2, [130, 0, 65])}      # a silent utterance (length 0): full attention over the T keys, forward and backward
CASES = [(c, p) for c in 'abcdef' for p in (0.0, 0.1)] + [('b', 0.5), ('d', 0.5), ('g', 0.0), ('g', 0.1)]      # T odd in (b) and (c): the last pair of a row is half used


@pytest.mark.parametrize('case,drop', CASES)
def test_mhsa_train_rows_vs_fp64(gpu, case, drop):
    """Worst row_err.max() measured on the MI355X over these cases (the log that conftest.bounded keeps), against ROW_BOUND = 2e-2 each:
    ctx 1.04e-2, dQ 1.28e-2 (1.04e-2 over padded queries), dK 1.16e-2, dV 1.07e-2; whole-tensor rel-L2 at most 2.5e-3 against 6.5e-3"""
    B, T, heads, lens = SHAPES[case]
    qkv, d_o = R.random_operands(B, T, heads, 1000 * T + B)
    if lens:                                    # padded query rows carry a non-zero d_o, so their dQ and their share of dK / dV are non-zero
        for b, n in enumerate(lens):
            assert (d_o[b * T + n:(b + 1) * T].float().abs().amax(dim=-1) > 0).all()
    out = _run(gpu, qkv, d_o, lens, B, T, heads, drop)
    _check(f'{case}:{B},{T},{heads},drop={drop}', out, qkv, d_o, lens, B, T, heads, drop, R.ROW_BOUND)


def test_mhsa_train_one_hot(gpu):
    """P is a permutation matrix to e^-64: ctx = V[perm] and dV[perm[i]] = d_o[i] bit for bit (the dkv kernel's transposed dO^T reads and the
    key <-> lane map of its epilogue), dS vanishes so dQ = dK = 0 to rounding"""
    B, T, heads = 1, 192, 1
    gen = torch.Generator().manual_seed(3)
    perm = torch.randperm(T, generator=gen)
    idx = torch.arange(T)
    assert ((perm // 64) != (idx // 64)).sum() > T // 2 and ((perm // 128) != (idx // 128)).sum() > T // 4       # across key tiles and workgroups
    code = torch.zeros(T, 64)
    for bit in range(8):
        code[:, bit] = ((idx >> bit) & 1).float() * 2 - 1
    K = code * 16.0
    Q = code[perm] * 16.0                       # query i matches key perm[i]: 8 * 256 / 8 = 256 nats, any other key <= 192
    V = torch.randn(T, 64, generator=gen).bfloat16()
    d_o = torch.randn(T, 64, generator=gen).bfloat16()
    qkv = torch.cat([Q, K, V.float()], dim=1).bfloat16()
    small = 1e-6 * d_o.float().abs().max().item() * 16.0
    # the statements hold in the reference for this seed
    rctx, rlse, rD, rdQ, rdK, rdV = R.mhsa_train_ref(qkv, d_o, None, B, T, heads)
    assert torch.equal(rctx.bfloat16(), V[perm]) and torch.equal(rdV.bfloat16()[perm], d_o)
    assert (rlse - 256 * math.log2(math.e)).abs().max().item() < 1e-9 and rdQ.abs().max().item() < small and rdK.abs().max().item() < small
    ctx, lse, dvec, dqkv = _run(gpu, qkv, d_o, None, B, T, heads, 0.0)
    assert torch.equal(ctx, V[perm])
    assert torch.equal(dqkv[:, 128:][perm], d_o)
    assert (lse.double() - 256 * math.log2(math.e)).abs().max().item() < 1e-3
    assert dqkv[:, :64].float().abs().max().item() < small, dqkv[:, :64].float().abs().max().item()
    assert dqkv[:, 64:128].float().abs().max().item() < small, dqkv[:, 64:128].float().abs().max().item()
    own = R.d_of(d_o, ctx, B, T, heads)
    assert (dvec.double() - own).abs().max().item() < 1e-5 * own.abs().max().item()


def test_mhsa_train_uniform_attention(gpu):
    """Q = 0 over 64 valid keys of T = 100: P = 1 / 64 exactly, small-integer V and d_o -> dK = 0 and dV = sum over ALL 100 queries of d_o / 64
    exactly (padded queries are streamed), padded keys zero, lse = 6"""
    B, T, heads, lens = 1, 100, 2, [64]
    H = heads * 64
    gen = torch.Generator().manual_seed(4)
    kk, dd = torch.arange(T)[:, None], torch.arange(H)[None, :]
    V = ((kk + 3 * dd) % 8 - 4 + kk % 2 + dd % 3).float()                 # column sums over the 64 valid keys: 64 (d % 3)
    V[64:] = torch.randint(-6, 7, (T - 64, H), generator=gen).float()     # padded keys: must not matter
    assert (V[:64].sum(0) % 64 == 0).all() and V[:64].sum(0).abs().max() > 0
    d_o = (torch.arange(T * H) % 7 - 3).float().reshape(T, H)
    tot = d_o.sum(0)
    assert tot.abs().max().item() <= 255 and torch.equal((tot / 64).bfloat16().float(), tot / 64)      # exact in bf16
    qkv = torch.cat([torch.zeros(T, H), torch.randn(T, H, generator=gen) * 1.5, V], dim=1).bfloat16()
    d_o = d_o.bfloat16()
    ctx, lse, dvec, dqkv = _run(gpu, qkv, d_o, lens, B, T, heads, 0.0)
    ref = R.mhsa_train_ref(qkv, d_o, lens, B, T, heads)
    mean = (V[:64].sum(0) / 64).expand(T, H)                              # integers
    exact_d = R.d_of(d_o, mean, B, T, heads)
    assert (ref[0] - mean).abs().max().item() < 1e-12 and ref[4].abs().max().item() == 0 and (ref[2] - exact_d).abs().max().item() < 1e-10
    assert (ref[5][:64] - (tot / 64)).abs().max().item() < 1e-12 and (ref[1] - 6.0).abs().max().item() < 1e-12
    assert torch.equal(ctx.float(), mean)
    assert (lse - 6.0).abs().max().item() < 1e-5
    assert torch.equal(dvec.double(), exact_d)                            # integers: the fp32 dot product is exact
    assert torch.count_nonzero(dqkv[:, H:2 * H]) == 0                     # dK = dS^T Q with Q = 0
    assert torch.equal(dqkv[:64, 2 * H:].float(), (tot / 64).expand(64, H))
    assert torch.count_nonzero(dqkv[64:, 2 * H:]) == 0
    e, where = R.row_err(dqkv[:, :H], ref[3], B, T, heads)
    bounded(f'mhsa_train[uniform] dQ row_err.max at (b, head, row) = {where}', e.max().item(), R.ROW_BOUND['dQ'])      # measured 2.1e-3


def _peaked(gpu, tag, qkv, d_o, lens, B, T, heads):
    out = _run(gpu, qkv, d_o, lens, B, T, heads, 0.0)
    _check(tag, out, qkv, d_o, lens, B, T, heads, 0.0, R.ROW_BOUND_PEAKED, floor=R.grad_floors(qkv, d_o, lens, B, T, heads))


def test_mhsa_train_rising_maxima(gpu):
    """the inputs of test_mhsa_rising_maxima (row maxima that climb tile after tile, below the forward's deferred-rescale threshold for some
    query rows and above it for others) through the training path: the backward's exp2(c S - lse) where that branch fired.
    Measured on the MI355X, against ROW_BOUND_PEAKED (gradient rows over max(RMS, grad_floors)): ctx 3.01e-3, dQ 6.80e-3, dK 1.28e-3, dV 7.0e-4"""
    B, T, heads = 1, 512, 2
    torch.manual_seed(11)
    u = torch.ones(64, device=gpu) / 8.0                                            # |u| = 1
    a = torch.rand(T, device=gpu) * 8.0                                             # per-query gain: growth per tile = a (nats)
    bk = 8.0 * (torch.arange(T, device=gpu) // 64).float() + torch.rand(T, device=gpu)
    q = a[:, None] * u[None, :] * 8.0                                               # score / sqrt(64) = a_i * b_j
    k = bk[:, None] * u[None, :]
    v = torch.randn(T, 64, device=gpu)
    one = torch.cat([q, k, v], dim=1)                                               # (T, 192) for one head
    qkv = torch.cat([one[:, 0:64], one[:, 0:64].flip(0), one[:, 64:128], one[:, 64:128], one[:, 128:], one[:, 128:]], dim=1).bfloat16().cpu()
    d_o = torch.randn(T, 128, generator=torch.Generator().manual_seed(11)).bfloat16()
    _peaked(gpu, 'rising maxima', qkv, d_o, [T - 30], B, T, heads)


@pytest.mark.parametrize('level', [-60.0, -20.0, 50.0])
def test_mhsa_train_scores_far_from_zero(gpu, level):
    """every score q . k / 8 sits near `level` nats (+-2 % over the keys), as in test_mhsa_prescaled_far_from_reference: lse up to ~90 in the log2
    domain at an absolute 1e-3, and the backward's exp2(c S - lse) on the difference of two large numbers.
    Worst over the levels measured on the MI355X, against ROW_BOUND_PEAKED (gradient rows over max(RMS, grad_floors)): ctx 2.76e-3, dQ 3.04e-3,
    dK 3.02e-3, dV 9.5e-4"""
    B, T, heads = 1, 200, 1
    gen = torch.Generator().manual_seed(int(abs(level)))
    u = torch.ones(64) / 8.0
    q = (u[None, :] * level * 8.0).repeat(T, 1)                                 # q . k / 8 = level (1 + small)
    k = u[None, :] * (1.0 + 0.02 * torch.randn(T, 1, generator=gen))
    v = torch.randn(T, 64, generator=gen)
    qkv = torch.cat([q, k, v], dim=1).bfloat16()
    d_o = torch.randn(T, 64, generator=gen).bfloat16()
    _peaked(gpu, f'level {level}', qkv, d_o, None, B, T, heads)
