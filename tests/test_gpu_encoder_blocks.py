"""GPU parity of the encoder building blocks (se_gemm_bf16, se_mhsa_fwd_bf16, se_layernorm_f32) through the
C ABI against plain PyTorch fp32 references of the same op on the SAME bf16-rounded operands (so the only
differences are accumulation order and the bf16 rounding of P / outputs).  Exact-integer checks catch
fragment-layout bugs (A = I with an asymmetric B)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def _lib():
    from speech_enhancement_by_s3prl_amd import _lib
    return _lib


def gemm(A, W, bias=None, residual=None, act=0, out='f32'):
    L = _lib()
    lib = L.load()
    M, K = A.shape
    N = W.shape[0]
    o32 = torch.empty(M, N, device=A.device, dtype=torch.float32) if out in ('f32', 'both') else None
    o16 = torch.empty(M, N, device=A.device, dtype=torch.bfloat16) if out in ('bf16', 'both') else None
    L.check(lib.se_gemm_bf16(L.ptr(A), K, L.ptr(W), K, L.ptr(bias), L.ptr(residual), M, N, K, act, L.ptr(o16), L.ptr(o32), N,
                             L.stream()), 'se_gemm_bf16')
    return o32, o16


def test_gemm_identity_asymmetric(gpu):
    """A = I (padded), W asymmetric small integers: exact in bf16 -> exact output, catches row/col swaps."""
    K = 128
    A = torch.zeros(256, K, device=gpu)
    A[:K, :K] = torch.eye(K, device=gpu)
    W = (torch.arange(200 * K, device=gpu).reshape(200, K) % 97 - 40).float()   # W[n][k]
    A16, W16 = A.bfloat16(), W.bfloat16()
    o32, _ = gemm(A16, W16)
    assert torch.equal(o32[:K].cpu(), W.T.cpu())
    assert torch.count_nonzero(o32[K:]) == 0


@pytest.mark.parametrize('M,N,K', [(128, 128, 64), (1001, 768, 768), (300, 201, 768), (2002, 2304, 768), (515, 768, 3072), (77, 768, 128)])
def test_gemm_vs_torch(gpu, M, N, K):
    torch.manual_seed(M + N + K)
    A = torch.randn(M, K, device=gpu).bfloat16()
    W = (torch.randn(N, K, device=gpu) * 0.05).bfloat16()
    bias = torch.randn(N, device=gpu)
    res = torch.randn(M, N, device=gpu)
    ref = A.float().double() @ W.float().double().T + bias.double()
    o32, o16 = gemm(A, W, bias, None, 0, 'both')
    scale = ref.abs().max().item()
    assert (o32.double() - ref).abs().max().item() < 2e-5 * scale + 1e-5 * math.sqrt(K)
    assert (o16.double() - ref).abs().max().item() < 8e-3 * scale
    # fused GELU + residual
    o32, _ = gemm(A, W, bias, res, 3)
    refg = torch.nn.functional.gelu(ref.float()).double() + res.double()
    assert (o32.double() - refg).abs().max().item() < 3e-5 * refg.abs().max().item() + 1e-4


@pytest.mark.parametrize('K', [1536, 2304, 3072])
@pytest.mark.parametrize('M', [4100, 4224])
def test_gemm_n768_row_complete_plain(gpu, M, K):
    """the row-complete kernel without its LayerNorm (gemm4.hip: se_gemm7_plain_launch, se_gemm_bf16's path for N = 768, K >= 1536 past the
    small-batch threshold; called directly so that SE_AMD_GEMM7_PLAIN cannot route around it): every operand combination (bias / residual present
    or not, fp32 / bf16 / both outputs), a ragged last row tile (4100 = 32 x 128 + 4) and a full one; an exact-integer case catches layout slips."""
    import ctypes
    L = _lib()
    lib = L.load()
    fn = lib.se_gemm7_plain_launch
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]

    def plain(A, W, bias=None, residual=None, out='f32'):
        o32 = torch.empty(M, 768, device=gpu, dtype=torch.float32) if out in ('f32', 'both') else None
        o16 = torch.empty(M, 768, device=gpu, dtype=torch.bfloat16) if out in ('bf16', 'both') else None
        L.check(fn(L.ptr(A), K, L.ptr(W), K, L.ptr(bias), L.ptr(residual), M, K, L.ptr(o16), L.ptr(o32), L.stream()), 'se_gemm7_plain_launch')
        return o32, o16

    torch.manual_seed(M + K)
    N = 768
    A = torch.randn(M, K, device=gpu).bfloat16()
    W = (torch.randn(N, K, device=gpu) * 0.05).bfloat16()
    bias = torch.randn(N, device=gpu)
    res = torch.randn(M, N, device=gpu)
    base = A.float().double() @ W.float().double().T
    for use_bias, use_res, out in [(True, True, 'f32'), (False, True, 'both'), (False, False, 'bf16'), (True, False, 'both'), (False, True, 'bf16')]:
        ref = base + (bias.double() if use_bias else 0.0) + (res.double() if use_res else 0.0)
        o32, o16 = plain(A, W, bias if use_bias else None, res if use_res else None, out)
        scale = ref.abs().max().item()
        if o32 is not None:
            assert (o32.double() - ref).abs().max().item() < 2e-5 * scale + 1e-5 * math.sqrt(K)
        if o16 is not None:
            assert (o16.double() - ref).abs().max().item() < 8e-3 * scale
    # exact: A rows are unit vectors (row m selects column m % K of W^T), W small integers
    Ai = torch.zeros(M, K, device=gpu)
    Ai[torch.arange(M, device=gpu), torch.arange(M, device=gpu) % K] = 1.0
    Wi = ((torch.arange(N * K, device=gpu).reshape(N, K) * 7) % 61 - 30).float()
    o32, _ = plain(Ai.bfloat16(), Wi.bfloat16())
    assert torch.equal(o32, Wi.T[torch.arange(M, device=gpu) % K])


GEMM_ROUTES = ('Tile128x2', 'RowComplete768', 'Persistent256', 'Tile256', 'PingPong256x128', 'Lockstep256x128')      # csrc/gemm_route.h


@pytest.mark.parametrize('M,N,K,residual,out,route', [
    (4100, 768, 1536, False, 'f32', 'Tile256'),                 # 33 row tiles: below the row-complete kernel's 160
    (4100, 768, 1536, True, 'bf16', 'PingPong256x128'),         # residual -> bf16: no 256 x 256 instantiation
    (4100, 1536, 128, False, 'both', 'PingPong256x128'),        # two outputs: the generic epilogue
    (7169, 2304, 256, False, 'bf16', 'Persistent256'),          # 29 x 9 = 261 tiles, ragged last row tile
    (7168, 2304, 256, False, 'bf16', 'Tile256'),                # 28 x 9 = 252 tiles: one workgroup per tile
    (4100, 768, 64, False, 'f32', 'Lockstep256x128'),           # one K-tile
    (4100, 201, 128, False, 'f32', 'PingPong256x128'),          # ragged N: the generic epilogue's scalar tail
])
def test_gemm_large_m_routes_vs_torch(gpu, M, N, K, residual, out, route):
    """se_gemm_bf16 past the small-batch threshold (test_gemm_vs_torch stays below it): one case per kernel the dispatch reaches there, at the
    smallest shape that does; M = 4100 and 7169 leave ragged last row tiles.  The route is asserted first (se_gemm_route_of), then the result
    against fp64 on the same bf16 operands with test_gemm_vs_torch's bounds, then an exact-integer case that catches layout slips."""
    import ctypes
    L = _lib()
    fn = L.load().se_gemm_route_of
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] * 12
    got = fn(M, N, K, K, K, N, 0, 1, int(residual), int(out in ('bf16', 'both')), int(out in ('f32', 'both')), 1)
    assert GEMM_ROUTES[got] == route

    def check_aligned(*ts):
        assert all(t is None or t.data_ptr() % 16 == 0 for t in ts)      # what the asserted route assumed

    torch.manual_seed(M + N + K)
    A = torch.randn(M, K, device=gpu).bfloat16()
    W = (torch.randn(N, K, device=gpu) * 0.05).bfloat16()
    bias = torch.randn(N, device=gpu)
    res = torch.randn(M, N, device=gpu) if residual else None
    check_aligned(A, W, bias, res)
    ref = A.float().double() @ W.float().double().T + bias.double() + (res.double() if residual else 0.0)
    o32, o16 = gemm(A, W, bias, res, 0, out)
    check_aligned(o32, o16)
    scale = ref.abs().max().item()
    if o32 is not None:
        err = (o32.double() - ref).abs().max().item()
        print(f'fp32 err {err:.3e} bound {2e-5 * scale + 1e-5 * math.sqrt(K):.3e}')
        assert err < 2e-5 * scale + 1e-5 * math.sqrt(K)
    if o16 is not None:
        err = (o16.double() - ref).abs().max().item()
        print(f'bf16 err {err:.3e} bound {8e-3 * scale:.3e}')
        assert err < 8e-3 * scale
    # exact: A rows are unit vectors (row m selects column m % K of W^T), W / bias / residual small integers (sums below 2^8: exact in bf16)
    rows = torch.arange(M, device=gpu)
    Ai = torch.zeros(M, K, device=gpu)
    Ai[rows, rows % K] = 1.0
    Wi = ((torch.arange(N * K, device=gpu).reshape(N, K) * 7) % 61 - 30).float()
    bi = (torch.arange(N, device=gpu) % 9 - 4).float()
    ri = ((rows[:, None] * 3 + torch.arange(N, device=gpu)[None, :]) % 17 - 8).float() if residual else None
    want = Wi.T[rows % K] + bi + (ri if residual else 0.0)
    o32, o16 = gemm(Ai.bfloat16(), Wi.bfloat16(), bi, ri, 0, out)
    if o32 is not None:
        assert torch.equal(o32, want)
    if o16 is not None:
        assert torch.equal(o16.float(), want)


def mhsa_ref(qkv, lengths, B, T, heads):
    H = heads * 64
    x = qkv.float().view(B, T, 3, heads, 64).permute(2, 0, 3, 1, 4).double()    # (3, B, h, T, 64)
    q, k, v = x[0], x[1], x[2]
    s = q @ k.transpose(-1, -2) / 8.0
    mask = torch.arange(T, device=qkv.device)[None, :] >= lengths[:, None]       # (B, T) True = masked
    s = s.masked_fill(mask[:, None, None, :], float('-inf'))
    p = torch.softmax(s, dim=-1)
    return (p @ v).permute(0, 2, 1, 3).reshape(B * T, H)


@pytest.mark.parametrize('B,T,heads,lens', [(2, 128, 2, None), (2, 1001, 12, None), (3, 200, 3, [200, 77, 1]), (1, 65, 1, [64]), (2, 333, 2, [300, 129])])
def test_mhsa_vs_torch(gpu, B, T, heads, lens):
    L = _lib()
    lib = L.load()
    torch.manual_seed(T)
    H = heads * 64
    qkv = (torch.randn(B * T, 3 * H, device=gpu) * 1.5).bfloat16()
    lengths = torch.tensor(lens if lens else [T] * B, device=gpu, dtype=torch.int32)
    ctx = torch.empty(B * T, H, device=gpu, dtype=torch.bfloat16)
    L.check(lib.se_mhsa_fwd_bf16(L.ptr(qkv), L.ptr(lengths) if lens else None, B, T, heads, L.ptr(ctx), L.stream()), 'se_mhsa_fwd_bf16')
    ref = mhsa_ref(qkv, lengths, B, T, heads)
    err = (ctx.double() - ref).abs().max().item()
    assert err < 2e-2 * ref.abs().max().item(), err      # P and the output are rounded to bf16 (2^-9 relative)


@pytest.mark.parametrize('B,T,heads,lens', [(2, 1001, 12, None), (3, 300, 4, [300, 17, 129]), (1, 64, 1, None), (2, 130, 2, [1, 65]), (8, 257, 1, [257, 200, 64, 63, 1, 128, 129, 256])])
@pytest.mark.parametrize('variant', [0, 10])
def test_mhsa_prescaled_vs_torch(gpu, B, T, heads, lens, variant):
    """the two inference kernels on pre-scaled queries (variant 0: csrc/mhsa.hip's 4-wave kernel, variant 10: csrc/mhsa8.hip's 8-wave kernel)
    vs fp64 on the SAME bf16 operands: softmax_base2(Q' K^T) V with Q' = bf16(Q log2(e) / 8)"""
    L = _lib()
    lib = L.load()
    torch.manual_seed(T + 1)
    H = heads * 64
    x = torch.randn(B * T, 3 * H, device=gpu) * 1.5
    x[:, :H] *= 1.4426950408889634 / 8.0
    qkv = x.bfloat16()
    lengths = torch.tensor(lens if lens else [T] * B, device=gpu, dtype=torch.int32)
    ctx = torch.empty(B * T, H, device=gpu, dtype=torch.bfloat16)
    L.check(lib.se_mhsa_fwd_prescaled_variant_bf16(L.ptr(qkv), L.ptr(lengths) if lens else None, B, T, heads, L.ptr(ctx), variant, L.stream()),
            'se_mhsa_fwd_prescaled_variant_bf16')
    # reference: undo the scale exactly in fp64 on the rounded operands (scores / 8 in nats == Q' K^T in bits)
    q = qkv.double().reshape(B, T, 3, heads, 64)
    Q, K, V = q[:, :, 0].transpose(1, 2), q[:, :, 1].transpose(1, 2), q[:, :, 2].transpose(1, 2)
    S = (Q @ K.transpose(-1, -2)) * 0.6931471805599453                       # bits -> nats
    mask = torch.arange(T, device=gpu)[None, :] >= lengths[:, None].long()
    S = S.masked_fill(mask[:, None, None, :], float('-inf'))
    ref = (torch.softmax(S, dim=-1) @ V).transpose(1, 2).reshape(B * T, H)
    valid = (torch.arange(T, device=gpu)[None, :] < lengths[:, None].long()).reshape(-1) if lens else None
    got = ctx.double()
    err = (got - ref).abs()
    assert torch.isfinite(got).all()
    assert err.max().item() < 8e-3 * ref.abs().max().item(), err.max().item()      # P and the output are rounded to bf16 (2^-9 relative)


MHSA_ROUTES = ('Wave4', 'Wave4Dropout', 'Wave4Prescaled', 'Wave8Prescaled')      # csrc/mhsa_route.h


@pytest.mark.parametrize('B,T,heads,route', [
    (768, 64, 1, 'Wave8Prescaled'),      # 768 8-wave workgroups, pairs % 8 == 0: the XCD mapping
    (767, 64, 1, 'Wave4Prescaled'),      # 767: below the threshold, the plain mapping
    (192, 257, 2, 'Wave8Prescaled'),     # 2 query tiles x 2 heads x 192 = 768, ragged second query tile
    (191, 257, 2, 'Wave4Prescaled'),     # 764
])
def test_mhsa_prescaled_default_dispatch(gpu, B, T, heads, route):
    """se_mhsa_fwd_prescaled_bf16 (the encoder's entry) on both sides of its threshold at the smallest shapes that cross it, ragged lengths
    including 1: bit-identical to the variant entry that se_mhsa_route_of names, and within test_mhsa_prescaled_vs_torch's bound of fp64"""
    import ctypes
    L = _lib()
    lib = L.load()
    fn = lib.se_mhsa_route_of
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] * 5
    got = fn(B, T, heads, 1, 0)
    assert 0 <= got < len(MHSA_ROUTES) and MHSA_ROUTES[got] == route, (got, L.last_error())
    variant = {'Wave4Prescaled': 0, 'Wave8Prescaled': 10}[route]
    torch.manual_seed(B + T)
    H = heads * 64
    x = torch.randn(B * T, 3 * H, device=gpu) * 1.5
    x[:, :H] *= 1.4426950408889634 / 8.0
    qkv = x.bfloat16()
    lengths = (1 + (torch.arange(B, device=gpu) * 37) % T).to(torch.int32)      # 1, 38, 75, ... in [1, T]
    lengths[1] = T
    assert lengths.min().item() == 1 and lengths.max().item() == T
    ctx = torch.full((B * T, H), float('nan'), device=gpu, dtype=torch.bfloat16)
    ctx_v = torch.full((B * T, H), float('nan'), device=gpu, dtype=torch.bfloat16)
    L.check(lib.se_mhsa_fwd_prescaled_bf16(L.ptr(qkv), L.ptr(lengths), B, T, heads, L.ptr(ctx), L.stream()), 'se_mhsa_fwd_prescaled_bf16')
    L.check(lib.se_mhsa_fwd_prescaled_variant_bf16(L.ptr(qkv), L.ptr(lengths), B, T, heads, L.ptr(ctx_v), variant, L.stream()),
            'se_mhsa_fwd_prescaled_variant_bf16')
    assert torch.isfinite(ctx.float()).all()
    assert torch.equal(ctx, ctx_v)
    q = qkv.double().reshape(B, T, 3, heads, 64)
    Q, K, V = q[:, :, 0].transpose(1, 2), q[:, :, 1].transpose(1, 2), q[:, :, 2].transpose(1, 2)
    S = (Q @ K.transpose(-1, -2)) * 0.6931471805599453                       # bits -> nats
    mask = torch.arange(T, device=gpu)[None, :] >= lengths[:, None].long()
    S = S.masked_fill(mask[:, None, None, :], float('-inf'))
    ref = (torch.softmax(S, dim=-1) @ V).transpose(1, 2).reshape(B * T, H)
    err = (ctx.double() - ref).abs().max().item()
    assert err < 8e-3 * ref.abs().max().item(), err      # P and the output are rounded to bf16 (2^-9 relative)


@pytest.mark.parametrize('variant', [0, 10])
def test_mhsa_prescaled_rising_maxima(gpu, variant):
    """rising row maxima across key tiles (both sides of the deferred-rescale branch, which here must also shift the S' tile computed ahead)"""
    L = _lib()
    lib = L.load()
    B, T, heads = 1, 512, 2
    torch.manual_seed(12)
    u = torch.ones(64, device=gpu) / 8.0
    a = torch.rand(T, device=gpu) * 8.0
    bk = 8.0 * (torch.arange(T, device=gpu) // 64).float() + torch.rand(T, device=gpu)
    q = a[:, None] * u[None, :] * 8.0 * (1.4426950408889634 / 8.0)
    k = bk[:, None] * u[None, :]
    v = torch.randn(T, 64, device=gpu)
    one = torch.cat([q, k, v], dim=1)
    qkv = torch.cat([one[:, 0:64], one[:, 0:64].flip(0), one[:, 64:128], one[:, 64:128], one[:, 128:], one[:, 128:]], dim=1).bfloat16()
    ctx = torch.empty(T, 128, device=gpu, dtype=torch.bfloat16)
    lengths = torch.tensor([T - 30], device=gpu, dtype=torch.int32)
    L.check(lib.se_mhsa_fwd_prescaled_variant_bf16(L.ptr(qkv), L.ptr(lengths), B, T, heads, L.ptr(ctx), variant, L.stream()), 'se_mhsa_fwd_prescaled_variant_bf16')
    x = qkv.double().reshape(1, T, 3, heads, 64)
    Q, K, V = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)
    S = (Q @ K.transpose(-1, -2)) * 0.6931471805599453
    S[..., T - 30:] = float('-inf')
    ref = (torch.softmax(S, dim=-1) @ V).transpose(1, 2).reshape(T, 128)
    err = (ctx.double() - ref).abs().max().item()
    assert err < 2e-2 * ref.abs().max().item(), err


@pytest.mark.parametrize('variant', [0, 10])
@pytest.mark.parametrize('level', [-90.0, -30.0, 70.0])
def test_mhsa_prescaled_far_from_reference(gpu, variant, level):
    """every score sits near `level` (base-2 exponent domain): far BELOW the initial reference 0 the speculative exp2(S) of the first tile
    underflows its range test, far ABOVE it overflows -- both must fall back to the exact online softmax (and -30 must not need to)."""
    L = _lib()
    lib = L.load()
    B, T, heads = 1, 200, 1
    torch.manual_seed(int(abs(level)))
    u = torch.ones(64, device=gpu) / 8.0
    q = (u[None, :] * level).repeat(T, 1)                                      # q' . k = level * (1 + small)
    k = u[None, :] * (1.0 + 0.02 * torch.randn(T, 1, device=gpu))
    v = torch.randn(T, 64, device=gpu)
    qkv = torch.cat([q, k, v], dim=1).bfloat16()
    ctx = torch.empty(T, 64, device=gpu, dtype=torch.bfloat16)
    L.check(lib.se_mhsa_fwd_prescaled_variant_bf16(L.ptr(qkv), None, B, T, heads, L.ptr(ctx), variant, L.stream()), 'se_mhsa_fwd_prescaled_variant_bf16')
    x = qkv.double()
    S = (x[:, :64] @ x[:, 64:128].T) * 0.6931471805599453
    ref = torch.softmax(S, dim=-1) @ x[:, 128:]
    got = ctx.double()
    assert torch.isfinite(got).all()
    assert (got - ref).abs().max().item() < 2e-2 * ref.abs().max().item()


def test_mhsa_rising_maxima(gpu):
    """Row maxima that climb tile after tile, by less than the deferred-rescale threshold for some query rows and by more for
    others in the same wave: exercises both sides of the (rare, data-dependent) rescale branch of the online softmax."""
    L = _lib()
    lib = L.load()
    B, T, heads = 1, 512, 2
    torch.manual_seed(11)
    u = torch.ones(64, device=gpu) / 8.0                                            # |u| = 1
    a = torch.rand(T, device=gpu) * 8.0                                             # per-query gain: growth per tile = a (nats)
    bk = 8.0 * (torch.arange(T, device=gpu) // 64).float() + torch.rand(T, device=gpu)
    q = a[:, None] * u[None, :] * 8.0                                               # score / sqrt(64) = a_i * b_j
    k = bk[:, None] * u[None, :]
    v = torch.randn(T, 64, device=gpu)
    one = torch.cat([q, k, v], dim=1)                                               # (T, 192) for one head
    qkv = torch.cat([one[:, 0:64], one[:, 0:64].flip(0), one[:, 64:128], one[:, 64:128], one[:, 128:], one[:, 128:]], dim=1).bfloat16()
    ctx = torch.empty(T, 128, device=gpu, dtype=torch.bfloat16)
    lengths = torch.tensor([T - 30], device=gpu, dtype=torch.int32)
    L.check(lib.se_mhsa_fwd_bf16(L.ptr(qkv), L.ptr(lengths), B, T, heads, L.ptr(ctx), L.stream()), 'se_mhsa_fwd_bf16')
    ref = mhsa_ref(qkv, lengths, B, T, heads)
    err = (ctx.double() - ref).abs().max().item()
    assert err < 2e-2 * ref.abs().max().item(), err


def test_mhsa_exact_integers(gpu):
    """uniform attention (Q = 0) over integer V: output = mean of V rows -> exercises the V^T / P operand maps."""
    L = _lib()
    lib = L.load()
    B, T, heads = 1, 64, 1
    qkv = torch.zeros(T, 192, device=gpu)
    V = (torch.arange(T * 64, device=gpu).reshape(T, 64) % 13 - 6).float()          # asymmetric small ints
    qkv[:, 128:] = V
    qkv[:, 64:128] = torch.randn(T, 64, device=gpu)                                  # K irrelevant when Q = 0
    ctx = torch.empty(T, 64, device=gpu, dtype=torch.bfloat16)
    qkv16 = qkv.bfloat16()
    L.check(lib.se_mhsa_fwd_bf16(L.ptr(qkv16), None, B, T, heads, L.ptr(ctx), L.stream()), 'se_mhsa_fwd_bf16')
    ref = V.mean(dim=0, keepdim=True).expand(T, 64)
    assert (ctx.float() - ref).abs().max().item() < 2e-2


def test_mhsa_one_hot_attention(gpu):
    """Q.K large on one key per query -> output row = that V row (checks the key <-> register map)."""
    L = _lib()
    lib = L.load()
    T = 128
    torch.manual_seed(3)
    perm = torch.randperm(T, device=gpu)
    basis = torch.zeros(T, 64, device=gpu)
    # orthogonal-ish codes: use 7-bit binary code of the key index in +-1, scaled
    idx = torch.arange(T, device=gpu)
    for bit in range(7):
        basis[:, bit] = ((idx >> bit) & 1).float() * 2 - 1
    K = basis * 16.0
    Q = basis[perm] * 16.0              # query i matches key perm[i] with score 7*256/8 = 224, others <= 160
    V = (torch.randn(T, 64, device=gpu)).bfloat16().float()
    qkv = torch.cat([Q, K, V], dim=1).bfloat16()
    ctx = torch.empty(T, 64, device=gpu, dtype=torch.bfloat16)
    L.check(lib.se_mhsa_fwd_bf16(L.ptr(qkv), None, 1, T, 1, L.ptr(ctx), L.stream()), 'se_mhsa_fwd_bf16')
    assert (ctx.float() - V[perm]).abs().max().item() < 1e-2


@pytest.mark.parametrize('M,H', [(1001, 768), (7, 768), (33, 320)])
def test_layernorm(gpu, M, H):
    L = _lib()
    lib = L.load()
    torch.manual_seed(M)
    x = torch.randn(M, H, device=gpu) * 3 + 1
    w, b = torch.randn(H, device=gpu), torch.randn(H, device=gpu)
    o32 = torch.empty_like(x)
    o16 = torch.empty(M, H, device=gpu, dtype=torch.bfloat16)
    L.check(lib.se_layernorm_f32(L.ptr(x), L.ptr(w), L.ptr(b), M, H, 1e-12, L.ptr(o32), L.ptr(o16), L.stream()), 'se_layernorm_f32')
    ref = torch.nn.functional.layer_norm(x.double(), (H,), w.double(), b.double(), 1e-12)
    assert (o32.double() - ref).abs().max().item() < 2e-5
    assert (o16.double() - ref).abs().max().item() < 4e-2


@pytest.mark.parametrize('M,K', [(1001, 768), (300, 3072), (129, 128), (32032, 768)])
def test_gemm_res_ln_vs_torch(gpu, M, K):
    """row-complete GEMM + bias + residual + LayerNorm (N = 768) vs fp64 on the same bf16 operands"""
    L = _lib()
    lib = L.load()
    torch.manual_seed(M + K)
    N = 768
    A = torch.randn(M, K, device=gpu).bfloat16()
    W = (torch.randn(N, K, device=gpu) * 0.03).bfloat16()
    bias, res = torch.randn(N, device=gpu) * 0.1, torch.randn(M, N, device=gpu)
    lw, lb = 1 + 0.1 * torch.randn(N, device=gpu), 0.1 * torch.randn(N, device=gpu)
    o32 = torch.empty(M, N, device=gpu)
    o16 = torch.empty(M, N, device=gpu, dtype=torch.bfloat16)
    L.check(lib.se_gemm_res_ln_bf16(L.ptr(A), K, L.ptr(W), K, L.ptr(bias), L.ptr(res), L.ptr(lw), L.ptr(lb), 1e-12, M, N, K,
                                    L.ptr(o32), L.ptr(o16), L.stream()), 'se_gemm_res_ln_bf16')
    x = A.double() @ W.double().T + bias.double() + res.double()
    ref = torch.nn.functional.layer_norm(x, (N,), lw.double(), lb.double(), 1e-12)
    assert (o32.double() - ref).abs().max().item() < 5e-5
    assert (o16.double() - ref).abs().max().item() < 4e-2


def test_gemm_res_ln_exact_rows(gpu):
    """A = one-hot rows selecting weight rows (exact in bf16): catches row / column mapping errors before the LayerNorm"""
    L = _lib()
    lib = L.load()
    M, K, N = 256, 128, 768
    A = torch.zeros(M, K, device=gpu)
    A[torch.arange(M), torch.arange(M) % K] = 1.0
    W = ((torch.arange(N * K, device=gpu).reshape(N, K) * 7 % 61) - 30).float()
    res = torch.zeros(M, N, device=gpu)
    ones, zeros = torch.ones(N, device=gpu), torch.zeros(N, device=gpu)
    o32 = torch.empty(M, N, device=gpu)
    A16, W16 = A.bfloat16(), W.bfloat16()        # keep the operands alive: a temporary's memory is recycled before the launch
    L.check(lib.se_gemm_res_ln_bf16(L.ptr(A16), K, L.ptr(W16), K, L.ptr(zeros), L.ptr(res), L.ptr(ones), L.ptr(zeros), 1e-12,
                                    M, N, K, L.ptr(o32), None, L.stream()), 'se_gemm_res_ln_bf16')
    x = W.T[torch.arange(M) % K].double()                      # row m of the product = column (m % K) of W^T
    ref = (x - x.mean(-1, keepdim=True)) / x.var(-1, unbiased=False, keepdim=True).sqrt()
    assert (o32.double() - ref).abs().max().item() < 1e-5


@pytest.mark.parametrize('M,K', [(32032, 3072), (602, 768), (1001, 3072), (257, 128)])
def test_gemm_res24_row_complete_vs_fp64(gpu, M, K):
    """The row-complete projection + residual + LayerNorm on the 24-bit residual stream (gemm4.hip: gemm7_res_ln_kernel, the encoder's out-proj / FFN2
    launch at bench size) through its measurement entry: both output forms (fp32 rows; bf16 + lo bytes) against fp64, ragged row counts (602 = 4 x 128
    + 90, 257: one row into the third tile), the bench shape; a non-zero low byte plane decodes as hi + lo * 2^-8 ulp(hi).  (The 256 x 384
    pair-exchange kernel this test used to compare with is parked under tools/experiments/kernels/ with its own test.)"""
    L = _lib()
    lib = L.load()
    torch.manual_seed(M + K)
    N = 768
    A = torch.randn(M, K, device=gpu).bfloat16()
    W = (torch.randn(N, K, device=gpu) * 0.03).bfloat16()
    bias = torch.randn(N, device=gpu) * 0.1
    res = torch.randn(M, N, device=gpu).bfloat16()
    nlo = lib.se_gemm_res24_lo_bytes(M)
    res_lo = torch.zeros(nlo, device=gpu, dtype=torch.uint8)            # low bytes 0: the residual is exactly the bf16 tensor
    lw, lb = torch.randn(N, device=gpu), torch.randn(N, device=gpu)
    scratch = torch.zeros(lib.se_gemm_res24_scratch_bytes(), device=gpu, dtype=torch.uint8)
    ref = torch.nn.functional.layer_norm(A.double() @ W.double().T + bias.double() + res.double(), (N,), lw.double(), lb.double(), 1e-12)

    def run(variant, fp32_out):
        o32 = torch.full((M, N), float('nan'), device=gpu) if fp32_out else None
        o16 = None if fp32_out else torch.zeros(M, N, device=gpu, dtype=torch.bfloat16)
        olo = None if fp32_out else torch.zeros(nlo, device=gpu, dtype=torch.uint8)
        rc = lib.se_gemm_res24_ln_bf16(L.ptr(A), K, L.ptr(W), K, L.ptr(bias), L.ptr(res), L.ptr(res_lo), L.ptr(lw), L.ptr(lb), 1e-12, M, N, K,
                                       L.ptr(o32), L.ptr(o16), L.ptr(olo), variant, L.ptr(scratch), L.stream())
        return rc, o32, o16, olo

    rc, o7, _, _ = run(7, True)
    assert rc == 0
    scale = ref.abs().max().item()
    assert (o7.double() - ref).abs().max().item() < 2e-5 * scale + 2e-4
    rc0, o0, _, _ = run(0, True)                                         # variant 0 = the encoder's dispatch: the same kernel in the product library
    assert rc0 == 0 and torch.equal(o0, o7)
    rc, _, b7, l7 = run(7, False)
    assert rc == 0 and (b7.double() - ref).abs().max().item() < 2 ** -8 * scale
    # the 24-bit value (bf16 + signed low byte on the fp32 bit pattern, gemm4.hip) is the fp32 row to 2^-16 relative: rows of the row-major part of
    # the tile-major low plane are not decoded here; the decode is exercised end to end by the next launch reading (b7, l7) as its residual
    rc, o_next, _, _ = (lambda: (lib.se_gemm_res24_ln_bf16(L.ptr(A), K, L.ptr(W), K, L.ptr(bias), L.ptr(b7), L.ptr(l7), L.ptr(lw), L.ptr(lb), 1e-12, M, N, K,
                                                           L.ptr(o7), None, None, 7, L.ptr(scratch), L.stream()), o7, None, None))()
    assert rc == 0
    ref2 = torch.nn.functional.layer_norm(A.double() @ W.double().T + bias.double() + ref, (N,), lw.double(), lb.double(), 1e-12)
    assert (o_next.double() - ref2).abs().max().item() < 1e-4 * ref2.abs().max().item() + 2e-4      # a bf16-only residual would be ~4e-3 off
    assert lib.se_gemm_res24_ln_bf16(L.ptr(A), K, L.ptr(W), K, L.ptr(bias), L.ptr(res), L.ptr(res_lo), L.ptr(lw), L.ptr(lb), 1e-12, M, N, K,
                                     L.ptr(o7), None, None, 8, L.ptr(scratch), L.stream()) != 0      # the parked experiment is refused, loudly


def test_gemm6_dual_gelu_launch_bit_identical_to_the_two_launches(gpu):
    """gemm6.hip: se_gemm6_dual_gelu_launch (the training forward's FFN1: pre-activation AND its GELU from one persistent launch; reached from
    encoder_train.hip only above 256 tiles, i.e. never by the small-shape training tests -- ADVICE r4): a ragged last row tile (8192 + 37 rows),
    both outputs in separate allocations with guard rows, bit-identical to se_gemm_bf16(identity) followed by se_gelu_bf16."""
    import ctypes
    L = _lib()
    lib = L.load()
    fn = lib.se_gemm6_dual_gelu_launch
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    M, N, K = 8192 + 37, 3072, 768
    torch.manual_seed(5)
    A = torch.randn(M, K, device=gpu).bfloat16()
    W = (torch.randn(N, K, device=gpu) * 0.05).bfloat16()
    bias = torch.randn(N, device=gpu)
    pre = torch.full((M + 8, N), 3.0, device=gpu, dtype=torch.bfloat16)
    act = torch.full((M + 8, N), 5.0, device=gpu, dtype=torch.bfloat16)
    assert fn(L.ptr(A), K, L.ptr(W), K, L.ptr(bias), M, N, K, L.ptr(pre), L.ptr(act), N, L.stream()) == 0
    _, ref_pre = gemm(A, W, bias, None, 0, 'bf16')
    ref_act = torch.empty_like(ref_pre)
    L.check(lib.se_gelu_bf16(L.ptr(ref_pre), ref_pre.numel(), L.ptr(ref_act), L.stream()), 'se_gelu_bf16')
    torch.cuda.synchronize()
    assert torch.equal(pre[:M], ref_pre) and torch.equal(act[:M], ref_act)
    assert torch.all(pre[M:] == 3.0) and torch.all(act[M:] == 5.0)
    # and against the fp64 product, so that the reference path is not the only witness
    ref = A[:512].double() @ W.double().T + bias.double()
    assert (pre[:512].double() - ref).abs().max().item() < 8e-3 * ref.abs().max().item()


@pytest.mark.parametrize('res,out', [(False, 'bf16'), (True, 'f32'), (False, 'f32')])
def test_gemm_bf16_large_m_n768_dispatch_vs_fp64(gpu, res, out):
    """se_gemm_bf16 at M > 20 352, N = 768, K = 3072: the dispatcher's >= 160-row-tile route (the row-complete kernel without its LayerNorm,
    gemm4.hip) that only the fine-tune bench reached -- with / without residual, fp32 / bf16 rows, against the fp64 product."""
    M, N, K = 20352 + 131, 768, 3072
    torch.manual_seed(9)
    A = torch.randn(M, K, device=gpu).bfloat16()
    W = (torch.randn(N, K, device=gpu) * 0.03).bfloat16()
    bias = torch.randn(N, device=gpu)
    r = torch.randn(M, N, device=gpu) if res else None
    o32, o16 = gemm(A, W, bias, r, 0, out)
    got = o32 if out == 'f32' else o16
    worst = 0.0
    for lo in range(0, M, 4096):
        hi = min(M, lo + 4096)
        ref = A[lo:hi].double() @ W.double().T + bias.double()
        if res:
            ref = ref + r[lo:hi].double()
        worst = max(worst, (got[lo:hi].double() - ref).abs().max().item() / ref.abs().max().item())
    assert worst < (8e-3 if out == 'bf16' else 5e-5), worst
