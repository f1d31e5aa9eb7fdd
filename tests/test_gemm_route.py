"""CPU: which kernel se_gemm_bf16 runs for a call (csrc/gemm_route.h).

(a) gemm_route_walk.cpp, a stand-alone program that includes only gemm_route.h, is built with the host compiler under -Wall -Werror and the
address / undefined-behaviour sanitizers and walks a grid of calls: the chosen route's predicate holds, dispatch is total, and the route equals
what the try-and-fall-through chain it replaced would have launched (restated there, launcher by launcher).
(b) se_gemm_route_of (the library's internal export; touches no device) returns the routes of the table below."""
import ctypes
import itertools
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'speech-enhancement-by-s3prl_amd', 'csrc')

ROUTES = ('Tile128x2', 'RowComplete768', 'Persistent256', 'Tile256', 'PingPong256x128', 'Lockstep256x128')      # enum class GemmRoute, in order
IDENTITY, RELU, SIGMOID, GELU, EXP = range(5)


def route_of(M, N, K, act=IDENTITY, bias=True, residual=False, bf16=False, f32=False, aligned=True, lda=None, ldw=None, ldc=None):
    from speech_enhancement_by_s3prl_amd import _lib
    fn = _lib.load().se_gemm_route_of
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] * 12
    r = fn(M, N, K, lda or K, ldw or K, ldc or N, act, int(bias), int(residual), int(bf16), int(f32), int(aligned))
    assert 0 <= r < len(ROUTES), (r, _lib.last_error())
    return ROUTES[r]


def test_route_walk_standalone(tmp_path):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'gemm_route_walk')
    subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-I', CSRC,
                    os.path.join(ROOT, 'tests', 'gemm_route_walk.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith('calls 69984 bad 0 '), r.stdout        # 3 tunings x 9 M x 6 N x 6 K x 3 activations x 2 x 2 x 3 outputs x 2


def test_route_header_is_host_only():
    """gemm_route.h compiles without HIP: it includes the C library only"""
    src = open(os.path.join(CSRC, 'gemm_route.h')).read()
    incs = [ln.split()[1] for ln in src.splitlines() if ln.startswith('#include')]
    assert incs and all(i in ('<stddef.h>', '<stdlib.h>') for i in incs), incs


def test_route_table_bench_shapes():
    """the headline pass at 32 utterances (M = 32 x 1001): QKV and FFN1 on the persistent kernel, the training path's FFN2 on the row-complete
    one, the K = 768 output projection and the ragged spec-head output on the 256 x 128 ping-pong kernel"""
    M = 32032
    assert route_of(M, 2304, 768, IDENTITY, bf16=True) == 'Persistent256'
    assert route_of(M, 3072, 768, GELU, bf16=True) == 'Persistent256'
    assert route_of(M, 768, 3072, IDENTITY, residual=True, f32=True) == 'RowComplete768'
    assert route_of(M, 768, 768, IDENTITY, residual=True, f32=True) == 'PingPong256x128'
    for act, bias, residual, (bf16, f32), aligned in itertools.product((IDENTITY, RELU, SIGMOID, GELU, EXP), (0, 1), (0, 1), ((1, 0), (0, 1), (1, 1)), (0, 1)):
        assert route_of(M, 201, 768, act, bias, residual, bf16, f32, aligned) == 'PingPong256x128'


def test_route_table_small_m():
    """up to 4096 rows every call runs on the 128 x 128 two-workgroups-per-CU kernel"""
    for M, N, K in itertools.product((1, 77, 1001, 4004, 4096), (128, 201, 768, 2304, 3072), (64, 768, 3072)):
        for act, residual, (bf16, f32), aligned in itertools.product((IDENTITY, GELU, RELU), (0, 1), ((1, 0), (0, 1), (1, 1)), (0, 1)):
            assert route_of(M, N, K, act, True, residual, bf16, f32, aligned) == 'Tile128x2'
    assert route_of(4097, 2304, 768, bf16=True) != 'Tile128x2'


def test_route_table_thresholds():
    assert route_of(4100, 768, 1536, IDENTITY, f32=True) == 'Tile256'                          # 33 row tiles < 160: not the row-complete kernel
    assert route_of(4100, 768, 1536, IDENTITY, residual=True, bf16=True) == 'PingPong256x128'   # no 256 x 256 instantiation: residual -> bf16
    assert route_of(4100, 1536, 128, bf16=True, f32=True) == 'PingPong256x128'                 # two outputs: the generic epilogue
    assert route_of(7169, 2304, 256, IDENTITY, bf16=True) == 'Persistent256'                   # 29 x 9 = 261 tiles > 256
    assert route_of(7168, 2304, 256, IDENTITY, bf16=True) == 'Tile256'                         # 28 x 9 = 252 tiles
    for act, residual, (bf16, f32) in itertools.product((IDENTITY, GELU), (0, 1), ((1, 0), (0, 1), (1, 1))):
        assert route_of(4100, 768, 64, act, True, residual, bf16, f32) == 'Lockstep256x128'    # one K-tile: the ping-pong prologue needs two
    # the row-complete kernel from 160 row tiles of 128 on
    assert route_of(20352, 768, 1536, IDENTITY, residual=True, f32=True) == 'Tile256'          # 159 row tiles
    assert route_of(20353, 768, 1536, IDENTITY, residual=True, f32=True) == 'RowComplete768'
    assert route_of(20353, 768, 1536, IDENTITY, residual=True, bf16=True, f32=True) == 'RowComplete768'
    assert route_of(20353, 768, 1536, GELU, f32=True) == 'Tile256'


def test_route_table_matches_the_recorded_kernel_names():
    """the first three rows of the table against the kernel names that the round-5 profiles recorded: QKV and FFN1 in the benchmark's pass; the
    N = 768, K = 3072 projection reaches se_gemm_bf16 in the fine-tune step only (the inference pass fuses it with its LayerNorm)"""
    names = open(os.path.join(ROOT, 'profiles', 'r05c_bench_kernel_stats.csv')).read()
    assert 'gemm6p_bf16_kernel<0, 2, 0>' in names and 'gemm6p_bf16_kernel<3, 2, 0>' in names      # QKV (identity), FFN1 (GELU): Persistent256
    assert 'gemm6_bf16_kernel' not in names and 'gemm3' not in names
    names = open(os.path.join(ROOT, 'profiles', 'r05c_finetune_bench_kernel_stats.csv')).read()
    assert 'gemm7_res_ln_kernel<0, 0, 0, 1, 0, 0>' in names                                        # RowComplete768


def test_route_of_rejects_invalid_calls():
    from speech_enhancement_by_s3prl_amd import _lib
    fn = _lib.load().se_gemm_route_of
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] * 12
    assert fn(128, 128, 100, 100, 100, 128, 0, 1, 0, 1, 0, 1) == -1          # K % 64 != 0: SE_ERR_INVALID, as se_gemm_bf16
    assert fn(128, 128, 64, 64, 64, 128, 0, 1, 0, 0, 0, 1) == -1             # no output
