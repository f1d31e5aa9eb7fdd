"""CPU: which kernel an attention forward call runs (csrc/mhsa_route.h).

(a) mhsa_route_walk.cpp, a stand-alone program that includes only mhsa_route.h, is built with the host compiler under -Wall -Werror and the
address / undefined-behaviour sanitizers and walks a grid of calls: the route and its grid equal what the launch chain it replaced would have
launched (restated there, function by function), and the route's predicate fails exactly where that chain failed the call.
(b) se_mhsa_route_of (the library's internal export; touches no device) returns the routes of the table below.
(c) the sources keep the dispatch in that one header."""
import ctypes
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'speech-enhancement-by-s3prl_amd', 'csrc')

ROUTES = ('Wave4', 'Wave4Dropout', 'Wave4Prescaled', 'Wave8Prescaled')      # enum class MhsaRoute, in order


def _route_fn():
    from speech_enhancement_by_s3prl_amd import _lib
    fn = _lib.load().se_mhsa_route_of
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] * 5
    return fn


def route_of(B, T, heads, prescaled, dropout=False):
    from speech_enhancement_by_s3prl_amd import _lib
    r = _route_fn()(B, T, heads, int(prescaled), int(dropout))
    assert 0 <= r < len(ROUTES), (r, _lib.last_error())
    return ROUTES[r]


def test_route_walk_standalone(tmp_path):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'mhsa_route_walk')
    subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-I', CSRC,
                    os.path.join(ROOT, 'tests', 'mhsa_route_walk.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith('calls 8640 bad 0 '), r.stdout        # 4 tunings x 12 B x 12 T x 5 heads x (plain, dropout, prescaled)


def test_route_header_is_host_only():
    """mhsa_route.h compiles without HIP: it includes the C library only"""
    src = open(os.path.join(CSRC, 'mhsa_route.h')).read()
    incs = [ln.split()[1] for ln in src.splitlines() if ln.startswith('#include')]
    assert incs and all(i in ('<stddef.h>', '<stdlib.h>') for i in incs), incs


def test_route_table():
    """the benchmark's pass (32 utterances of 1001 frames, 12 heads) on the 8-wave kernel; the threshold of 768 8-wave workgroups
    (4 query tiles x 12 heads x B) lies between B = 15 and B = 16; the training entries on the 4-wave kernels"""
    assert route_of(32, 1001, 12, True) == 'Wave8Prescaled'
    assert route_of(15, 1001, 12, True) == 'Wave4Prescaled'       # 720 workgroups
    assert route_of(16, 1001, 12, True) == 'Wave8Prescaled'       # 768 workgroups
    assert route_of(767, 64, 1, True) == 'Wave4Prescaled'
    assert route_of(768, 64, 1, True) == 'Wave8Prescaled'
    assert route_of(191, 257, 2, True) == 'Wave4Prescaled'        # 2 query tiles x 2 heads x 191 = 764
    assert route_of(192, 257, 2, True) == 'Wave8Prescaled'
    for B, T, heads in ((1, 1, 1), (32, 1001, 12), (768, 64, 1), (3, 200, 3)):
        assert route_of(B, T, heads, False) == 'Wave4'
        assert route_of(B, T, heads, False, dropout=True) == 'Wave4Dropout'


def test_route_of_fails_where_the_call_fails():
    """invalid shapes as the entries reject them; a call whose route cannot run it fails (SE_ERR_INVALID, as the launch) and is not re-routed"""
    fn = _route_fn()
    assert fn(0, 100, 4, 1, 0) == -1 and fn(65536, 100, 4, 1, 0) == -1 and fn(2, 0, 4, 1, 0) == -1 and fn(2, 100, 0, 1, 0) == -1
    assert fn(2, 100, 4, 1, 1) == -1                              # the prescaled entries have no dropout
    assert fn(64, 466033, 12, 1, 0) == ROUTES.index('Wave8Prescaled')
    assert fn(64, 466034, 12, 1, 0) == -1                         # T * 3 H * 2 = 2^31 + 1024 bytes: past the 8-wave kernel's 31-bit DMA offsets
    assert fn(64, 20000, 12, 0, 1) == -1                          # 64 x 12 x 20000 x 10000 dropout pairs > 2^32
    assert fn(64, 20000, 12, 0, 0) == ROUTES.index('Wave4')


def test_route_table_matches_the_recorded_kernel_name():
    """the first row of the table against the round-5 profile of the benchmark's pass, which recorded the 8-wave kernel under its earlier name"""
    names = open(os.path.join(ROOT, 'profiles', 'r05c_bench_kernel_stats.csv')).read()
    fwd = set(re.findall(r'mhsa\w*_fwd_kernel<[^>]*>', names))
    assert fwd == {'mhsaN_fwd_kernel<8, 4, 1>'}, fwd


def test_dispatch_lives_in_the_route_header():
    """no attention environment switch is read outside mhsa_route.h, and the two files carry no experiment call sites (the DROP == 2 entry,
    one experiment across three files, keeps its own #ifdef)"""
    for f in sorted(os.listdir(CSRC)):
        if f != 'mhsa_route.h' and os.path.isfile(os.path.join(CSRC, f)):
            assert 'getenv("SE_AMD_MHSA' not in open(os.path.join(CSRC, f)).read(), f
    assert '#ifdef SE_AMD_EXPERIMENTS' not in open(os.path.join(CSRC, 'mhsa8.hip')).read()
    src = open(os.path.join(CSRC, 'mhsa.hip')).read()
    blocks = re.findall(r'#ifdef SE_AMD_EXPERIMENTS.*?#endif', src, flags=re.S)
    assert len(blocks) == 1 and 'se_mhsa_fwd_lse_masked_bf16' in blocks[0], [b[:80] for b in blocks]
