"""CPU: the FFT core of the general STFT plan (csrc/fftg.h, csrc/fftg_plan.h) and the argument validation of se_plan_create_any.

(a) fftg_walk.cpp, a stand-alone program that includes only the two headers, is built with the host compiler under -Wall -Werror and the
address / undefined-behaviour sanitizers.  For every m in {16, 18, 20, 30, 45, 100, 160, 200, 256, 375, 512} (each radix alone, all mixed,
and the complex sizes of the 400- and 512-point front ends) it runs the run-time-scheduled Stockham transform -- the same functions the
kernels run on LDS rows -- the real-transform post pass and the inverse pre-pass on a random input and four impulses, against a float64
direct DFT.  Bound: 1e-5 of the spectrum's maximum, what the project holds the 400-point kernel to (test_stft_vs_float64_dft).  Measured
when the bound was fixed: 4e-8 (m = 16) ... 3.1e-7 (m = 512, inverse), every size 30x or more inside the bound, so no size has a bound of
its own.
(b) se_plan_create_any refuses every geometry outside the supported set with SE_ERR_UNSUPPORTED and a message naming the violated rule,
without a device; se_plan_create keeps refusing everything but 201 / 160 / win <= 400."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'speech-enhancement-by-s3prl_amd', 'csrc')
SIZES = (16, 18, 20, 30, 45, 100, 160, 200, 256, 375, 512)
BOUND = 1e-5


@functools.lru_cache(maxsize=None)
def _walk(tmp):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = os.path.join(tmp, 'fftg_walk')
    subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-I', CSRC,
                    os.path.join(ROOT, 'tests', 'fftg_walk.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.fixture(scope='module')
def walk(tmp_path_factory):
    return _walk(str(tmp_path_factory.mktemp('fftg')))


def test_core_vs_float64_dft(walk):
    rows = {}
    for ln in walk.splitlines():
        mt = re.match(r'm (\d+) radices (\S+) fft (\S+) rfft (\S+) inv (\S+) rinv (\S+)$', ln)
        if mt:
            rows[int(mt.group(1))] = (mt.group(2), [float(mt.group(i)) for i in range(3, 7)])
    assert tuple(sorted(rows)) == SIZES, walk
    for m, (radices, errs) in rows.items():
        print(m, radices, errs)
        prod = 1
        for r in radices.split('x'):
            assert int(r) in (2, 3, 4, 5), (m, radices)
            prod *= int(r)
        assert prod == m, (m, radices)                      # the schedule's radices multiply to m
        for name, e in zip(('fft', 'rfft', 'inv', 'rinv'), errs):
            assert e == e and e < BOUND, (m, name, e)


def test_rules_in_the_walk(walk):
    """the rule numbering of fftg_check_geometry, exercised under the sanitizers too"""
    assert walk.rstrip().endswith('rules ok'), walk


def test_headers_are_host_only():
    """fftg.h includes nothing; fftg_plan.h the C library, <initializer_list> and fftg.h: both compile without HIP"""
    inc = lambda f: [ln.split()[1] for ln in open(os.path.join(CSRC, f)).read().splitlines() if ln.startswith('#include')]      # noqa: E731
    assert inc('fftg.h') == []
    assert set(inc('fftg_plan.h')) == {'<math.h>', '<stddef.h>', '<stdio.h>', '<initializer_list>', '"fftg.h"'}
    assert '__builtin_amdgcn' not in open(os.path.join(CSRC, 'fftg.h')).read()


# (win, hop, n_freq, n_mels) -> a fragment of the message that names the rule
REFUSED = [
    ((14, 7, 8, 40), 'it has the factor 7'),                   # m = 7
    ((70, 35, 36, 40), 'it has the factor 7'),                 # m = 35 = 5 x 7
    ((400, 201, 201, 40), 'must not exceed win / 2'),          # hop > win / 2
    ((400, 49, 201, 40), 'at least ceil(n_fft / 8)'),          # hop < n_fft / 8
    ((401, 160, 201, 40), 'win = 401 must lie in [2, n_fft'),  # win > n_fft
    ((400, 160, 1025, 40), 'must lie in [32, 1024]'),          # n_fft = 2048
    ((16, 8, 9, 40), 'must lie in [32, 1024]'),                # n_fft = 16
    ((400, 160, 201, 129), 'n_mels = 129'),
]


@pytest.mark.parametrize('geom,fragment', REFUSED)
def test_create_any_names_the_violated_rule(geom, fragment):
    from speech_enhancement_by_s3prl_amd import _lib
    lib = _lib.load()
    out = ctypes.c_void_p()
    rc = lib.se_plan_create_any(_lib.Geometry(16000, *geom), out)
    msg = lib.se_last_error().decode()
    assert rc == -2 and 'unsupported geometry' in msg and fragment in msg, (rc, msg)
    assert out.value is None


@pytest.mark.parametrize('geom', [(32, 8, 17, 40), (50, 20, 31, 40), (200, 80, 101, 40), (320, 160, 161, 40), (400, 160, 201, 128),
                                  (512, 128, 257, 40), (1024, 256, 513, 80), (1024, 128, 513, 40)])
def test_create_any_supported_geometry_needs_a_device(geom):
    from speech_enhancement_by_s3prl_amd import _lib
    lib = _lib.load()
    out = ctypes.c_void_p()
    rc = lib.se_plan_create_any(_lib.Geometry(16000, *geom), out)
    if torch.cuda.is_available():
        assert rc == 0, lib.se_last_error()
        assert lib.se_plan_n_fft(out) == 2 * (geom[2] - 1)
        assert lib.se_plan_chunk_frames(out, 0) >= 1 and lib.se_plan_chunk_frames(out, 1) >= 1
        lib.se_plan_destroy(out)
    else:
        assert rc == -5 and b'no HIP device' in lib.se_last_error()          # SE_ERR_NO_DEVICE: fails loudly, no fallback


def test_fixed_plan_still_refuses_other_geometries():
    from speech_enhancement_by_s3prl_amd import _lib
    lib = _lib.load()
    out = ctypes.c_void_p()
    assert lib.se_plan_create(_lib.Geometry(16000, 400, 160, 257, 40), out) == -2 and b'unsupported geometry' in lib.se_last_error()
    assert lib.se_plan_create(_lib.Geometry(16000, 512, 128, 257, 40), out) == -2
    assert lib.se_plan_n_fft(None) == -1 and lib.se_plan_chunk_frames(None, 0) == -1


def test_preprocessor_geometry_is_a_setting():
    """construction, pickling and the plan choice need no device; the pseudo waveform of the zero-argument probe is long enough for reflect padding"""
    from speech_enhancement_by_s3prl_amd.preprocessor import OnlinePreprocessor
    p = OnlinePreprocessor(sample_rate=8000, win_ms=25, hop_ms=10, n_freq=101)
    assert p._win_args == {'n_fft': 200, 'hop_length': 80, 'win_length': 200}
    p = OnlinePreprocessor(sample_rate=1000, win_ms=64, hop_ms=16, n_freq=513)
    assert p._pseudo_wavs.shape[1] == 1024 > p._win_args['n_fft'] // 2
    assert OnlinePreprocessor()._pseudo_wavs.shape[1] == 16000
