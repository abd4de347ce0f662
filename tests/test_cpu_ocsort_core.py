"""CPU: the shared OC-SORT core (csrc/ocsort_core.h) under sanitizers, without HIP.

The header is the one text the host tracker (ocsort_tracker.cpp) and the device tracker (batched_assoc.hip) both compile.
tests/native/ocsort_core_check.cpp drives its routines on BOTH track types - DTrack, the fixed-window record the kernels
keep in device memory, and Track, the host tracker's - with one stream of boxes and requires all state equal on the bytes
after every step.  Built here with AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program and run as a
child process: an index past the device record's window, which no GPU test would report, ends it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ['-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']


def _compiler():
    for cxx in ('g++', 'clang++', '/opt/rocm/llvm/bin/clang++'):
        path = shutil.which(cxx)
        if path:
            return path
    return None


def test_core_check_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip('no host C++ compiler (g++, clang++, /opt/rocm/llvm/bin/clang++)')
    exe = str(tmp_path / 'ocsort_core_check')
    # g++ links the sanitizer runtimes as shared libraries unless told otherwise, and a shared AddressSanitizer runtime
    # refuses to start behind any preloaded library; linked in (clang++'s default), the program starts anywhere
    static = ['-static-libasan', '-static-libubsan'] if os.path.basename(cxx).startswith('g++') else []
    src = os.path.join(ROOT, 'tests', 'native', 'ocsort_core_check.cpp')
    build = subprocess.run([cxx] + FLAGS + static + ['-I', os.path.join(ROOT, 'stereotracking_amd', 'csrc'), src, '-o', exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, f'{cxx} failed:\n{build.stderr}'
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, f'exit status {run.returncode}:\n{run.stderr}'
    assert run.stderr == ''
