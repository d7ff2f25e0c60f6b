"""mgdt_yolo_amd/csrc/launch_host.h - the view binder in front of every 32-bit-descriptor launch and the experiment-knob readers - checked on the
CPU: tests/host/launch_host_check.cpp is a stand-alone program (its own main) built with the host compiler, under AddressSanitizer and
UndefinedBehaviorSanitizer where an empty program links with them, and run as a child process.  Nothing of it is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']


def _host_compiler():
    for cxx in (os.environ.get('CXX'), 'c++', 'g++', 'clang++', '/opt/rocm/llvm/bin/clang++'):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_launch_host_header(tmp_path):
    cxx = _host_compiler()
    assert cxx, 'no host C++ compiler found (CXX, c++, g++, clang++)'
    empty = tmp_path / 'empty.cpp'
    empty.write_text('int main() { return 0; }\n')
    trial = subprocess.run([cxx, *SAN, str(empty), '-o', str(tmp_path / 'empty')], capture_output=True, text=True)
    # linked and starts in this environment: only then are the flags used
    san = SAN if trial.returncode == 0 and subprocess.run([str(tmp_path / 'empty')]).returncode == 0 else []
    print(f'{cxx}: sanitizers {"on" if san else "not available, built without them"}')
    exe = tmp_path / 'launch_host_check'
    build = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-Wno-comment', *san, os.path.join(ROOT, 'tests', 'host', 'launch_host_check.cpp'),
                            '-o', str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    env = {k: v for k, v in os.environ.items() if not k.startswith('MGDT_')}      # the program sets and unsets its own knob
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and 'launch_host_check: ok' in run.stdout, run.stdout + run.stderr
