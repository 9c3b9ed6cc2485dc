"""not-gpu: csrc/attach_checks.hpp, the argument checks every recorder's _begin and _read share, message by message
(tests/attach_checks_check.cpp).  The header includes nothing of HIP and nothing of the handle, so the host compiler builds the
check alone — a stand-alone program with the address and undefined-behaviour sanitizers linked in.  Whether the host compiler has
their runtimes is found out with a one-line program; only where that cannot be built and run is the check built without them,
and the program's own last line says which build ran."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']


def _has_sanitizers(cxx, tmp_path):
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    exe = str(tmp_path / 'probe')
    if subprocess.run([cxx, str(probe), '-o', exe] + SANITIZE, capture_output=True).returncode != 0:
        return False
    return subprocess.run([exe], capture_output=True).returncode == 0


def test_every_check_says_what_the_entry_points_have_always_said(tmp_path):
    cxx = os.environ.get('CXX') or shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    sanitized = _has_sanitizers(cxx, tmp_path)
    src, exe = os.path.join(ROOT, 'tests', 'attach_checks_check.cpp'), str(tmp_path / 'attach_checks_check')
    # (a diagnostic of the check's own source fails the test whichever build it is: nothing falls back from here on)
    build = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', src, '-o', exe] + (SANITIZE if sanitized else []),
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout.strip())
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'attach_checks_check: ok' in r.stdout
    assert ('address sanitizer on' if sanitized else 'no sanitizer') in r.stdout, r.stdout
