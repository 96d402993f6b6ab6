"""The two racing passes of the frame linking on 16 host threads under ThreadSanitizer: profiles/micro/link_threads.cpp, a stand-alone
C++ program (its own main; no GPU, no Python in the process) that includes csrc/link_math.hpp with the atomics spelled as relaxed
std::atomic_ref operations, built with g++ -fsanitize=thread and run as a child process.  It exits non-zero when a threaded result
differs from that of one thread or when ThreadSanitizer reports a race.  Skipped where g++ cannot build and run a ThreadSanitizer
program at all."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, 'profiles', 'micro', 'link_threads.cpp')
FLAGS = ['-std=c++20', '-O1', '-g', '-fsanitize=thread', '-pthread']
PROBE = 'int main() { return 0; }\n'


def test_threaded_insert_and_best_under_thread_sanitizer(tmp_path):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('no g++')
    probe = tmp_path / 'probe.cpp'
    probe.write_text(PROBE)
    built = subprocess.run([gxx] + FLAGS + [str(probe), '-o', str(tmp_path / 'probe')], capture_output=True, text=True)
    if built.returncode != 0 or subprocess.run([str(tmp_path / 'probe')], capture_output=True).returncode != 0:
        pytest.skip('g++ cannot build and run a ThreadSanitizer program here: %s' % built.stderr[-300:])
    exe = tmp_path / 'link_threads'
    subprocess.run([gxx] + FLAGS + ['-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'occlusions-4d_amd', 'csrc'), SOURCE,
                    '-o', str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert 'ThreadSanitizer' not in run.stderr and run.stdout.count(', 0 mismatches') == 4
    assert 'overflow 1' in run.stdout and run.stdout.count('overflow 0') == 3
    assert run.stdout.rstrip().endswith('ok: every threaded overlap and match equals that of one thread')
