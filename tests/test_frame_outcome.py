"""The outcome table of the one-call filter frame (orcvio_amd/csrc/host/frame_outcome.hpp: status_first, status_prune, which stats[3]
are cleared, whether the second update's outcome is evaluated, the return value -- one table for the one-pass and the repair path) as
a stand-alone program on the CPU (tests/cpp/test_frame_outcome.cpp), built plainly and under AddressSanitizer and
UndefinedBehaviorSanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('flags', [['-O2'], ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']], ids=['plain', 'sanitizers'])
def test_every_combination_against_the_two_paths_it_replaced(tmp_path, flags):
    exe = str(tmp_path / 'test_frame_outcome')
    subprocess.check_call(['g++', '-std=c++17', '-Wall'] + flags + ['-o', exe, os.path.join(ROOT, 'tests', 'cpp', 'test_frame_outcome.cpp')])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'frame outcome ok' in out.stdout
