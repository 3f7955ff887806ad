"""The bookkeeping of the resident covariance and of its square-root factor (orcvio_amd/csrc/host/cov_book.hpp: which buffers change
roles, the new dimension, whether the factor follows -- one rule per edit) as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer, on the CPU (tests/cpp/test_cov_book.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_edit_of_the_resident_covariance_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / 'test_cov_book')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-o', exe, os.path.join(ROOT, 'tests', 'cpp', 'test_cov_book.cpp')])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'cov book ok' in out.stdout
