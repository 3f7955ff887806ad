"""The host's staging of the object update (scan, integer-arena layout, per-track pack, rows grouped by clone, arrow lists:
orcvio_amd/csrc/host/object_stage.hpp) as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer, on the CPU
(tests/cpp/test_object_stage.cpp), against a second builder written from the layout's description."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_staging_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / 'test_object_stage')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-o', exe, os.path.join(ROOT, 'tests', 'cpp', 'test_object_stage.cpp')])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'object stage ok' in out.stdout
