"""Host half of orcvio_msckf_io_triangulate_prune (the layout of the second pinned block, validation and staging of the prune features'
observation list, the frame call's coverage check: orcvio_amd/csrc/triangulate_arm.hpp) as a stand-alone program under AddressSanitizer
and UndefinedBehaviorSanitizer, on the CPU (tests/cpp/test_prune_tri_arm.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_validation_and_staging_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / 'test_prune_tri_arm')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-o', exe, os.path.join(ROOT, 'tests', 'cpp', 'test_prune_tri_arm.cpp')])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'prune tri arm ok' in out.stdout
