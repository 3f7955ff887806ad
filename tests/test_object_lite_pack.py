"""Host half of the lite object mapper (validation, packing, unpacking: orcvio_amd/csrc/object_mapper_pack.hpp) as a stand-alone
program under AddressSanitizer and UndefinedBehaviorSanitizer, on the CPU (tests/cpp/test_object_lite_pack.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pack_and_validation_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / 'test_object_lite_pack')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-o', exe, os.path.join(ROOT, 'tests', 'cpp', 'test_object_lite_pack.cpp')])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'object lite pack ok' in out.stdout
