"""The shared host/device header of the prior's upper-trapezoid pull (host/ingest_sym_map.hpp: the arithmetic k_ingest_sym and the
copying calls' staging run) as a stand-alone program under the sanitizers: tests/cpp/test_ingest_sym_map.cpp replays one pull lane by
lane for every n = 1 .. 260.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_image_entry_once_from_the_upper_tiles_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / 'test_ingest_sym_map')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-o', exe, os.path.join(ROOT, 'tests', 'cpp', 'test_ingest_sym_map.cpp')])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'ingest sym map ok' in out.stdout
