"""The plan and the outcome table of the five zero-velocity calls (orcvio_amd/csrc/host/zupt_frame_outcome.hpp) as a stand-alone
program under AddressSanitizer and UndefinedBehaviorSanitizer, on the CPU (tests/cpp/test_zupt_frame_outcome.cpp): every combination of
form, stage codes, status word, verdict, arming and remove_previous against a transcription of the bodies the table replaced -- return
code, *applied / *n_after, message, marginalisation and every field of the resident covariance's book."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_table_reproduces_the_five_exit_sequences_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / 'test_zupt_frame_outcome')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-o', exe, os.path.join(ROOT, 'tests', 'cpp', 'test_zupt_frame_outcome.cpp')])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'zupt frame outcome ok' in out.stdout
    m = re.search(r'compared (\d+) combinations \(each with three factors\), skipped (\d+), 0 differ', out.stdout)
    assert m, out.stdout
    compared, skipped = int(m.group(1)), int(m.group(2))
    assert compared > 0 and skipped < compared, out.stdout
