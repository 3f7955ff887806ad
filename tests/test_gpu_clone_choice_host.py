"""The C++ host layer's checked choice of the clones that leave (orcvio_amd/csrc/host/orcvio_msckf_host.hpp:
MsckfBackend::findRedundantImuStates and the frame call site ::stepFrameChosen), run from tests/cpp/test_host_clone_choice.cpp on
std::map containers: an agreeing and a disagreeing prune frame, each compared with the same frame through the separate calls in the
reference's order (the choice made on the host after the first update)."""
import subprocess

import pytest

from test_host_shim import _build

pytestmark = pytest.mark.gpu


def test_host_call_site_against_the_separate_calls(built, tmp_path):
    exe = str(tmp_path / 'test_host_clone_choice')
    _build('test_host_clone_choice.cpp', exe)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'host clone choice ok' in run.stdout
    assert 'agree:' in run.stdout and 'path 1' in run.stdout and 'differ:' in run.stdout and 'path 2' in run.stdout
