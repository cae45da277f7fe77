"""The planner's switch between the two forcing paths of k_pipe2d (xinv_pipe_forcing_ring in xinvert_amd/csrc/xinv_tiles.h):
the launches on which the two paths were timed fall on the side that won (CPU; tests/csrc/pipe_forcing_ring_check.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which('g++') is None, reason='no g++')
def test_forcing_ring_switch_puts_the_timed_launches_on_the_side_that_won(tmp_path):
    exe = str(tmp_path / 'pipe_forcing_ring_check')
    subprocess.run(['g++', '-O1', '-std=c++17', '-I', os.path.join(ROOT, 'xinvert_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'csrc', 'pipe_forcing_ring_check.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith('OK'), r.stdout + r.stderr
