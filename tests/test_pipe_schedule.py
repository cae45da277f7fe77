"""The schedule of the wave-pipelined pass (xinv_pipe_* in xinvert_amd/csrc/xinv_tiles.h, shared by k_pipe2d and the
planner): compiled with g++ and simulated step by step for every tile height 1..300 and both barrier spacings -- ring
hand-over, barrier counts, the step bound and the planner's step count (CPU; tests/csrc/pipe_schedule_check.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which('g++') is None, reason='no g++')
def test_pipelined_schedule_hand_over_barriers_and_step_count(tmp_path):
    exe = str(tmp_path / 'pipe_schedule_check')
    subprocess.run(['g++', '-O1', '-std=c++17', '-I', os.path.join(ROOT, 'xinvert_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'csrc', 'pipe_schedule_check.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith('OK'), r.stdout + r.stderr
