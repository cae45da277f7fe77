"""Buffer rotation of the sweep loops (xinvert_amd/csrc/xinv_rotation.h): which buffer each launch writes, where a member's
final state lives and how a pass the stop rule fired in is redone -- compiled with g++ and checked exhaustively against a
simulation of labelled buffers (CPU)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which('g++') is None, reason='no g++')
def test_rotation_redo_and_final_buffer(tmp_path):
    exe = str(tmp_path / 'rotation_check')
    subprocess.run(['g++', '-O1', '-std=c++17', '-I', os.path.join(ROOT, 'xinvert_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'csrc', 'rotation_check.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith('OK'), r.stdout + r.stderr
