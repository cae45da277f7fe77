"""k_pipe2d's tile records (PipeTileRec in xinvert_amd/csrc/xinv_tiles.h, built with the plan): compiled with g++ and
compared, field by field and lane by lane, with what the kernel's entry derived from the tile id before the records
existed, over a sweep of plans (CPU; tests/csrc/pipe_tile_record_check.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which('g++') is None, reason='no g++')
def test_tile_records_equal_the_entry_code_they_replace(tmp_path):
    exe = str(tmp_path / 'pipe_tile_record_check')
    subprocess.run(['g++', '-O1', '-std=c++17', '-I', os.path.join(ROOT, 'xinvert_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'csrc', 'pipe_tile_record_check.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith('OK'), r.stdout + r.stderr
