"""The layout part of csrc/hoststage.h (up256, StageLayout, plane_count, plane_bytes): the scratch blocks of the sixteen sites that stage host arrays, laid out by
a stand-alone program under the sanitizers, and with them the mask part of csrc/stageobj.h (popcount64, mask_check).  No GPU, nothing loaded into Python."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which('g++') is None and shutil.which('clang++') is None, reason='no host C++ compiler')
def test_stage_layouts_under_the_sanitizers(tmp_path):
    """tools/stage_layout_asan.cpp: every site's part list at zero counts, absent optional parts, one row, parts around 256 bytes, pitched NV12 / RGB planes and every
    orient residue, on heap blocks of exact size under -fsanitize=address,undefined; then mask_check and popcount64 on masks 0, bit n_streams - 1, bit n_streams and
    all 64 bits at n_streams 1 and 64 (seven calls).  A stand-alone program that includes only the plain parts of the two headers"""
    cxx = shutil.which('g++') or shutil.which('clang++')
    exe = str(tmp_path / 'stage_layout_asan')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', os.path.join(ROOT, 'tools', 'stage_layout_asan.cpp'), '-o', exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and 'stage layout ok' in r.stdout and '7 masks)' in r.stdout, r.stdout + r.stderr
