"""FACE records without a GPU: tests/host_emu/face_check.cpp (the per-cell code of mc33_cell.h built with g++) checks the record
k_cells makes for a cell on the grid's 0-faces against the generic plan of the same cell, for every sign index x the 7 face-flag
combinations (and the interior), and the clamped owner of every foreign edge against owner_of."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_face_records_match_the_generic_plan(tmp_path):
    exe = str(tmp_path / "face_check")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", os.path.join(ROOT, "tests", "host_emu", "face_check.cpp"), "-o", exe])
    out = subprocess.run([exe, "20"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok ") and int(out.stdout.split()[1]) == 8 * 254 * 20
