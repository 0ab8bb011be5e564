"""The windowed tile predicate (lm_tb_window + lm_tb_tile_skip_win in
locomouse_cpp_amd/csrc/lm_tail_bound.h: what k_tile_bound evaluates, the
vertical part of the reduction taken once per window row) against
lm_tb_tile_skip (what k_tile_bound_ref evaluates), on the host without a GPU:
a stand-alone program (tests/cpp/tile_window_check.cpp) compares the two on
seeded random range tables -- oh % 4 in {0, 1, 2, 3}, oh < 4, kh in {1, 2, 16,
30}, one and several tile columns, whole detectors and bands of tile rows,
biases that put U on both sides of 0 and exactly on it; once more under the
sanitizers.  Nothing is loaded into Python."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "tile_window_check.cpp")
INC = "-I" + os.path.join(ROOT, "locomouse_cpp_amd", "csrc")
ROW = re.compile(r"cases (\d+) tiles (\d+) skipped (\d+) mismatch (\d+)")


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    cases, tiles, skipped, mismatch = map(int, ROW.search(r.stdout).groups())
    assert mismatch == 0, r.stdout
    # 14 heights x 4 kernel heights x 3 widths x 3 tables x 4 biases; both outcomes well represented
    assert cases == 14 * 4 * 3 * 3 * 4, r.stdout
    assert 0.2 * tiles < skipped < 0.8 * tiles, r.stdout


def test_windowed_predicate_equals_the_reference_predicate(tmp_path):
    exe = str(tmp_path / "tile_window_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", INC, SRC, "-o", exe])
    _run(exe)


def test_windowed_predicate_is_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "tile_window_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", INC, SRC, "-o", exe])
    _run(exe)
