"""The host's plan of a submitted batch (locomouse_cpp_amd/csrc/
lm_batch_plan.h: how a batch continues the video, its slot table with the two
bounds rules, the corners the next batch inherits, the source-map decision) on
the host, without a GPU: a stand-alone program (tests/cpp/
batch_plan_check.cpp) drives the header through seeded scripts of submissions
the way submit_batch does and compares every batch with the reference's
per-frame loop: one set of corners per video frame, the ones passed when the
frame was first submitted, and cropBoundingBox's formula on them.  Planted
errors in a copy of the header must each be caught.  Once more under the
sanitizers; nothing is loaded into Python."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "batch_plan_check.cpp")
CSRC = os.path.join(ROOT, "locomouse_cpp_amd", "csrc")
HEADER = os.path.join(CSRC, "lm_batch_plan.h")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
LINE = re.compile(
    r"(?P<scripts>\d+) scripts, (?P<batches>\d+) batches, (?P<slots>\d+) slots, modes first (?P<first>\d+) given (?P<given>\d+) "
    r"carry (?P<carry>\d+) handoff (?P<handoff>\d+), refused roi_bottom (?P<roi_bottom>\d+) roi_side (?P<roi_side>\d+) "
    r"lut (?P<lut>\d+) gap (?P<gap>\d+) failed (?P<failed>\d+), views uniform (?P<uniform>\d+) nonuniform (?P<nonuniform>\d+), "
    r"carried slot0 (?P<carried0>\d+), (?P<checks>\d+) checks, (?P<failures>\d+) failures")

# (name, the header's text, its replacement): each must make the checker fail
PLANTED = (
    ("bb indexed by s - 1 also with a given halo", "cr = bb + 3 * (M.given_halo ? s : s - 1);", "cr = bb + 3 * (s - 1);"),
    ("the new last_bb from slot 0", "if (s == n) std::memcpy(new_last_bb,", "if (s == 0) std::memcpy(new_last_bb,"),
    ("s_proc0 ignores a hand-off", "M.s_proc0 = M.halo ? 0 : 1;", "M.s_proc0 = M.given_halo ? 0 : 1;"),
    ("the side view's row from the bottom view's corner", "(unsigned)(g.pad_pre_rows + cr[2])", "(unsigned)(g.pad_pre_rows + cr[1])"),
    ("the + 1 dropped from the side crop's column", "(unsigned)(g.bb_side_mouse_pad.width - g.spost_t_w) + 1u", "(unsigned)(g.bb_side_mouse_pad.width - g.spost_t_w)"),
    ("the ROI rule from s_lut0", "if (s >= M.s_proc0) lm_bp_check_roi(g, S);", "if (s >= M.s_lut0) lm_bp_check_roi(g, S);"),
    ("carry without the lane's state", "lane == ctx_last_lane && lane_have_state &&", "lane == ctx_last_lane && (lane_have_state || true) &&"),)


def _build(exe, flags, inc=()):
    # (the header must also be clean under the warnings the host library is built with)
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-Wextra", "-Werror", *("-I" + i for i in inc), "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe])
    return exe


def _run(exe, fails=False):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert (r.returncode == 1) if fails else (r.returncode == 0), r.stdout[-3000:] + r.stderr[-3000:]
    m = LINE.search(r.stdout)
    assert m, r.stdout[-2000:]
    return {k: int(v) for k, v in m.groupdict().items()}


def _clean(exe):
    n = _run(exe)
    assert n["failures"] == 0
    # every mode, every refusal, both answers of the source-map decision were reached
    for k, v in n.items():
        assert v > 0 or k == "failures", (k, n)
    assert n["slots"] > n["batches"] > n["scripts"] and n["checks"] > 10 * n["slots"]


def test_batch_plan_is_the_per_frame_loop(tmp_path):
    _clean(_build(str(tmp_path / "batch_plan_check"), ["-O2"]))


def test_batch_plan_is_clean_under_the_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined; nothing is
    loaded into Python."""
    _clean(_build(str(tmp_path / "batch_plan_check_san"), SAN))


@pytest.mark.parametrize("name,old,new", PLANTED, ids=[p[0].replace(" ", "_") for p in PLANTED])
def test_planted_errors_are_caught(name, old, new, tmp_path):
    with open(HEADER) as fh:
        text = fh.read()
    assert text.count(old) == 1, (name, old)
    with open(tmp_path / "lm_batch_plan.h", "w") as fh:
        fh.write(text.replace(old, new))
    n = _run(_build(str(tmp_path / "batch_plan_check_planted"), ["-O2"], inc=(str(tmp_path),)), fails=True)
    assert n["failures"] > 0, (name, n)
