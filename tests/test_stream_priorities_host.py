"""CPU: the arithmetic of the stream-priority policy (csrc/aej_sched.h, option "stream_priorities"), compiled alone from the header the
library compiles (tests/native/sched_check.cpp prints it as a table) and compared with the rule as include/aej.h states it:

  * priorities are in use when the option is 2 (always), or 1 (automatic) with fewer than 8 hardware queues; never when it is 0;
  * the effective queue count is queues x levels in use (2 levels, 3 for the round-robin pattern) then, the plain count otherwise;
  * only "always" can pass the 32 queues a process may hold, and is refused exactly when queues x levels > 32; the automatic mode
    tops out at 7 x 3 = 21;
  * the levels are dealt in creation order and evenly: any run of consecutive streams spreads over the levels of its pattern."""
import os
import shutil
import subprocess

from conftest import ROOT

NORMAL, HIGH, LOW = 0, 1, 2
PATTERNS = {0: (NORMAL, HIGH), 1: (NORMAL, LOW), 2: (NORMAL, HIGH, LOW), 3: (HIGH, LOW)}


def policy_table(tmp_path):
    exe = str(tmp_path / "sched_check")
    cxx = next((c for c in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), "g++")      # any host C++ compiler
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "sched_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0] == "limits 32 8 4", lines[0]
    rows = {}
    for line in lines[1:]:
        key, val = line.split(" -> ")
        in_use, levels, effective, refused, dealt = val.split()
        rows[tuple(int(v) for v in key.split())] = (int(in_use), int(levels), int(effective), int(refused), [int(c) for c in dealt])
    return rows


def test_effective_queues_cap_and_refusal(tmp_path):
    rows = policy_table(tmp_path)
    assert len(rows) == 3 * 4 * 40
    for (mode, pattern, q), (in_use, levels, effective, refused, dealt) in rows.items():
        what = f"stream_priorities={mode} pattern={pattern} queues={q}"
        want_levels = len(PATTERNS[pattern])
        want_in_use = mode == 2 or (mode == 1 and q < 8)
        assert levels == want_levels, what
        assert bool(in_use) == want_in_use, what
        assert effective == (q * want_levels if want_in_use else q), what
        assert bool(refused) == (mode == 2 and q * want_levels > 32), what
        if mode != 2:
            assert not refused and effective <= max(q, 21), what      # never, automatic: at most 7 x 3 queues, or the runtime's own count
        if not refused and want_in_use:
            assert effective <= 32, what
    # the cases the schedule turns on
    assert rows[(1, 0, 4)][2] == 8 and rows[(1, 2, 4)][2] == 12 and rows[(0, 0, 4)][2] == 4      # HIP's default of 4 queues
    assert rows[(1, 0, 7)][2] == 14 and rows[(1, 2, 7)][2] == 21 and rows[(1, 2, 8)][2] == 8     # the automatic mode ends at 8 queues
    assert rows[(1, 0, 16)][:3] == (0, 2, 16)                                                    # nothing changes with 16
    assert rows[(2, 0, 16)][2:4] == (32, 0) and rows[(2, 0, 17)][3] == 1                          # two levels: 16 queues are the most "always" takes
    assert rows[(2, 2, 10)][2:4] == (30, 0) and rows[(2, 2, 11)][3] == 1                          # three levels: 10


def test_levels_are_dealt_evenly_in_creation_order(tmp_path):
    rows = policy_table(tmp_path)
    for pattern, levels in PATTERNS.items():
        dealt = rows[(1, pattern, 4)][4]
        assert dealt == [levels[k % len(levels)] for k in range(12)], pattern
        # parts that run together are created together: any window of consecutive streams differs by at most one per level
        for n in (2, 3, 4, 8):
            for start in range(12 - n + 1):
                window = dealt[start:start + n]
                counts = [window.count(level) for level in levels]
                assert max(counts) - min(counts) <= 1, (pattern, n, start)
