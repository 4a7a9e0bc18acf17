"""The screened GATE pool's helpers (step_lean.h: gate_thr_entry, screen_hot, screen_fold) on the
host: tools/step_screen_check.cpp compiled for the host alone and run. The fold of a 64-lane ballot
to one bit per window offset against the per-offset OR for W in {4, 8} (zero, all-ones, every single
bit, 10^5 random ballots each); the image's gate thresholds never fall over cargo 0 .. 50; and in
20000 windows of 1 .. 16 carrier lanes, with thresholds taken at the vote, cargo that only falls
and words at every edge, every step on which the exact gate test fires has its bit set. No GPU is
involved."""
import os
import re
import subprocess

from conftest import ROOT


def test_screen_helpers_on_the_host(tmp_path):
    from shippingenv_amd import build

    exe = str(tmp_path / "step_screen_check")
    src = os.path.join(ROOT, "tools", "step_screen_check.cpp")
    subprocess.run([build.hipcc(), "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, src],
                   check=True, capture_output=True, text=True, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.match(r"step_screen_check: (\d+) folds, 51 thresholds, (\d+) windows \((\d+) fires, (\d+) after a fall, (\d+) clear bits, "
                 r"(\d+) set bits\), fold == OR, every fire on a hot step", p.stdout)
    assert m, p.stdout
    assert int(m.group(1)) == 2 * (2 + 64 + 100000) and int(m.group(2)) == 20000
    assert int(m.group(3)) >= 10000 and int(m.group(4)) >= 1000 and int(m.group(5)) >= 1000 and int(m.group(6)) >= 1000
