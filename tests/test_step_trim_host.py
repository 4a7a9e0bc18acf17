"""What the state-only step reads in place of its former forms (step_lean.h's fuel scale as one FMA
and one add, the move test as one compare of act - 4 against a bound, the GATE pool's window choice;
philox.h's draws under a key schedule computed once) against those forms, on the host:
tools/step_trim_check.cpp compiled for the host alone, without contraction as the library is, and
run. The fuel scale for all 2^32 words on at most 16 threads, every action in [-70, 330] and at the
int32 ends for P in {0, 1, 5, 64, 254} under every nodest / inb, the scheduled draws of FUEL, GATE,
LOSS_0 .. LOSS_3 and ARRIVE against draw() with e1 != 0 and counters on both sides of 2^32, and
m W <= 64 for every m in 1 .. 16. No GPU is involved."""
import os
import re
import subprocess

from conftest import ROOT


def test_trimmed_forms_equal_the_former_forms_on_the_host(tmp_path):
    from shippingenv_amd import build

    exe = str(tmp_path / "step_trim_check")
    src = os.path.join(ROOT, "tools", "step_trim_check.cpp")
    subprocess.run([build.hipcc(), "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-o", exe, src],
                   check=True, capture_output=True, text=True, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.match(r"step_trim_check: (\d+) fuel words on (\d+) threads, (\d+) move cases \((\d+) moves\), (\d+) draws "
                 r"\((\d+) tuples with e1 != 0, (\d+) with t \+ offset past 2\^32\), 16 windows, new == former", p.stdout)
    assert m, p.stdout
    assert int(m.group(1)) == 2 ** 32 and 1 <= int(m.group(2)) <= 16
    # 401 actions in [-70, 330] and 16 at the int32 ends, 5 worlds, 4 combinations of the two bits
    assert int(m.group(3)) >= (401 + 16) * 5 * 4 and int(m.group(4)) >= 32  # 8 moves pass in each of the 4 worlds with ports
    # 7 slots per tuple
    assert int(m.group(5)) >= 7 * 20000 and int(m.group(6)) >= 1000 and int(m.group(7)) >= 100
