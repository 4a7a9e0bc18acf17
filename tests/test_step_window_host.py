"""The GATE pool's windows sized to the carriers and the arrival test by the cell code (step_lean.h:
gate_window_entry, gate_lane_offset, gate_lane_carrier, gate_pool_index, gate_screen_mask,
gate_screen_step, ports_on_distinct_cells, arrive_by_code) on the host: tools/step_window_check.cpp
compiled for the host alone and run. For every m in 1 .. 16: W = min(16, 64 / m) is 4 .. 16 with
m W <= 64, the lane mapping is a bijection from the lanes below m W onto (carrier, offset), and
every entry any lane can read lies inside the wave's rows; the screen's walk (the ballot shifted by
m per step, its low m bits tested) equals the per-offset OR for zero, all-ones, every single bit and
10^5 random ballots per m; in 32000 windows with thresholds taken at the vote, cargo that only falls
and takes of fuel and refused takes in mid-window every step on which the exact gate test fires has
its bit set; and on maps of 1 x 1, 1 x 7, 5 x 9 and 100 x 100 cells with 1, 5 and 253 ports on
distinct cells the arrival test by the code equals the position compare for a ship on every cell,
every dest < P and do_move both ways, with the host's distinct-cells flag false as soon as two ports
share a cell. No GPU is involved."""
import os
import re
import subprocess

from conftest import ROOT


def test_window_helpers_on_the_host(tmp_path):
    from shippingenv_amd import build

    exe = str(tmp_path / "step_window_check")
    src = os.path.join(ROOT, "tools", "step_window_check.cpp")
    subprocess.run([build.hipcc(), "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, src],
                   check=True, capture_output=True, text=True, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.match(r"step_window_check: (\d+) lanes, (\d+) reads, (\d+) walks, (\d+) windows \((\d+) fires, (\d+) after a fall, "
                 r"(\d+) after a kept take, (\d+) clear bits, (\d+) set bits\), (\d+) worlds \((\d+) arrival tests, (\d+) arrivals\): "
                 r"mapping a bijection, reads in rows, walk == OR, every fire on a hot step, by code == by position", p.stdout)
    assert m, p.stdout
    lanes, reads, walks, windows, fires, after_fall, after_take, clear_bits, set_bits, worlds, tests, arrivals = map(int, m.groups())
    W = [min(16, 64 // k) for k in range(1, 17)]
    assert lanes == 16 * 64 and reads == sum((k + 1) * w for k, w in zip(range(1, 17), W))
    assert walks == 16 * (2 + 64 + 100000) and windows == 32000
    assert min(fires, after_fall, after_take, clear_bits, set_bits) > 0
    cells = {(1, 1): (1,), (1, 7): (1, 5), (5, 9): (1, 5), (100, 100): (1, 5, 253)}
    assert worlds == 8 and tests == sum(2 * h * w * P for (h, w), Ps in cells.items() for P in Ps)
    assert arrivals == sum(P for Ps in cells.values() for P in Ps)  # one cell per dest, do_move set
