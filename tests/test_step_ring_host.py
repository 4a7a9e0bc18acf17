"""The regular state-only step's decode on the bordered cell table (step_lean.h: the table, the
biased position, ring_do_move / ring_moved) against the general form's bounds test, cell select,
ground test and lean_do_move_val, on the host: tools/step_ring_check.cpp compiled for the host
alone and run. Maps of 1 x 1, 1 x 7, 7 x 1, 5 x 9 and 100 x 100 with P in {0, 1, 5, 253}, a ship on
every cell, every action in [-70, 330] and at the int32 ends, every class of cell code (water,
ground, a port's, one past P) under the ship and at the target; the table's bytes against the
image, the bias round trip for every x, y < 256, and the launch's choice to carry no table for
P = 254 and for a world without LDS room. No GPU is involved."""
import os
import re
import subprocess

from conftest import ROOT


def test_regular_decode_equals_the_general_form_on_the_host(tmp_path):
    from shippingenv_amd import build

    exe = str(tmp_path / "step_ring_check")
    src = os.path.join(ROOT, "tools", "step_ring_check.cpp")
    subprocess.run([build.hipcc(), "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, src],
                   check=True, capture_output=True, text=True, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.match(r"step_ring_check: (\d+) decode cases \((\d+) moves off the map, (\d+) blocked by ground, (\d+) moves\), (\d+) tables, "
                 r"(\d+) bias round trips, 9 launch choices, regular == general", p.stdout)
    assert m, p.stdout
    cells = 1 * 1 + 1 * 7 + 7 * 1 + 5 * 9 + 100 * 100
    # 401 actions in [-70, 330] and 16 at the int32 ends, 4 worlds, 4 phases of the codes
    assert int(m.group(1)) == cells * (401 + 16) * 4 * 4
    assert int(m.group(2)) >= 1000 and int(m.group(3)) >= 1000 and int(m.group(4)) >= 1000
    assert int(m.group(5)) == 5 * 4 * 4 and int(m.group(6)) == 256 * 256
