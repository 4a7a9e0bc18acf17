"""The carried cell address of the regular state-only step (step_lean.h: ring_delta,
ring_byte_deltas, ring_unindex_mul, ring_unindex) against the packed position, on the host:
tools/step_addr_check.cpp compiled for the host alone and run. For every map width 1 .. 256: the
multiply-and-shift division against / and % for every index a bordered table of that width can hold
(258 rows), the per-direction delta against the packed add for every cell of 256 rows and every
move, the way back to x, y from every target (the border ring included), and the choice of byte
deltas up to W = 125 and no further. No GPU is involved."""
import os
import re
import subprocess

from conftest import ROOT


def test_cell_address_equals_the_packed_position_on_the_host(tmp_path):
    from shippingenv_amd import build

    exe = str(tmp_path / "step_addr_check")
    src = os.path.join(ROOT, "tools", "step_addr_check.cpp")
    subprocess.run([build.hipcc(), "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, src],
                   check=True, capture_output=True, text=True, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.match(r"step_addr_check: (\d+) divisions, (\d+) move targets, (\d+) widths with byte deltas, address == packed position", p.stdout)
    assert m, p.stdout
    widths = range(1, 257)
    assert int(m.group(1)) == sum(258 * (W + 2) for W in widths)
    assert int(m.group(2)) == sum(4 * 256 * W for W in widths) and int(m.group(3)) == 125
