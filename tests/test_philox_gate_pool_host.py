"""philox.h's single-block draws for the state-only step's GATE pool (draw_gate_pooled from the
four words a carrier lane hands over, draw_fuel from the lane's own invariants) against philox10,
on the host: tools/philox_gate_pool_check.cpp compiled for the host alone and run. Several
thousand (key, quad id, window start, offset) tuples: quad ids with e1 != 0 and either side of an
e1 step, and window starts whose start + offset wraps 2^32. No GPU is involved."""
import os
import subprocess

from conftest import ROOT


def test_pooled_gate_draw_equals_philox10_on_the_host(tmp_path):
    from shippingenv_amd import build

    exe = str(tmp_path / "philox_gate_pool_check")
    src = os.path.join(ROOT, "tools", "philox_gate_pool_check.cpp")
    subprocess.run([build.hipcc(), "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-o", exe, src],
                   check=True, capture_output=True, text=True, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "pooled == philox10" in p.stdout and int(p.stdout.split()[1]) >= 9000, p.stdout
