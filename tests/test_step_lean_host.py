"""step_lean.h's helpers of the state-only step (the action decode by two unsigned range compares,
the fuel update as one FMA) against the forms they replaced, on the host:
tools/step_lean_check.cpp compiled for the host alone, without contraction as the library is, and
run. More than 10^7 (fuel, FUEL word, moved) cases with +-0, subnormals, +-inf, 1e308 and random
bit patterns, and every action in [-70, 330] and at the int32 ends for P in {0, 1, 5, 64, 254} under
every combination of nodest, inb and same. No GPU is involved."""
import os
import re
import subprocess

from conftest import ROOT


def test_lean_decode_and_fuel_equal_the_former_forms_on_the_host(tmp_path):
    from shippingenv_amd import build

    exe = str(tmp_path / "step_lean_check")
    src = os.path.join(ROOT, "tools", "step_lean_check.cpp")
    subprocess.run([build.hipcc(), "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, src],
                   check=True, capture_output=True, text=True, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.match(r"step_lean_check: (\d+) fuel cases .* (\d+) decode cases .* lean == former", p.stdout)
    assert m, p.stdout
    assert int(m.group(1)) >= 10 ** 7
    # 401 actions in [-70, 330] and 28 at the int32 ends, 5 worlds, 8 combinations of the three bits
    assert int(m.group(2)) >= (401 + 16) * 5 * 8
