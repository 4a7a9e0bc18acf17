"""The C-ABI library loads, exports every symbol include/shipenv.h declares, and
reports API misuse as a status (no compute: runs without a GPU)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT


def header_symbols():
    text = open(os.path.join(ROOT, "include", "shipenv.h")).read()
    return sorted(set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(se_\w+)\s*\(", text, re.M)))


@pytest.fixture(scope="module")
def lib():
    from shippingenv_amd import _native, build

    build.build(verbose=False)
    return _native.lib()


def test_exports_every_declared_symbol(lib):
    from shippingenv_amd import _native

    syms = header_symbols()
    assert len(syms) >= 19
    assert sorted(_native.EXPORTS) == syms
    for s in syms:
        assert hasattr(lib, s), s


def test_abi_version(lib):
    import re
    from shippingenv_amd import _native
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "shipenv.h")).read()
    want = int(re.search(r"#define SHIPENV_ABI_VERSION (\d+)", hdr).group(1))
    assert lib.se_abi_version() == want == _native.ABI_VERSION == 2


def test_library_is_gfx950():
    from shippingenv_amd import _native

    blob = open(_native.LIB_PATH, "rb").read()
    assert b"gfx950" in blob


def test_misuse_is_a_status_not_a_crash(lib):
    from shippingenv_amd import _native

    h = C.c_void_p()
    water = (C.c_uint8 * 4)(1, 1, 1, 1)
    # bad map side -> SE_EINVAL before touching the device
    rc = lib.se_create(C.byref(h), 0, 16, 0, 0, 2, water, 0, None, None, None, None, 0, 0)
    assert rc == -1 and b"map sides" in lib.se_last_error()
    assert lib.se_step(None, None, None) == -1
    assert lib.se_destroy(None) == 0
    with pytest.raises(_native.ShipEnvError):
        _native.check(lib.se_bind(None, None))


def test_every_source_is_a_build_dependency(monkeypatch, tmp_path):
    """build.DEPS holds every source under csrc/ (shipenv.hip's fragments included), and a
    header newer than the library makes it stale. The timestamps are a temporary copy's."""
    from shippingenv_amd import build

    csrc = os.path.join(ROOT, "shippingenv_amd", "csrc")
    sources = [os.path.join(d, f) for d, _, files in os.walk(csrc) for f in files
               if f.endswith((".hip", ".cpp", ".h"))]
    assert len(sources) >= 17  # shipenv.hip, mapload.cpp, philox.h, 9 + 5 fragments
    deps = {os.path.realpath(d) for d in build.DEPS}
    for s in sources:
        assert os.path.realpath(s) in deps, s
    assert os.path.realpath(os.path.join(ROOT, "include", "shipenv.h")) in deps

    copies = []
    for k, d in enumerate(build.DEPS):
        c = tmp_path / ("%02d_%s" % (k, os.path.basename(d)))
        c.write_text("")
        os.utime(c, (1000, 1000))
        copies.append(str(c))
    out = tmp_path / "libshipenv_hip.so"
    out.write_text("")
    os.utime(out, (2000, 2000))
    (tmp_path / "libshipenv_hip.so.cmd").write_text(" ".join(build._flags()))
    monkeypatch.setattr(build, "DEPS", copies)
    monkeypatch.setattr(build, "OUT", str(out))
    monkeypatch.setattr(build, "STAMP", str(out) + ".cmd")
    assert build.up_to_date()
    for c in copies:  # each one alone, the fragments as much as shipenv.hip
        os.utime(c, (3000, 3000))
        assert not build.up_to_date(), c
        os.utime(c, (1000, 1000))
    assert build.up_to_date()


def test_product_path_has_no_fallback(monkeypatch, tmp_path):
    """A missing library raises instead of silently stepping on the CPU."""
    from shippingenv_amd import _native

    monkeypatch.setattr(_native, "LIB_PATH", str(tmp_path / "missing.so"))
    monkeypatch.setattr(_native, "_LIB", None)
    with pytest.raises(_native.NativeLibraryError):
        _native.lib()


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "shippingenv_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in re.sub(r"#.*|//.*", "", text).replace("oracles", ""), f
