"""Every entry point that include/nxg_codec.h declares, and every debug entry the test suite looks
up, resolves in the built libnxg_codec.so. No GPU.

The host half of the library is several translation units, and a shared library links without
complaint when a definition is missing: a source file left out of the Makefile's SRCS would drop
its entry points silently until some GPU test happened to call one.
"""
import glob
import os
import re

import netidx_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def declared_functions():
    """The nxg_* functions declared in the public header (comments stripped first)."""
    src = _read("include", "nxg_codec.h")
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    return sorted(set(re.findall(r"\b(nxg_\w+)\s*\(", src)))


def debug_entries_used():
    """The debug entries (not ABI) that the tests and the Python binding look up by name."""
    files = glob.glob(os.path.join(ROOT, "tests", "*.py"))
    files.append(os.path.join(ROOT, "netidx_amd", "codec.py"))
    names = set()
    for path in files:
        with open(path) as f:
            names.update(re.findall(r"nxg_debug_\w+", f.read()))
    return sorted(names)


def _missing(names):
    lib = netidx_amd.lib()
    return [n for n in names if not hasattr(lib, n)]


def test_every_declared_function_is_defined():
    names = declared_functions()
    assert len(names) > 80, "the header parse found too few declarations"
    assert "nxg_ctx_new" in names and "nxg_frame_reader_buffered" in names
    assert _missing(names) == []


def test_every_debug_entry_the_suite_uses_is_defined():
    names = debug_entries_used()
    assert "nxg_debug_f64s_plan" in names and "nxg_debug_devbuf_grow" in names
    assert _missing(names) == []
