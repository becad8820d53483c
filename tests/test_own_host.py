"""The owners of the handle's GPU resources (contrack_amd/csrc/ctk_own.h) without a GPU: the live counters of a fresh process, and the
move / swap / release / scope-exit rules of the types in a stand-alone program (tests/own_host.cpp) against a stub of the HIP calls,
built with the address and undefined-behaviour sanitizers of the host compiler and run as a process of its own."""
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_nothing_is_alive_in_a_fresh_process():
    code = "from contrack_amd import _native; _native.lib(); print(_native.debug_live())"
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert p.stdout.strip() == "(0, 0, 0, 0)", p.stdout


def test_debug_live_is_bound_and_listed():
    from contrack_amd import _native
    assert "ctk_debug_live" in _native.EXPORTS and hasattr(_native.lib(), "ctk_debug_live")
    live = _native.debug_live()
    assert len(live) == 4 and all(isinstance(v, int) and v >= 0 for v in live)


def test_owners_free_everything_exactly_once(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    # the sanitizer runtimes linked into the program: it runs whatever else the environment preloads
    static = ["-static-libsan"] if "clang" in version else ["-static-libasan", "-static-libubsan"]
    exe = str(tmp_path / "own_host")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static
    b = subprocess.run(cmd + ["-o", exe, os.path.join(ROOT, "tests", "own_host.cpp")], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "own_host: ok" in p.stdout, (p.returncode, p.stdout, p.stderr)
