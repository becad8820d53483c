"""The launch rules of contrack_amd/csrc/ctk_forms.h at slabs of 2^31 +- 1, 2^32 +- 1, 2^33 and 2^40 elements, without a GPU: a stand-alone
program (tests/forms_large_host.cpp) that asks them and checks what the launches rely on, built with the address and
undefined-behaviour sanitizers of the host compiler -- a signed overflow inside a rule is an error -- and run as a process of its own."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rules_hold_past_2_32_elements(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    # the sanitizer runtimes linked into the program: it runs whatever else the environment preloads
    static = ["-static-libsan"] if "clang" in version else ["-static-libasan", "-static-libubsan"]
    exe = str(tmp_path / "forms_large_host")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static
    b = subprocess.run(cmd + ["-o", exe, os.path.join(ROOT, "tests", "forms_large_host.cpp")], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "forms_large_host: ok" in p.stdout, (p.returncode, p.stdout[-4000:], p.stderr[-4000:])
