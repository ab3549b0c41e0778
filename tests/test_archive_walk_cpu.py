"""No device: the walk over an archive's streams (scalce_amd/csrc/archive_walk.hpp) under AddressSanitizer and UBSan.
tools/archive_walk_check.cpp is a program of its own that builds the streams of small archives in memory, hands them out one
byte or odd-sized pieces at a time, and compares what the walk makes of them -- directory entries, slices, names, entries,
and the code, mate, stream and literal message of every failure of a malformed or truncated stream -- with what is written
out by hand in it; here it is compiled and run as a plain child process.  (The sanitizer runtimes are linked statically:
the program is complete in itself.)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_archive_walk_under_sanitizers(tmp_path):
    exe = str(tmp_path / "archive_walk_check")
    cc = subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tools", "archive_walk_check.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "archive_walk_check: ok", r.stdout + r.stderr
