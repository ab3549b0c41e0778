"""No device: the stream cursor of the decompress host (scalce_amd/csrc/stream_src.hpp) under AddressSanitizer and UBSan.
tools/src_check.cpp is a program of its own that drives need / fill / pass / read_into over read callbacks that hand out one
byte, odd-sized pieces, an error at the k-th call or an early end, and over every kind of skip callback; here it is compiled
and run as a plain child process.  (The sanitizer runtimes are linked statically: the program is complete in itself.)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_cursor_under_sanitizers(tmp_path):
    exe = str(tmp_path / "src_check")
    cc = subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tools", "src_check.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "src_check: ok", r.stdout + r.stderr
