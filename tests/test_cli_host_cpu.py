"""No device: the host pieces of the `scalce` tool (scalce_amd/csrc/cli_io.hpp, cli_input.hpp, cli_shares.hpp, cli_sink.hpp)
under AddressSanitizer and UBSan.  tools/cli_host_check.cpp is a program of its own that checks, on small files it writes
into the directory it is given, the record cuts and the placement of a --gpus run with every rank computed in one process,
MateSource over plain and gzipped files, OutFile's gzip members, TextSink's -S parts and that no descriptor stays open; here
it is compiled and run as a plain child process.  (The sanitizer runtimes are linked statically: the program is complete in
itself.)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cli_host_pieces_under_sanitizers(tmp_path):
    exe = str(tmp_path / "cli_host_check")
    work = tmp_path / "files"
    work.mkdir()
    cc = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tools", "cli_host_check.cpp"), "-o", exe,
                         "-lz", "-lpthread"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    r = subprocess.run([exe, str(work)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "cli_host_check: ok", r.stdout + r.stderr
