"""The slot-writer table of the leaflet add-on passes (csrc/ms_slot_writers.h) on the host:
tests/slot_writer_rules.cpp includes only that header, is compiled here with AddressSanitizer and UBSan, and runs as a
program of its own -- nothing is loaded into this process.  It walks every subset of the table's ten module bits, both
values of rsm_inner and the three phases (2 x 1024 x 3 combinations) and compares, for every writer, the table's cell
mode and launch decision with the expressions the passes carried before the table, written out long-hand; and the
derived masks and the run order with the literals of that code."""

import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "membrane_solver_amd", "csrc")
INCLUDE = os.path.join(HERE, "..", "include")


def test_slot_writer_rules_under_sanitizers(tmp_path):
    exe = str(tmp_path / "slot_writer_rules")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", CSRC, "-I", INCLUDE,
                            os.path.join(HERE, "slot_writer_rules.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.rstrip().endswith("6144 combinations ok")
