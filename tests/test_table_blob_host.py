"""The setters' one-allocation table builder (csrc/ms_table_blob.h) on the host: tests/table_blob_layout.cpp includes
only that header, is compiled here with AddressSanitizer and UBSan, and runs as a program of its own -- nothing is
loaded into this process.  It builds the shapes a miscount would hurt (every section empty; one double and one int; an
odd int count in front of a byte table that is no multiple of 8 long, as ms_set_thetab_boundary's with 1, 3 and 9 rows;
ms_set_rim_match's with one rim row, two outer rows and no disk) and checks, per shape: sections inside the image and
disjoint, doubles 8-byte and ints 4-byte aligned, sources copied in, every other byte zero, and every element of every
section written through the resolved pointers without leaving an allocation of exactly bytes() bytes."""

import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "membrane_solver_amd", "csrc")


def test_table_blob_layout_under_sanitizers(tmp_path):
    exe = str(tmp_path / "table_blob_layout")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "table_blob_layout.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.rstrip().endswith("all shapes ok")
    assert run.stdout.count("\nok ") + run.stdout.startswith("ok ") == 8
