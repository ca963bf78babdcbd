"""A stand-alone refusal program of tests/ (bfv_*_args_main.cpp: it includes csrc/bfv_pir_args.h, which needs no HIP) under the address and
undefined-behaviour sanitizers: compiled with g++ together with csrc/he_params.cpp, the sanitizer runtimes linked statically (the program
needs nothing of its environment and runs in the caller's, unchanged), and run as a child process."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "reference-seal-backend_amd", "csrc")


def run(tmp_path, main_cpp, expect_line):
    """build tests/<main_cpp> into tmp_path and run it: exit status 0 and `expect_line` on its output"""
    exe = str(tmp_path / os.path.splitext(main_cpp)[0])
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-mfma", "-ffp-contract=off", "-DHE355_U64_FOLD=0", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(HERE, main_cpp), os.path.join(CSRC, "he_params.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert expect_line in r.stdout
