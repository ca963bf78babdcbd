"""The device-free argument checks of the BFV PIR calls (csrc/bfv_pir_args.h: one check per call, returning the plan the call runs on) under
the sanitizers: tests/bfv_pir_args_main.cpp, a stand-alone program, includes the header -- which needs no HIP -- builds the parameter object
of the CPU refusal tests (N = 4096, {60, 40, 40, 60}, t of 20 bits) and calls every check at the accepted and refused edge arguments those
tests use (levels and widths past their ends, n F at 2^32, grids at 2^31, strides that take a span past 2^60 words or wrap 64 bits, overlaps
one word inside and right behind), and reads the plans back.  Compiled with g++ -fsanitize=address,undefined, the sanitizer runtimes linked
statically (the program needs nothing of its environment and runs in the caller's, unchanged), and run as a child process: exit status 0.  The same refusals through the C ABI, with their return codes, are held by the tests/test_bfv_*_core_cpu.py modules.  No GPU."""
import sanitized_program


def test_plan_program_under_the_sanitizers(tmp_path):
    sanitized_program.run(tmp_path, "bfv_pir_args_main.cpp", "bfv_pir_args ok")
