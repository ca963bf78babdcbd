"""The test-only CPU build of the product's host-compilable code (tests/csim): `make` once per process, one library per form of the
u64 engine's multiply-by-constant (csrc/modarith.h)."""
import ctypes as C
import functools
import os
import subprocess

CSIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csim")


@functools.lru_cache(maxsize=None)
def _make():
    subprocess.run(["make", "-C", CSIM, "-s"], check=True)


def load(fold=False):
    """libcsim.so (Shoup quotients, any prime) or, fold, libcsim_fold.so (fold reduction, primes 2^60 - c).  A ctypes handle of the
    caller's own: the argtypes one test module sets are not another's."""
    _make()
    return C.CDLL(os.path.join(CSIM, "_build", "libcsim_fold.so" if fold else "libcsim.so"))
