"""The numpy reference of the PIR database codec that the GPU tests compare with (held to Python integers in test_bfv_bytes_core_cpu.py)."""
import numpy as np


def np_fields(data, w, N):
    """[n][B] bytes -> [n][N] coefficients: bits [e w, e w + w) of each row read as one little-endian integer, zero-extended"""
    n, B = data.shape
    bits = np.zeros((n, N * w), dtype=np.uint8)
    bits[:, :8 * B] = np.unpackbits(data, axis=1, bitorder="little")
    weights = np.uint64(1) << np.arange(w, dtype=np.uint64)
    return (bits.reshape(n, N, w).astype(np.uint64) * weights).sum(axis=2, dtype=np.uint64)
