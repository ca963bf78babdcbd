"""What the BFV probes (tools/bfv_*_probe.py) share: a slab offset, and the timing method -- regions between the context's timer events,
every candidate warmed up first, the candidates' regions taken in turn so that a drift of the clock meets all of them alike, min / median /
max of the regions reported.  tests/bfv_gpu_helpers.py takes `At` from here."""
import ctypes as C
import statistics


class At:
    """a device pointer `off` words into a slab (what a host hands the C ABI for one ciphertext of a batch)"""

    def __init__(self, buf, off):
        self.ptr = C.c_void_p(buf.ptr.value + int(off) * 8)


def region(g, f, n_calls):
    """us per call of one timed region of n_calls calls"""
    g.timer_begin()
    for _ in range(n_calls):
        f()
    return g.timer_end() / n_calls * 1e3


def alternated(g, fs, n_calls, repeats, warmup=2):
    """(min, median, max) us per call of every f of fs, n_calls[k] calls of fs[k] per region: `repeats` regions each, in turn, after
    `warmup` calls of each"""
    for f in fs:
        for _ in range(warmup):
            f()
    g.sync()
    t = [[] for _ in fs]
    for _ in range(repeats):
        for k, f in enumerate(fs):
            t[k].append(region(g, f, n_calls[k]))
    return [(min(v), statistics.median(v), max(v)) for v in t]


def fmt(t):
    return " / ".join(f"{v:11.1f}" for v in t)


def verdict(ta, tb):
    """(b)'s spread (max - min), and whether (a)'s median is not above (b)'s by more than it"""
    spread = tb[2] - tb[0]
    ok = ta[1] <= tb[1] + spread
    return spread, "accepted" if ok else "NOT accepted: slower than the composition"
