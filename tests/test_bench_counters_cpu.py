"""bench.py's roofline object quotes committed counter files (PMC passes cannot run inside a bench run): the files it looks for exist for
the three key-switch configurations, carry the fields the line uses, and are consistent with themselves."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_committed_counter_files_feed_the_bench_line():
    b = _bench()
    for config, ops in (("mul_relin_rescale", 1024), ("dot", 64), ("bfv_matmul", 64)):
        got = b.committed_counters(config, 1, ops)
        assert got, config
        j, path = got
        assert path.startswith("profiles/r") and path.endswith(f"_{config}_kernel_bounds.json")
        assert j["ops_per_step"] == ops
        assert j["hbm_bytes_per_op"] > 0 and j["valu_wave_instr_per_op"] > 0 and 1000 < j["sustained_mhz_time_weighted"] < 2500
        ks = j["kernels"]
        assert abs(sum(k["valu_wave_instr"] for k in ks) - j["valu_wave_instr_per_step"]) <= 1e-6 * j["valu_wave_instr_per_step"]
        for k in ks:  # a fraction above ~1 would mean a broken unit somewhere (GRBM under-counts on sub-millisecond dispatches: allow 1.1)
            assert 0 <= k["hbm_frac_of_8TBps"] < 1.0 and 0 <= k["valu_issue_frac"] < 1.1, (config, k["kernel"])
    assert b.committed_counters("eltwise_mul", 1, 256) is None  # streaming configurations: SURVEY 8d's HBM roofline, no counter file
    # the headline's algorithmic bytes and the traffic ratio the line prints
    j, _ = b.committed_counters("mul_relin_rescale", 1, 1024)
    assert 5.5 < j["hbm_bytes_per_op"] / 24780800 < 7.5


def test_power_sample_reads_the_devices_hwmon_or_reports_nothing(tmp_path, monkeypatch):
    """bench.py's `roofline.power`: without the device's hwmon files the line simply carries no power block (never an exception); with them
    (a stand-in directory tree here) it reports median / maximum watts of the run's last two thirds against the cap."""
    import glob as globmod
    import types
    b = _bench()
    props = types.SimpleNamespace(pci_domain_id=0, pci_bus_id=0xfe, pci_device_id=0x1f)
    ran = []
    assert b.sample_power(props, lambda k: ran.append(k), 0.01, window_seconds=0.05) is None and not ran  # no such PCI function here
    hw = tmp_path / "hwmon" / "hwmon3"
    hw.mkdir(parents=True)
    (hw / "power1_input").write_text("1370000000\n")
    (hw / "power1_cap").write_text("1400000000\n")
    (hw / "freq1_input").write_text("1975000000\n")
    real_glob = globmod.glob
    monkeypatch.setattr(globmod, "glob", lambda pat: [str(hw)] if pat.endswith("/hwmon/hwmon*") else real_glob(pat))
    import time
    got = b.sample_power(props, lambda k: (ran.append(k), time.sleep(0.4)), 0.1, window_seconds=0.4)
    assert ran == [4] and got["package_w_median"] == 1370.0 and got["cap_w"] == 1400.0 and got["frac_of_cap"] == 0.979
    assert got["sclk_mhz_median"] == 1975.0 and got["samples"] >= 3


def test_dump_sample_is_fixed_and_within_budget():
    """--dump-outputs: the sample of results and coefficient positions is a function of the step's shape only (two runs of the same
    arguments write the same positions), holds the first and the last result, and stays under the 64 MB the dump may take."""
    b = _bench()
    for n, polys, N in ((1024, 30, 32768), (64, 32, 32768), (64, 6, 32768), (256, 24, 16384), (4096, 4, 8192), (1, 30, 32768), (2, 4, 8192), (3, 4, 8192)):
        idx, cols = b.dump_sample(n, polys, N)
        idx2, cols2 = b.dump_sample(n, polys, N)
        assert list(idx) == list(idx2) and (cols is None) == (cols2 is None) and (cols is None or list(cols) == list(cols2))
        assert len(idx) == min(n, b.DUMP_RESULTS) and idx[0] == 0 and idx[-1] == n - 1 and all(idx[:-1] < idx[1:])
        m = N if cols is None else len(cols)
        assert cols is None or (all(cols[:-1] < cols[1:]) and 0 <= cols[0] and cols[-1] < N)
        assert len(idx) * polys * m * 2 * 8 <= 64e6


def test_dump_outputs_writes_exact_words(tmp_path):
    """Every u64 residue word of the sampled results comes back exactly from its two float64 halves."""
    import types
    import numpy as np
    b = _bench()
    n, per, N = 5, (2, 3), 64
    words = np.random.default_rng(3).integers(0, 1 << 61, size=n * per[0] * per[1] * N, dtype=np.uint64)

    class Buf:
        def download_range(self, off, shape):
            k = int(np.prod(shape))
            return words[off:off + k].reshape(shape).copy()

    wl = types.SimpleNamespace(n=n, N=N, result_slab=lambda: (Buf(), per))
    info = b.dump_outputs(wl, str(tmp_path / "out"), 0, 1)
    got = np.load(tmp_path / "out" / "result.npy")
    assert got.dtype == np.float64 and got.shape == (n, per[0], per[1], N, 2) and info["files"] == ["result.npy"]
    back = (got[..., 0].astype(np.uint64) << np.uint64(32)) | got[..., 1].astype(np.uint64)
    assert np.array_equal(back, words.reshape((n,) + per + (N,)))


def test_plain_run_rejects_the_checks_of_full():
    """The checker legs belong to --full: asking for a parity or CPU sample without it is an error, before any GPU work."""
    import subprocess
    import sys
    for flag in ("--parity-sample", "--cpu-sample"):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", flag, "1"], capture_output=True, text=True, timeout=120)
        assert p.returncode == 2 and "--full" in p.stderr
