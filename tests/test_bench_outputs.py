"""bench.py's `--dump-outputs DIR` and `--full`: the dump holds every value of
the fetched arrays exactly (float64), stays inside its byte budget with a fixed
sample, and a plain run prints the headline fields only while `--full` adds the
objects that take runs of their own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _outputs(n=1000):
    rng = np.random.default_rng(7)
    pl = rng.integers(-1, 200000, n).astype(np.int32)
    pl[:3] = (-1, 0, 199999)
    cp = rng.integers(0, 2 ** 63, (n, 4), dtype=np.uint64) * np.uint64(2) + np.uint64(1)   # bits 0 and 63 in use
    cp[0] = 0
    cp[1] = np.uint64(0xFFFFFFFFFFFFFFFF)
    dv = rng.integers(0, 2 ** 32, (n, 2), dtype=np.uint64).astype(np.uint32)
    return {"placements": pl, "cpusets": cp, "devices": dv}


def test_dump_holds_every_value_exactly(tmp_path):
    o = _outputs()
    bench.dump_outputs(str(tmp_path), o)
    assert sorted(os.listdir(tmp_path)) == ["cpusets.npy", "devices.npy", "placements.npy"]
    pl, cp, dv = (np.load(tmp_path / f"{k}.npy") for k in ("placements", "cpusets", "devices"))
    assert pl.dtype == cp.dtype == dv.dtype == np.float64
    assert np.array_equal(pl.astype(np.int32), o["placements"])
    assert np.array_equal(dv.astype(np.uint32), o["devices"])
    assert cp.shape == (1000, 4, 2)      # [..., 0] the low 32 bits, [..., 1] the high
    back = cp[..., 0].astype(np.uint64) | (cp[..., 1].astype(np.uint64) << np.uint64(32))
    assert np.array_equal(back, o["cpusets"])


def test_dump_over_budget_is_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 3 * 4096)
    o = _outputs()
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), o)
    bench.dump_outputs(str(b), o)
    total = 0
    for k, full in (("placements", o["placements"].astype(np.float64)),
                    ("devices", o["devices"].astype(np.float64))):
        x, y = np.load(a / f"{k}.npy"), np.load(b / f"{k}.npy")
        assert np.array_equal(x, y)                      # the same rows every run
        assert x.nbytes <= 4096 and 0 < len(x) < len(full)
        rows = np.sort(np.random.default_rng(0).choice(len(full), size=len(x), replace=False))
        assert np.array_equal(x, full[rows])
        total += x.nbytes
    total += np.load(a / "cpusets.npy").nbytes
    assert total <= 3 * 4096
    # an array inside its share is written whole
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 64 << 20)
    bench.dump_outputs(str(tmp_path / "c"), o)
    assert len(np.load(tmp_path / "c" / "placements.npy")) == 1000


def test_check_belongs_to_full():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--check", "--probe-ranks"],
                       capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert r.returncode != 0 and "--full" in r.stderr


HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"}
FULL_ONLY = {"roofline", "eval_roofline", "latency", "cpu_baseline", "speedup_vs_best_cpu_leg", "check"}
NODES, PODS = 3000, 4000


@pytest.fixture(scope="module")
def oracle_placements():
    import oracle
    from koordinator_amd import synth
    from koordinator_amd.config import shipped_profile, to_c_config
    prof = shipped_profile()
    table, pods = synth.config_workload(4, prof, n_nodes=NODES, n_pods=PODS)
    return oracle.Oracle(to_c_config(prof), table).place_stream(pods)


@pytest.mark.gpu
@pytest.mark.parametrize("full", [False, True], ids=["plain", "full"])
def test_bench_line_and_dump(tmp_path, oracle_placements, full):
    """A small config-4 stream through bench.py: --steps sets the timed steps,
    the dumped placements are the oracle's, a plain line carries none of the
    objects that need runs of their own and a --full line all of them."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--nodes", str(NODES), "--pods", str(PODS), "--dump-outputs", str(tmp_path / "out")]
    if full:
        cmd += ["--full", "--check", "--cpu-budget", "0.3"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert HEADLINE <= set(d) and d["steps"] == 2 and d["warmup"] == 1
    assert d["unit"] == "pods/s" and d["higher_is_better"] is True and d["dtype"] == "int64"
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(PODS / (d["ms_per_step"] * 1e-3), rel=1e-3)
    if full:
        assert FULL_ONLY <= set(d) and d["check"] is True
    else:
        assert not (FULL_ONLY & set(d))
    assert os.listdir(tmp_path / "out") == ["placements.npy"]
    got = np.load(tmp_path / "out" / "placements.npy")
    assert got.dtype == np.float64 and np.array_equal(got, oracle_placements.astype(np.float64))
    assert d["unschedulable"] == int((oracle_placements < 0).sum())
