"""bench.py without --full: exactly --steps timed steps, the contract's keys and nothing of the further legs, and --dump-outputs
writing the commitment the timed path returned -- checked against the CPU oracle's MSM of the same seeded streams.  The bench
runs as a child process; this parent never touches HIP."""
import json, os, subprocess, sys
import numpy as np
import pytest
import orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_its_steps_and_dumps_the_commitment(tmp_path):
    lg = 12
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MZK_BENCH_SHARED_GPU_TEST")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--log2n", str(lg),
                        "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, "bench failed (rc %d):\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["n_gpus"] == 1 and rec["config"]["pairs_per_gpu"] == 1 << lg
    assert rec["unit"] == "pairs/s" and rec["higher_is_better"] is True and rec["metric"].startswith("G1 MSM pairs/sec") and rec["dtype"]
    assert rec["ms_per_step"] > 0 and abs(rec["value"] - (1 << lg) / (rec["ms_per_step"] * 1e-3)) <= 1e-9 * rec["value"]
    assert not {"parity", "roofline", "cpu_baseline", "legs_ms", "detail_file"} & set(rec)          # --full only
    got = np.load(str(tmp_path / "kzg_commitment.npy"))
    assert got.dtype == np.float64 and got.shape == (2, 8) and os.listdir(str(tmp_path)) == ["kzg_commitment.npy"]
    x, y = (sum(int(w) << (32 * i) for i, w in enumerate(row)) for row in got)
    sys.path.insert(0, ROOT)
    import bench
    n = 1 << lg
    assert (x, y) == orc.msm_fast(orc.synth_vector(orc.FR, bench.SEED, n), orc.synth_points(bench.SEED + 7, n))
