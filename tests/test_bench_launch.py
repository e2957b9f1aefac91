"""bench.py's launch plumbing without a GPU: `python bench.py --gpus N` must start N ranks itself, and a rank count that
does not match --gpus must fail instead of silently measuring one GPU (Algorithm/FastSlam.py:25-27 is the sharding axis the
N-GPU number is about).  `--spawn-check` stops before any GPU work."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, drop=("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")):
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, capture_output=True, text=True, env=env, timeout=300)


def _json_line(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def test_bench_starts_its_own_ranks():
    res = _run(["--gpus", "2", "--spawn-check"])
    assert res.returncode == 0, res.stderr[-2000:]
    d = _json_line(res.stdout)
    assert d["n_gpus"] == 2 and d["ranks_seen"] == 2 and d["gpus_requested"] == 2


def test_bench_single_rank_needs_no_launcher():
    res = _run(["--gpus", "1", "--spawn-check"])
    assert res.returncode == 0, res.stderr[-2000:]
    assert _json_line(res.stdout)["n_gpus"] == 1


def test_bench_refuses_a_rank_count_that_is_not_gpus():
    res = _run(["--gpus", "8", "--spawn-check"], {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert res.returncode != 0
    assert "--gpus 8 but WORLD_SIZE=1" in res.stderr


def test_traffic_file_is_refused_when_the_kernels_changed(tmp_path, monkeypatch):
    sys.path.insert(0, REPO)
    import bench
    entry = {"hbm_bytes_corrected": 1.0, "launches_per_step": 1.0, "in_step": True}
    (tmp_path / "profiles").mkdir()
    monkeypatch.setattr(bench, "REPO", str(tmp_path))
    json.dump({"source_sha256": "0" * 64, "entries": {"config2:k_blur_clamp": entry}}, open(tmp_path / "profiles" / "traffic.json", "w"))
    got, note = bench.load_traffic("config2")
    assert got == {} and "refused" in note
    json.dump({"source_sha256": bench.source_sha256(), "entries": {"config2:k_blur_clamp": entry, "config5:k_bound1": entry}},
              open(tmp_path / "profiles" / "traffic.json", "w"))
    got, note = bench.load_traffic("config2")
    assert note is None and list(got) == ["k_blur_clamp"]


def test_full_and_dump_options_are_accepted():
    res = _run(["--gpus", "1", "--full", "--dump-outputs", "unused", "--spawn-check"])
    assert res.returncode == 0, res.stderr[-2000:]
    assert _json_line(res.stdout)["n_gpus"] == 1


def test_dumped_maps_are_seeded_samples_and_whole_sums(tmp_path):
    """bench.map_outputs on host-side stand-ins of the engine's maps (packed visited << 16 | total cells, a padded pitch):
    whole-map sums, the same sampled cells in every map and from run to run, particle 0's map whole; write_outputs keeps
    to float32 / float64 and refuses more than 64 MB."""
    import numpy as np
    import pytest
    import torch
    sys.path.insert(0, REPO)
    import bench

    class Map:
        wide = False

        def __init__(self, v, t):
            self.v, self.t = v, t
            self.rows, self.cols = v.shape
            packed = np.zeros((self.rows, self.cols + 5), dtype=np.uint32)
            packed[:, :self.cols] = (v.astype(np.uint32) << np.uint32(16)) | t.astype(np.uint32)
            self.cells = torch.from_numpy(packed.view(np.int32))

        def _materialise(self):
            pass

        def download(self):
            return self.v.astype(np.float64), self.t.astype(np.float64)

    rs = np.random.RandomState(3)
    maps = [Map(rs.randint(0, 40000, size=(300, 200)), rs.randint(0, 60000, size=(300, 200))) for _ in range(3)]
    a, b = bench.map_outputs(maps), bench.map_outputs(maps)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a["map_counts_sum"].dtype == np.float64 and a["map_sample"].dtype == np.float32
    for p, m in enumerate(maps):
        assert a["map_counts_sum"][p].tolist() == [float(m.v.sum()), float(m.t.sum())]
    idx = bench._sample_index(300, 200, bench.MAP_SAMPLE_CELLS, 1)
    assert a["map_sample"].shape == (3, len(idx), 2)
    assert np.array_equal(a["map_sample"][2, :, 0], maps[2].v.reshape(-1)[idx]) and np.array_equal(a["map_sample"][1, :, 1], maps[1].t.reshape(-1)[idx])
    assert np.array_equal(a["map0_visited"], maps[0].v) and np.array_equal(a["map0_total"], maps[0].t)
    bench.write_outputs(str(tmp_path / "out"), a)
    assert np.array_equal(np.load(tmp_path / "out" / "map_sample.npy"), a["map_sample"])
    with pytest.raises(SystemExit):
        bench.write_outputs(str(tmp_path / "big"), {"x": np.zeros((64 << 20) // 8 + 1)})
