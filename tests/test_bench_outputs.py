"""bench.py --dump-outputs and the plain / --full split.  CPU: dump_outputs on synthetic records
(every u64 bit survives, the dense visit counts, the fixed sample).  GPU: one plain bench run at a
small size dumps exactly the records an engine of the same arguments returns in this process, its
line holds the headline fields and none of the --full legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402  (stdlib-only at import time)

NAMES = ("games", "states", "info", "ctr", "values", "final", "n_moves", "visit_counts", "expansions")
FULL_ONLY = ("kernel_ms", "roofline", "coach", "config3_shape", "predict_f16", "arena", "train", "cpu_baseline")


def _fake_records(E, M, seed):
    rng = np.random.default_rng(seed)
    nm = rng.integers(1, M + 1, size=E).astype(np.int32)
    off, vis = np.zeros(E * M + 1, dtype=np.int64), []
    for e in range(E):
        for m in range(M):
            k = int(rng.integers(1, 6)) if m < nm[e] else 0
            acts = rng.choice(bench.A, size=k, replace=False)
            vis.append(np.stack([acts, rng.integers(1, 100, size=k)], axis=1).astype(np.int32).reshape(k, 2))
            off[e * M + m + 1] = off[e * M + m] + k
    return dict(states=rng.integers(0, 2**64, size=(E, M, 8), dtype=np.uint64),
                info=rng.integers(-5, 4000, size=(E, M, 8)).astype(np.int32),
                ctr=rng.integers(0, 2**64, size=(E, M, 2), dtype=np.uint64), values=rng.standard_normal((E, M)),
                final=rng.integers(0, 2**64, size=(E, 8), dtype=np.uint64), n_moves=nm, visits_off=off,
                visits=np.concatenate(vis))


def _check_dump(d, rec, expansions):
    """The dumped arrays against the records they were taken from."""
    E, M = rec["values"].shape
    pick = d["games"].astype(np.int64)
    assert len(pick) == min(E, bench.DUMP_GAMES) and np.all(np.diff(pick) > 0) and pick.max() < E
    assert all(d[k].dtype == (np.float32 if k == "visit_counts" else np.float64) for k in NAMES)
    assert sum(d[k].nbytes for k in NAMES) <= 64 * 10**6
    for k in ("states", "ctr", "final"):  # (low, high) halves back to the u64 words
        w = d[k].astype(np.uint64)
        assert np.array_equal(w[..., 0::2] | (w[..., 1::2] << np.uint64(32)), rec[k][pick]), k
    for k in ("info", "values", "n_moves"):
        assert np.array_equal(d[k], rec[k][pick].astype(np.float64)), k
    assert d["visit_counts"].shape == (len(pick), M, bench.A)
    for r, e in enumerate(pick):
        for m in range(M):
            v = rec["visits"][rec["visits_off"][e * M + m]:rec["visits_off"][e * M + m + 1]]
            c = np.zeros(bench.A, dtype=np.float32)
            c[v[:, 0]] = v[:, 1]
            assert np.array_equal(d["visit_counts"][r, m], c), (e, m)
    assert d["expansions"].tolist() == [float(expansions)]


@pytest.mark.parametrize("E", [5, 70])  # fewer games than the sample keeps, and more
def test_dump_outputs_on_synthetic_records(tmp_path, E):
    rec = _fake_records(E, 6, seed=E)
    for sub in ("a", "b"):
        bench.dump_outputs(rec, 1234, str(tmp_path / sub))
    a, b = ({k: np.load(tmp_path / sub / f"{k}.npy") for k in NAMES} for sub in ("a", "b"))
    assert sorted(os.listdir(tmp_path / "a")) == sorted(k + ".npy" for k in NAMES)
    _check_dump(a, rec, 1234)
    assert all(np.array_equal(a[k], b[k]) for k in NAMES)  # the sample is fixed


@pytest.mark.gpu
def test_plain_bench_dumps_the_last_timed_steps_records(tmp_path):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    envs, sims, steps, warmup, seed = 96, 8, 2, 1, 5
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--envs", str(envs), "--sims", str(sims), "--seed", str(seed),
                        "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=200,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == warmup and d["n_gpus"] == 1
    assert d["unit"] == "expansions/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["metric"] == bench.METRIC and d["value"] > 0 and d["ms_per_step"] > 0
    # value = expansions of the timed steps / their time, ms_per_step = that time / steps
    assert d["value"] * d["ms_per_step"] * 1e-3 == pytest.approx(d["expansions_per_episode_batch"], rel=1e-9)
    assert not [k for k in FULL_ONLY if k in d]
    dump = {k: np.load(tmp_path / "out" / f"{k}.npy") for k in NAMES}
    assert sorted(os.listdir(tmp_path / "out")) == sorted(k + ".npy" for k in NAMES)
    # the same net, engine and stream seed in this process: the last timed step is step warmup + steps - 1
    from yacht_amd.engine import SelfPlayEngine
    from yacht_amd.nnet import YachtNNet, YkNet
    torch.manual_seed(seed)
    net = YkNet(YachtNNet(hidden=bench.H, nblocks=bench.NB).state_dict(), bench.H, bench.NB)
    eng = SelfPlayEngine(envs, sims, 1.5, 15, net=net, max_moves=bench.GAME_MOVES)
    eng.run(seed + warmup + steps - 1, 0)
    st = eng.stats()
    assert st["errors"] == 0
    _check_dump(dump, eng.records(), st["expansions"])
    eng.close()
