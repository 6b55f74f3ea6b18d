"""The solve's results through the sweep driver, on the CPU: a fake solving compute (a deterministic
function of the global flat index, as in tests/test_sweep_dist.py) under gloo at world sizes 1, 2 and
3 -- the gathered result table (what solve.npy holds) and the summary block must be the same for every
world size and on every rank; each checkpointed chunk has its .solve.npy sibling, a resume reloads
both, and a table shard without its sibling is an error.  Also the spec's "solve" section: parsing,
the to_json round trip and the checkpoint key, and the refusals with their reasons."""
import json
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import pkg
from test_sweep_dist import fake_compute, free_port

SOLVE = {"field": "source_shape_sigma_y", "lo": 1.0, "hi": 50.0}
TOTAL, CHUNK = 1003, 97


def fake_results(start, n):
    """(n, 6) results of the global indices: x rising with the index, every status present."""
    idx = torch.arange(start, start + n, dtype=torch.float64)
    status = torch.remainder(idx, 7).clamp(max=4)
    ok = status <= 1
    nan = torch.full_like(idx, float("nan"))
    x = torch.where(ok, 2.0 + idx / 64.0, nan)
    return torch.stack([x, torch.where(ok, x - 1e-3, torch.full_like(idx, 1.0)), torch.where(ok, x + 1e-3, torch.full_like(idx, 50.0)),
                        torch.where(ok, idx * 1e-15, nan), 2.0 + torch.remainder(idx, 23), status], dim=1)


def make_fake():
    def compute(start, n, out):
        fake_compute(start, n, out)
        compute.solve_last = fake_results(start, n)
    compute.solve = pkg("solve").normalize(SOLVE)
    compute.solve_last = compute.solve_local = None
    return compute


def _worker(rank, world, port, out_dir, res_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sw, V = pkg("sweep"), pkg("solve")
    s, e = sw.shard_range(TOTAL, rank, world)
    compute = make_fake()
    local = sw.run_local(compute, s, e, lambda n: torch.empty((n, 6), dtype=torch.float64), CHUNK, out_dir)
    table = sw.gather_table(local, TOTAL, rank, world)
    solved = sw.gather_table(compute.solve_local, TOTAL, rank, world)
    np.save(res_path + f".table.{rank}.npy", table.numpy())
    np.save(res_path + f".solve.{rank}.npy", solved.numpy())          # what main() writes as solve.npy
    with open(res_path + f".summary.{rank}.json", "w") as f:
        json.dump(V.summary(SOLVE, solved.numpy()), f)
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def reference():
    table = torch.empty((TOTAL, 6), dtype=torch.float64)
    fake_compute(0, TOTAL, table)
    sol = fake_results(0, TOTAL).numpy()
    return table.numpy(), sol, pkg("solve").summary(SOLVE, sol)


@pytest.mark.parametrize("world", [1, 2, 3])
def test_solve_table_and_summary_are_the_same_at_every_world_size(world, reference):
    sw = pkg("sweep")
    table, sol, summary = reference
    assert sum(summary["status"].values()) == TOTAL and all(v > 0 for v in summary["status"].values())
    with tempfile.TemporaryDirectory() as d:
        res = os.path.join(d, "res")
        mp.spawn(_worker, args=(world, free_port(), d, res), nprocs=world, join=True)
        for r in range(world):
            assert np.array_equal(np.load(res + f".table.{r}.npy"), table)
            got = np.load(res + f".solve.{r}.npy")
            assert got.shape == (TOTAL, 6) and got.tobytes() == sol.tobytes(), r
            with open(res + f".summary.{r}.json") as f:
                assert json.load(f) == json.loads(json.dumps(summary)), r
        # every checkpointed chunk has its sibling
        shards = sorted(f for f in os.listdir(d) if f.startswith("shard_") and not f.endswith(".solve.npy"))
        assert shards and all(os.path.exists(os.path.join(d, f[:-4] + ".solve.npy")) for f in shards)
        # resume: nothing is recomputed, both arrays come back
        for r in range(world):
            s, e = sw.shard_range(TOTAL, r, world)

            def boom(*a):
                raise AssertionError("recomputed a checkpointed chunk")
            boom.solve, boom.solve_last, boom.solve_local = SOLVE, None, None
            loc = sw.run_local(boom, s, e, lambda n: torch.empty((n, 6), dtype=torch.float64), CHUNK, d, resume=True)
            assert np.array_equal(loc.numpy(), table[s:e])
            assert boom.solve_local.numpy().tobytes() == sol[s:e].tobytes()
        # a table shard without its sibling is an error
        os.remove(os.path.join(d, shards[0][:-4] + ".solve.npy"))
        c = make_fake()
        with pytest.raises(RuntimeError, match="no solve record"):
            sw.run_local(c, 0, TOTAL, lambda n: torch.empty((n, 6), dtype=torch.float64), CHUNK, d, resume=True)


def test_a_plain_compute_is_untouched():
    sw = pkg("sweep")
    with tempfile.TemporaryDirectory() as d:
        sw.run_local(fake_compute, 0, 50, lambda n: torch.empty((n, 6), dtype=torch.float64), 20, d)
        assert not [f for f in os.listdir(d) if f.endswith(".solve.npy")]


class NoFit:
    """run_local's keep_table=False needs an accumulator; this one keeps nothing."""
    def update(self, view, c0):
        pass


def _worker_no_table(rank, world, port, res_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sw = pkg("sweep")
    s, e = sw.shard_range(TOTAL, rank, world)
    compute = make_fake()
    out = sw.run_local(compute, s, e, lambda n: torch.empty((n, 6), dtype=torch.float64), CHUNK, None, fit=NoFit(),
                       keep_table=False)
    assert out is None and compute.solve_local is None and compute.solve_x.shape == (e - s,)
    with open(res_path + f".summary.{rank}.json", "w") as f:
        json.dump(sw.solve_summary_streamed(compute, TOTAL, rank, world), f)
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [1, 2, 3])
def test_fit_only_sweep_keeps_the_summary_block(world, reference):
    """keep_table=False (--no-table): no result table, the block from the x column and integer counts --
    the block of the full table, on every rank and at every world size."""
    summary = reference[2]
    with tempfile.TemporaryDirectory() as d:
        res = os.path.join(d, "res")
        mp.spawn(_worker_no_table, args=(world, free_port(), res), nprocs=world, join=True)
        assert not [f for f in os.listdir(d) if f.endswith(".npy")]
        for r in range(world):
            with open(res + f".summary.{r}.json") as f:
                assert json.load(f) == json.loads(json.dumps(summary)), r
    # without a process group: the local shard is the grid
    sw = pkg("sweep")
    c = make_fake()
    sw.run_local(c, 0, TOTAL, lambda n: torch.empty((n, 6), dtype=torch.float64), CHUNK, None, fit=NoFit(),
                 keep_table=False)
    assert sw.solve_summary_streamed(c, TOTAL, 0, 1) == summary


AXES = [{"field": "m_chi_GeV", "values": [0.5, 1.0, 2.0]}, {"field": "v_w", "values": [0.2, 0.3]}]


def test_spec_section_round_trip_and_key():
    sw, V = pkg("sweep"), pkg("solve")
    spec = sw.spec_from_json({"name": "s", "axes": AXES, "solve": SOLVE})
    assert spec.solve == V.normalize(SOLVE)
    j = spec.to_json()
    assert j["solve"] == V.normalize(SOLVE)
    again = sw.spec_from_json(json.loads(json.dumps(j)))
    assert again.solve == spec.solve and again.to_json() == j
    plain = sw.spec_from_json({"name": "s", "axes": AXES})
    assert plain.solve is None and "solve" not in plain.to_json()
    other = sw.spec_from_json({"name": "s", "axes": AXES, "solve": dict(SOLVE, hi=40.0)})
    assert len({sw.spec_key(spec), sw.spec_key(plain), sw.spec_key(other)}) == 3
    # the CLI form gives the same section
    assert V.parse_cli("source_shape_sigma_y:1:50") == spec.solve
    win = sw.spec_from_json({"name": "w", "axes": AXES, "window": {"kind": "plateau", "half_width": 3.0},
                             "solve": {"field": "window_half_width", "lo": 0.0, "hi": 40.0}})
    assert win.to_json()["solve"]["field"] == "window_half_width"


@pytest.mark.parametrize("extra,solve,msg", [
    ({"base": {"Gamma_wash_over_H": 0.5}}, SOLVE, "ODE fallback"),
    ({"axes": AXES + [{"field": "sigma_v_chi_GeV_m2", "values": [0.0, 1e-30]}]}, SOLVE, "ODE fallback"),
    ({"crossings": {"n_cross": 2}}, {"field": "P_chi_to_B", "lo": 0.01, "hi": 1.0}, "crossings or a profile"),
    ({"window": {"kind": "plateau"}, "axes": AXES + [{"field": "window_sigma", "values": [2.0, 3.0]},
                                                     {"field": "window_sigma_lo", "values": [1.0, 2.0]}]},
     {"field": "window_half_width", "lo": 0.0, "hi": 40.0}, "collide"),
    ({}, {"field": "I_p", "lo": 0.1, "hi": 1.0}, "z-sum tables"),
    ({}, {"field": "m_chi_GeV", "lo": 0.1, "hi": 1.0}, "writes the solve field"),
    ({}, {"field": "window_half_width", "lo": 0.0, "hi": 40.0}, "needs a window"),
    ({}, {"field": "v_w", "lo": 0.5, "hi": 0.1}, "lo < hi"),
])
def test_spec_refusals_say_why(extra, solve, msg):
    sw = pkg("sweep")
    d = dict({"name": "s", "axes": AXES, "solve": solve}, **extra)
    with pytest.raises(ValueError, match=msg):
        sw.spec_from_json(d)
