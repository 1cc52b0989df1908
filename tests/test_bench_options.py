"""bench.py's options without a device: a plain run measures the headline only and --full adds everything else; --dump-outputs writes
a fixed selection of the last step's outputs as float32 / float64 .npy files under 64 MB."""
import types

import numpy as np
import torch

import bench


def test_a_plain_run_and_full():
    a = bench.parse_args(["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert a.full is False and a.repeat is None and a.workloads is None and a.dump_outputs is None and (a.steps, a.warmup) == (5, 2)
    b = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert b.full is True and b.dump_outputs == "out" and b.repeat is None and b.workloads is None


def test_dump_rows_are_fixed_and_bounded():
    assert np.array_equal(bench._seeded_rows(10, 16, 1), np.arange(10))
    r = bench._seeded_rows(1 << 22, bench.DUMP_CALL_ROWS, 1)
    assert r.size == bench.DUMP_CALL_ROWS and np.all(np.diff(r) > 0) and r[-1] < 1 << 22
    assert np.array_equal(r, bench._seeded_rows(1 << 22, bench.DUMP_CALL_ROWS, 1))
    # the most a dump can hold: a call row is 4 fp32 + its fp64 index, a probability row 24 fp32 + its fp64 index
    assert bench.DUMP_CALL_ROWS * (16 + 8) + bench.DUMP_PROB_SITES * (96 + 8) < 64 << 20


def test_dump_outputs_writes_the_selected_rows(tmp_path):
    n = bench.DUMP_PROB_SITES + 1000                                     # more windows than the probability sample holds
    g = torch.Generator().manual_seed(3)
    gt = torch.rand((n, 21), generator=g)
    zy = torch.rand((n, 3), generator=g)
    merged = torch.stack([gt.argmax(1).float(), zy.argmax(1).float(), gt.max(1).values, zy.max(1).values], 1)
    stage = types.SimpleNamespace(torch=torch, dev=torch.device("cpu"), gt_all=gt, zy_all=zy, sync=lambda: None)
    bench.dump_outputs(str(tmp_path / "d"), stage, merged, n)
    f = {p.stem: np.load(p) for p in (tmp_path / "d").glob("*.npy")}
    assert set(f) == {"calls", "calls_sites", "gt_prob", "zy_prob", "prob_sites"}
    assert all(a.dtype in (np.float32, np.float64) for a in f.values())
    assert np.array_equal(f["calls"], merged.numpy()) and np.array_equal(f["calls_sites"], np.arange(n))
    rows = f["prob_sites"].astype(np.int64)
    assert rows.size == bench.DUMP_PROB_SITES and np.array_equal(rows, bench._seeded_rows(n, bench.DUMP_PROB_SITES, 2))
    assert np.array_equal(f["gt_prob"], gt.numpy()[rows]) and np.array_equal(f["zy_prob"], zy.numpy()[rows])
