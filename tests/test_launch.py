"""
``fit --gpus N`` without a GPU (tapqir_amd/launch.py): the posterior read-out keyed by global AOI index, the merge of
the ranks' output files, the launcher end to end over gloo on the g++ host build of the kernels' math, its supervision
of failing ranks (CPU processes only), the command line's exit codes and the ABI of ``tq_probs_args``.
"""

import ctypes
import os
import subprocess
import time

import pytest
import torch
from typer.testing import CliRunner

import launch_fixture as lf
from helpers import HostCheckEngine
from tapqir_amd import _lib, launch
from tapqir_amd.parallel import shard_bounds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
runner = CliRunner()


# -- 1. read-out is shard-invariant (host build) ------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,all_on,worlds", lf.READOUT_CASES, ids=lf.READOUT_IDS)
def test_readout_is_shard_invariant_host_build(N, K, all_on, worlds):
    """``compute_probs`` of the whole set equals, BITWISE, the concatenation over the shards: the per-unit arithmetic is
    the same function of the same draws once the streams are keyed by the global unit index."""
    d, o = lf.readout_problem(N, K, all_on)
    make = lambda data, **kw: HostCheckEngine(data, K=K, device="cpu", seed=5, **kw)
    full = lf.full_engine(make, d, o)
    z, th = lf.readout(full)
    assert float(z[..., 1].max()) > 0  # the read-out did draw
    for world in worlds:
        zs, ths = lf.sharded_readout(make, d, full, world)
        assert torch.equal(zs, z), world
        assert torch.equal(ths, th), world


def test_readout_rejects_a_negative_offset():
    a = _lib.ProbsArgs()
    keep = torch.zeros(64)
    for f in ("params", "is_ontarget", "globals_p", "gbase_p", "z_probs", "theta_probs"):
        setattr(a, f, _lib.ptr(keep))
    a.Nt, a.F, a.C, a.P, a.K, a.particles, a.draw, a.n_offset = 1, 1, 1, 14, 1, 1, 1, -1
    lib = _lib.load()
    assert lib.tq_cosmos_probs(ctypes.byref(a), None) == 1  # TQ_ERR_ARG, before any launch
    assert b"n_offset" in lib.tq_last_error()


# -- 2. merge -----------------------------------------------------------------------------------------------------------
def _ci_stats(K=2, Nt=5, F=3, Q=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(s, generator=g, dtype=torch.float64)
    iv = lambda *s: {"LL": r(*s), "UL": r(*s), "Mean": r(*s)}
    out = {"gain": iv(), "pi": iv(Q, 2), "lamda": iv(Q), "proximity": iv(), "background": iv(Nt, F, Q)}
    for n in ("height", "width", "x", "y"):
        out[n] = iv(K, Nt, F, Q)
    out["m_probs"] = r(K, Nt, F, Q).float()
    out["z_probs"] = r(Nt, F, Q, 2).float()
    out["theta_probs"] = r(K, Nt, F, Q).float()
    out["z_map"] = torch.argmax(out["z_probs"], -1)
    out["p_specific"] = out["theta_probs"].sum(0)
    out["chi2"] = {"values": r(Nt, F, Q).float()}
    return out


def _slice(full, lo, hi):
    out = {}
    for name, v in full.items():
        ax = launch.AOI_AXIS.get(name)
        cut = (lambda t: t) if ax is None else (lambda t: t.narrow(ax, lo, hi - lo).clone())
        out[name] = {k: cut(t) for k, t in v.items()} if isinstance(v, dict) else cut(v)
        if isinstance(v, dict) and ax is not None:
            out[name]["vmin"], out[name]["vmax"] = -1.0 * lo, 1.0 * hi  # per-rank plot ranges are not merged
    return out


@pytest.mark.parametrize("world", [2, 3])
def test_merge_restores_the_unsharded_statistics(world):
    full = _ci_stats()
    ranks = [_slice(full, *shard_bounds(5, r, world)) for r in range(world)]
    merged = launch.merge_ci_stats(ranks)
    assert lf.signature(merged) == lf.signature(full)
    assert list(merged) == list(full)
    for name, v in full.items():
        for k in (v if isinstance(v, dict) else [None]):
            a, b = (merged[name], v) if k is None else (merged[name][k], v[k])
            assert torch.equal(a, b), (name, k)


def test_merge_names_a_global_entry_that_differs():
    full = _ci_stats()
    ranks = [_slice(full, *shard_bounds(5, r, 3)) for r in range(3)]
    ranks[2]["lamda"]["UL"] = ranks[2]["lamda"]["UL"] + 1e-12
    with pytest.raises(ValueError, match="lamda"):
        launch.merge_ci_stats(ranks)


# -- 3. end to end through launch_fit -----------------------------------------------------------------------------------
FIT = {"mode": "fit", "model": "cosmos", "learning_rate": 0.005, "nbatch_size": 6, "fbatch_size": 5, "num_iter": 4,
       "matlab": False, "pg_timeout": 120}
SETTINGS = {"S": 1, "K": 2, "device": "cpu", "dtype": "double"}


@pytest.fixture
def workspace(tmp_path):
    from tapqir_amd.utils.dataset import save
    from tapqir_amd.utils.simulate import TEST_PARAMS, simulate

    cd, ref = tmp_path / "sharded", tmp_path / "one_process"
    for p in (cd, ref):
        p.mkdir()
        save(simulate(2, 6, 5, 1, 14, 0, TEST_PARAMS), p)
    return cd, ref


@pytest.mark.timeout(300)
def test_launch_fit_end_to_end(workspace, monkeypatch):
    from tapqir_amd.models import cosmos
    from tapqir_amd.utils.dataset import load
    from tapqir_amd.utils.safe_load import load_tpqr

    import pandas as pd

    cd, ref = workspace
    monkeypatch.setenv(launch.BACKEND_ENV, "gloo")
    assert launch.launch_fit(cd, 2, SETTINGS, FIT, worker=lf.host_worker) == 0
    assert (cd / ".tapqir" / "world").read_text().split() == ["2"]

    m = cosmos(K=2, device="cpu")  # the one-process fit of the same data
    m.load(ref)
    m._make_engine(engine_cls=HostCheckEngine)
    m.init(0.005, 6, 5)
    m.run(4, progress_bar=lambda it: it)
    m.compute_stats()
    assert m.iter == 4

    merged = load_tpqr(cd / "cosmos_params.tpqr")
    one = load_tpqr(ref / "cosmos_params.tpqr")
    assert lf.signature(merged) == lf.signature(one)
    assert list(merged) == list(one)
    assert "snr" not in merged
    ranks = [load_tpqr(cd / f"rank{r}" / "cosmos_params.tpqr") for r in range(2)]
    lf.assert_merged_is_concatenation(merged, ranks)
    for g in ("gain", "pi", "lamda", "proximity"):
        assert all(torch.equal(merged[g][k], ranks[0][g][k]) for k in ("LL", "UL", "Mean"))
    summary = pd.read_csv(cd / "cosmos_summary.csv", index_col=0)
    assert list(summary.index) == list(pd.read_csv(ref / "cosmos_summary.csv", index_col=0).index)
    lf.assert_classification_rows(summary, merged["z_map"], load(cd))
    lf.assert_final_state_agrees(cd, m, 2)  # after all four steps

    # stats through the launcher: the ranks load their checkpoints (the final state of the fit), recompute and merge.
    # The read-out is seeded and shard-invariant: the fit's own z_probs come back bitwise, and they are those of ONE
    # unsharded engine holding the same checkpoint parameters
    (cd / "cosmos_params.tpqr").unlink()
    assert launch.launch_fit(cd, 2, SETTINGS, dict(FIT, mode="stats", matlab=True), worker=lf.host_worker) == 0
    again = load_tpqr(cd / "cosmos_params.tpqr")
    assert lf.signature(again) == lf.signature(one) and (cd / "cosmos_params.mat").is_file()
    z, th = lf.unsharded_readout_of_rank_checkpoints(cd, 2, lambda data: HostCheckEngine(data, K=2, device="cpu"))
    assert torch.equal(again["z_probs"], z) and torch.equal(again["theta_probs"], th)
    assert torch.equal(again["z_probs"], merged["z_probs"]) and torch.equal(again["theta_probs"], merged["theta_probs"])


# -- 4. supervision (CPU processes only) --------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("fail", ["before", "after"])
def test_a_failing_rank_ends_the_fit(tmp_path, monkeypatch, fail):
    """Rank 1 raises; rank 0 is left waiting for it (rendezvous or barrier) for up to PG_TIMEOUT seconds.  ``launch_fit``
    must notice the failure, end rank 0 and return non-zero BEFORE that timeout would have released rank 0."""
    PG_TIMEOUT = 10.0
    started = []
    real = subprocess.Popen

    def spy(*a, **k):
        p = real(*a, **k)
        started.append(p)
        return p

    monkeypatch.setattr(launch.subprocess, "Popen", spy)
    monkeypatch.setenv(launch.BACKEND_ENV, "gloo")
    t0 = time.time()
    rc = launch.launch_fit(tmp_path, 2, SETTINGS, dict(FIT, fail=fail, pg_timeout=PG_TIMEOUT), worker=lf.failing_worker)
    returned = time.time()
    print(f"fail={fail}: launch_fit returned after {returned - t0:.2f} s (process-group timeout {PG_TIMEOUT} s)")
    assert returned - t0 < PG_TIMEOUT  # start-up of the ranks included: rank 0 cannot have been released by its own timeout
    assert rc != 0
    assert len(started) == 2 and all(p.poll() is not None for p in started)  # nothing it started is alive
    stamp = tmp_path / "waiting_since"
    if stamp.is_file():  # (rank 0 may not even have come up when rank 1 failed at once)
        waited = returned - float(stamp.read_text())
        print(f"fail={fail}: rank 0 had waited {waited:.2f} s of {PG_TIMEOUT} s")
        assert waited < PG_TIMEOUT
    assert started[0].returncode != 0  # rank 0 was ended, it did not finish
    assert launch.read_world(tmp_path) is None  # a launch that failed before any rank held its shard leaves no mark


# -- 5. command line -----------------------------------------------------------------------------------------------------
@pytest.fixture
def no_children(monkeypatch):
    calls = []

    def refuse(*a, **k):
        calls.append(a)
        raise AssertionError("a rank process was started")

    monkeypatch.setattr(launch.subprocess, "Popen", refuse)
    monkeypatch.delenv(launch.BACKEND_ENV, raising=False)
    return calls


def _fit(path, *extra):
    from tapqir_amd.main import app

    return runner.invoke(app, ["--cd", str(path), "fit", "--num-iter", "1", "--no-input", *extra])


def test_cli_gpus_exit_codes(tmp_path, no_children):
    assert _fit(tmp_path, "--gpus", "0", "--cuda").exit_code == 1
    assert _fit(tmp_path, "--gpus", "2", "--cpu").exit_code == 1
    r = _fit(tmp_path, "--gpus", "2", "--cuda", "--model", "crosstalk")
    assert r.exit_code == 1 and "cosmos only" in r.output
    too_many = max(2, torch.cuda.device_count() + 1)
    r = _fit(tmp_path, "--gpus", str(too_many), "--cuda")
    assert r.exit_code == 1 and str(too_many) in r.output and f"{torch.cuda.device_count()} GPU" in r.output
    assert not (tmp_path / ".tapqir" / "world").exists()
    assert no_children == []


def test_cli_refuses_another_world_size(tmp_path, no_children):
    (tmp_path / ".tapqir").mkdir()
    (tmp_path / ".tapqir" / "world").write_text("2\n")
    r = _fit(tmp_path, "--gpus", "3", "--cuda")
    assert r.exit_code == 1 and "--gpus 2" in r.output
    r = _fit(tmp_path, "--cuda")  # a one-process fit next to the rank checkpoints
    assert r.exit_code == 1 and "--gpus 2" in r.output
    from tapqir_amd.main import app

    r = runner.invoke(app, ["--cd", str(tmp_path), "stats", "--cuda", "--no-input"])
    assert r.exit_code == 1 and "--gpus 2" in r.output
    assert (tmp_path / ".tapqir" / "world").read_text() == "2\n"
    assert no_children == []


def test_rank_batch_size_rule():
    assert [launch.rank_batch_size(5, n, 7) for n in (4, 3)] == [2, 2]  # 20 // 7, 15 // 7
    assert launch.rank_batch_size(1, 3, 400) == 1      # at least one
    assert launch.rank_batch_size(1000, 3, 6) == 3     # at most the rank's AOIs (a full batch stays a full batch)


# -- 6. ABI -----------------------------------------------------------------------------------------------------------------
def test_probs_args_layout_matches_the_c_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "tapqir_hip.h"
int main(void) {
  printf("%zu %zu %zu\n", sizeof(tq_probs_args), offsetof(tq_probs_args, seed), offsetof(tq_probs_args, n_offset));
  return 0;
}'''
    (tmp_path / "s.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "s")]).split()]
    P = _lib.ProbsArgs
    assert got == [ctypes.sizeof(P), P.seed.offset, P.n_offset.offset]
    assert P._fields_[-1][0] == "n_offset"  # appended: the callers of the old layout leave it zero
