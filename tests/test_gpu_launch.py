"""
``fit --gpus N`` on the GPU (tapqir_amd/launch.py): the posterior read-out of libtapqir_hip.so keyed by global AOI
index, and the command line end to end -- two ranks, their merged output files, ``stats --gpus 2`` -- as a rehearsal
over gloo on one GPU (both ranks on cuda:0, the all-reduce staged through the host) and, where the box has two GPUs,
over RCCL with one GPU per rank.
"""

import os
import shutil
import subprocess
import sys

import pytest
import torch
from typer.testing import CliRunner

import launch_fixture as lf
from tapqir_amd import _lib
from tapqir_amd.models.engine import CosmosEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


# -- A. read-out through libtapqir_hip.so ------------------------------------------------------------------------------
def _make(K):
    return lambda data, **kw: CosmosEngine(data, K=K, device="cuda:0", seed=5, **kw)


@pytest.mark.parametrize("N,K,all_on,worlds", lf.READOUT_CASES, ids=lf.READOUT_IDS)
def test_readout_is_shard_invariant(N, K, all_on, worlds):
    d, o = lf.readout_problem(N, K, all_on)
    full = lf.full_engine(_make(K), d, o)
    assert full.lib is _lib.load()  # the HIP library, not a host build
    z, th = lf.readout(full)
    assert float(z[..., 1].max()) > 0
    for world in worlds:
        zs, ths = lf.sharded_readout(_make(K), d, full, world)
        assert torch.equal(zs, z), world
        assert torch.equal(ths, th), world


def test_zero_offset_is_the_old_call():
    """``n_offset = 0`` equals, bitwise, a call whose argument block never mentions the new field (zero-initialised: what
    a caller of the previous layout passes)."""
    K = 2
    d, o = lf.readout_problem(6, K, False)
    eng = lf.full_engine(_make(K), d, o)
    assert eng.n_offset == 0
    z, th = lf.readout(eng)
    gsz, bsz = eng.struct_sizes()
    f32, dev, S = torch.float32, eng.device, lf.PARTICLES
    ws = [torch.zeros(S * gsz // 4, dtype=f32, device=dev), torch.zeros(S * bsz // 8, dtype=torch.float64, device=dev),
          torch.zeros(eng.Nt, eng.F, eng.C, 2, dtype=f32, device=dev), torch.zeros(K, eng.Nt, eng.F, eng.C, dtype=f32, device=dev)]
    a = _lib.ProbsArgs()
    a.params, a.is_ontarget = _lib.ptr(eng.params), _lib.ptr(eng.is_ontarget)
    a.globals_p, a.gbase_p, a.z_probs, a.theta_probs = (_lib.ptr(t) for t in ws)
    a.Nt, a.F, a.C, a.P, a.K = eng.Nt, eng.F, eng.C, eng.P, K
    a.particles, a.draw, a.eps, a.seed = S, 1, eng.eps, eng.seed + 0x5EED
    eng.run_probs(a)
    torch.cuda.synchronize()
    assert torch.equal(ws[2].cpu(), z) and torch.equal(ws[3].cpu(), th)


# -- B / C. command line end to end ---------------------------------------------------------------------------------------
def _cli(cd, *args, env):
    return subprocess.run([sys.executable, "-m", "tapqir_amd", "--cd", str(cd), *args], env=env, cwd=ROOT, timeout=300,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


FIT_ARGS = ["--cuda", "--num-iter", "4", "--nbatch-size", "6", "--fbatch-size", "5", "--no-input"]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("backend", ["gloo", "nccl"])
def test_cli_fit_gpus_2(tmp_path, backend):
    if backend == "nccl" and torch.cuda.device_count() < 2:
        pytest.skip("RCCL needs one GPU per rank; this box has one")
    import pandas as pd

    from tapqir_amd.main import app
    from tapqir_amd.utils.dataset import load, save
    from tapqir_amd.utils.safe_load import load_tpqr
    from tapqir_amd.utils.simulate import TEST_PARAMS, simulate

    cd, ref = tmp_path / "sharded", tmp_path / "one_process"
    cd.mkdir()
    ref.mkdir()
    save(simulate(2, 6, 5, 1, 14, 0, TEST_PARAMS), cd)
    shutil.copy(cd / "data.tpqr", ref / "data.tpqr")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("TAPQIR_AMD_DIST_BACKEND", None)
    if backend == "gloo":
        env["TAPQIR_AMD_DIST_BACKEND"] = "gloo"

    r = _cli(cd, "fit", "--gpus", "2", *FIT_ARGS, env=env)
    assert r.returncode == 0, r.stdout
    assert (cd / ".tapqir" / "world").read_text().split() == ["2"]
    # the one-process fit of a copy of the directory, with the command's settings, kept in this process so that its state
    # after the last step can be compared (its checkpoint FILE holds iteration 0: run() writes one every 200 iterations)
    from tapqir_amd.main import PRIOR_DEFAULTS
    from tapqir_amd.models import models

    m = models["cosmos"](S=1, K=2, device="cuda", dtype="double", priors={k: float(v) for k, v in PRIOR_DEFAULTS.items()})
    m.load(ref)
    m.init(0.005, 6, 5)
    m.run(4, progress_bar=lambda it: it)
    m.compute_stats()
    assert m.iter == 4

    merged = load_tpqr(cd / "cosmos_params.tpqr")
    one = load_tpqr(ref / "cosmos_params.tpqr")
    assert lf.signature(merged) == lf.signature(one)
    assert list(merged) == list(one)
    ranks = [load_tpqr(cd / f"rank{k}" / "cosmos_params.tpqr") for k in range(2)]
    lf.assert_merged_is_concatenation(merged, ranks)
    summary = pd.read_csv(cd / "cosmos_summary.csv", index_col=0)
    assert list(summary.index) == list(pd.read_csv(ref / "cosmos_summary.csv", index_col=0).index)
    lf.assert_classification_rows(summary, merged["z_map"], load(cd))
    lf.assert_final_state_agrees(cd, m, 2)  # after all four steps

    # ttfb and dwelltime read the merged files unchanged
    cli = CliRunner()
    r = cli.invoke(app, ["--cd", str(cd), "ttfb", "--cuda", "--num-samples", "10", "--num-iter", "50", "--no-input"])
    assert r.exit_code == 0, r.output
    assert (cd / "cosmos_ttfb-params-channel0.csv").is_file()
    r = cli.invoke(app, ["--cd", str(cd), "dwelltime", "-K", "1", "--cuda", "--num-samples", "10", "--num-iter", "50", "--no-input"])
    assert r.exit_code == 0, r.output
    assert (cd / "cosmos_dwelltime-intervals-channel0.pkl").is_file()

    # stats --gpus 2: the ranks load their checkpoints (which the launcher ended with the fit's final state), recompute
    # their statistics and merge.  The read-out is seeded and shard-invariant: the fit's own z_probs come back bitwise,
    # and they are those of ONE unsharded engine holding the same checkpoint parameters.
    (cd / "cosmos_params.tpqr").unlink()
    r = _cli(cd, "stats", "--gpus", "2", "--cuda", "--nbatch-size", "6", "--fbatch-size", "5", "--matlab", "--no-input", env=env)
    assert r.returncode == 0, r.stdout
    again = load_tpqr(cd / "cosmos_params.tpqr")
    assert lf.signature(again) == lf.signature(merged)
    assert (cd / "cosmos_params.mat").is_file()
    z, th = lf.unsharded_readout_of_rank_checkpoints(cd, 2, lambda data: CosmosEngine(data, K=2, device="cuda:0"))
    assert torch.equal(again["z_probs"], z) and torch.equal(again["theta_probs"], th)
    assert torch.equal(again["z_map"], torch.argmax(z, -1))
    assert torch.equal(again["z_probs"], merged["z_probs"]) and torch.equal(again["theta_probs"], merged["theta_probs"])
