"""Shared pieces of tests/test_launch.py (CPU, host build) and tests/test_gpu_launch.py (libtapqir_hip.so): the
shard-invariance problem of the posterior read-out, the rank workers that ``launch_fit`` imports by name, and the
comparisons of merged output files."""

import types

import numpy as np
import torch

from helpers import make_dataset, make_oracle, oracle_to_engine
from tapqir_amd.models.posterior import compute_probs
from tapqir_amd.parallel import shard_bounds, shard_dataset
from tapqir_amd.utils.dataset import CosmosDataset

PARTICLES = 5
# (N, K, all AOIs on-target, worlds).  6 AOIs / K = 2 is the problem of the sharded-step tests: 3 on-target AOIs, world 2
# splits 3 + 3 and world 4 splits 2, 2, 1, 1 (ranks without an on-target AOI).  N = 2 / K = 1 at world 2 is the smallest
# case in which a shard starts at a non-zero unit offset -- but the simulated sets put their on-target AOIs first and the
# off-target ones are left at zero whatever their streams are keyed by, so with the simulated flags that case (and world 2
# of the first) holds under ANY keying: they check the zero rows and shapes of a shard without an on-target AOI.  The
# all-on-target variants make EVERY shard draw; they, and world 4 of the first case, fail with local-index keys.
READOUT_CASES = [(6, 2, False, (2, 4)), (2, 1, False, (2,)), (6, 2, True, (2, 4)), (2, 1, True, (2,))]
READOUT_IDS = ["N6_K2", "N2_K1", "N6_K2_all_ontarget", "N2_K1_all_ontarget"]


def readout_problem(N, K, all_on):
    d = make_dataset(N=N, F=5, K=K)
    o = make_oracle(d, K)  # one perturbed parameter set
    if all_on:
        d = CosmosDataset(d.images, d.xy, torch.ones(N, dtype=torch.bool), offset_samples=d.offset.samples,
                          offset_weights=d.offset.weights)
    return d, o


def copy_shard_params(full, eng, lo, hi):
    """The slice [lo, hi) of the AOIs of ``full``'s parameters into the shard engine ``eng``."""
    fv, sv = full.named("params"), eng.named("params")
    for n in sv:
        sv[n].copy_(fv[n][:, lo:hi] if sv[n].dim() == 4 else (fv[n][lo:hi] if sv[n].dim() == 3 else fv[n]))


def readout(eng):
    z, th = compute_probs(types.SimpleNamespace(engine=eng), particles=PARTICLES)
    return z.cpu().clone(), th.cpu().clone()


def sharded_readout(make_engine, d, full, world):
    """``compute_probs`` of every shard of ``d`` (engines built by ``make_engine(data, **kw)`` with the slice of ``full``'s
    parameters), concatenated in rank order along the AOI axis."""
    zs, ths = [], []
    for r in range(world):
        sub, lo, Ntg = shard_dataset(d, r, world)
        eng = make_engine(sub, n_offset=lo, Nt_global=Ntg)
        copy_shard_params(full, eng, lo, lo + sub.images.shape[0])
        z, th = readout(eng)
        zs.append(z)
        ths.append(th)
    return torch.cat(zs, 0), torch.cat(ths, 1)


def full_engine(make_engine, d, o):
    full = make_engine(d)
    oracle_to_engine(o, full)
    return full


# -- rank workers (imported by name in the rank processes) ------------------------------------------------------------
def host_worker(rank, world, port, cd, settings, fit_kwargs):
    """``rank_fit`` on the g++ host build of the kernels' math: the launcher, the sharding and the merge without a GPU."""
    from helpers import HostCheckEngine
    from tapqir_amd.launch import rank_fit

    rank_fit(rank, world, port, cd, settings, fit_kwargs, engine_cls=HostCheckEngine)


def failing_worker(rank, world, port, cd, settings, fit_kwargs):
    """Rank 1 raises before or after the process group is up (``fit_kwargs["fail"]``); rank 0 then waits for a peer that
    is gone, for at most the process group's timeout.  Rank 0 records when it started to wait."""
    import time
    from datetime import timedelta
    from pathlib import Path

    import torch.distributed as dist

    if rank == 1 and fit_kwargs["fail"] == "before":
        raise RuntimeError("rank 1 fails before init_process_group")
    if rank == 0:
        (Path(cd) / "waiting_since").write_text(repr(time.time()))
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
                            timeout=timedelta(seconds=fit_kwargs["pg_timeout"]))
    if rank == 1:
        raise RuntimeError("rank 1 fails after init_process_group")
    (Path(cd) / "waiting_since").write_text(repr(time.time()))
    dist.barrier()


# -- comparisons of output files ---------------------------------------------------------------------------------------
def signature(obj):
    """Key set, shapes and dtypes of a ``<name>_params.tpqr`` payload (nested dicts of tensors and numbers)."""
    if isinstance(obj, dict):
        return {k: signature(v) for k, v in obj.items()}
    if isinstance(obj, torch.Tensor):
        return ("tensor", tuple(obj.shape), obj.dtype)
    if isinstance(obj, np.ndarray):
        return ("ndarray", obj.shape, obj.dtype)
    return type(obj).__name__


def assert_merged_is_concatenation(merged, ranks):
    from tapqir_amd.launch import AOI_AXIS

    for name, ax in AOI_AXIS.items():
        if isinstance(merged[name], dict):
            for k in ("LL", "UL", "Mean", "values"):
                if k in merged[name]:
                    assert torch.equal(merged[name][k], torch.cat([r[name][k] for r in ranks], ax)), (name, k)
        else:
            assert torch.equal(merged[name], torch.cat([r[name] for r in ranks], ax)), name


def assert_classification_rows(summary, z_map, data):
    """The classification rows of a merged summary against sklearn on the merged ``z_map`` and the FULL labels."""
    from sklearn.metrics import confusion_matrix, matthews_corrcoef, precision_score, recall_score

    on = data.is_ontarget.cpu()
    pred = (z_map[on] > 0).numpy().ravel().astype(int)
    true = np.asarray(data.labels["z"])[: data.N].ravel().astype(int)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = {"MCC": matthews_corrcoef(true, pred), "Recall": recall_score(true, pred, zero_division=0),
                "Precision": precision_score(true, pred, zero_division=0)}
    tn, fp, fn, tp = confusion_matrix(true, pred, labels=(0, 1)).ravel()
    want.update(TN=tn, FP=fp, FN=fn, TP=tp)
    for row, v in want.items():
        assert float(summary.loc[row, "Mean"]) == float(v), (row, summary.loc[row, "Mean"], v)


def final_elbo(loginfo):
    """The -ELBO of the last step, as the rank logged it (``repr`` of the float)."""
    import re

    found = re.findall(r"final -ELBO (\S+)", open(loginfo).read())
    assert found, loginfo
    return float(found[-1])


def assert_final_state_agrees(cd, model, world, name="cosmos"):
    """The ranks' state AFTER THE LAST STEP of ``fit --gpus N`` (their checkpoint files, which the launcher ends with the
    final state, and the -ELBO of the last step from their logs) against the one-process ``model`` that ran the same
    number of iterations on the same data, at the bounds of the sharded-step tests for four steps
    (tests/test_gpu_multirank.py: ELBO 2e-6 relative, unconstrained parameters 5e-6 absolute)."""
    from tapqir_amd.utils.safe_load import load_tpqr

    model.engine.join()
    ref = {n: v.detach().cpu().double() for n, v in model.engine.named("params").items()}
    elbo, Nt = float(model.iter_loss), model.data.Nt
    for r in range(world):
        ck = load_tpqr(cd / ".tapqir" / f"rank{r}" / f"{name}_model.tpqr", map_location="cpu")
        assert ck["iter"] == model.iter
        got = final_elbo(cd / ".tapqir" / f"rank{r}" / "loginfo")
        print(f"rank {r}: final -ELBO {got!r} one-process {elbo!r} rel {abs(got - elbo) / abs(elbo):.2e}")
        assert abs(got - elbo) <= 2e-6 * abs(elbo)
        lo, hi = shard_bounds(Nt, r, world)
        worst = 0.0
        for n, v in ck["params"]["params"].items():
            fp = ref[n]
            want = fp[:, lo:hi] if v.dim() == 4 else (fp[lo:hi] if v.dim() == 3 else fp)
            err = float((v.double() - want).abs().max())
            worst = max(worst, err)
            assert err <= 5e-6, (r, n, err)
        print(f"rank {r}: worst |unconstrained parameter - one-process| {worst:.2e}")


def unsharded_readout_of_rank_checkpoints(cd, world, make_engine, name="cosmos"):
    """``(z_probs, theta_probs)`` of ONE engine over the whole data set of ``cd`` (``make_engine(data)``) holding the
    parameters of the ranks' checkpoints, at the read-out's default particle count: what ``stats --gpus N`` must
    reproduce bitwise from the same files, however the AOIs are split."""
    from tapqir_amd.utils.dataset import load
    from tapqir_amd.utils.safe_load import load_tpqr

    cks = [load_tpqr(cd / ".tapqir" / f"rank{r}" / f"{name}_model.tpqr", map_location="cpu")["params"]["params"]
           for r in range(world)]
    eng = make_engine(load(cd))
    for n, v in eng.named("params").items():
        parts = [c[n] for c in cks]
        full = torch.cat(parts, 1) if v.dim() == 4 else (torch.cat(parts, 0) if v.dim() == 3 else parts[0])
        v.copy_(full.reshape(v.shape).to(v.dtype))
    z, th = compute_probs(types.SimpleNamespace(engine=eng))
    return z.cpu().clone(), th.cpu().clone()
