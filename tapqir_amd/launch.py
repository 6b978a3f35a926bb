"""
``fit --gpus N`` / ``stats --gpus N``: the launcher of an AOI-sharded fit (``tapqir_amd.parallel``) and the merge of
its per-rank outputs into the single ``<name>_params.tpqr`` / ``<name>_summary.csv`` that every reader of Tapqir files
expects.  The reference has no distributed code; all of this is new work.

Three parts:

* ``launch_fit`` -- the PARENT.  It never initialises the GPU.  It starts one fresh process per rank
  (``python -m tapqir_amd.launch <job>``), polls them, and on the first rank that exits non-zero ends the others
  (terminate, up to ``GRACE`` seconds, kill -- exactly the processes it started).  It never restarts a rank.
* ``rank_fit`` -- ONE RANK: device, process group (finite timeout), model, ``parallel.attach``, fit, per-rank
  statistics, barrier, merge on rank 0.
* ``merge_rank_outputs`` -- rank 0, after the barrier: per-unit entries concatenated in rank order (contiguous shards
  keep the AOI order of the data set), global entries checked for bitwise equality, and everything that depends on all
  AOIs recomputed by ``utils.stats.summarise`` from the merged tensors and the full data set's labels.
"""

import json
import logging
import os
import socket
import subprocess
import sys
import time
from pathlib import Path

logger = logging.getLogger(__name__)

BACKEND_ENV = "TAPQIR_AMD_DIST_BACKEND"  # rehearsal hook: "gloo" = ranks share devices, all-reduce staged through the host
WORLD_FILE = "world"                     # <cd>/.tapqir/world: the world size of the sharded fit in this directory
GRACE = 10.0                             # seconds between terminate and kill when a rank has failed
PG_TIMEOUT = 1800.0                      # default timeout (s) of the process group's collectives

# where the AOI axis of every per-unit entry of <name>_params.tpqr is (cosmos.compute_params, utils/stats.unit_stats)
AOI_AXIS = {"background": 0, "height": 1, "width": 1, "x": 1, "y": 1, "m_probs": 1, "z_probs": 0, "theta_probs": 1,
            "z_map": 0, "p_specific": 0, "chi2": 0}
INTERVAL_KEYS = ("LL", "UL", "Mean")


# ---------------------------------------------------------------------------------------------------------------------
# workspace bookkeeping
# ---------------------------------------------------------------------------------------------------------------------
def read_world(cd):
    """World size recorded by the first sharded fit in ``cd`` (``.tapqir/world``), or None."""
    path = Path(cd) / ".tapqir" / WORLD_FILE
    try:
        return int(path.read_text().split()[0])
    except (OSError, ValueError, IndexError):
        return None


def rank_batch_size(nbatch_size, Nt_rank, Nt):
    """AOIs rank r subsamples per step when ``--nbatch-size`` (the GLOBAL number) is ``nbatch_size``:
    ``max(1, nbatch_size * Nt_rank // Nt)`` -- its share in proportion to its AOIs, rounded down, at least one (and, as in a
    one-process fit, at most the AOIs it holds).  ``CosmosEngine._nb_global`` turns it back into the global plate scale."""
    return min(int(Nt_rank), max(1, int(nbatch_size) * int(Nt_rank) // int(Nt)))


def choose_backend(gpus):
    """("nccl" | "gloo", None) or (None, message): RCCL with rank r on device r needs ``gpus`` devices; with fewer the fit
    is refused unless the rehearsal hook asks for gloo (ranks then share devices as ``rank % device_count``)."""
    import torch

    if os.environ.get(BACKEND_ENV, "").lower() == "gloo":
        return "gloo", None
    have = torch.cuda.device_count()  # does not initialise the HIP runtime
    if have < gpus:
        return None, f"--gpus {gpus} but this node exposes {have} GPU(s)"
    return "nccl", None


# ---------------------------------------------------------------------------------------------------------------------
# one rank
# ---------------------------------------------------------------------------------------------------------------------
def rank_fit(rank, world, port, cd, settings, fit_kwargs, engine_cls=None):
    """One rank of ``fit --gpus N`` (``fit_kwargs["mode"] == "fit"``) or ``stats --gpus N`` ("stats").  ``engine_cls``: CPU
    tests pass the host-check engine through a module-level worker of their own."""
    from datetime import timedelta

    import torch
    import torch.distributed as dist

    from tapqir_amd import parallel
    from tapqir_amd.models import models

    cd = Path(cd)
    kw = dict(fit_kwargs)
    backend = kw.get("backend") or choose_backend(world)[0]
    settings = dict(settings)
    dev = None
    if str(settings.get("device", "cpu")).startswith("cuda"):
        index = rank if backend == "nccl" else rank % max(1, torch.cuda.device_count())
        dev = torch.device("cuda", index)
        torch.cuda.set_device(dev)
        settings["device"] = str(dev)
    pg = dict(backend=backend, init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
              timeout=timedelta(seconds=float(kw.get("pg_timeout", PG_TIMEOUT))))
    if backend == "nccl":
        pg["device_id"] = dev
    dist.init_process_group(**pg)
    m = models[kw.get("model", "cosmos")](**settings)
    m.load(cd)
    Nt = m.data.Nt
    if Nt < world:
        raise ValueError(f"--gpus {world} but the data set has {Nt} AOI(s): every rank needs at least one")
    parallel.attach(m)
    if rank == 0:
        # the data are loaded and sharded: from here on the directory holds a fit over `world` ranks.  (A launch that
        # fails before this point -- no data.tpqr, fewer AOIs than ranks, no rendezvous -- leaves no mark.)
        (cd / ".tapqir" / WORLD_FILE).write_text(f"{world}\n")
    m._make_engine(engine_cls=engine_cls)
    nb = rank_batch_size(kw["nbatch_size"], m.data.Nt, Nt)
    if kw.get("mode", "fit") == "fit":
        m.init(kw["learning_rate"], nb, kw["fbatch_size"])
        m.run(kw["num_iter"], progress_bar=None if rank == 0 else (lambda it: it))
        # The ranks' checkpoint files end with the state the statistics below are computed from (run() itself writes a
        # file every 200 iterations): `stats --gpus N` then reproduces them, and a resumed fit goes on from here.  The
        # write is agreed between the ranks and keeps the last file if any rank's state is not finite.
        m._ckpt_file_stale = True
        m._final_state_file()
        logger.info(f"Iteration #{m.iter}: final -ELBO {m.iter_loss!r}")
    else:
        m.load_checkpoint(param_only=True)
        m.nbatch_size, m.fbatch_size = nb, kw["fbatch_size"]
    m.compute_stats(save_matlab=False)  # this rank's AOIs, under rank<r>/
    m._join_checkpoint_writer(close=True)
    dist.barrier(**({"device_ids": [dev.index]} if backend == "nccl" else {}))
    if rank == 0:
        merge_rank_outputs(cd, m.name, world, 0.95, bool(kw.get("matlab")))
    # (reached on success only: a rank that failed leaves at once -- its peers may be inside a collective -- and the
    # launcher ends them)
    dist.destroy_process_group()


# ---------------------------------------------------------------------------------------------------------------------
# merge (rank 0)
# ---------------------------------------------------------------------------------------------------------------------
def merge_ci_stats(ranks):
    """The ``ci_stats`` dict of the whole data set from those of the ranks (in rank order): per-unit entries concatenated
    along their AOI axis, global entries (identical on every rank by construction) taken from rank 0 after a bitwise
    comparison -- a difference raises ValueError naming the parameter.  Plot ranges (``vmin`` / ``vmax``) depend on all
    AOIs and are left out: ``utils.stats.summarise`` computes them from the merged tensors."""
    import torch

    out = {}
    for name, first in ranks[0].items():
        parts = [r[name] for r in ranks]
        if name in AOI_AXIS:
            ax = AOI_AXIS[name]
            if isinstance(first, dict):
                keys = [k for k in first if k not in ("vmin", "vmax")]
                out[name] = {k: torch.cat([p[k] for p in parts], ax) for k in keys}
            else:
                out[name] = torch.cat(parts, ax)
        elif isinstance(first, dict) and all(k in first for k in INTERVAL_KEYS):
            for r, p in enumerate(parts[1:], 1):
                for k in INTERVAL_KEYS:
                    if p[k].dtype != first[k].dtype or not torch.equal(p[k], first[k]):
                        raise ValueError(f"global parameter {name!r} ({k}) differs between rank 0 and rank {r}: the ranks "
                                         f"of a sharded fit hold the same global parameters by construction")
            out[name] = {k: first[k] for k in INTERVAL_KEYS}
        else:
            raise ValueError(f"{name!r}: no merge rule for this entry of the ranks' parameter files")
    return out


def merge_rank_outputs(cd, name, world, CI=0.95, save_matlab=False):
    """Write ``<cd>/<name>_params.tpqr`` (and ``.mat``) and ``<cd>/<name>_summary.csv`` from the ranks' files under
    ``<cd>/rank<r>/``: the key set, shapes and dtypes of a one-process fit of the same data."""
    from tapqir_amd.utils.dataset import load
    from tapqir_amd.utils.safe_load import load_tpqr
    from tapqir_amd.utils.stats import SNR_FILE, summarise, write_stats
    import torch

    cd = Path(cd)
    ranks = [load_tpqr(cd / f"rank{r}" / f"{name}_params.tpqr", map_location="cpu") for r in range(world)]
    snr = torch.cat([load_tpqr(cd / f"rank{r}" / SNR_FILE.format(name=name), map_location="cpu")["snr"]
                     for r in range(world)], 1)
    data = load(cd)  # the FULL data set (CPU): labels, acquisition times
    ci_stats = merge_ci_stats(ranks)
    if ci_stats["z_map"].shape[0] != data.Nt:
        raise ValueError(f"the ranks' files hold {ci_stats['z_map'].shape[0]} AOIs, the data set {data.Nt}")
    summary = summarise(ci_stats, snr, data, CI)
    write_stats(ci_stats, summary, cd, name, save_matlab)
    return ci_stats, summary


# ---------------------------------------------------------------------------------------------------------------------
# parent
# ---------------------------------------------------------------------------------------------------------------------
def _stop(procs):
    """End exactly the processes in ``procs`` that still run: terminate, wait up to GRACE seconds in all, then kill."""
    alive = [p for p in procs if p.poll() is None]
    for p in alive:
        p.terminate()
    deadline = time.monotonic() + GRACE
    for p in alive:
        try:
            p.wait(max(0.0, deadline - time.monotonic()))
        except subprocess.TimeoutExpired:
            p.kill()
    for p in alive:
        p.wait()


def launch_fit(cd, gpus, settings, fit_kwargs, worker=rank_fit):
    """Run ``worker`` as ``gpus`` fresh rank processes on the workspace ``cd`` and supervise them.

    ``settings``: keyword arguments of the model (JSON-able); ``fit_kwargs``: ``mode`` ("fit" | "stats"), ``learning_rate``,
    ``nbatch_size`` (global), ``fbatch_size``, ``num_iter``, ``matlab``, ``model`` and optionally ``pg_timeout`` (seconds).
    ``worker`` is a module-level function ``(rank, world, port, cd, settings, fit_kwargs)``; it is imported by name in the
    rank processes.  Returns 0 when every rank exited with 0, else 1.  Nothing here touches the GPU."""
    cd, gpus = Path(cd), int(gpus)
    have = read_world(cd)
    if have is not None and have != gpus:
        logger.error(f"{cd} holds a fit sharded over {have} ranks (.tapqir/{WORLD_FILE}): pass --gpus {have}, not --gpus {gpus}")
        return 1
    if have is None and fit_kwargs.get("mode", "fit") == "stats":
        logger.error(f"{cd} holds no sharded fit (.tapqir/{WORLD_FILE} is missing): run `fit --gpus {gpus}` first")
        return 1
    backend, why = choose_backend(gpus)
    if backend is None:
        logger.error(f"{why}: a sharded fit runs one rank per GPU ({BACKEND_ENV}=gloo rehearses it on fewer)")
        return 1
    (cd / ".tapqir").mkdir(exist_ok=True)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]

    env = dict(os.environ)
    # the ranks import this package from where this process did, and the worker's module (a test's) from its own directory;
    # nothing else of this process's sys.path is handed on
    paths = [str(Path(__file__).resolve().parents[1])]
    if worker.__module__.split(".")[0] != "tapqir_amd":
        paths.append(str(Path(sys.modules[worker.__module__].__file__).resolve().parent))
    env["PYTHONPATH"] = os.pathsep.join(paths + [p for p in env.get("PYTHONPATH", "").split(os.pathsep) if p])
    if backend == "nccl":
        # the all-reduce through torch.distributed: RCCL on the launch stream has not run with more than one rank
        env.setdefault("TAPQIR_AMD_RCCL_DIRECT", "0")
    job = {"world": gpus, "port": port, "cd": str(cd), "settings": settings, "fit_kwargs": dict(fit_kwargs, backend=backend),
           "worker": f"{worker.__module__}:{worker.__qualname__}"}
    procs, logs = [], []
    try:
        for r in range(gpus):
            out = None  # rank 0: this process's console
            if r:
                (cd / ".tapqir" / f"rank{r}").mkdir(parents=True, exist_ok=True)
                out = open(cd / ".tapqir" / f"rank{r}" / "log", "ab")
                logs.append(out)
            procs.append(subprocess.Popen([sys.executable, "-m", "tapqir_amd.launch", json.dumps(dict(job, rank=r))],
                                          env=env, stdin=subprocess.DEVNULL, stdout=out, stderr=out))
        while True:
            codes = [p.poll() for p in procs]
            failed = [r for r, c in enumerate(codes) if c not in (None, 0)]
            if failed:
                logger.error(f"rank {failed[0]} exited with status {codes[failed[0]]}: ending the other ranks")
                return 1
            if all(c == 0 for c in codes):
                return 0
            time.sleep(0.05)
    finally:
        _stop(procs)  # (also on KeyboardInterrupt: no rank outlives its launcher)
        for f in logs:
            f.close()


# ---------------------------------------------------------------------------------------------------------------------
# entry point of a rank process
# ---------------------------------------------------------------------------------------------------------------------
def _rank_logging(cd, rank):
    """Every rank: INFO lines tagged with the rank on stdout (rank 0: the console; the others: .tapqir/rank<r>/log) and
    its own .tapqir/rank<r>/loginfo.  (.tapqir/loginfo stays the launching process's file.)"""
    tp = cd / ".tapqir" / f"rank{rank}"
    tp.mkdir(parents=True, exist_ok=True)
    ch = logging.StreamHandler(sys.stdout)
    ch.setLevel(logging.INFO)
    ch.setFormatter(logging.Formatter(f"rank {rank} - %(levelname)s - %(message)s"))
    fh = logging.FileHandler(tp / "loginfo")
    fh.setLevel(logging.DEBUG)
    fh.setFormatter(logging.Formatter(fmt=f"%(asctime)s - rank {rank} - %(levelname)s - %(message)s", datefmt="%m/%d/%Y %I:%M %p"))
    for name in ("tapqir_amd", "tapqir"):
        lg = logging.getLogger(name)
        lg.setLevel(logging.DEBUG)
        lg.addHandler(ch)
        lg.addHandler(fh)


def _rank_main(job):
    import importlib

    rank, cd = int(job["rank"]), Path(job["cd"])
    _rank_logging(cd, rank)
    log = logging.getLogger("tapqir_amd.launch")
    try:
        module, _, attr = job["worker"].partition(":")
        worker = importlib.import_module(module)
        for part in attr.split("."):
            worker = getattr(worker, part)
        worker(rank, int(job["world"]), int(job["port"]), str(cd), job["settings"], job["fit_kwargs"])
    except BaseException:
        log.exception(f"rank {rank} failed")
        logging.shutdown()
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(1)  # no unwinding: nothing may wait for a process group whose other ranks are being ended
    return 0


if __name__ == "__main__":
    sys.exit(_rank_main(json.loads(sys.argv[1])))
