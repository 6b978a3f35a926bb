"""
Command line of the MI355X build: the ``glimpse`` / ``fit`` / ``stats`` / ``ttfb`` / ``dwelltime`` / ``log`` commands
of ``tapqir`` (tapqir/main.py:66-318, 321-576, 873-884, 926-1147, 1150-1384, 1387-1488) over the same workspace (``<cd>/.tapqir/config.yaml``, ``loginfo``, ``<model>_model.tpqr``,
``<model>_params.tpqr``, ``<model>_summary.csv``).  Options, defaults and exit codes (0 / 1) follow the reference;
``--cpu`` exits with 1 because the SVI step has no CPU path here.  ``glimpse`` takes its inputs from flags or from
``config.yaml`` (there are no interactive prompts).  ``ttfb`` (tapqir/main.py:926-1147) samples first-binding times and
fits the association kinetics on the GPU from ``data.tpqr`` and ``<model>_params.tpqr``; ``dwelltime``
(tapqir/main.py:1150-1384) samples bound and unbound intervals and fits the dissociation and association rates there too.
Plotting (``show``) is outside the scope of this build.

    python -m tapqir_amd --cd <dir> fit --model cosmos --cuda --num-iter 0 --no-input
"""

import logging
import sys
from enum import Enum
from pathlib import Path
from typing import List, Optional

import typer
import yaml

from tapqir_amd import __version__

app = typer.Typer()

PRIOR_DEFAULTS = {  # main.py:1431-1439
    "background_mean_std": 1000, "background_std_std": 100, "lamda_rate": 1, "height_std": 10000,
    "width_min": 0.75, "width_max": 2.25, "proximity_rate": 1, "gain_std": 50,
}
CONFIG_DEFAULTS = {  # main.py:1423-1445
    "P": 14, "nbatch-size": 10, "fbatch-size": 512, "learning-rate": 0.005, "num-channels": 1, "cuda": True,
    "matlab": False, "priors": dict(PRIOR_DEFAULTS), "offset-x": 10, "offset-y": 10, "offset-P": 30, "bin-size": 1,
}
DEFAULTS = {"cd": Path.cwd()}


class avail_models(str, Enum):  # main.py:27-28: the keys of tapqir.models.models
    cosmos = "cosmos"
    crosstalk = "crosstalk"
    hmm = "cosmos+hmm"


def _default(key):
    return lambda: DEFAULTS.get(key, CONFIG_DEFAULTS.get(key))


def _version(value: bool):
    if value:
        typer.echo(f"Tapqir-AMD version: {__version__}")
        raise typer.Exit()


def _write_config(cd: Path):
    with open(cd / ".tapqir" / "config.yaml", "w") as f:
        yaml.dump({k: v for k, v in DEFAULTS.items() if k != "cd"}, f, sort_keys=False)


GPUS_HELP = ("Number of GPUs: N > 1 shards the AOIs contiguously over N rank processes, one per GPU (cosmos only).  "
             "--nbatch-size stays the global number: rank r subsamples max(1, nbatch_size * Nt_r // Nt) of its Nt_r AOIs "
             "per step (Nt: all AOIs).")


def _check_gpus(command, gpus, model, cuda, logger):
    """The checks `fit` and `stats` share for --gpus, before anything is written or started.  Returns True for a sharded
    run (N > 1); a one-process run in a directory that holds a sharded fit is refused."""
    from tapqir_amd.launch import read_world

    if gpus < 1:
        logger.error(f"{command}: --gpus must be at least 1, got {gpus}")
        raise typer.Exit(1)
    if gpus == 1:
        world = read_world(DEFAULTS["cd"])
        if world is not None:
            logger.error(f"{command}: this directory holds a fit sharded over {world} ranks (.tapqir/world, rank "
                         f"checkpoints under .tapqir/rank<r>): pass --gpus {world}")
            raise typer.Exit(1)
        return False
    if not cuda:
        logger.error(f"{command}: --gpus {gpus} needs the AMD GPUs (--cuda): the SVI step has no CPU path")
        raise typer.Exit(1)
    if model.value != "cosmos":
        logger.error(f"{command}: --gpus {gpus} is not available for the {model.value} model (cosmos only)")
        raise typer.Exit(1)
    return True


def _build_model(name: str, logger, **settings):
    from tapqir_amd.exceptions import HipExtensionError
    from tapqir_amd.models import models

    try:
        return models[name](**settings)
    except (NotImplementedError, HipExtensionError):
        logger.exception(f"Model {name} is not available in this build")
        return None


@app.command()
def glimpse(
    dataset: str = typer.Option(_default("dataset"), help="Dataset name"),
    P: int = typer.Option(_default("P"), "--aoi-size", "-P", min=5, max=50, help="AOI image size - number of pixels along the axis"),
    offset_x: int = typer.Option(_default("offset-x"), "--offset-x", min=0, help="x-axis position of the top-left corner of the offset region"),
    offset_y: int = typer.Option(_default("offset-y"), "--offset-y", min=0, help="y-axis position of the top-left corner of the offset region"),
    offset_P: int = typer.Option(_default("offset-P"), "--offset-P", min=5, help="Offset region size - number of pixels along the axis"),
    bin_size: int = typer.Option(_default("bin-size"), "--bin-size", min=1, max=21, help="Offset histogram bin size (odd number)"),
    frame_range: bool = typer.Option(_default("frame-range"), help="Specify frame range."),
    frame_start: Optional[int] = typer.Option(_default("frame-start"), min=0, help="Starting frame."),
    frame_end: Optional[int] = typer.Option(_default("frame-end"), min=1, help="Ending frame."),
    use_offtarget: bool = typer.Option(_default("use-offtarget"), help="Use off-target AOI locations."),
    num_channels: int = typer.Option(_default("num-channels"), "--num-channels", "-C", min=1, help="Number of color channels"),
    name: Optional[List[str]] = typer.Option(None, help="Channel name (once per channel)"),
    glimpse_folder: Optional[List[Path]] = typer.Option(None, exists=True, file_okay=False, resolve_path=True),
    driftlist: Optional[List[Path]] = typer.Option(None, exists=True, dir_okay=False, resolve_path=True),
    ontarget_aoiinfo: Optional[List[Path]] = typer.Option(None, exists=True, dir_okay=False, resolve_path=True),
    offtarget_aoiinfo: Optional[List[Path]] = typer.Option(None, exists=True, dir_okay=False, resolve_path=True),
    ontarget_labels: Optional[List[Path]] = typer.Option(None, exists=True, dir_okay=False, resolve_path=True),
    offtarget_labels: Optional[List[Path]] = typer.Option(None, exists=True, dir_okay=False, resolve_path=True),
    overwrite: bool = typer.Option(True, "--overwrite", "-w", help="Overwrite defaults values."),
    no_input: bool = typer.Option(False, "--no-input", help="Accepted for compatibility (there are no prompts)."),
    labels: bool = typer.Option(False, "--labels", "-l", help="Add on-target binding labels."),
    progress_bar=None,
):
    """
    Extract AOIs from raw glimpse images (tapqir/main.py:66-318) into ``<cd>/data.tpqr``.

    Needs, per colour channel: the header/glimpse folder, the aoiinfo file of the target molecules (on-target AOIs),
    optionally the aoiinfo file of the off-target control locations, and the driftlist file.  Values not given as flags
    are taken from ``.tapqir/config.yaml`` (``channels: [{name, glimpse-folder, driftlist, ontarget-aoiinfo, ...}]``).
    """
    from tapqir_amd.exceptions import HipExtensionError
    from tapqir_amd.imscroll import read_glimpse

    cd = DEFAULTS["cd"]
    logger = logging.getLogger("tapqir")
    DEFAULTS.update({"dataset": dataset, "P": P, "offset-P": offset_P, "offset-x": offset_x, "offset-y": offset_y,
                     "bin-size": bin_size, "frame-range": bool(frame_range), "frame-start": frame_start,
                     "frame-end": frame_end, "use-offtarget": bool(use_offtarget), "num-channels": num_channels,
                     "labels": labels})
    flags = {"name": name, "glimpse-folder": glimpse_folder, "driftlist": driftlist, "ontarget-aoiinfo": ontarget_aoiinfo,
             "offtarget-aoiinfo": offtarget_aoiinfo, "ontarget-labels": ontarget_labels, "offtarget-labels": offtarget_labels}
    channels = [dict(ch) for ch in DEFAULTS.get("channels") or []]
    for c in range(num_channels):
        if len(channels) < c + 1:
            channels.append({})
        for key, values in flags.items():
            if values and c < len(values):
                channels[c][key] = str(values[c])
        needed = ["name", "glimpse-folder", "driftlist", "ontarget-aoiinfo"] + (["offtarget-aoiinfo"] if use_offtarget else [])
        missing = [key for key in needed if channels[c].get(key) is None]
        if missing:
            logger.error(f"Channel #{c}: missing {', '.join('--' + k for k in missing)} (flag or config.yaml)")
            raise typer.Exit(1)
        if labels:
            channels[c].setdefault("ontarget-labels", None)
            channels[c].setdefault("offtarget-labels", None)
    DEFAULTS["channels"] = channels[:num_channels]
    if overwrite:
        _write_config(cd)

    logger.info("Extracting AOIs ...")
    try:
        read_glimpse(path=cd, progress_bar=progress_bar, **{k: v for k, v in DEFAULTS.items() if k != "cd"})
    except HipExtensionError:
        logger.exception("Failed to extract AOIs: the extraction needs an AMD GPU and the built HIP library")
        raise typer.Exit(1)
    logger.info("Extracting AOIs: Done")


@app.command()
def fit(
    model: avail_models = typer.Option("cosmos", help="Tapqir model"),
    S: int = typer.Option(1, "--num-states", "-S", help="Number of spot states"),
    cuda: bool = typer.Option(_default("cuda"), "--cuda/--cpu", help="Run computations on GPU or CPU", show_default=False),
    nbatch_size: int = typer.Option(_default("nbatch-size"), "--nbatch-size", "-nbs", help="AOI batch size"),
    fbatch_size: int = typer.Option(_default("fbatch-size"), "--fbatch-size", "-fbs", help="Frame batch size"),
    learning_rate: float = typer.Option(_default("learning-rate"), "--learning-rate", "-lr", help="Learning rate"),
    num_iter: int = typer.Option(0, "--num-iter", "-it", help="Number of iterations (0 = until converged)"),
    k_max: int = typer.Option(2, "--k-max", "-k", help="Maximum number of spots per image"),
    matlab: bool = typer.Option(_default("matlab"), "--matlab", help="Save parameters in matlab format"),
    gpus: int = typer.Option(1, "--gpus", help=GPUS_HELP),
    funsor: bool = typer.Option(False, "--funsor/--pyro", help="Accepted for compatibility; ignored"),
    pykeops: bool = typer.Option(True, "--pykeops/--no-pykeops", help="Accepted for compatibility; ignored"),
    overwrite: bool = typer.Option(True, "--overwrite", "-w", help="Overwrite defaults values."),
    no_input: bool = typer.Option(False, "--no-input", help="Accepted for compatibility (there are no prompts)."),
    progress_bar=None,
):
    """
    Fit the data to the selected model (cosmos, crosstalk).
    """
    from tapqir_amd.exceptions import CudaOutOfMemoryError, HipExtensionError, TapqirFileNotFoundError

    cd = DEFAULTS["cd"]
    logger = logging.getLogger("tapqir")
    sharded = _check_gpus("fit", gpus, model, cuda, logger)
    settings = {"S": S, "K": k_max, "device": "cuda" if cuda else "cpu", "dtype": "double", "use_pykeops": pykeops,
                "priors": {k: float(v) for k, v in DEFAULTS.get("priors", PRIOR_DEFAULTS).items()}}
    if overwrite:
        DEFAULTS.update({"cuda": cuda, "nbatch-size": nbatch_size, "fbatch-size": fbatch_size,
                         "learning-rate": learning_rate, "matlab": matlab})
        _write_config(cd)

    if sharded:
        from tapqir_amd.launch import launch_fit

        logger.info(f"Fitting the data on {gpus} GPUs ...")
        if launch_fit(cd, gpus, settings, {"mode": "fit", "model": model.value, "learning_rate": learning_rate,
                                            "nbatch_size": nbatch_size, "fbatch_size": fbatch_size, "num_iter": num_iter,
                                            "matlab": bool(matlab)}):
            logger.error("Failed to fit the data")
            raise typer.Exit(1)
        logger.info("Fitting the data and computing stats: Done")
        return

    logger.info("Fitting the data ...")
    m = _build_model(model.value, logger, **settings)
    if m is None:
        raise typer.Exit(1)
    try:
        m.load(cd)
    except TapqirFileNotFoundError as err:
        logger.exception(f"Failed to load {err.name} file")
        raise typer.Exit(1)
    try:
        m.init(learning_rate, nbatch_size, fbatch_size)
        m.run(num_iter, progress_bar=progress_bar)
    except HipExtensionError:
        logger.exception("Failed to fit the data: the SVI step needs an AMD GPU (--cuda) and the built HIP library")
        raise typer.Exit(1)
    except CudaOutOfMemoryError:
        logger.exception("Failed to fit the data")
        raise typer.Exit(1)
    logger.info("Fitting the data: Done")

    logger.info("Computing stats ...")
    try:
        m.compute_stats(save_matlab=matlab)
    except CudaOutOfMemoryError:
        logger.exception("Failed to compute stats")
        raise typer.Exit(1)
    logger.info("Computing stats: Done")


@app.command()
def stats(
    model: avail_models = typer.Option("cosmos", help="Tapqir model"),
    cuda: bool = typer.Option(_default("cuda"), "--cuda/--cpu", help="Run computations on GPU or CPU", show_default=False),
    nbatch_size: int = typer.Option(_default("nbatch-size"), "--nbatch-size", "-nbs", help="AOI batch size"),
    fbatch_size: int = typer.Option(_default("fbatch-size"), "--fbatch-size", "-fbs", help="Frame batch size"),
    matlab: bool = typer.Option(_default("matlab"), "--matlab", help="Save parameters in matlab format"),
    gpus: int = typer.Option(1, "--gpus", help=GPUS_HELP),
    funsor: bool = typer.Option(False, "--funsor/--pyro", help="Accepted for compatibility; ignored"),
    no_input: bool = typer.Option(False, "--no-input", help="Accepted for compatibility (there are no prompts)."),
):
    """
    Compute credible intervals and classification statistics from the last checkpoint.
    """
    from tapqir_amd.exceptions import CudaOutOfMemoryError, HipExtensionError, TapqirFileNotFoundError

    cd = DEFAULTS["cd"]
    logger = logging.getLogger("tapqir")
    if _check_gpus("stats", gpus, model, cuda, logger):
        from tapqir_amd.launch import launch_fit

        logger.info(f"Computing stats on {gpus} GPUs ...")
        if launch_fit(cd, gpus, {"device": "cuda", "dtype": "double"},
                      {"mode": "stats", "model": model.value, "nbatch_size": nbatch_size, "fbatch_size": fbatch_size,
                       "matlab": bool(matlab)}):
            logger.error("Failed to compute stats")
            raise typer.Exit(1)
        logger.info("Computing stats: Done")
        return
    logger.info("Computing stats ...")
    m = _build_model(model.value, logger, device="cuda" if cuda else "cpu", dtype="double")
    if m is None:
        raise typer.Exit(1)
    try:
        m.load(cd)
    except TapqirFileNotFoundError:
        logger.exception("Failed to load data file")
        raise typer.Exit(1)
    try:
        m.load_checkpoint(param_only=True)
        m.nbatch_size = nbatch_size
        m.fbatch_size = fbatch_size
        m.compute_stats(save_matlab=matlab)
    except TapqirFileNotFoundError as err:
        logger.exception(f"Failed to load {err.name} file")
        raise typer.Exit(1)
    except HipExtensionError:
        logger.exception("Failed to compute stats: the posterior read-out needs an AMD GPU (--cuda) and the built HIP library")
        raise typer.Exit(1)
    except CudaOutOfMemoryError:
        logger.exception("Failed to compute stats")
        raise typer.Exit(1)
    logger.info("Computing stats: Done")


def _kinetics_inputs(command, model, cuda, progress_bar):
    """The checks `ttfb`, `dwelltime`, `rates` and `smooth` share, in the order the exit-status tests rely on (``--cpu``
    fails before any file is read).  Returns the loaded model, the mask of the on-target AOIs and the progress bar."""
    import torch

    from tapqir_amd.exceptions import TapqirFileNotFoundError
    from tapqir_amd.models import models

    cd = DEFAULTS["cd"]
    logger = logging.getLogger("tapqir")
    if model.value != "cosmos":
        # the reference has no z_sample for crosstalk, and cosmos+hmm is not part of this build
        logger.error(f"{command} is not available for the {model.value} model (cosmos only)")
        raise typer.Exit(1)
    if not cuda:
        logger.error(f"{command} runs on the AMD GPU only (--cuda): the sampler and the fits have no CPU path")
        raise typer.Exit(1)
    m = models[model.value](device="cpu", dtype="float")
    try:
        m.load(cd, data_only=False)
    except TapqirFileNotFoundError as err:
        logger.exception(f"Failed to load {err.name} file")
        raise typer.Exit(1)
    if "z_probs" not in m.params:
        logger.error(f"{m.name}_params.tpqr has no z_probs: run `fit` first")
        raise typer.Exit(1)
    if not torch.cuda.is_available():
        logger.error(f"{command} needs an AMD GPU (--cuda): no HIP device is visible")
        raise typer.Exit(1)
    if progress_bar is None:
        try:
            from tqdm import tqdm as progress_bar
        except Exception:  # pragma: no cover
            progress_bar = None
    mask = m.data.mask[: m.data.N].cpu().bool()
    if not bool(mask.any()):
        logger.error(f"{command}: no on-target AOI is selected by the data mask")
        raise typer.Exit(1)
    return m, mask, progress_bar


def _joint_pair(command, joint, logger):
    """The value of ``--joint A,B`` of `smooth`, `dwelltime` and `ttfb`: two different channel indices (A, B), or exit
    status 1."""
    import re

    match = re.fullmatch(r"\s*(\d+)\s*,\s*(\d+)\s*", joint)
    if not match or int(match.group(1)) == int(match.group(2)):
        logger.error(f"{command}: --joint takes A,B with two different channel indices, got {joint!r}")
        raise typer.Exit(1)
    return int(match.group(1)), int(match.group(2))


def _chain_states(command, model, cuda, smooth, U, B, logger, G=1, joint=None, censored=False):
    """The checks of ``--unbound-states`` / ``--bound-states`` / ``--populations`` / ``--joint`` of `ttfb` and `dwelltime`:
    the bound on the sum of the states, the range of the populations and the value of ``--joint`` where `smooth` checks
    them (after the model, before ``--cpu``), and, once the model and ``--cpu`` have passed, that a chain other than
    (1, 1), more than one population or a joint chain comes with ``--smooth``; then what ``--joint`` does not go with.
    Returns the pair (A, B) of ``--joint``, or None."""
    if model.value != "cosmos":
        return None
    if U + B > 4:
        logger.error(f"{command}: --unbound-states + --bound-states must be at most 4, got {U} + {B}")
        raise typer.Exit(1)
    if not 1 <= G <= 4:
        logger.error(f"{command}: --populations must lie in 1 .. 4, got {G}")
        raise typer.Exit(1)
    pair = None if joint is None else _joint_pair(command, joint, logger)
    if cuda and not smooth and (U, B) != (1, 1):
        logger.error(f"{command}: --unbound-states and --bound-states need --smooth: they choose the chain of `smooth` "
                     f"whose rasters are sampled")
        raise typer.Exit(1)
    if cuda and not smooth and G > 1:
        logger.error(f"{command}: --populations needs --smooth: it chooses the mixture of `smooth --populations` whose "
                     f"rasters are sampled")
        raise typer.Exit(1)
    if pair is None:
        return None
    if cuda and not smooth:
        logger.error(f"{command}: --joint needs --smooth: it chooses the chain of `smooth --joint` whose rasters are sampled")
        raise typer.Exit(1)
    if (U, B) != (1, 1):
        logger.error(f"{command}: --joint samples the chain of two two-state channels: it does not go with --unbound-states / "
                     f"--bound-states other than 1 and 1")
        raise typer.Exit(1)
    if G > 1:
        logger.error(f"{command}: --joint does not go with --populations: the joint chain is fitted to all AOIs")
        raise typer.Exit(1)
    if censored:
        logger.error(f"{command}: --joint does not go with --censored: the censored histograms are not split by the "
                     f"partner's state")
        raise typer.Exit(1)
    return pair


def _smooth_suffix(U, B, G=1):
    """What follows ``smooth`` in the file names of a chain: nothing for the two-state chain, ``-u<U>b<B>`` otherwise, and
    ``-u<U>b<B>g<G>`` for a mixture of G > 1 populations at any (U, B)."""
    if G > 1:
        return f"-u{U}b{B}g{G}"
    return "" if (U, B) == (1, 1) else f"-u{U}b{B}"


def _smoothed_posterior(command, cd, name, mask, logger, U=1, B=1, G=1):
    """``<name>_smooth.tpqr`` (``<name>_smooth-u<U>b<B>.tpqr`` for a chain other than (1, 1), ``<name>_smooth-u<U>b<B>g<G>.tpqr``
    for a mixture of G > 1 populations) for the ``--smooth`` switch of `ttfb` and `dwelltime`: the chain of every channel
    (``theta``, ``prior``), the smoothed ``z_probs`` and the Viterbi path ``z_map``.  Exits with status 1 when the file is
    missing or was written for another selection of AOIs."""
    import torch

    from tapqir_amd.utils.safe_load import load_tpqr

    path = cd / f"{name}_smooth{_smooth_suffix(U, B, G)}.tpqr"
    again = "smooth" if (U, B) == (1, 1) else f"smooth --unbound-states {U} --bound-states {B}"
    if G > 1:
        again += f" --populations {G}"
    if not path.is_file():
        logger.error(f"{command} --smooth needs {path.name}: run `{again}` first")
        raise typer.Exit(1)
    sm = load_tpqr(path)
    if sm["mask"].shape != mask.shape or not torch.equal(sm["mask"].bool(), mask):
        logger.error(f"{command} --smooth: {path.name} was written for another mask of on-target AOIs than the data "
                     f"has now: run `{again}` again")
        raise typer.Exit(1)
    return sm


def _smoothed_filter(sm, c, p_bound, U=1, B=1):
    """The filtered marginals of channel ``c`` under the chain of ``smooth``: one E-step on the fit's ``p_bound`` at the
    stored theta and prior.  Returns (filt, theta) on the device of ``p_bound``: the inputs of the backward sampler."""
    import torch

    from tapqir_amd.utils.mle_analysis import hmm_estep, smooth_estep

    theta = sm["theta"][c].to(device=p_bound.device, dtype=torch.float64)
    if (U, B) == (1, 1):
        return smooth_estep(p_bound, theta, float(sm["prior"][c]))["filt"], theta
    return hmm_estep(p_bound, theta, float(sm["prior"][c]), U, B)["filt"], theta


def _mixture_filter(sm, c, p_bound, mask, U, B, logger):
    """The inputs of the mixture's backward sampler for channel ``c`` from the file of `smooth --populations`: the filtered
    marginals under every population's chain (one E-step per population on the fit's ``p_bound`` at the stored theta_g and
    prior), the chains and the responsibilities of the on-target AOIs.  Returns (filt (G, N, F, M), thetas (G, M * M + M),
    resp (G, N)) on the device of ``p_bound``, and logs the stored weights."""
    import torch

    from tapqir_amd.utils.mle_analysis import hmm_estep

    logger.info(f"rasters of the mixture of {sm['theta'][c].shape[0]} populations fitted by `smooth`, weights "
                + ", ".join(f"{x:.4f}" for x in sm["phi"][c].tolist()))
    thetas = sm["theta"][c].to(device=p_bound.device, dtype=torch.float64).contiguous()
    prior = float(sm["prior"][c])
    filt = torch.stack([hmm_estep(p_bound, thetas[g], prior, U, B)["filt"] for g in range(thetas.shape[0])])
    resp = sm["population_probs"][:, :, c][mask].T.to(device=p_bound.device, dtype=torch.float64).contiguous()
    return filt, thetas, resp


def _joint_posterior(command, cd, m, mask, pair, logger):
    """``<name>_smooth-joint<A><B>.tpqr`` for the ``--smooth --joint A,B`` switch of `ttfb` and `dwelltime`: the joint chain
    (``theta``, ``prior``) of `smooth --joint A,B`.  Exits with status 1 when the data lacks a channel of the pair, the
    file is missing or was written for another pair or another selection of AOIs."""
    import torch

    from tapqir_amd.utils.safe_load import load_tpqr

    a, b = pair
    C = m.data.C
    if a >= C or b >= C:
        logger.error(f"{command}: --joint {a},{b} needs channels {a} and {b}, the data has {C} channel{'s' if C != 1 else ''}")
        raise typer.Exit(1)
    path = cd / f"{m.name}_smooth-joint{a}{b}.tpqr"
    if not path.is_file():
        logger.error(f"{command} --smooth --joint needs {path.name}: run `smooth --joint {a},{b}` first")
        raise typer.Exit(1)
    sm = load_tpqr(path)
    if tuple(int(c) for c in sm["channels"]) != (a, b):
        logger.error(f"{command} --smooth --joint: {path.name} was written for the channels {tuple(sm['channels'])}: run "
                     f"`smooth --joint {a},{b}` again")
        raise typer.Exit(1)
    if sm["mask"].shape != mask.shape or not torch.equal(sm["mask"].bool(), mask):
        logger.error(f"{command} --smooth --joint: {path.name} was written for another mask of on-target AOIs than the data "
                     f"has now: run `smooth --joint {a},{b}` again")
        raise typer.Exit(1)
    return sm


def _joint_filter(sm, m, mask, pair, dev, logger):
    """The inputs of the joint chain's backward sampler from the file of `smooth --joint`: one E-step on the two channels'
    p(z = 1) of the fit at the stored theta and priors.  Returns (filt (N, F, 4), theta (20,)) on ``dev``."""
    import torch

    from tapqir_amd.utils.joint_analysis import joint_estep

    a, b = pair
    logger.info(f"rasters of the joint chain of channels #{a} and #{b} fitted by `smooth --joint` (structure {sm['chosen']})")
    theta = sm["theta"].to(device=dev, dtype=torch.float64).reshape(1, -1).contiguous()
    p_a, p_b = (m.params["z_probs"][: m.data.N, :, c, 1][mask].float().to(dev) for c in (a, b))
    filt = joint_estep(p_a, p_b, theta, float(sm["prior"][0]), float(sm["prior"][1]))["filt"][0]
    return filt, theta[0]


def _finite_summary(rows):
    """``_summary_table`` over the finite values of every row (a sample in which a population has no member, or none that
    bound, has no value there); a row without any finite value is NaN."""
    import pandas as pd
    import torch

    tables = []
    for label, values in rows:
        x = values[torch.isfinite(values)]
        if x.numel():
            tables.append(_summary_table([(label, x)]))
        else:
            tables.append(pd.DataFrame({"Mean": [float("nan")], "95% LL": [float("nan")], "95% UL": [float("nan")]},
                                       index=[label]))
    return pd.concat(tables)


def _summary_table(rows):
    """Mean and 95% highest-density interval of each ``(label, values)`` pair, one row per label."""
    import pandas as pd

    from tapqir_amd.utils.stats import hpdi

    results = pd.DataFrame(columns=["Mean", "95% LL", "95% UL"], dtype=float)
    for label, values in rows:
        ll, ul = hpdi(values, 0.95)
        results.loc[label] = [values.mean().item(), ll.item(), ul.item()]
    return results


def _pyplot():
    """(matplotlib, pyplot) on the Agg backend with the commands' font settings, or (None, None) without matplotlib."""
    try:
        import matplotlib as mpl

        mpl.use("Agg")
        import matplotlib.pyplot as plt
    except Exception:
        return None, None
    mpl.rcParams["font.family"] = "sans-serif"
    mpl.rcParams.update({"font.size": 8})
    return mpl, plt


def _ttfb_plots(cd, stem, c, z_masked, sdx, r_type, Tmax, fb_mean, fb_ll, fb_ul, best_fit, logger):
    """Rastergram and cumulative-fraction plot of one channel (main.py:988-1005, 1108-1147); ``stem`` is the start of the
    file names, ``<model>_ttfb`` or ``<model>_ttfb-smooth``."""
    mpl, plt = _pyplot()
    if plt is None:
        logger.warning("matplotlib is not available: the ttfb plots are not drawn")
        return
    fig, ax = plt.subplots()
    ax.imshow(z_masked[sdx].numpy(), norm=mpl.colors.Normalize(vmin=0, vmax=1), aspect="equal", interpolation="none")
    ax.set_xlabel("Time (frame)")
    ax.set_ylabel("AOI")
    ax.set_title(f"Channel {c}")
    plt.savefig(cd / f"{stem}-rastergram-channel{c}.png", dpi=600)
    plt.close(fig)
    logger.info(f"Saved a {r_type} rastergram in {stem}-rastergram-channel{c}.png file")

    t = range(Tmax)
    fig, ax = plt.subplots()
    ax.fill_between(t, fb_ll, fb_ul, alpha=0.3, color="C2")
    ax.plot(t, fb_mean, color="C2")
    ax.plot(t, best_fit, color="k")
    plt.minorticks_on()
    ax.tick_params(direction="in", which="minor", length=1, bottom=True, top=True, left=True, right=True)
    ax.tick_params(direction="in", which="major", length=2, bottom=True, top=True, left=True, right=True)
    ax.set_yticks([0, 0.2, 0.4, 0.6, 0.8, 1])
    ax.set_yticklabels([r"$0$", r"$0.2$", r"$0.4$", r"$0.6$", r"$0.8$", r"$1$"])
    ax.set_xlabel("Time (frame)")
    ax.set_ylabel("Cumulative fraction")
    ax.set_title(f"Channel {c}")
    ax.set_ylim(-0.05, 1.05)
    plt.savefig(cd / f"{stem}-plot-channel{c}.png", dpi=600)
    plt.close(fig)
    logger.info(f"Saved data plots in {stem}-plot-channel{c}.png file")


def _ttfb_populations(cd, stem, c, split, G, Tmax, Af, logger):
    """``<stem>-populations-channel<c>.csv`` of `ttfb --smooth --populations G`: mean and 95% HPDI over the samples (those in
    which the population has a member, for the last two a member that bound) of, per population g, ``g<g>_share`` (AOIs
    drawn into g), ``g<g>_never_bound`` (of those, the share with no bound frame), ``g<g>_first_binding`` (mean
    first-binding frame of those that bound), and the cumulative fraction bound of the AOIs of g at every frame t,
    ``g<g>_fraction_bound_<t>``: the columns of the fraction-bound file, one row per frame.  Logs the fitted ``Af`` next to
    the mixture's estimate of the active fraction, sum_g share_g (1 - never_bound_g)."""
    import pandas as pd
    import torch

    from tapqir_amd.utils.mle_analysis import hpdi_columns

    host = {k: v.cpu() for k, v in split.items()}
    table = _finite_summary((f"g{g}_{key}", host[key][:, g]) for g in range(G)
                            for key in ("share", "never_bound", "first_binding"))
    curves = []
    for g in range(G):
        fb = host["fraction_bound"][:, g][host["share"][:, g] > 0]  # (samples with a member, Tmax)
        if fb.shape[0]:
            ll, ul = hpdi_columns(fb, 0.95)
            block = {"Mean": fb.mean(0).numpy(), "95% LL": ll.numpy(), "95% UL": ul.numpy()}
        else:
            block = {name: torch.full((Tmax,), float("nan")).numpy() for name in ("Mean", "95% LL", "95% UL")}
        curves.append(pd.DataFrame(block, index=[f"g{g}_fraction_bound_{t}" for t in range(Tmax)]))
    pd.concat([table, *curves]).to_csv(cd / f"{stem}-populations-channel{c}.csv")
    logger.info(f"Saved the share, the never-bound share, the mean first-binding frame and the fraction bound of every "
                f"population in {stem}-populations-channel{c}.csv file")
    active = (host["share"] * (1.0 - torch.nan_to_num(host["never_bound"], nan=1.0))).sum(1)
    logger.info(f"active fraction: fitted Af = {Af:.4f}; the mixture's rasters give sum_g share_g (1 - never-bound share of "
                f"g) = {active.mean().item():.4f} (per population: "
                + ", ".join(f"g{g} {table.loc[f'g{g}_share', 'Mean']:.4f} x (1 - {table.loc[f'g{g}_never_bound', 'Mean']:.4f})"
                            for g in range(G)) + ")")


def _ttfb_joint(cd, m, mask, sm, pair, num_samples, logger):
    """`ttfb --smooth --joint A,B`: the order of arrival of the two channels from posterior rasters
    of the joint chain, both channels walked at the seed A.  Writes ``<model>_ttfb-smooth-joint<A><B>-order.csv`` alone: the
    rows of ``joint_arrival_order`` with A as the lead (``a_*``) and with B as the lead (``b_*``), mean and 95% HPDI over
    the samples in which the quantity exists."""
    import pandas as pd
    import torch

    from tapqir_amd.utils.joint_analysis import ORDER_NAMES, joint_arrival_order, joint_dwell_sample
    from tapqir_amd.utils.mle_analysis import hpdi_columns

    a, b = pair
    stem = f"{m.name}_ttfb-smooth-joint{a}{b}"
    F = m.data.F
    filt, theta = _joint_filter(sm, m, mask, pair, torch.device("cuda"), logger)
    drawn = [joint_dwell_sample(filt, theta, which, num_samples, seed=a) for which in (0, 1)]  # seed A: `smooth --joint`'s
    rows = {}
    for lead, label in ((0, "a"), (1, "b")):
        order = joint_arrival_order(drawn[lead]["tau"], drawn[lead]["tau_after"], drawn[1 - lead]["tau"], F)
        for key in ORDER_NAMES:
            x = order[key].cpu()
            x = x[torch.isfinite(x)]
            if x.numel():
                ll, ul = hpdi_columns(x[:, None], 0.95)
                rows[f"{label}_{key}"] = [x.mean().item(), ll.item(), ul.item()]
            else:
                rows[f"{label}_{key}"] = [float("nan")] * 3
    pd.DataFrame.from_dict(rows, orient="index", columns=["Mean", "95% LL", "95% UL"]).to_csv(cd / f"{stem}-order.csv")
    logger.info(f"Saved the order of arrival of channels #{a} and #{b} in {stem}-order.csv file")


@app.command()
def ttfb(
    model: avail_models = typer.Option("cosmos", help="Tapqir model"),
    binary: bool = typer.Option(False, "--binary/--probabilistic", help="Plot a binary or probabilistic rastergram"),
    cuda: bool = typer.Option(_default("cuda"), "--cuda/--cpu", help="Run computations on GPU or CPU", show_default=False),
    num_samples: int = typer.Option(2000, "--num-samples", "-n", min=1, help="Number of posterior samples"),
    num_iter: int = typer.Option(15000, "--num-iter", "-it", min=1, help="Number of iterations"),
    smooth: bool = typer.Option(False, "--smooth", help="Sample the rasters of the chain fitted by `smooth`"),
    unbound_states: int = typer.Option(1, "--unbound-states", min=1, help="Hidden states that look unbound (z = 0)"),
    bound_states: int = typer.Option(1, "--bound-states", min=1, help="Hidden states that look bound (z = 1); at most 4 in all"),
    populations: int = typer.Option(1, "--populations", help="Populations of AOIs, each with a chain of its own (1 to 4): a mixture of chains"),
    joint: Optional[str] = typer.Option(None, "--joint", help="A,B: the order of arrival of the colour channels A and B from the chain of `smooth --joint A,B`"),
    no_input: bool = typer.Option(False, "--no-input", help="Accepted for compatibility (there are no prompts)."),
    progress_bar=None,
):
    """
    Time-to-first-binding analysis (tapqir/main.py:926-1147): posterior samples of the first-binding frame of every
    on-target AOI, one censored two-exponential fit (ka, kns, Af) per sample, and the cumulative fraction bound.
    Needs ``data.tpqr`` and ``<model>_params.tpqr`` of a cosmos fit.

    With ``--smooth`` the first-binding frames are those of posterior rasters of the two-state chain that `smooth` fitted
    (``<model>_smooth.tpqr``; the rasters behind its rate table) instead of independent draws of every frame, the
    rastergram shows the smoothed posterior, and the files are named ``<model>_ttfb-smooth-...``.

    With ``--smooth --unbound-states U --bound-states B`` other than 1 and 1 the rasters are those of the chain of U + B <= 4
    hidden states that `smooth` fitted with the same two options (``<model>_smooth-u<U>b<B>.tpqr``), walked at the level
    of the classes z = 0 / z = 1, and the files are named ``<model>_ttfb-smooth-u<U>b<B>-...``.  They
    are rasters of the same chain at the same seed as those behind ``<model>_smooth-u<U>b<B>-channel<c>.csv``, but not bit
    for bit: the filtered marginals are computed again at the stored chain, and a draw whose uniform lies within rounding
    of a threshold can fall on the other side.

    With ``--smooth --populations G`` (2 to 4) the rasters are those of the mixture of G chains that `smooth` fitted with
    the same ``--populations`` and state options (``<model>_smooth-u<U>b<B>g<G>.tpqr``): every raster draws a population for
    every AOI from its responsibilities and then that population's chain, and the files are named
    ``<model>_ttfb-smooth-u<U>b<B>g<G>-...``.  The same caveat holds: the rasters of the same mixture
    at the same seed as those behind ``<model>_smooth-u<U>b<B>g<G>-channel<c>.csv``, not bit for bit.  The (ka, kns, Af)
    fit is pooled over all AOIs; ``...-populations-channel<c>.csv`` adds, per population, the share of AOIs drawn into it,
    the share of those never bound, the mean first-binding frame of those that bound and the cumulative fraction bound,
    and the fitted Af is logged next to the mixture's own estimate of the active fraction.  There are no per-population
    ttfb fits: the members of a population change from sample to sample, and the fit takes rectangular data.

    With ``--smooth --joint A,B`` the rasters are those of the chain of four joint states that `smooth --joint A,B` chose
    (``<model>_smooth-joint<A><B>.tpqr``), both channels walked in the same rasters, and only
    ``<model>_ttfb-smooth-joint<A><B>-order.csv`` is written: with A as the lead (rows ``a_*``) and
    with B as the lead (``b_*``), per sample the share of AOIs in which the lead binds (``binds``); of those, the shares in
    which the partner is there at that frame (``together``), arrives later (``later``) or never does (``never``); the mean
    delay of the late arrivals (``mean_delay``); the partner's probability per frame of arriving once the lead is there
    (``k_after``) and from the start of the record (``k_base``), both as events over frames at risk with right censoring;
    and their ``ratio``.  There is no (ka, kns, Af) fit: it takes one observation window for all AOIs, and here the window
    after the lead's arrival differs from AOI to AOI.  The rasters are those of the same chain at the same seed as the
    ones behind ``<model>_smooth-joint<A><B>.csv``, not bit for bit: the filtered marginals are computed again at the
    stored chain.  ``--joint`` does not go with state or population options.
    """
    import pandas as pd
    import torch

    from tapqir_amd.exceptions import HipExtensionError
    from tapqir_amd.utils.imscroll import time_to_first_binding
    from tapqir_amd.utils.mle_analysis import (fraction_bound, fraction_bound_fit, hmm_dwell_sample, hpdi_columns,
                                               mixture_dwell_sample, population_first_binding, smooth_dwell_sample,
                                               ttfb_fit, ttfb_sample)

    cd = DEFAULTS["cd"]
    logger = logging.getLogger("tapqir")
    U, B, G = unbound_states, bound_states, populations
    pair = _chain_states("ttfb", model, cuda, smooth, U, B, logger, G, joint)
    m, mask, progress_bar = _kinetics_inputs("ttfb", model, cuda, progress_bar)
    data = m.data
    if pair is not None:
        try:
            _ttfb_joint(cd, m, mask, _joint_posterior("ttfb", cd, m, mask, pair, logger), pair, num_samples, logger)
        except HipExtensionError:
            logger.exception("ttfb failed: it needs an AMD GPU (--cuda) and the built HIP library")
            raise typer.Exit(1)
        return
    sm = _smoothed_posterior("ttfb", cd, m.name, mask, logger, U, B, G) if smooth else None
    stem = f"{m.name}_ttfb-smooth{_smooth_suffix(U, B, G)}" if smooth else f"{m.name}_ttfb"
    if smooth:
        z = sm["z_map"].float() if binary else sm["z_probs"].float()
    else:
        p_specific = m.params["p_specific"][: data.N].float()
        z = (p_specific > 0.5).float() if binary else p_specific
    r_type = "binary" if binary else "probabilistic"
    Tmax = data.F
    try:
        dev = torch.device("cuda")
        for c in range(data.C):
            logger.info(f"Channel #{c} ({data.channels[c]})")
            z_masked = z[:, :, c][mask]
            sdx = torch.argsort(time_to_first_binding(z_masked), descending=True)

            p_bound = m.params["z_probs"][: data.N, :, c, 1][mask].float().to(dev)
            drawn = None
            if smooth and G > 1:  # seed c: the default of `smooth`
                drawn = mixture_dwell_sample(*_mixture_filter(sm, c, p_bound, mask, U, B, logger), U, B, num_samples, seed=c)
                tau = drawn["tau"]
            elif smooth and (U, B) != (1, 1):  # seed c: the default of `smooth`
                tau = hmm_dwell_sample(*_smoothed_filter(sm, c, p_bound, U, B), U, B, num_samples, seed=c)["tau"]
            elif smooth:  # seed c: the default of `smooth`, so these are the rasters of its rate table
                tau = smooth_dwell_sample(*_smoothed_filter(sm, c, p_bound), num_samples, seed=c)["tau"]
            else:
                tau = ttfb_sample(p_bound, num_samples, seed=c)
            tau_host = tau.cpu()
            pd.DataFrame(data=tau_host.numpy()).to_csv(cd / f"{stem}-data-points-channel{c}.csv")
            logger.info(f"Saved time-to-first-binding values in {stem}-data-points-channel{c}.csv file")

            fit = ttfb_fit(tau, Tmax, lr=5e-3, n_steps=num_iter, progress_bar=progress_bar)
            results = _summary_table((name, fit[name].squeeze(-1).cpu()) for name in ("ka", "kns", "Af"))
            results.to_csv(cd / f"{stem}-params-channel{c}.csv")
            logger.info(f"Saved fit parameters in {stem}-params-channel{c}.csv file")

            fb = fraction_bound(tau_host, Tmax)
            fb_ll, fb_ul = hpdi_columns(fb, 0.95)
            fb_mean = fb.mean(0)
            best_fit = fraction_bound_fit(tau_host, Tmax, results.loc["ka", "Mean"], results.loc["kns", "Mean"],
                                          results.loc["Af", "Mean"])
            pd.DataFrame(data={"time": torch.arange(Tmax).numpy(), "best fit": best_fit.numpy(),
                               "fraction bound mean": fb_mean.numpy(), "fraction bound 95% ll": fb_ll.numpy(),
                               "fraction bound 95% ul": fb_ul.numpy()}).to_csv(
                cd / f"{stem}-fraction-bound-channel{c}.csv")
            logger.info(f"Saved fit data in {stem}-fraction-bound-channel{c}.csv file")
            _ttfb_plots(cd, stem, c, z_masked.cpu(), sdx.cpu(), r_type, Tmax, fb_mean.numpy(), fb_ll.numpy(),
                        fb_ul.numpy(), best_fit.numpy(), logger)
            if drawn is not None:
                _ttfb_populations(cd, stem, c, population_first_binding(tau, drawn["pop"], G, Tmax), G, Tmax,
                                  results.loc["Af", "Mean"], logger)
    except HipExtensionError:
        logger.exception("ttfb failed: it needs an AMD GPU (--cuda) and the built HIP library")
        raise typer.Exit(1)


def _dwell_plot(cd, stem, c, kind, map_dt, A, k, t_max, logger):
    """Dwell-time histogram of the MAP raster with the fitted mixture (main.py:1266-1296, 1350-1381); ``stem`` is the
    start of the file name, ``<model>_dwelltime`` or ``<model>_dwelltime-smooth``."""
    mpl, plt = _pyplot()
    if plt is None:
        logger.warning("matplotlib is not available: the dwelltime plots are not drawn")
        return
    import numpy as np

    fig, ax = plt.subplots()
    if map_dt.size:
        ax.hist(map_dt[0], bins=100, density=True)
    t = np.arange(t_max)
    y = 0
    for a_i, k_i in zip(A, k):
        comp = a_i * k_i * np.exp(-k_i * t)
        y = y + comp
        ax.plot(comp, "k--")
    ax.plot(y, "k-")
    ax.set_xlabel("Time interval (frame)")
    ax.set_ylabel("Density")
    ax.set_title(f"{kind.capitalize()} dwell times channel {c}")
    plt.savefig(cd / f"{stem}-{kind}-histogram-channel{c}.png", dpi=600)
    plt.close(fig)
    logger.info(f"Saved {kind} dwell-time histograms in {stem}-{kind}-histogram-channel{c}.png file")


def _dwell_population_fits(cd, stem, c, sample, G, K, num_iter, kinds, z_map, population_map, progress_bar, logger):
    """The fits of `dwelltime --smooth --populations G` for one channel: for every kind, one K-exponential fit per
    population from ``sample["hist_<kind>"][:, g]`` -- the interior intervals of the AOIs a sample drew into g -- written
    together as ``<stem>-<rate>-channel<c>.csv`` with rows ``g<g>_A<i>`` and ``g<g>_<rate><i>``, and one histogram per
    population, ``<stem>-g<g>-<kind>-histogram-channel<c>.png``, of the Viterbi paths ``z_map`` (N, F) of the AOIs whose
    ``population_map`` is g.  A sample in which g has no interior interval of the kind is left out of that fit and logged;
    a kind no sample has for g is skipped with a warning."""
    import pandas as pd
    import torch

    from tapqir_amd.utils.imscroll import count_intervals
    from tapqir_amd.utils.mle_analysis import dwell_csr_from_hist, dwell_fit

    for kind, rate, title, host_dwell_times in kinds:
        logger.info(f"{title} calculation ...")
        tables = []
        for g in range(G):
            hist = sample[f"hist_{kind}"][:, g].contiguous()
            keep = hist.sum(1) > 0
            n_out = int((~keep).sum())
            if n_out == hist.shape[0]:
                logger.warning(f"dwelltime: no posterior sample has an interior {kind} interval in population {g}: its "
                               f"{rate} is not fitted")
                continue
            if n_out:
                logger.info(f"population {g}: {n_out} of {hist.shape[0]} posterior samples have no interior {kind} interval "
                            f"and are left out of the {rate} fit")
            hist = hist[keep]
            fit = dwell_fit(dwell_csr_from_hist(hist), K, lr=5e-3, n_steps=num_iter, progress_bar=progress_bar)
            results = _summary_table(pair for i in range(K) for pair in (
                (f"g{g}_A{i}", fit["A"][:, i].cpu()), (f"g{g}_{rate}{i}", fit["k"][:, i].cpu())))
            tables.append(results)
            A_mean = [results.loc[f"g{g}_A{i}", "Mean"] for i in range(K)]
            k_mean = [results.loc[f"g{g}_{rate}{i}", "Mean"] for i in range(K)]
            t_max = int(torch.nonzero(hist.sum(0)).max().item())  # the largest sampled dwell time
            members = (population_map == g).cpu()
            map_dt = (host_dwell_times(count_intervals(z_map[members][None].cpu().numpy())) if bool(members.any())
                      else torch.zeros(0).numpy())
            _dwell_plot(cd, f"{stem}-g{g}", c, kind, map_dt, A_mean, k_mean, t_max, logger)
        if tables:
            pd.concat(tables).to_csv(cd / f"{stem}-{rate}-channel{c}.csv")
            logger.info(f"Saved {title.lower()} parameters of the populations in {stem}-{rate}-channel{c}.csv file")


def _dwell_censored_fits(cd, stem, c, sample, cens, G, K, num_iter, kinds, progress_bar, logger):
    """The fits of `dwelltime --censored` for one channel.  For every kind, and every population g
    of ``G`` (None: no populations), one K-exponential fit per posterior sample of the complete interior runs
    ``sample["hist_<kind>"]`` with the open last runs ``cens["cens_<kind>"]`` as right-censored observations, written as
    ``<stem>-censored-<rate>-channel<c>.csv`` with the rows of the fit without the switch; and per kind (and population,
    ``<stem>-g<g>-censored-...``) the Kaplan-Meier survival of every sample with the fitted survival at the mean
    parameters, as ``...-censored-<kind>-survival-channel<c>.csv`` and ``.png``.  A sample (or a population of one) without
    a complete interval of the kind is left out and logged; a kind no sample has is skipped with a warning."""
    import pandas as pd
    import torch

    from tapqir_amd.utils.censored_analysis import (dwell_censored_fit, dwell_csr_from_censored_hist, dwell_survival,
                                                    mixture_survival)
    from tapqir_amd.utils.mle_analysis import dwell_csr_from_hist, hpdi_columns

    for kind, rate, title, _ in kinds:
        logger.info(f"{title} calculation with the open last runs ...")
        tables = []
        for g in (range(G) if G else (None,)):
            hist, open_runs = sample[f"hist_{kind}"], cens[f"cens_{kind}"]
            if g is not None:
                hist, open_runs = hist[:, g].contiguous(), open_runs[:, g].contiguous()
            who, pre, gstem = ("", "", stem) if g is None else (f" in population {g}", f"g{g}_", f"{stem}-g{g}")
            keep = hist.sum(1) > 0
            n_out = int((~keep).sum())
            if n_out == hist.shape[0]:
                logger.warning(f"dwelltime: no posterior sample has an interior {kind} interval{who}: {rate} is not fitted")
                continue
            if n_out:
                logger.info(f"{n_out} of {hist.shape[0]} posterior samples have no interior {kind} interval{who} and are "
                            f"left out of the {rate} fit")
            hist, open_runs = hist[keep], open_runs[keep]
            logger.info(f"{int(hist.sum())} complete and {int(open_runs[:, 2:].sum())} open {kind} intervals{who} enter "
                        f"the {rate} fit")
            fit = dwell_censored_fit(dwell_csr_from_hist(hist), dwell_csr_from_censored_hist(open_runs), K, lr=5e-3,
                                     n_steps=num_iter, progress_bar=progress_bar)
            results = _summary_table(pair for i in range(K) for pair in (
                (f"{pre}A{i}", fit["A"][:, i].cpu()), (f"{pre}{rate}{i}", fit["k"][:, i].cpu())))
            tables.append(results)
            A_mean = [results.loc[f"{pre}A{i}", "Mean"] for i in range(K)]
            k_mean = [results.loc[f"{pre}{rate}{i}", "Mean"] for i in range(K)]

            t_max = int(torch.nonzero(hist.sum(0) + open_runs.sum(0)).max().item())  # the largest sampled dwell time
            surv = dwell_survival(hist, open_runs)[:, : t_max + 1].cpu()
            ll, ul = hpdi_columns(surv, 0.95)
            mean = surv.mean(0)
            fitted = mixture_survival(A_mean, k_mean, torch.arange(t_max + 1))
            name = f"{gstem}-censored-{kind}-survival-channel{c}"
            pd.DataFrame(data={"time": torch.arange(t_max + 1).numpy(), "best fit": fitted.numpy(),
                               "survival mean": mean.numpy(), "survival 95% ll": ll.numpy(),
                               "survival 95% ul": ul.numpy()}).to_csv(cd / f"{name}.csv")
            logger.info(f"Saved {kind} survival curves in {name}.csv file")
            _survival_plot(cd, name, c, kind, mean.numpy(), ll.numpy(), ul.numpy(), fitted.numpy(), logger)
        if tables:
            pd.concat(tables).to_csv(cd / f"{stem}-censored-{rate}-channel{c}.csv")
            logger.info(f"Saved {title.lower()} parameters in {stem}-censored-{rate}-channel{c}.csv file")


def _survival_plot(cd, name, c, kind, mean, ll, ul, fitted, logger):
    """Kaplan-Meier band of the posterior samples with the fitted survival over it (`dwelltime --censored`)."""
    mpl, plt = _pyplot()
    if plt is None:
        logger.warning("matplotlib is not available: the survival plots are not drawn")
        return
    import numpy as np

    fig, ax = plt.subplots()
    t = np.arange(mean.shape[0])
    ax.fill_between(t, ll, ul, alpha=0.3, step="post")
    ax.step(t, mean, where="post")
    ax.plot(t, fitted, "k-")
    ax.set_ylim(0, 1.02)
    ax.set_xlabel("Time interval (frame)")
    ax.set_ylabel("Fraction of dwells longer than t")
    ax.set_title(f"{kind.capitalize()} dwell survival channel {c}")
    plt.savefig(cd / f"{name}.png", dpi=600)
    plt.close(fig)
    logger.info(f"Saved {kind} survival plot in {name}.png file")


def _dwell_joint(cd, m, mask, sm, pair, K, num_samples, num_iter, kinds, savemat, progress_bar, logger):
    """`dwelltime --smooth --joint A,B`: for each channel c of the pair, the runs of c in posterior
    rasters of the joint chain (seed A for both, so both tables describe the same rasters), written as
    ``<model>_dwelltime-smooth-joint<A><B>-intervals-channel<c>.pkl`` / ``.mat`` with the partner's state at the ends of
    every run, and for every kind one K-exponential fit per partner state q at the run's first frame from
    ``sample["hist_<kind>"][:, q]``, written together as ``...-<rate>-channel<c>.csv`` with rows ``q<q>_A<i>`` and
    ``q<q>_<rate><i>``.  A sample without an interior interval of the kind for q is left out of that fit and logged; a
    kind no sample has for q is skipped with a warning.  No plots."""
    import pandas as pd
    import torch

    from tapqir_amd.utils.joint_analysis import joint_dwell_intervals, joint_dwell_sample
    from tapqir_amd.utils.mle_analysis import dwell_csr_from_hist, dwell_fit

    a, b = pair
    stem = f"{m.name}_dwelltime-smooth-joint{a}{b}"
    filt, theta = _joint_filter(sm, m, mask, pair, torch.device("cuda"), logger)
    for which, c in enumerate(pair):
        logger.info(f"Channel #{c} ({m.data.channels[c]}), partner #{pair[1 - which]}")
        sample = joint_dwell_sample(filt, theta, which, num_samples, seed=a)  # seed A: the default of `smooth --joint`
        intervals = joint_dwell_intervals(filt, theta, which, num_samples, seed=a, sample=sample)
        intervals.to_pickle(cd / f"{stem}-intervals-channel{c}.pkl")
        logger.info(f"Saved time intervals in {stem}-intervals-channel{c}.pkl file")
        if savemat is not None:
            savemat(cd / f"{stem}-intervals-channel{c}.mat", intervals.to_dict("list"))
            logger.info(f"Saved time intervals in {stem}-intervals-channel{c}.mat file")
        else:
            logger.info("scipy is not available: the .mat file of the intervals is not written")
        for kind, rate, title, _ in kinds:
            logger.info(f"{title} calculation by the partner's state ...")
            tables = []
            for q in (0, 1):
                hist = sample[f"hist_{kind}"][:, q].contiguous()
                keep = hist.sum(1) > 0
                n_out = int((~keep).sum())
                if n_out == hist.shape[0]:
                    logger.warning(f"dwelltime: no posterior sample has an interior {kind} interval that starts with the "
                                   f"partner at {q}: its {rate} is not fitted")
                    continue
                if n_out:
                    logger.info(f"partner at {q}: {n_out} of {hist.shape[0]} posterior samples have no interior {kind} "
                                f"interval and are left out of the {rate} fit")
                fit = dwell_fit(dwell_csr_from_hist(hist[keep]), K, lr=5e-3, n_steps=num_iter, progress_bar=progress_bar)
                tables.append(_summary_table(row for i in range(K) for row in (
                    (f"q{q}_A{i}", fit["A"][:, i].cpu()), (f"q{q}_{rate}{i}", fit["k"][:, i].cpu()))))
            if tables:
                pd.concat(tables).to_csv(cd / f"{stem}-{rate}-channel{c}.csv")
                logger.info(f"Saved {title.lower()} parameters by the partner's state in {stem}-{rate}-channel{c}.csv file")


@app.command()
def dwelltime(
    model: avail_models = typer.Option("cosmos", help="Tapqir model"),
    K: int = typer.Option(3, "-K", help="Number of exponentials"),
    cuda: bool = typer.Option(_default("cuda"), "--cuda/--cpu", help="Run computations on GPU or CPU", show_default=False),
    num_samples: int = typer.Option(500, "--num-samples", "-n", min=1, help="Number of posterior samples"),
    num_iter: int = typer.Option(10000, "--num-iter", "-it", min=1, help="Number of iterations"),
    smooth: bool = typer.Option(False, "--smooth", help="Sample the rasters of the chain fitted by `smooth`"),
    unbound_states: int = typer.Option(1, "--unbound-states", min=1, help="Hidden states that look unbound (z = 0)"),
    bound_states: int = typer.Option(1, "--bound-states", min=1, help="Hidden states that look bound (z = 1); at most 4 in all"),
    populations: int = typer.Option(1, "--populations", help="Populations of AOIs, each with a chain of its own (1 to 4): a mixture of chains"),
    censored: bool = typer.Option(False, "--censored", help="Count the run still open at the last frame as a right-censored dwell"),
    joint: Optional[str] = typer.Option(None, "--joint", help="A,B: the dwell times of the colour channels A and B by each other's state, from the chain of `smooth --joint A,B`"),
    no_input: bool = typer.Option(False, "--no-input", help="Accepted for compatibility (there are no prompts)."),
    progress_bar=None,
):
    """
    Dwell-time analysis (tapqir/main.py:1150-1384): the bound and unbound intervals of posterior samples of every
    on-target AOI's z raster, and one K-exponential fit per sample of the interior bound (koff) and unbound (kon) dwell
    times.  Needs ``data.tpqr`` and ``<model>_params.tpqr`` of a cosmos fit.

    Unlike the reference, a sample without an interior interval of a kind is left out of that kind's fit and statistics
    (the count is logged), and a kind that no sample has is skipped with a warning.

    With ``--smooth`` the rasters are posterior rasters of the two-state chain that `smooth` fitted
    (``<model>_smooth.tpqr``; the rasters behind its rate table) instead of independent draws of every frame, the plotted
    histogram is that of its Viterbi path, and the files are named ``<model>_dwelltime-smooth-...``.

    With ``--smooth --unbound-states U --bound-states B`` other than 1 and 1 the rasters are those of the chain of U + B <= 4
    hidden states that `smooth` fitted with the same two options (``<model>_smooth-u<U>b<B>.tpqr``), walked at the level
    of the classes z = 0 / z = 1, and the files are named ``<model>_dwelltime-smooth-u<U>b<B>-...``.
    They are rasters of the same chain at the same seed as those behind ``<model>_smooth-u<U>b<B>-channel<c>.csv``, but not
    bit for bit: the filtered marginals are computed again at the stored chain, and a draw whose uniform lies within
    rounding of a threshold can fall on the other side.

    With ``--smooth --populations G`` (2 to 4) the rasters are those of the mixture of G chains that `smooth` fitted with
    the same ``--populations`` and state options (``<model>_smooth-u<U>b<B>g<G>.tpqr``): every raster draws a population for
    every AOI from its responsibilities and then that population's chain.  The interval table gains the column
    ``population``, every population has its own K-exponential fits (rows ``g<g>_A<i>`` and ``g<g>_koff<i>`` / ``g<g>_kon<i>``)
    from the interior intervals of the AOIs drawn into it, and its own histograms, of the Viterbi paths of the AOIs whose
    most probable population it is; the files are named ``<model>_dwelltime-smooth-u<U>b<B>g<G>-...`` (DESIGN.md section
    30).  The same caveat holds: the rasters of the same mixture at the same seed as those behind
    ``<model>_smooth-u<U>b<B>g<G>-channel<c>.csv``, not bit for bit.

    With ``--censored``, in any of the forms above, a run that opened inside the record and is still open at the last frame
    enters the fit as a right-censored dwell (d seen frames: d - 1 stays, the term ``log sum_j A_j exp(-k_j (d - 1))``)
    instead of being dropped, which removes the bias towards short dwells of slow complexes in short records.  First runs
    (``start_frame == 0``, a run that spans the record included) stay out: their start was not observed, and the first
    unbound run is `ttfb`'s subject.  The interval files are written as without the switch; the rate tables go to
    ``<stem>-censored-<rate>-channel<c>.csv`` and, per kind (and population), the Kaplan-Meier survival of the samples with
    the fitted survival to ``...-censored-<kind>-survival-channel<c>.csv`` and ``.png``.  The MAP raster's histogram is not
    drawn: it holds interior runs only, and a correct fit would look wrong next to it.  The files of the fit without the
    switch are neither written nor touched.

    With ``--smooth --joint A,B`` the rasters are those of the chain of four joint states that `smooth --joint A,B` chose
    (``<model>_smooth-joint<A><B>.tpqr``), and each channel c of the pair is walked in the same rasters with the other
    channel as its partner.  ``<model>_dwelltime-smooth-joint<A><B>-intervals-channel<c>`` gains the
    columns ``partner_start``, ``partner_before``, ``partner_stop`` and ``partner_after``: the partner's state at the first
    frame of the run, the frame before it, its last frame and the frame after it, -1 where the record has no such frame.
    Every kind has one K-exponential fit per partner state q at the first frame of the run, rows ``q<q>_A<i>`` and
    ``q<q>_koff<i>`` / ``q<q>_kon<i>`` of ``...-koff-channel<c>.csv`` / ``...-kon-channel<c>.csv``.  There are no plots.
    The rasters are those of the same chain at the same seed as the ones behind ``<model>_smooth-joint<A><B>.csv``, not
    bit for bit: the filtered marginals are computed again at the stored chain.  ``--joint`` does not go with state or
    population options or with ``--censored``, whose histograms are not split by the partner's state.
    """
    import torch

    from tapqir_amd import _lib
    from tapqir_amd.exceptions import HipExtensionError
    from tapqir_amd.utils.censored_analysis import dwell_censored_hist
    from tapqir_amd.utils.imscroll import bound_dwell_times, count_intervals, unbound_dwell_times
    from tapqir_amd.utils.mle_analysis import (dwell_csr_from_hist, dwell_fit, dwell_intervals, dwell_sample,
                                               hmm_dwell_intervals, hmm_dwell_sample, mixture_dwell_intervals,
                                               mixture_dwell_sample, smooth_dwell_intervals, smooth_dwell_sample)

    cd = DEFAULTS["cd"]
    logger = logging.getLogger("tapqir")
    # the -K range is checked after the model and before --cpu: a model other than cosmos is left to _kinetics_inputs
    if model.value == "cosmos" and not 1 <= K <= _lib.DWELL_KMAX:
        logger.error(f"dwelltime: -K must be between 1 and {_lib.DWELL_KMAX}, got {K}")
        raise typer.Exit(1)
    U, B, G = unbound_states, bound_states, populations
    pair = _chain_states("dwelltime", model, cuda, smooth, U, B, logger, G, joint, censored)
    m, mask, progress_bar = _kinetics_inputs("dwelltime", model, cuda, progress_bar)
    try:
        from scipy.io import savemat
    except Exception:
        savemat = None

    data = m.data
    kinds = (("bound", "koff", "Off-rate", bound_dwell_times), ("unbound", "kon", "On-rate", unbound_dwell_times))
    if pair is not None:
        try:
            _dwell_joint(cd, m, mask, _joint_posterior("dwelltime", cd, m, mask, pair, logger), pair, K, num_samples, num_iter,
                         kinds, savemat, progress_bar, logger)
        except HipExtensionError:
            logger.exception("dwelltime failed: it needs an AMD GPU (--cuda) and the built HIP library")
            raise typer.Exit(1)
        return
    sm = _smoothed_posterior("dwelltime", cd, m.name, mask, logger, U, B, G) if smooth else None
    stem = f"{m.name}_dwelltime-smooth{_smooth_suffix(U, B, G)}" if smooth else f"{m.name}_dwelltime"
    if smooth:
        z_map = sm["z_map"]
    else:
        z_map = m.params["z_map"][: data.N] if "z_map" in m.params else None
    try:
        dev = torch.device("cuda")
        for c in range(data.C):
            logger.info(f"Channel #{c} ({data.channels[c]})")
            p_bound = m.params["z_probs"][: data.N, :, c, 1][mask].float().to(dev)
            if smooth and G > 1:  # seed c: the default of `smooth`
                chains = _mixture_filter(sm, c, p_bound, mask, U, B, logger)
                sample = mixture_dwell_sample(*chains, U, B, num_samples, seed=c)
                intervals = mixture_dwell_intervals(*chains, U, B, num_samples, seed=c, sample=sample,
                                                    device_table=censored)
            elif smooth and (U, B) != (1, 1):  # seed c: the default of `smooth`
                filt, theta = _smoothed_filter(sm, c, p_bound, U, B)
                sample = hmm_dwell_sample(filt, theta, U, B, num_samples, seed=c)
                intervals = hmm_dwell_intervals(filt, theta, U, B, num_samples, seed=c, sample=sample,
                                                device_table=censored)
            elif smooth:  # seed c: the default of `smooth`, so these are the rasters of its rate table
                filt, theta = _smoothed_filter(sm, c, p_bound)
                sample = smooth_dwell_sample(filt, theta, num_samples, seed=c)
                intervals = smooth_dwell_intervals(filt, theta, num_samples, seed=c, sample=sample,
                                                   device_table=censored)
            else:
                sample = dwell_sample(p_bound, num_samples, seed=c)
                intervals = dwell_intervals(p_bound, num_samples, seed=c, sample=sample, device_table=censored)
            if censored:  # the open last runs, counted from the table while it is still on the device
                intervals, table = intervals
                mixture = smooth and G > 1
                cens = dwell_censored_hist(table, num_samples, p_bound.shape[0], p_bound.shape[1],
                                           pop=sample["pop"] if mixture else None, populations=G if mixture else None)
                del table
            intervals.to_pickle(cd / f"{stem}-intervals-channel{c}.pkl")
            logger.info(f"Saved time intervals in {stem}-intervals-channel{c}.pkl file")
            if savemat is not None:
                savemat(cd / f"{stem}-intervals-channel{c}.mat", intervals.to_dict("list"))
                logger.info(f"Saved time intervals in {stem}-intervals-channel{c}.mat file")
            else:
                logger.info("scipy is not available: the .mat file of the intervals is not written")

            if censored:
                _dwell_censored_fits(cd, stem, c, sample, cens, G if smooth and G > 1 else None, K, num_iter, kinds,
                                     progress_bar, logger)
                continue
            if smooth and G > 1:
                _dwell_population_fits(cd, stem, c, sample, G, K, num_iter, kinds, z_map[mask, :, c],
                                       sm["population_map"][:, c][mask], progress_bar, logger)
                continue
            for kind, rate, title, host_dwell_times in kinds:
                logger.info(f"{title} calculation ...")
                hist = sample[f"hist_{kind}"]
                keep = hist.sum(1) > 0
                n_out = int((~keep).sum())
                if n_out == hist.shape[0]:
                    logger.warning(f"dwelltime: no posterior sample has an interior {kind} interval: {rate} is not fitted")
                    continue
                if n_out:
                    logger.info(f"{n_out} of {hist.shape[0]} posterior samples have no interior {kind} interval and "
                                f"are left out of the {rate} fit")
                hist = hist[keep]
                fit = dwell_fit(dwell_csr_from_hist(hist), K, lr=5e-3, n_steps=num_iter, progress_bar=progress_bar)
                results = _summary_table(pair for i in range(K) for pair in (
                    (f"A{i}", fit["A"][:, i].cpu()), (f"{rate}{i}", fit["k"][:, i].cpu())))
                A_mean = [results.loc[f"A{i}", "Mean"] for i in range(K)]
                k_mean = [results.loc[f"{rate}{i}", "Mean"] for i in range(K)]
                results.to_csv(cd / f"{stem}-{rate}-channel{c}.csv")
                logger.info(f"Saved {title.lower()} parameters in {stem}-{rate}-channel{c}.csv file")

                t_max = int(torch.nonzero(hist.sum(0)).max().item())  # the largest sampled dwell time
                map_dt = (host_dwell_times(count_intervals(z_map[None, mask, :, c].cpu().numpy()))
                          if z_map is not None else torch.zeros(0).numpy())
                _dwell_plot(cd, stem, c, kind, map_dt, A_mean, k_mean, t_max, logger)
    except HipExtensionError:
        logger.exception("dwelltime failed: it needs an AMD GPU (--cuda) and the built HIP library")
        raise typer.Exit(1)


@app.command()
def rates(
    model: avail_models = typer.Option("cosmos", help="Tapqir model"),
    cuda: bool = typer.Option(_default("cuda"), "--cuda/--cpu", help="Run computations on GPU or CPU", show_default=False),
    num_samples: int = typer.Option(1000, "--num-samples", "-n", min=1, help="Number of posterior samples"),
    ci: float = typer.Option(0.95, "--ci", help="Probability mass of the interval, in (0, 1)"),
    bootstrap: bool = typer.Option(True, "--bootstrap/--no-bootstrap", help="Resample the AOIs of every posterior sample"),
    seed: Optional[int] = typer.Option(None, "--seed", help="Seed of the posterior samples (default: the channel index)"),
    no_input: bool = typer.Option(False, "--no-input", help="Accepted for compatibility (there are no prompts)."),
    progress_bar=None,
):
    """
    Two-state rate estimates (tapqir/utils/imscroll.py:199-317): kon = P(0 -> 1) and koff = P(1 -> 0) per frame, pooled
    over the on-target AOIs of every posterior sample of the z raster (resampled with replacement unless
    ``--no-bootstrap``), with mean and percentile interval over the samples and the rates of the MAP raster.
    Needs ``data.tpqr`` and ``<model>_params.tpqr`` of a cosmos fit.

    A sample whose rate has a zero denominator is left out of that rate's mean and interval (the count is logged), and a
    rate that no sample determines is skipped with a warning.
    """
    import pandas as pd
    import torch

    from tapqir_amd.exceptions import HipExtensionError
    from tapqir_amd.utils.mle_analysis import rates_estimate, rates_sample, rates_summary

    cd = DEFAULTS["cd"]
    logger = logging.getLogger("tapqir")
    # like -K of dwelltime: checked after the model and before --cpu
    if model.value == "cosmos" and not 0.0 < ci < 1.0:
        logger.error(f"rates: --ci must be between 0 and 1, got {ci}")
        raise typer.Exit(1)
    m, mask, progress_bar = _kinetics_inputs("rates", model, cuda, progress_bar)
    data = m.data
    z_map = m.params["z_map"][: data.N] if "z_map" in m.params else None
    pct = f"{ci * 100:g}%"
    try:
        dev = torch.device("cuda")
        for c in range(data.C):
            logger.info(f"Channel #{c} ({data.channels[c]})")
            p_bound = m.params["z_probs"][: data.N, :, c, 1][mask].float().to(dev)
            chan_seed = c if seed is None else seed
            estimate = rates_estimate(rates_sample(p_bound, num_samples, seed=chan_seed), bootstrap=bootstrap,
                                      seed=chan_seed)
            summary = rates_summary(estimate, ci)
            map_rate = {"kon": float("nan"), "koff": float("nan")}
            if z_map is not None:  # the MAP raster through the same count kernel: p = 0 never binds, p = 1 always does
                map_p = z_map[:, :, c][mask].float().to(dev)
                map_est = rates_estimate(rates_sample(map_p, 1, seed=chan_seed))
                map_rate = {rate: map_est[rate][0].item() for rate in map_rate}
            results = pd.DataFrame(columns=["Mean", f"{pct} LL", f"{pct} UL", "MAP"], dtype=float)
            for rate in ("kon", "koff"):
                row = summary[rate]
                if row["left_out"] == num_samples:
                    logger.warning(f"rates: no posterior sample determines {rate} (zero denominators): it is skipped")
                elif row["left_out"]:
                    logger.info(f"{row['left_out']} of {num_samples} posterior samples have a zero {rate} denominator "
                                f"and are left out of its mean and interval")
                results.loc[rate] = [row["mean"], row["ll"], row["ul"], map_rate[rate]]
            results.to_csv(cd / f"{m.name}_rates-channel{c}.csv")
            logger.info(f"Saved rate estimates in {m.name}_rates-channel{c}.csv file")
    except HipExtensionError:
        logger.exception("rates failed: it needs an AMD GPU (--cuda) and the built HIP library")
        raise typer.Exit(1)


def _smooth_multistart_options(U, B, restarts, restart_seed, forbid, logger, mixture=False):
    """The checks of ``--restarts``, ``--restart-seed`` and ``--forbid`` of `smooth`, made where ``--ci`` is checked (after
    the model, before ``--cpu``).  Returns ``{"restarts", "seed", "allow"}``, allow an (M, M) list of booleans.  A mixture
    (``--populations``) has several optima at (1, 1) too, so it takes the options there."""
    M = U + B
    if (U, B) == (1, 1) and not mixture:
        logger.error("smooth: --restarts, --restart-seed and --forbid need a chain of more than two states "
                     "(--unbound-states, --bound-states): the two-state EM has one optimum and one topology")
        raise typer.Exit(1)
    return {"restarts": restarts, "seed": restart_seed, "allow": _smooth_forbid(M, forbid, logger)}


def _smooth_forbid(M, forbid, logger):
    """The values of ``--forbid`` of `smooth` as an (M, M) list of booleans, True where the transition is free."""
    import re

    allow = [[True] * M for _ in range(M)]
    for item in forbid or []:
        match = re.fullmatch(r"(\d+)-(\d+)", item.strip())
        i, j = (int(match.group(1)), int(match.group(2))) if match else (-1, -1)
        if not match or i == j or i >= M or j >= M:
            logger.error(f"smooth: --forbid takes i-j with two different states below {M}, got {item!r}")
            raise typer.Exit(1)
        allow[i][j] = False
    if not all(any(row) for row in allow):
        logger.error("smooth: --forbid leaves a state without a free transition")
        raise typer.Exit(1)
    return allow


def _smooth_multistate(m, mask, cd, logger, U, B, num_iter, tol, num_samples, ci, bootstrap, seed, progress_bar,
                       multistart=None, refit=None):
    """`smooth` with U + B > 2 hidden states: ``<model>_smooth-u<U>b<B>.tpqr`` and, per channel,
    ``<model>_smooth-u<U>b<B>-channel<c>.csv``.  AOIs outside the mask keep the fit's z_probs and have NaN state
    probabilities and state 255.  With ``multistart`` (``--restarts`` / ``--forbid``, section 26) every channel is fitted
    by ``hmm_fit_restarts`` and the file gains ``restart_logliks``, ``restart_best`` and ``topology``.  With ``refit``
    (``--refit``, section 33) the files of ``_smooth_refit`` are written next to them."""
    import pandas as pd
    import torch

    from tapqir_amd.exceptions import HipExtensionError
    from tapqir_amd.utils.mle_analysis import (estimand_summary, hmm_estimate, hmm_fit, hmm_fit_restarts, hmm_n_params,
                                               hmm_sample, hmm_summary, hmm_viterbi, rates_estimate, rates_sample,
                                               rates_summary)

    data, M = m.data, U + B
    stem = f"{m.name}_smooth-u{U}b{B}"
    pct = f"{ci * 100:g}%"
    columns = ["EM", "Mean", f"{pct} LL", f"{pct} UL", "MAP"]
    z_raw = m.params["z_probs"][: data.N, :, :, 1].float()  # (N, F, C)
    out = {"z_probs": z_raw.clone(), "state_probs": torch.full((*z_raw.shape, M), float("nan")), "z_map": z_raw > 0.5,
           "state_map": torch.full(z_raw.shape, 255, dtype=torch.uint8),
           "log_evidence": torch.full((data.N, data.C), float("nan"), dtype=torch.float64),
           "theta": torch.zeros(data.C, M * M + M, dtype=torch.float64), "prior": torch.zeros(data.C, dtype=torch.float64),
           "bic": torch.zeros(data.C, dtype=torch.float64), "n_params": M * (M - 1) + (M - 1), "loglik_trace": [],
           "mask": mask, "unbound": U, "bound": B}
    if multistart is not None:
        topology = torch.tensor(multistart["allow"], dtype=torch.bool)
        out.update({"n_params": hmm_n_params(topology), "topology": topology,
                    "restart_logliks": torch.zeros(data.C, multistart["restarts"] + 1, dtype=torch.float64),
                    "restart_best": torch.zeros(data.C, dtype=torch.int64),
                    "topology_by_channel": torch.ones(data.C, M, M, dtype=torch.bool)})
    refits = []
    try:
        dev = torch.device("cuda")
        for c in range(data.C):
            logger.info(f"Channel #{c} ({data.channels[c]})")
            prior = float(torch.as_tensor(m.params["pi"]["Mean"]).reshape(-1, 2)[c, 1])
            p = z_raw[:, :, c][mask].to(dev)
            chan_seed = c if seed is None else seed
            if multistart is None:
                fit = hmm_fit(p, prior, U, B, num_iter=num_iter, tol=tol, progress_bar=progress_bar)
            else:
                fit = hmm_fit_restarts(p, prior, U, B, restarts=multistart["restarts"], seed=multistart["seed"],
                                       allow=topology, num_iter=num_iter, tol=tol, progress_bar=progress_bar)
                best = fit["best"]
                logger.info(f"EM from {multistart['restarts'] + 1} starts: log evidence {fit['logliks'][0].item():.6f} from "
                            f"the default start, {fit['logliks'][best].item():.6f} from the best one, start #{best}"
                            + (" (the default start)" if best == 0 else f" (random start {best} of seed {multistart['seed']})"))
                out["restart_logliks"][c] = fit["logliks"]
                out["restart_best"][c] = best
                out["topology_by_channel"][c] = fit["allow"]  # in the canonical order of the states, as theta is
                fit = {**fit, "iterations": fit["iterations"][best], "converged": fit["converged"][best]}
            theta = fit["theta"]
            A = theta[: M * M].reshape(M, M).cpu()
            logger.info(f"EM with {U} unbound and {B} bound states: log evidence = {fit['loglik']:.6f}, BIC = "
                        f"{fit['bic']:.6f} ({fit['n_params']} parameters; the lower, the better) after "
                        f"{fit['iterations']} iterations")
            if not fit["converged"]:
                logger.warning(f"smooth: the EM did not converge to --tol {tol:g} within {fit['iterations']} iterations")
            path = hmm_viterbi(p, theta, prior, U, B)
            sample = hmm_sample(fit["filt"], theta, U, B, num_samples, seed=chan_seed, trans=True)
            est = hmm_estimate(sample["trans"], bootstrap=bootstrap, seed=chan_seed)
            summary = hmm_summary(est, ci)
            pairs = torch.bincount((path[:, :-1].long() * M + path[:, 1:].long()).reshape(-1), minlength=M * M)
            A_map = (pairs.double().reshape(M, M) / pairs.double().reshape(M, M).sum(1, keepdim=True)).cpu()
            results = pd.DataFrame(columns=columns, dtype=float)
            for i in range(M):
                for j in range(M):
                    row = summary[f"A{i}{j}"]
                    results.loc[f"A{i}{j}"] = [A[i, j].item(), row["mean"], row["ll"], row["ul"], A_map[i, j].item()]
            for i in range(M):  # mean dwell of state i in frames, 1 / (1 - A_ii)
                row = estimand_summary(1.0 / (1.0 - est["A"][:, i, i]), ci)
                results.loc[f"dwell{i}"] = [1.0 / (1.0 - A[i, i].item()), row["mean"], row["ll"], row["ul"],
                                            (1.0 / (1.0 - A_map[i, i])).item()]
            pair_sums = fit["rows"][:, : M * M].sum(0).reshape(M, M).cpu()  # expected pairs by state, summed over AOIs
            em = {"kon": (pair_sums[:U, U:].sum() / pair_sums[:U].sum()).item(),
                  "koff": (pair_sums[U:, :U].sum() / pair_sums[U:].sum()).item()}
            rates = rates_summary(rates_estimate(sample["counts"], bootstrap=bootstrap, seed=chan_seed), ci)
            map_est = rates_estimate(rates_sample((path >= U).float(), 1, seed=chan_seed))  # p in {0, 1} is drawn as itself
            for rate in ("kon", "koff"):
                row = rates[rate]
                results.loc[rate] = [em[rate], row["mean"], row["ll"], row["ul"], map_est[rate][0].item()]
            results.to_csv(cd / f"{stem}-channel{c}.csv")
            logger.info(f"Saved the transition matrix, dwells and rates in {stem}-channel{c}.csv file")
            out["z_probs"][:, :, c][mask] = fit["gamma"][..., U:].sum(-1).float().cpu()
            out["state_probs"][:, :, c][mask] = fit["gamma"].float().cpu()
            out["z_map"][:, :, c][mask] = (path >= U).cpu()
            out["state_map"][:, :, c][mask] = path.cpu()
            out["log_evidence"][:, c][mask] = fit["rows"][:, -1].cpu()
            out["theta"][c] = theta.cpu()
            out["prior"][c] = prior
            out["bic"][c] = fit["bic"]
            out["loglik_trace"].append(fit["trace"].cpu())
            if refit:
                # the topology in the canonical order of the states, as theta is
                allow = fit["allow"] if multistart is not None else None
                refits.append(_smooth_refit(cd, stem, c, p, prior, theta, U, B, refit, allow, num_iter, tol, ci, progress_bar,
                                            logger))
        torch.save(out, cd / f"{stem}.tpqr")
        logger.info(f"Saved the smoothed posterior in {stem}.tpqr file")
        if refit:
            _smooth_refit_save(cd, stem, refits, refit, U, B, logger)
    except HipExtensionError:
        logger.exception("smooth failed: it needs an AMD GPU (--cuda) and the built HIP library")
        raise typer.Exit(1)


def _smooth_refit(cd, stem, c, p, prior, theta, U, B, refit, allow, num_iter, tol, ci, progress_bar, logger):
    """`smooth --refit R` for one channel: ``hmm_fit_refits`` from the fitted ``theta`` (M * M + M)
    and ``<stem>-refit-channel<c>.csv`` with the row labels of the channel CSV -- every A_ij, every state's mean dwell
    1 / (1 - A_ii), the class-level kon and koff from the expected pair counts, as `smooth` forms them -- and the columns
    EM (replica 0: the data as they are), Mean, SE (the standard deviation) and the percentile interval over the refits
    that met ``--tol``.  Returns the result of ``hmm_fit_refits``."""
    import pandas as pd
    import torch

    from tapqir_amd.utils.mle_analysis import estimand_summary, hmm_fit_refits

    M, R = U + B, refit["refits"]
    fit = hmm_fit_refits(p, prior, theta, U, B, R, seed=refit["seed"], allow=allow, num_iter=num_iter, tol=tol,
                         progress_bar=progress_bar)
    A, pairs = fit["thetas"][:, : M * M].reshape(R + 1, M, M), fit["pairs"]
    values = {f"A{i}{j}": A[:, i, j] for i in range(M) for j in range(M)}
    values.update({f"dwell{i}": 1.0 / (1.0 - A[:, i, i]) for i in range(M)})
    values["kon"] = pairs[:, :U, U:].sum((1, 2)) / pairs[:, :U].sum((1, 2))
    values["koff"] = pairs[:, U:, :U].sum((1, 2)) / pairs[:, U:].sum((1, 2))
    keep = torch.tensor(fit["converged"][1:], dtype=torch.bool)
    left_out = R - int(keep.sum())
    logger.info(f"{R} refits of the chain on resampled AOIs (seed {refit['seed']}): {left_out} did not converge to --tol "
                f"{tol:g} within {num_iter} iterations and {'are' if left_out != 1 else 'is'} left out of the summary")
    if not fit["converged"][0]:
        logger.warning(f"smooth: the refit of the data as they are did not converge to --tol {tol:g} within {num_iter} "
                       f"iterations")
    pct = f"{ci * 100:g}%"
    results = pd.DataFrame(columns=["EM", "Mean", "SE", f"{pct} LL", f"{pct} UL"], dtype=float)
    for name, x in values.items():
        x = x.double()
        kept = x[1:][keep]
        row = estimand_summary(kept, ci)
        se = kept[torch.isfinite(kept)].std().item() if int(torch.isfinite(kept).sum()) > 1 else float("nan")
        results.loc[name] = [x[0].item(), row["mean"], se, row["ll"], row["ul"]]
    results.to_csv(cd / f"{stem}-refit-channel{c}.csv")
    logger.info(f"Saved the standard errors and intervals of the refits in {stem}-refit-channel{c}.csv file")
    return fit


def _smooth_refit_save(cd, stem, fits, refit, U, B, logger):
    """``<stem>-refit.tpqr``: per channel the refitted chains, their weighted log evidences and pair counts, the iteration
    counts and the converged flags; the seed and R."""
    import torch

    out = {"thetas": torch.stack([f["thetas"] for f in fits]), "logliks": torch.stack([f["logliks"] for f in fits]),
           "pairs": torch.stack([f["pairs"] for f in fits]),
           "converged": torch.tensor([f["converged"] for f in fits], dtype=torch.bool),
           "iterations": torch.tensor([f["iterations"] for f in fits], dtype=torch.int64),
           "seed": refit["seed"], "refits": refit["refits"], "unbound": U, "bound": B}
    torch.save(out, cd / f"{stem}-refit.tpqr")
    logger.info(f"Saved the refitted chains in {stem}-refit.tpqr file")


def _smooth_mixture_options(populations, U, B, joint, structure, restarts, restart_seed, forbid, logger):
    """The checks of ``--populations`` of `smooth`, made where ``--ci`` is checked (after the model, before ``--cpu``).
    Returns None for one population, else ``{"populations", "restarts", "seed", "allow"}``."""
    if not 1 <= populations <= 4:
        logger.error(f"smooth: --populations must lie in 1 .. 4, got {populations}")
        raise typer.Exit(1)
    if populations == 1:
        return None
    if joint is not None or structure is not None:
        logger.error("smooth: --populations does not go with --joint / --structure: the joint chain is fitted to all AOIs")
        raise typer.Exit(1)
    if (restarts + 1) * populations > 64:
        logger.error(f"smooth: (--restarts + 1) * --populations must be at most 64, got ({restarts} + 1) * {populations}")
        raise typer.Exit(1)
    return {"populations": populations,
            **_smooth_multistart_options(U, B, restarts, restart_seed, forbid, logger, mixture=True)}


def _smooth_mixture(m, mask, cd, logger, U, B, mixture, num_iter, tol, num_samples, ci, bootstrap, seed, progress_bar):
    """`smooth --populations G`: every channel fitted by ``mixture_fit`` as a mixture of G chains of
    (U, B) states over the on-target AOIs.  Writes ``<model>_smooth-u<U>b<B>g<G>.tpqr`` and, per channel,
    ``<model>_smooth-u<U>b<B>g<G>-channel<c>.csv``; no other file is touched.  AOIs outside the mask keep the fit's z_probs
    and have NaN state and population probabilities and population 255.

    The CSV has, per population g, its weight, every entry of its A, the mean dwell of every state and the class-level kon
    and koff: ``EM`` is the fitted value, ``Mean`` and the interval come from posterior rasters that draw a population for
    every AOI (the share of AOIs drawn into g; the quotients of the state pairs of those AOIs)."""
    import pandas as pd
    import torch

    from tapqir_amd.exceptions import HipExtensionError
    from tapqir_amd.utils.mle_analysis import (estimand_summary, hmm_n_params, mixture_estimate, mixture_fit, mixture_sample,
                                               mixture_viterbi)

    data, M, G = m.data, U + B, mixture["populations"]
    stem = f"{m.name}_smooth-u{U}b{B}g{G}"
    pct = f"{ci * 100:g}%"
    topology = torch.tensor(mixture["allow"], dtype=torch.bool)
    z_raw = m.params["z_probs"][: data.N, :, :, 1].float()  # (N, F, C)
    out = {"z_probs": z_raw.clone(), "z_map": z_raw > 0.5, "state_probs": torch.full((*z_raw.shape, M), float("nan")),
           "population_probs": torch.full((data.N, G, data.C), float("nan"), dtype=torch.float64),
           "population_map": torch.full((data.N, data.C), 255, dtype=torch.uint8),
           "theta": torch.zeros(data.C, G, M * M + M, dtype=torch.float64), "phi": torch.zeros(data.C, G, dtype=torch.float64),
           "log_evidence": torch.full((data.N, data.C), float("nan"), dtype=torch.float64),
           "bic": torch.zeros(data.C, dtype=torch.float64), "n_params": G * hmm_n_params(topology) + G - 1, "loglik_trace": [],
           "restart_logliks": torch.zeros(data.C, mixture["restarts"] + 1, dtype=torch.float64), "topology": topology,
           "prior": torch.zeros(data.C, dtype=torch.float64), "mask": mask, "unbound": U, "bound": B, "populations": G}
    try:
        dev = torch.device("cuda")
        for c in range(data.C):
            logger.info(f"Channel #{c} ({data.channels[c]})")
            prior = float(torch.as_tensor(m.params["pi"]["Mean"]).reshape(-1, 2)[c, 1])
            p = z_raw[:, :, c][mask].to(dev)
            chan_seed = c if seed is None else seed
            fit = mixture_fit(p, prior, U, B, populations=G, restarts=mixture["restarts"], seed=mixture["seed"],
                              allow=topology, num_iter=num_iter, tol=tol, progress_bar=progress_bar)
            best = fit["best"]
            logger.info(f"EM of {G} populations of {U} unbound and {B} bound states from {mixture['restarts'] + 1} start"
                        f"{'s' if mixture['restarts'] else ''}: log evidence = {fit['loglik']:.6f}, mixture BIC = "
                        f"{fit['bic']:.6f} ({fit['n_params']} parameters; the lower, the better) after "
                        f"{fit['iterations'][best]} iterations, weights {', '.join(f'{x:.4f}' for x in fit['phi'].tolist())}")
            logger.info("compare this BIC with that of `smooth --bound-states` (or --unbound-states) without --populations: "
                        "populations are molecules that differ, more states are one kind of molecule that switches")
            if not fit["converged"][best]:
                logger.warning(f"smooth: the EM did not converge to --tol {tol:g} within {fit['iterations'][best]} iterations")
            thetas, resp = fit["thetas"], fit["resp"]
            vit = mixture_viterbi(p, thetas, resp, prior, U, B)
            sample = mixture_sample(fit["filt"], thetas, resp, U, B, num_samples, seed=chan_seed, trans=True)
            est = mixture_estimate(sample["trans"], sample["pop"], G, bootstrap=bootstrap, seed=chan_seed)
            tot = est["totals"].double()  # (S, G, M, M)
            drawn = {"kon": tot[:, :, :U, U:].sum((2, 3)) / tot[:, :, :U].sum((2, 3)),
                     "koff": tot[:, :, U:, :U].sum((2, 3)) / tot[:, :, U:].sum((2, 3))}
            share = est["members"].double() / est["members"].sum(1, keepdim=True).double()
            results = pd.DataFrame(columns=["EM", "Mean", f"{pct} LL", f"{pct} UL"], dtype=float)
            for g in range(G):
                A = thetas[g, : M * M].reshape(M, M).cpu()
                row = estimand_summary(share[:, g], ci)
                results.loc[f"g{g}_phi"] = [fit["phi"][g].item(), row["mean"], row["ll"], row["ul"]]
                for i in range(M):
                    for j in range(M):
                        row = estimand_summary(est["A"][:, g, i, j], ci)
                        results.loc[f"g{g}_A{i}{j}"] = [A[i, j].item(), row["mean"], row["ll"], row["ul"]]
                for i in range(M):  # mean dwell of state i in frames, 1 / (1 - A_ii)
                    row = estimand_summary(1.0 / (1.0 - est["A"][:, g, i, i]), ci)
                    results.loc[f"g{g}_dwell{i}"] = [1.0 / (1.0 - A[i, i].item()), row["mean"], row["ll"], row["ul"]]
                pairs = fit["pair_sums"][g].cpu()
                em = {"kon": (pairs[:U, U:].sum() / pairs[:U].sum()).item(), "koff": (pairs[U:, :U].sum() / pairs[U:].sum()).item()}
                for rate in ("kon", "koff"):
                    row = estimand_summary(drawn[rate][:, g], ci)
                    results.loc[f"g{g}_{rate}"] = [em[rate], row["mean"], row["ll"], row["ul"]]
            results.to_csv(cd / f"{stem}-channel{c}.csv")
            logger.info(f"Saved the weights, transition matrices, dwells and rates of the populations in {stem}-channel{c}.csv "
                        f"file")
            out["z_probs"][:, :, c][mask] = fit["gamma"][..., U:].sum(-1).float().cpu()
            out["state_probs"][:, :, c][mask] = fit["gamma"].float().cpu()
            out["z_map"][:, :, c][mask] = (vit["path"] >= U).cpu()
            out["population_probs"][:, :, c][mask] = resp.T.cpu()
            out["population_map"][:, c][mask] = vit["population_map"].to(torch.uint8).cpu()
            out["theta"][c] = thetas.cpu()
            out["phi"][c] = fit["phi"].cpu()
            out["log_evidence"][:, c][mask] = fit["evidence"].cpu()
            out["bic"][c] = fit["bic"]
            out["prior"][c] = prior
            out["loglik_trace"].append(fit["trace"].cpu())
            out["restart_logliks"][c] = fit["logliks"]
        torch.save(out, cd / f"{stem}.tpqr")
        logger.info(f"Saved the smoothed posterior of the mixture in {stem}.tpqr file")
    except HipExtensionError:
        logger.exception("smooth failed: it needs an AMD GPU (--cuda) and the built HIP library")
        raise typer.Exit(1)


def _smooth_joint_options(joint, structure, U, B, restarts, restart_seed, forbid, logger):
    """The checks of ``--joint`` and ``--structure`` of `smooth`, made where ``--ci`` is checked (after the model, before
    ``--cpu``).  Returns ``{"a", "b", "structure"}``, structure a name or None for ``auto``."""
    import re

    from tapqir_amd._lib_joint import STRUCTURES

    names = [name for name, _ in STRUCTURES]
    if joint is None:
        logger.error("smooth: --structure needs --joint A,B")
        raise typer.Exit(1)
    a, b = _joint_pair("smooth", joint, logger)
    if (U, B) != (1, 1):
        logger.error("smooth: --joint smooths two two-state channels together: it does not go with --unbound-states / "
                     "--bound-states other than 1 and 1")
        raise typer.Exit(1)
    if restarts or restart_seed or forbid:
        logger.error("smooth: --joint does not go with --restarts, --restart-seed or --forbid: its structures are fitted from "
                     "the chain of the two separate fits")
        raise typer.Exit(1)
    if structure is not None and structure != "auto" and structure not in names:
        logger.error(f"smooth: --structure takes auto, {', '.join(names)}; got {structure!r}")
        raise typer.Exit(1)
    return {"a": a, "b": b, "structure": None if structure in (None, "auto") else structure}


def _smooth_joint(m, mask, cd, logger, pair, num_iter, tol, num_samples, ci, bootstrap, seed, progress_bar):
    """`smooth --joint A,B`: the two channels as one chain of four states, s = z_A + 2 z_B, fitted
    under the five structures side by side from the chain of the two separate two-state fits and ranked by BIC.  Writes
    ``<model>_smooth-joint<A><B>.tpqr`` and ``<model>_smooth-joint<A><B>.csv``; no other file is touched.

    The CSV has the sixteen entries of A, the eight conditional rates and their four ratios.  ``EM`` is the fitted value
    under the chosen structure, ``MAP`` the quotient of the Viterbi path's pair counts, and ``Mean`` with its interval comes
    from the pair counts of posterior rasters of the chain.  Those quotients are unconstrained: under a constrained
    structure the intervals are those of free count quotients, not of the constrained estimator, so they need not be
    centred on ``EM`` and do not vanish for a rate the structure ties to another."""
    import pandas as pd
    import torch

    from tapqir_amd.exceptions import HipExtensionError
    from tapqir_amd.utils.joint_analysis import (RATE_NAMES, RATIO_NAMES, STRUCTURE_NAMES, joint_fit, joint_rates,
                                                 joint_start_from, joint_viterbi)
    from tapqir_amd.utils.mle_analysis import estimand_summary, hmm_estimate, hmm_sample, smooth_fit

    data, a, b = m.data, pair["a"], pair["b"]
    if a >= data.C or b >= data.C:
        logger.error(f"smooth: --joint {a},{b} needs channels {a} and {b}, the data has {data.C} "
                     f"channel{'s' if data.C != 1 else ''}")
        raise typer.Exit(1)
    stem = f"{m.name}_smooth-joint{a}{b}"
    pct = f"{ci * 100:g}%"
    z_raw = m.params["z_probs"][: data.N, :, :, 1].float()  # (N, F, C)
    try:
        dev = torch.device("cuda")
        p, prior, two_state = {}, {}, {}
        for c in (a, b):
            prior[c] = float(torch.as_tensor(m.params["pi"]["Mean"]).reshape(-1, 2)[c, 1])
            p[c] = z_raw[:, :, c][mask].to(dev)
            two_state[c] = smooth_fit(p[c], prior[c], num_iter=num_iter, tol=tol, progress_bar=progress_bar)
        ll_sep = sum(two_state[c]["rows"][:, 4].sum().item() for c in (a, b))
        logger.info(f"Channels #{a} ({data.channels[a]}) and #{b} ({data.channels[b]}): log evidence of the two separate "
                    f"two-state fits = {ll_sep:.6f}")
        start = joint_start_from(two_state[a]["theta"], two_state[b]["theta"])
        fit = joint_fit(p[a], p[b], prior[a], prior[b], start=start, num_iter=num_iter, tol=tol, choose=pair["structure"],
                        progress_bar=progress_bar)
        fits = fit["fits"]
        for f in fits:
            logger.info(f"structure {f['name']}: log evidence = {f['loglik']:.6f}, {f['n_params']} parameters, BIC = "
                        f"{f['bic']:.6f} after {f['iterations']} iterations")
            if not f["converged"]:
                logger.warning(f"smooth: the EM of structure {f['name']} did not converge to --tol {tol:g} within "
                               f"{f['iterations']} iterations")
        # independent is nested in both driven structures, those in coupled, and every structure in full
        nested = {1: (0,), 2: (0,), 3: (0, 1, 2), 4: (0, 1, 2, 3)}
        for big, smalls in nested.items():
            for small in smalls:
                if fits[big]["loglik"] < fits[small]["loglik"] - 1e-6 * abs(fits[small]["loglik"]):
                    logger.warning(f"smooth: structure {fits[big]['name']} ends below {fits[small]['name']}, which is nested in "
                                   f"it ({fits[big]['loglik']:.6f} < {fits[small]['loglik']:.6f}): a local optimum")
        chosen = fit["chosen"]
        logger.info(f"chosen structure: {STRUCTURE_NAMES[chosen]} ("
                    + ("forced by --structure" if pair["structure"] is not None else "the lowest BIC") + ")")
        theta = fit["theta"]
        A = theta[:16].reshape(4, 4).cpu()
        path = joint_viterbi(p[a], p[b], theta, prior[a], prior[b])
        chan_seed = a if seed is None else seed
        sample = hmm_sample(fit["filt"], theta, 2, 2, num_samples, seed=chan_seed, trans=True)
        est = hmm_estimate(sample["trans"], bootstrap=bootstrap, seed=chan_seed)
        pairs = torch.bincount((path[:, :-1].long() * 4 + path[:, 1:].long()).reshape(-1), minlength=16).double().reshape(4, 4)
        A_map = (pairs / pairs.sum(1, keepdim=True)).cpu()
        em, drawn, mapped = joint_rates(A), joint_rates(est["A"]), joint_rates(A_map)
        results = pd.DataFrame(columns=["EM", "Mean", f"{pct} LL", f"{pct} UL", "MAP"], dtype=float)
        for i in range(4):
            for j in range(4):
                row = estimand_summary(est["A"][:, i, j], ci)
                results.loc[f"A{i}{j}"] = [A[i, j].item(), row["mean"], row["ll"], row["ul"], A_map[i, j].item()]
        for name in RATE_NAMES + RATIO_NAMES:
            row = estimand_summary(drawn[name], ci)
            results.loc[name] = [em[name].item(), row["mean"], row["ll"], row["ul"], mapped[name].item()]
        results.to_csv(cd / f"{stem}.csv")
        logger.info(f"Saved the joint transition matrix, conditional rates and ratios in {stem}.csv file")

        gamma = fit["gamma"].float().cpu()  # (n, F, 4)
        state_probs = torch.full((data.N, data.F, 4), float("nan"))
        state_probs[mask] = gamma
        z_probs = torch.stack([state_probs[..., 1] + state_probs[..., 3], state_probs[..., 2] + state_probs[..., 3]], -1)
        state_map = torch.full((data.N, data.F), 255, dtype=torch.uint8)
        state_map[mask] = path.cpu()
        z_map = torch.stack([state_map & 1, state_map >> 1], -1)
        z_map[~mask] = 255
        log_evidence = torch.full((data.N,), float("nan"), dtype=torch.float64)
        log_evidence[mask] = fit["rows"][:, -1].cpu()
        out = {"state_probs": state_probs, "z_probs": z_probs, "state_map": state_map, "z_map": z_map,
               "log_evidence": log_evidence, "theta": theta.cpu(),
               "prior": torch.tensor([prior[a], prior[b]], dtype=torch.float64), "channels": (a, b),
               "structures": [f["name"] for f in fits], "logliks": torch.tensor([f["loglik"] for f in fits], dtype=torch.float64),
               "bics": torch.tensor([f["bic"] for f in fits], dtype=torch.float64),
               "n_params": torch.tensor([f["n_params"] for f in fits], dtype=torch.int64), "chosen": STRUCTURE_NAMES[chosen],
               "loglik_trace": [f["trace"] for f in fits], "mask": mask}
        torch.save(out, cd / f"{stem}.tpqr")
        logger.info(f"Saved the jointly smoothed posterior in {stem}.tpqr file")
    except HipExtensionError:
        logger.exception("smooth failed: it needs an AMD GPU (--cuda) and the built HIP library")
        raise typer.Exit(1)


def _smooth_timed(m, mask, cd, logger, U, B, allow, frame_time, time_scale, num_iter, tol, progress_bar):
    """`smooth --timed`: the continuous-time chain on the frames' time stamps --
    ``data.ttb * time_scale``, or ``arange(F) * frame_time`` -- fitted by ``timed_fit`` next to the per-frame chain of
    ``hmm_fit`` at the same (U, B).  Writes ``<model>_smooth-timed<suffix>.tpqr`` and, per channel,
    ``<model>_smooth-timed<suffix>-channel<c>.csv`` with the rates in 1 / s; no other file is touched."""
    import pandas as pd
    import torch

    from tapqir_amd.exceptions import HipExtensionError
    from tapqir_amd.utils.mle_analysis import hmm_fit, timed_fit, timed_gaps

    data, M = m.data, U + B
    stem = f"{m.name}_smooth-timed{_smooth_suffix(U, B)}"
    if frame_time is not None:
        if not frame_time > 0.0:
            logger.error(f"smooth: --frame-time must be positive, got {frame_time}")
            raise typer.Exit(1)
        times = (torch.arange(data.F, dtype=torch.float64) * frame_time)[:, None].expand(data.F, data.C).clone()
    elif getattr(data, "ttb", None) is None:
        logger.error("smooth: --timed needs the time stamps of the frames: data.tpqr has no ttb (written by `glimpse`); "
                     "give --frame-time SECONDS for an equally spaced record")
        raise typer.Exit(1)
    else:
        times = torch.as_tensor(data.ttb).double().reshape(data.F, -1)[:, : data.C] * time_scale
    for c in range(data.C):
        try:
            timed_gaps(times[:, c])
        except ValueError:
            logger.error(f"smooth: the time stamps of channel {c} are not finite and strictly increasing")
            raise typer.Exit(1)
    topology = torch.tensor(allow, dtype=torch.bool)
    z_raw = m.params["z_probs"][: data.N, :, :, 1].float()  # (N, F, C)
    out = {"z_probs": z_raw.clone(), "state_probs": torch.full((*z_raw.shape, M), float("nan")), "z_map": z_raw > 0.5,
           "log_evidence": torch.full((data.N, data.C), float("nan"), dtype=torch.float64),
           "theta": torch.zeros(data.C, M * M + M, dtype=torch.float64), "prior": torch.zeros(data.C, dtype=torch.float64),
           "times": times, "bic": torch.zeros(data.C, dtype=torch.float64), "n_params": 0, "loglik_trace": [],
           "log_evidence_per_frame": torch.zeros(data.C, dtype=torch.float64), "mask": mask, "unbound": U, "bound": B,
           "topology_by_channel": torch.ones(data.C, M, M, dtype=torch.bool)}
    try:
        dev = torch.device("cuda")
        for c in range(data.C):
            logger.info(f"Channel #{c} ({data.channels[c]})")
            prior = float(torch.as_tensor(m.params["pi"]["Mean"]).reshape(-1, 2)[c, 1])
            p = z_raw[:, :, c][mask].to(dev)
            fit = timed_fit(p, prior, times[:, c], U, B, allow=topology, num_iter=num_iter, tol=tol, progress_bar=progress_bar)
            frame = hmm_fit(p, prior, U, B, num_iter=num_iter, tol=tol, progress_bar=progress_bar)
            logger.info(f"Continuous-time EM with {U} unbound and {B} bound states: log evidence = {fit['loglik']:.6f}, BIC = "
                        f"{fit['bic']:.6f} ({fit['n_params']} parameters) after {fit['iterations']} iterations")
            logger.info(f"Per-frame EM on the same data: log evidence = {frame['loglik']:.6f} ({frame['n_params']} parameters); "
                        f"the time stamps gain {fit['loglik'] - frame['loglik']:+.6f}")
            for name, f in (("continuous-time", fit), ("per-frame", frame)):
                if not f["converged"]:
                    logger.warning(f"smooth: the {name} EM did not converge to --tol {tol:g} within {f['iterations']} "
                                   f"iterations")
            theta = fit["theta"].cpu()
            Q = theta[: M * M].reshape(M, M)
            sums = fit["rows"][:, : M * M].sum(0).reshape(M, M).cpu()  # jumps off the diagonal, seconds on it
            jumps = sums - torch.diag(sums.diagonal())
            results = pd.DataFrame(columns=["EM"], dtype=float)
            for i in range(M):
                for j in range(M):
                    if i != j:
                        results.loc[f"q{i}{j}"] = [Q[i, j].item()]
            for i in range(M):  # mean dwell of state i in seconds, -1 / q_ii
                results.loc[f"dwell{i}"] = [(-1.0 / Q[i, i]).item()]
            results.loc["kon"] = [(jumps[:U, U:].sum() / sums.diagonal()[:U].sum()).item()]
            results.loc["koff"] = [(jumps[U:, :U].sum() / sums.diagonal()[U:].sum()).item()]
            results.to_csv(cd / f"{stem}-channel{c}.csv")
            logger.info(f"Saved the rates (1 / s) and dwells (s) in {stem}-channel{c}.csv file")
            smoothed = fit["gamma"][..., U:].sum(-1).float().cpu()
            out["z_probs"][:, :, c][mask] = smoothed
            out["state_probs"][:, :, c][mask] = fit["gamma"].float().cpu()
            out["z_map"][:, :, c][mask] = smoothed > 0.5
            out["log_evidence"][:, c][mask] = fit["rows"][:, -1].cpu()
            out["theta"][c] = theta
            out["prior"][c] = prior
            out["bic"][c] = fit["bic"]
            out["n_params"] = fit["n_params"]
            out["loglik_trace"].append(fit["trace"].cpu())
            out["log_evidence_per_frame"][c] = frame["loglik"]
            out["topology_by_channel"][c] = fit["allow"]  # in the canonical order of the states, as theta is
        torch.save(out, cd / f"{stem}.tpqr")
        logger.info(f"Saved the smoothed posterior in {stem}.tpqr file")
    except HipExtensionError:
        logger.exception("smooth failed: it needs an AMD GPU (--cuda) and the built HIP library")
        raise typer.Exit(1)


@app.command()
def smooth(
    model: avail_models = typer.Option("cosmos", help="Tapqir model"),
    cuda: bool = typer.Option(_default("cuda"), "--cuda/--cpu", help="Run computations on GPU or CPU", show_default=False),
    num_iter: int = typer.Option(200, "--num-iter", min=1, help="Largest number of EM iterations"),
    tol: float = typer.Option(1e-9, "--tol", help="Stop once an iteration gains at most tol * |log evidence|"),
    num_samples: int = typer.Option(1000, "--num-samples", "-n", min=1, help="Number of posterior rasters"),
    ci: float = typer.Option(0.95, "--ci", help="Probability mass of the interval, in (0, 1)"),
    bootstrap: bool = typer.Option(True, "--bootstrap/--no-bootstrap", help="Resample the AOIs of every posterior raster"),
    seed: Optional[int] = typer.Option(None, "--seed", help="Seed of the posterior rasters (default: the channel index)"),
    unbound_states: int = typer.Option(1, "--unbound-states", min=1, help="Hidden states that look unbound (z = 0)"),
    bound_states: int = typer.Option(1, "--bound-states", min=1, help="Hidden states that look bound (z = 1); at most 4 in all"),
    restarts: int = typer.Option(0, "--restarts", min=0, max=63, help="Random starts of the EM fitted next to the default start; the best one is kept"),
    restart_seed: int = typer.Option(0, "--restart-seed", help="Seed of the random starts"),
    forbid: Optional[List[str]] = typer.Option(None, "--forbid", help="i-j: fix the transition from state i to state j at the floor, 1e-9 (repeatable)"),
    populations: int = typer.Option(1, "--populations", help="Populations of AOIs, each with a chain of its own (1 to 4): a mixture of chains"),
    joint: Optional[str] = typer.Option(None, "--joint", help="A,B: smooth the colour channels A and B together as one chain of four states"),
    structure: Optional[str] = typer.Option(None, "--structure", help="With --joint: auto (the lowest BIC, the default), independent, a-drives-b, b-drives-a, coupled or full"),
    refit: int = typer.Option(0, "--refit", min=0, max=4096, help="Bootstrap refits of the chain over AOIs: the standard error and interval of the EM values"),
    refit_seed: int = typer.Option(0, "--refit-seed", help="Seed of the resamples of --refit"),
    timed: bool = typer.Option(False, "--timed", help="Fit a continuous-time chain on the frames' time stamps: rates in 1/s for records that are not equally spaced"),
    frame_time: Optional[float] = typer.Option(None, "--frame-time", help="With --timed: seconds between frames of an equally spaced record, in the place of the stamps of data.tpqr"),
    time_scale: float = typer.Option(0.001, "--time-scale", help="With --timed: seconds per unit of the time stamps of data.tpqr (Glimpse writes milliseconds)"),
    no_input: bool = typer.Option(False, "--no-input", help="Accepted for compatibility (there are no prompts)."),
    progress_bar=None,
):
    """
    Two-state hidden Markov smoothing of the fitted z posterior (the post-hoc counterpart of the reference's experimental
    cosmos+hmm model): the fit's ``z_probs`` are the evidence of a chain over the frames whose kon,
    koff and initial probability are fitted by EM over the on-target AOIs.  Writes the smoothed p(z = 1) and the Viterbi
    path to ``<model>_smooth.tpqr`` and, per channel, the rates to ``<model>_smooth-channel<c>.csv``: the EM value, mean and
    percentile interval over posterior rasters of the chain (resampled over AOIs unless ``--no-bootstrap``) and the rates
    of the Viterbi raster.  Needs ``data.tpqr`` and ``<model>_params.tpqr`` of a cosmos fit.

    With ``--unbound-states U --bound-states B`` other than 1 and 1 the chain has U + B <= 4 hidden states, U of them
    emitting the evidence of z = 0 and B that of z = 1: short-lived and long-lived complexes side by
    side.  The files are then ``<model>_smooth-u<U>b<B>.tpqr`` (with the state marginals, the Viterbi path in hidden
    states and the BIC: the lower, the better) and ``<model>_smooth-u<U>b<B>-channel<c>.csv`` (every entry of the
    transition matrix, the mean dwell of every state and the class-level kon and koff); the two-state files stay.

    With ``--restarts R`` the EM of such a chain runs from the default start and from R random starts (``--restart-seed``)
    side by side, and the start with the largest log evidence is kept; ``--forbid i-j`` (repeatable) removes the transition
    from hidden state i to hidden state j from the chain.  The file names do not change; the
    ``.tpqr`` gains ``restart_logliks``, ``restart_best`` and ``topology``, and the BIC counts the free entries only.
    Neither option applies to the two-state chain.

    With ``--joint A,B`` the colour channels A and B are smoothed together as one chain of the four states neither / only A
    / only B / both bound, fitted under five structures of its transition matrix -- ``independent``,
    ``a-drives-b``, ``b-drives-a``, ``coupled``, ``full`` -- side by side; the BIC ranks them and ``--structure`` forces one.
    Only ``<model>_smooth-joint<A><B>.tpqr`` and ``<model>_smooth-joint<A><B>.csv`` are written: the matrix, the on and off
    rates of each channel given the partner's state, and their ratios.

    With ``--populations G`` (2 to 4) the AOIs are a mixture of G populations, each with a chain of its own of the same
    ``--unbound-states`` / ``--bound-states``: molecules that differ -- an inactive fraction, two
    conformers -- where more bound states model one kind of molecule that switches; compare the BICs.  ``--restarts``,
    ``--restart-seed`` and ``--forbid`` apply, at (1, 1) too.  Only ``<model>_smooth-u<U>b<B>g<G>.tpqr`` (with every AOI's
    population probabilities) and ``<model>_smooth-u<U>b<B>g<G>-channel<c>.csv`` (weight, matrix, dwells and rates of
    every population) are written.

    With ``--refit R`` (1 to 4096) the EM of the single chain, at any (U, B) and under ``--forbid``, is run again from the
    fitted values on R resamples of the AOIs with replacement (``--refit-seed``), side by side.  The
    ``Mean`` / ``LL`` / ``UL`` of the channel CSV come from rasters drawn at the fitted chain and leave the uncertainty of
    the chain itself out; ``<model>_smooth<suffix>-refit-channel<c>.csv`` has, for the same rows, the EM value, the mean,
    the standard error and the percentile interval over the refits, and ``<model>_smooth<suffix>-refit.tpqr`` every
    refitted chain.  No other file changes.  ``--refit`` does not go with ``--joint`` or ``--populations``.

    With ``--timed`` the chain runs in continuous time on the time stamps of the frames: a generator
    Q in the place of the per-frame matrix, the transition over a gap d its exponential exp(Q d), fitted by EM.  Records
    whose frame interval changes, that pause for a reagent exchange or that drop frames are not equally spaced, and a
    per-frame matrix is then the wrong model.  The stamps are ``ttb`` of ``data.tpqr`` times ``--time-scale`` (seconds per
    unit; Glimpse writes milliseconds), or ``--frame-time SECONDS`` apart.  Runs at any ``--unbound-states`` /
    ``--bound-states`` and under ``--forbid`` (a forbidden rate is exactly 0), and fits the per-frame chain next to it: the
    difference of the two log evidences says whether the time stamps matter for the record.  Only
    ``<model>_smooth-timed<suffix>.tpqr`` and ``<model>_smooth-timed<suffix>-channel<c>.csv`` (every rate in 1 / s, every
    state's mean dwell in s, the class-level kon and koff) are written.  ``--timed`` does not go with ``--restarts``,
    ``--refit``, ``--joint``, ``--structure`` or ``--populations``.
    """
    import pandas as pd
    import torch

    from tapqir_amd.exceptions import HipExtensionError
    from tapqir_amd.utils.mle_analysis import (rates_estimate, rates_sample, rates_summary, smooth_fit, smooth_sample,
                                               smooth_viterbi)

    cd = DEFAULTS["cd"]
    logger = logging.getLogger("tapqir")
    if model.value == "cosmos" and not 0.0 < ci < 1.0:  # as in rates: after the model, before --cpu
        logger.error(f"smooth: --ci must be between 0 and 1, got {ci}")
        raise typer.Exit(1)
    if model.value == "cosmos" and unbound_states + bound_states > 4:
        logger.error(f"smooth: --unbound-states + --bound-states must be at most 4, got {unbound_states} + {bound_states}")
        raise typer.Exit(1)
    if model.value == "cosmos" and refit and (joint is not None or structure is not None or populations != 1):
        logger.error("smooth: --refit does not go with --joint or --populations: their M-steps (structure constraints, "
                     "responsibilities) have no weighted form yet")
        raise typer.Exit(1)
    if model.value == "cosmos" and timed and (restarts or restart_seed or refit or joint is not None or structure is not None
                                              or populations != 1):
        logger.error("smooth: --timed does not go with --restarts, --refit, --joint, --structure or --populations: the "
                     "replicas of those fits run the per-frame kernels")
        raise typer.Exit(1)
    if model.value == "cosmos" and not timed and frame_time is not None:
        logger.error("smooth: --frame-time needs --timed")
        raise typer.Exit(1)
    if model.value == "cosmos" and timed:
        allow = _smooth_forbid(unbound_states + bound_states, forbid, logger)
        m, mask, progress_bar = _kinetics_inputs("smooth", model, cuda, progress_bar)
        _smooth_timed(m, mask, cd, logger, unbound_states, bound_states, allow, frame_time, time_scale, num_iter, tol,
                      progress_bar)
        return
    mixture = None
    if model.value == "cosmos":
        mixture = _smooth_mixture_options(populations, unbound_states, bound_states, joint, structure, restarts, restart_seed,
                                          forbid, logger)
    pair = None
    if model.value == "cosmos" and (joint is not None or structure is not None):
        pair = _smooth_joint_options(joint, structure, unbound_states, bound_states, restarts, restart_seed, forbid, logger)
    multistart = None
    if model.value == "cosmos" and mixture is None and (restarts or restart_seed or forbid):
        multistart = _smooth_multistart_options(unbound_states, bound_states, restarts, restart_seed, forbid, logger)
    m, mask, progress_bar = _kinetics_inputs("smooth", model, cuda, progress_bar)
    if pair is not None:
        _smooth_joint(m, mask, cd, logger, pair, num_iter, tol, num_samples, ci, bootstrap, seed, progress_bar)
        return
    if mixture is not None:
        _smooth_mixture(m, mask, cd, logger, unbound_states, bound_states, mixture, num_iter, tol, num_samples, ci, bootstrap,
                        seed, progress_bar)
        return
    if (unbound_states, bound_states) != (1, 1):
        _smooth_multistate(m, mask, cd, logger, unbound_states, bound_states, num_iter, tol, num_samples, ci, bootstrap,
                           seed, progress_bar, multistart, refit and {"refits": refit, "seed": refit_seed})
        return
    data = m.data
    pct = f"{ci * 100:g}%"
    z_raw = m.params["z_probs"][: data.N, :, :, 1].float()  # (N, F, C)
    out = {"z_probs": z_raw.clone(), "z_map": z_raw > 0.5,
           "log_evidence": torch.full((data.N, data.C), float("nan"), dtype=torch.float64),
           "theta": torch.zeros(data.C, 3, dtype=torch.float64), "prior": torch.zeros(data.C, dtype=torch.float64),
           "loglik_trace": [], "mask": mask}
    refits = []
    try:
        dev = torch.device("cuda")
        for c in range(data.C):
            logger.info(f"Channel #{c} ({data.channels[c]})")
            prior = float(torch.as_tensor(m.params["pi"]["Mean"]).reshape(-1, 2)[c, 1])
            p = z_raw[:, :, c][mask].to(dev)
            chan_seed = c if seed is None else seed
            fit = smooth_fit(p, prior, num_iter=num_iter, tol=tol, progress_bar=progress_bar)
            theta = fit["theta"]
            kon, koff, pi0 = theta.tolist()
            logger.info(f"EM: kon = {kon:.6g}, koff = {koff:.6g}, pi0 = {pi0:.6g}, log evidence = "
                        f"{fit['rows'][:, 4].sum().item():.6f} after {fit['iterations']} iterations")
            if not fit["converged"]:
                logger.warning(f"smooth: the EM did not converge to --tol {tol:g} within {fit['iterations']} iterations")
            path = smooth_viterbi(p, theta, prior)
            summary = rates_summary(rates_estimate(smooth_sample(fit["filt"], theta, num_samples, seed=chan_seed),
                                                   bootstrap=bootstrap, seed=chan_seed), ci)
            map_est = rates_estimate(rates_sample(path.float(), 1, seed=chan_seed))  # p in {0, 1} is drawn as itself
            results = pd.DataFrame(columns=["EM", "Mean", f"{pct} LL", f"{pct} UL", "MAP"], dtype=float)
            for rate, em in (("kon", kon), ("koff", koff)):
                row = summary[rate]
                if row["left_out"]:
                    logger.info(f"{row['left_out']} of {num_samples} posterior rasters have a zero {rate} denominator "
                                f"and are left out of its mean and interval")
                results.loc[rate] = [em, row["mean"], row["ll"], row["ul"], map_est[rate][0].item()]
            results.to_csv(cd / f"{m.name}_smooth-channel{c}.csv")
            logger.info(f"Saved smoothed rate estimates in {m.name}_smooth-channel{c}.csv file")
            out["z_probs"][:, :, c][mask] = fit["gamma"].float().cpu()
            out["z_map"][:, :, c][mask] = path.bool().cpu()
            out["log_evidence"][:, c][mask] = fit["rows"][:, 4].cpu()
            out["theta"][c] = theta.cpu()
            out["prior"][c] = prior
            out["loglik_trace"].append(fit["trace"].cpu())
            if refit:  # the general kernels at U = B = 1 from (A, rho) of (kon, koff, pi0)
                start = torch.tensor([1.0 - kon, kon, koff, 1.0 - koff, 1.0 - pi0, pi0], dtype=torch.float64)
                refits.append(_smooth_refit(cd, f"{m.name}_smooth", c, p, prior, start, 1, 1,
                                            {"refits": refit, "seed": refit_seed}, None, num_iter, tol, ci, progress_bar, logger))
        torch.save(out, cd / f"{m.name}_smooth.tpqr")
        logger.info(f"Saved the smoothed posterior in {m.name}_smooth.tpqr file")
        if refit:
            _smooth_refit_save(cd, f"{m.name}_smooth", refits, {"refits": refit, "seed": refit_seed}, 1, 1, logger)
    except HipExtensionError:
        logger.exception("smooth failed: it needs an AMD GPU (--cuda) and the built HIP library")
        raise typer.Exit(1)


@app.command()
def log():
    """Show logging info (``.tapqir/loginfo``)."""
    path = DEFAULTS["cd"] / ".tapqir" / "loginfo"
    if path.is_file():
        typer.echo(path.read_text())


@app.callback()
def main(
    cd: Path = typer.Option(Path.cwd(), help="Change working directory.", show_default=False, exists=True,
                            file_okay=False, dir_okay=True),
    version: Optional[bool] = typer.Option(None, "--version", callback=_version, is_eager=True,
                                           help="Show version and exit."),
):
    """
    Bayesian analysis of co-localization single-molecule microscopy image data on AMD MI355X.

    Initializes a Tapqir workspace in the working directory: a ``.tapqir`` sub-directory with ``config.yaml``,
    ``loginfo`` and the files written by ``fit``.
    """
    DEFAULTS.clear()
    DEFAULTS["cd"] = cd
    tp = cd / ".tapqir"
    tp.mkdir(exist_ok=True)
    cfg = tp / "config.yaml"
    if not cfg.is_file():
        DEFAULTS.update({k: (dict(v) if isinstance(v, dict) else v) for k, v in CONFIG_DEFAULTS.items()})
        _write_config(cd)
        typer.echo(f"Initialized Tapqir at {tp}.")

    # the package's modules log under "tapqir_amd.*" (getLogger(__name__)); "tapqir" is kept for code written against the
    # reference's logger name (main.py:1353-1372)
    ch = logging.StreamHandler(sys.stdout)
    ch.setLevel(logging.INFO)
    ch.setFormatter(logging.Formatter("%(levelname)s - %(message)s"))
    fh = logging.FileHandler(tp / "loginfo")
    fh.setLevel(logging.DEBUG)
    fh.setFormatter(logging.Formatter(fmt="%(asctime)s - %(levelname)s - %(message)s", datefmt="%m/%d/%Y %I:%M %p"))
    for name in ("tapqir_amd", "tapqir"):
        lg = logging.getLogger(name)
        lg.setLevel(logging.DEBUG)
        for h in list(lg.handlers):  # repeated invocations in one process (tests) must not stack handlers
            lg.removeHandler(h)
            h.close()
        lg.addHandler(ch)
        lg.addHandler(fh)
    logger = logging.getLogger("tapqir_amd")

    with open(cfg) as f:
        DEFAULTS.update(yaml.safe_load(f) or {})
    logger.info(f"Configuration options are read from {cfg}.")


if __name__ == "__main__":
    app()
