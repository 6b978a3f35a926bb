"""
Generate the golden vectors of the dwell-time interval helpers from the reference.

Run it with a checkout of the reference Tapqir:

    python tests/golden/make_dwell_golden.py <path to the Tapqir checkout>

It loads ``<checkout>/tapqir/utils/imscroll.py`` by file path, with stub ``pyro`` / ``pyro.ops`` / ``pyro.ops.stats``
/ ``pyroapi`` modules in ``sys.modules`` (the interval helpers use none of them), runs ``count_intervals``,
``bound_dwell_times`` and ``unbound_dwell_times`` on random and edge-case rasters, and stores inputs and outputs in
``tests/golden/dwell_golden.npz``.  The .npz holds data only; no reference source travels with the repo.
"""

import importlib.util
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dwell_golden.npz")
COLUMNS = ["posterior_sample", "aoi", "start_frame", "stop_frame", "dwell_time", "low_or_high", "z"]


def load_reference(checkout):
    pyro = types.ModuleType("pyro")
    ops = types.ModuleType("pyro.ops")
    stats = types.ModuleType("pyro.ops.stats")
    stats.pi = None
    stats.resample = None
    pyro.ops, ops.stats = ops, stats
    pyroapi = types.ModuleType("pyroapi")
    pyroapi.distributions = torch.distributions
    sys.modules.update({"pyro": pyro, "pyro.ops": ops, "pyro.ops.stats": stats, "pyroapi": pyroapi})
    path = os.path.join(checkout, "tapqir", "utils", "imscroll.py")
    spec = importlib.util.spec_from_file_location("ref_imscroll", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    return ref


def rasters(rng):
    """name -> (S, N, F) int64 0/1 rasters."""
    out = {}
    z = (rng.random((6, 9, 40)) < rng.choice([0.05, 0.3, 0.7, 0.95], size=(1, 9, 1))).astype(np.int64)
    z[:, 0] = 0                 # all 0
    z[:, 1] = 1                 # all 1
    z[:, 2] = np.arange(40) % 2  # alternating, starting unbound
    z[:, 3] = 1 - np.arange(40) % 2
    out["rand"] = z
    out["f1"] = (rng.random((4, 5, 1)) < 0.5).astype(np.int64)
    out["f2"] = np.array([[[0, 0], [0, 1], [1, 0], [1, 1]]] * 3, dtype=np.int64)
    z = (rng.random((5, 6, 25)) < 0.4).astype(np.int64)
    z[0] = 0                    # sample 0 has no interval of either interior kind: the padded rows shift
    z[3, :, 10:] = 1            # sample 3 has no interior bound run ...
    z[3, :, :10] = np.array([0, 1] * 5)
    out["gap"] = z
    out["long"] = (rng.random((3, 4, 300)) < 0.1).astype(np.int64)
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = load_reference(sys.argv[1])
    rng = np.random.default_rng(20261016)
    out = {}
    for name, z in rasters(rng).items():
        out[f"{name}_raster"] = z
        table = ref.count_intervals(z)
        table_t = ref.count_intervals(torch.from_numpy(z))
        for col in COLUMNS:
            a, b = table[col].to_numpy(), np.asarray(table_t[col])
            assert np.array_equal(a, b) and a.dtype == np.int64, (name, col)
            out[f"{name}_{col}"] = a
        for kind, fn in (("bound", ref.bound_dwell_times), ("unbound", ref.unbound_dwell_times)):
            if ((table["low_or_high"] == (1 if kind == "bound" else 0)).any()):
                out[f"{name}_{kind}"] = fn(table)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(out)} arrays")


if __name__ == "__main__":
    main()
