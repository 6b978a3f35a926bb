"""Writes tests/golden/mixture_golden.npz: the numpy oracle's results of the model-choice table of the mixture-of-chains tests
(mixture_fixture.choice_summary: 150 EM iterations of four models on five data sets in float64 and longdouble, about a
minute), so that the GPU tests read them; test_mixture_host.py recomputes them and compares bit for bit.

    python tests/golden/make_mixture_golden.py
"""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import mixture_fixture as mf  # noqa: E402

if __name__ == "__main__":
    np.savez(mf.GOLDEN, **mf.choice_summary())
    print("wrote", mf.GOLDEN)
