"""Writes tests/golden/mmd_matrix.npz: the reference's own ``_calculate_mmd2`` (ava/plotting/mmd_plots.py:337-434) on the
golden case of tests/mmd_matrix_cases.py.  Needs the reference package, scipy, scikit-learn, joblib and matplotlib; run
from the repository root as ``python tests/golden/make_golden_mmd_matrix.py /path/to/reference``.  The tests only read
the npz.

The case: ``synthetic.latent_conditions(n_per=(12, 9, 17, 2), z=8, salt=9200)``, the conditions renamed to
``[40, -3, 7, 0]``, the rows interleaved by ``np.argsort(synthetic.gauss(N, 77), kind='stable')``, ``sigma = 2.0``, a
stub container whose ``request`` hands out the latent means and file names that ``condition_from_fn`` parses back to
the condition.  The serial branch runs (``parallel=False``), so no joblib worker starts.

Recorded:
  ``quadratic``, ``linear``  the ``[4, 4]`` MMD^2 matrices of the two estimators
  ``conditions``             the sorted conditions the reference returns (and saves): ``[-3, 0, 7, 40]``
The files the reference saves are read back and asserted equal to what it returned, and the numpy restatement of
tests/mmd_matrix_cases.py is asserted to agree to 1e-11 relative before anything is written.
"""
import contextlib
import io
import os
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mmd_matrix_cases as MC                                # noqa: E402  (before the reference's ``ava`` shadows nothing of ours)

REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("AVA_REFERENCE", "../reference")


def load_reference_mmd_plots():
    """``ava/plotting/mmd_plots.py`` of the reference as a module of its own: the file only imports third-party
    packages, and loading it by path keeps the repository's ``ava`` shim package out of the way"""
    import importlib.util
    path = os.path.join(REFERENCE, "ava", "plotting", "mmd_plots.py")
    spec = importlib.util.spec_from_file_location("reference_mmd_plots", path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def main():
    mp = load_reference_mmd_plots()
    latent, condition = MC.golden_case()
    out = {}
    root = tempfile.mkdtemp()
    try:
        for alg in ('quadratic', 'linear'):
            dc = MC.StubDC(latent, condition)
            mmd2_fn, condition_fn = os.path.join(root, alg + "_mmd2.npy"), os.path.join(root, alg + "_cond.npy")
            with contextlib.redirect_stdout(io.StringIO()):
                result, conditions = mp._calculate_mmd2(dc, MC.condition_from_fn, mmd2_fn=mmd2_fn,
                                                        condition_fn=condition_fn, alg=alg, sigma=MC.GOLDEN_SIGMA)
            assert np.array_equal(np.load(mmd2_fn), result) and np.array_equal(np.load(condition_fn), conditions)
            want, want_conditions = MC.matrix_oracle(latent, condition, alg, MC.GOLDEN_SIGMA)
            assert np.array_equal(conditions, want_conditions)
            dev = MC.max_rel(want, result)
            off = np.abs(result[~np.eye(len(result), dtype=bool)])
            print("%-9s conditions %s, off-diagonal |mmd2| %.4g .. %.4g, restatement within %.3g relative, %.3g absolute"
                  % (alg, conditions.tolist(), off.min(), off.max(), dev, np.abs(want - result).max()))
            assert dev < 1e-11 and np.array_equal(np.diag(result), np.zeros(len(result)))
            out[alg] = result
            if "conditions" in out:
                assert np.array_equal(out["conditions"], conditions)
            out["conditions"] = np.asarray(conditions, dtype=np.int64)
    finally:
        shutil.rmtree(root)
    assert out["conditions"].tolist() == sorted(MC.GOLDEN_LABELS)
    path = os.path.join(HERE, "mmd_matrix.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
