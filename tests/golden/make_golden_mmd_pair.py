"""Writes tests/golden/mmd_pair_gpu.npz: what the per-pair MMD^2 estimators of ava_amd.mmd give ON THE DEVICE, recorded
at the last commit whose ``_terms`` and ``_estimate_mmd2_linear_time`` ran kernels of their own (``mmd_pair`` /
``mmd_linear`` / ``mmd_finalize`` of csrc/mmd.hip), before they became two-condition calls of the one-pass matrix
kernels.  Needs the MI355X; run from the repository root as ``python tests/golden/make_golden_mmd_pair.py``.  It calls
only ``mmd._latent_dev``, ``mmd._terms``, ``mmd._estimate_mmd2`` and ``mmd._estimate_mmd2_linear_time`` on the cases of
tests/mmd_matrix_cases.py and tests/test_mmd.py, so it runs unchanged at that commit and at every later one, where it
must reproduce every array bit for bit (``--check`` compares with the committed file instead of writing it).

Recorded:
  ``terms_z1``, ``terms_z32``, ``terms_z128``  ``[15, 4]``: ``_terms`` of every pair a < b (row-major) of ``MC.edge_case(z)``
                                               with ``MC.edge_sigma(z)``
  ``linear_edge`` ``[15]``, ``linear_two_workgroups`` ``[3]``  ``_estimate_mmd2_linear_time`` of every pair of
                                               ``MC.edge_case(32)`` and ``MC.linear_case()``, ``MC.edge_sigma(32)``
  ``quad`` ``[5]``                             the ``_estimate_mmd2`` calls of tests/test_mmd.py with a given sigma: the
                                               pairs (0, 1), (0, 2), (1, 2), the pair (0, 2) under ``max_n=40, seed=3``
                                               and the two halves of condition 1 at half the bandwidth

The file holds results of this device's ``exp``: it is a regression pin for this toolchain (ROCm's device libraries on
gfx950), not a portable reference.  The portable check stays the 1e-11 comparison with oracle/mmd_oracle.py that
tests/test_mmd.py and tests/test_gpu_mmd_matrix.py make.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mmd_matrix_cases as MC                                # noqa: E402
import test_mmd as TM                                        # noqa: E402

PATH = os.path.join(HERE, "mmd_pair_gpu.npz")


def compute():
    from ava_amd import mmd
    out = {}
    for z in (1, 32, 128):
        latent, condition = MC.edge_case(z)
        _, idx = MC.pair_indices(condition)
        L = mmd._latent_dev(latent)
        out["terms_z%d" % z] = np.array([mmd._terms(L, idx[a], idx[b], MC.edge_sigma(z))
                                         for a in range(len(idx) - 1) for b in range(a + 1, len(idx))])
    for key, (latent, condition) in (("linear_edge", MC.edge_case(32)), ("linear_two_workgroups", MC.linear_case())):
        _, idx = MC.pair_indices(condition)
        L = mmd._latent_dev(latent)
        out[key] = np.array([mmd._estimate_mmd2_linear_time(L, idx[a], idx[b], sigma=MC.edge_sigma(32))
                             for a in range(len(idx) - 1) for b in range(a + 1, len(idx))])
    latent, idx = TM._sets()
    sigma = float(np.load(os.path.join(HERE, "mmd.npz"))["sigma_default_seed"])
    quad = [mmd._estimate_mmd2(latent, idx[a].copy(), idx[b].copy(), sigma=sigma) for a, b in ((0, 1), (0, 2), (1, 2))]
    quad.append(mmd._estimate_mmd2(latent, idx[0].copy(), idx[2].copy(), sigma=sigma, max_n=40, seed=3))
    quad.append(mmd._estimate_mmd2(latent, idx[1][:26].copy(), idx[1][26:].copy(), sigma=0.5 * sigma))
    out["quad"] = np.array(quad)
    return out


def main():
    out = compute()
    assert all(v.dtype == np.float64 and np.isfinite(v).all() for v in out.values())
    assert out["terms_z32"].shape == (15, 4) and out["linear_edge"].shape == (15,)
    assert out["linear_two_workgroups"].shape == (3,) and out["quad"].shape == (5,)
    if "--check" in sys.argv[1:]:
        want = dict(np.load(PATH, allow_pickle=False))
        assert sorted(want) == sorted(out)
        for k in sorted(out):
            assert np.array_equal(out[k], want[k]), k
        print("reproduced every array of", PATH, "bit for bit:", sorted(out))
        return
    np.savez_compressed(PATH, **out)
    print("wrote", PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
