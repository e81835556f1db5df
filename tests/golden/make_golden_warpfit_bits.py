"""Writes tests/golden/warpfit_bits.npz: the bit patterns of what the loss, apply and grouped-mean kernels of
csrc/warp_fit.hip compute, recorded on an MI355X at commit d080acb ("Silhouette and cluster-validity scores on the
device (f21)"), the last one with a loss body, a loss kernel and a launch path per warp form and per plain / grouped
fit.  The kernels have been folded into one of each since; tests/test_gpu_warpfit.py holds them to these bits, which no
comparison of two outputs of today's code with each other can do.

Outputs only: ``warpfit_cases.bits_record`` regenerates the hashed inputs and makes every call, here and in the test.
Needs the device and a built library; run from the repository root as
``python tests/golden/make_golden_warpfit_bits.py`` -- at a commit whose bits are known to be right: after a deliberate
change of the warp objective's arithmetic, not to make a failing test pass.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import warpfit_cases as FC                                      # noqa: E402


def main():
    out = FC.bits_record()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "warpfit_bits.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d values, %d bytes" % (path, len(out), sum(v.size for v in out.values()),
                                                       os.path.getsize(path)))


if __name__ == "__main__":
    main()
