"""Every dispatch path of ava_gemm on the device, over the case table of gemm_cases.py: the limb kernel, the skinny kernel
at both block sizes, all 24 instantiations of the LDS-tiled kernel and the split-K reduce behind them, at M, N and K tails,
with padded leading dimensions, misaligned pointers and every epilogue.

Per case: the dispatcher (ava_gemm_path on the very arguments of the call) takes the path the case names; operand rows are
padded with NaN, so a read past an extent that reaches the product shows; C and the column sums are pre-filled with a
sentinel that must survive outside [0, M) x [0, N); split products repeat bit for bit.

Accuracy: e = max |C - want| / (|A| |B|) against an fp64 reference, and the bound is 4 x e_seq, the same figure for a plain
sequential fp32 accumulation of the same case on a 16 x 64 sample (gemm_cases.e_seq).  e_seq is the fp32 noise of the
worst ordering a correct fp32 kernel can have; 4 covers sample against whole matrix and differences of order; one lost
term is about 1 / K on this metric, and test_cpu_gemm_cases.py shows that at K = 64 the bound rejects a limb kernel that
drops a single third-order limb pair.  Column sums: the same metric against sum_k |A|, the same bound (both are K-term fp32
accumulations measured against the sum of the terms' magnitudes).  Run with -m gpu on the MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_cases as G
from gpu_util import gemm


def _embed(x, ld, off):
    """x [rows, cols] -> device view of a [rows, ld] buffer, NaN behind every row, `off` floats into its allocation"""
    rows, cols = x.shape
    flat = torch.full((off + rows * ld,), float("nan"), dtype=torch.float32)
    flat[off:].view(rows, ld)[:, :cols] = torch.from_numpy(np.ascontiguousarray(x)).float()
    return flat.cuda()[off:]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c.name)
def test_gemm_path(c):
    A, B, bias, mask = G.make_inputs(c)
    pre, denom = G.reference(c, A, B, bias)
    e_seq = G.e_seq(c, A, B, bias, pre, denom)
    bound = 4.0 * e_seq
    (lda, ldb, ldc), (sa, sb, sc) = G.leading_dims(c)
    Ad = _embed(A if c.ak else A.T, sa, c.offA)
    Bd = _embed(B.T if c.bk else B, sb, c.offB)
    biasd = torch.from_numpy(bias).float().cuda() if c.bias else None
    maskd = _embed(mask, sc, 0) if c.mask else None

    def run():
        info = []
        try:
            C, cs = gemm(Ad, Bd, c.M, c.N, c.K, c.ak, c.bk, bias=biasd, act=c.act, mask=maskd, colsum=c.colsum, lda=lda,
                         ldb=ldb, ldc=ldc, guard_rows=G.GUARD_ROWS, fill=G.SENTINEL, c_offset=c.offC, path_info=info)
            return info[0], C.cpu().numpy(), (cs.cpu().numpy() if c.colsum else None)
        except RuntimeError as err:       # a device error poisons the context: no further kernels on it
            pytest.exit("device error in %s: %s" % (c.name, err), returncode=3)

    (path, info), got, cs = run()
    assert (path,) + info[:4] == c.expect, "the dispatcher no longer takes the path this case is there for"

    # guards: nothing outside [0, M) x [0, N) is written
    sent = _bits(np.float32(G.SENTINEL))
    outside = np.ones(got.shape, bool)
    outside[:c.M, :c.N] = False
    assert (_bits(got)[outside] == sent).all(), "C written outside [0, M) x [0, N)"
    inner = got[:c.M, :c.N]
    assert np.isfinite(inner).all(), "NaN / inf in C: an out-of-range operand reached the product"
    if c.mask:
        assert (inner[~(mask > 0)] == 0.0).all()
    e = G.metric(c, inner, pre, denom, mask)
    print("\n%s path %d: e %.3g  e_seq %.3g  ratio %.2f" % (c.name, path, e, e_seq, e / e_seq), end="")
    e_cs = 0.0
    if c.colsum:
        assert (_bits(cs[c.M:]) == sent).all(), "colsum written behind M"
        assert np.isfinite(cs[:c.M]).all()
        e_cs = float((np.abs(cs[:c.M].astype(np.float64) - A.sum(axis=1)) / np.abs(A).sum(axis=1)).max())
        print("  colsum e %.3g ratio %.2f" % (e_cs, e_cs / e_seq), end="")
    assert e <= bound
    assert e_cs <= bound

    if info[3] > 1:          # split-K: the slabs are summed in a fixed order
        _, got2, cs2 = run()
        assert (_bits(got2) == _bits(got)).all()
        assert cs is None or (_bits(cs2) == _bits(cs)).all()
