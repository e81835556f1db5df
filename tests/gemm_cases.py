"""The case table of ava_gemm's dispatch paths, shared by test_cpu_gemm_cases.py (which kernel does each case reach:
asked of the library's own ava_gemm_path, no device) and test_gpu_gemm_paths.py (is that kernel right, on the device).

ava_gemm picks one of 36 kernel instantiations: the three-limb bf16 kernel (4), the skinny 16x16 kernel (4 operand
layouts x {256, 512} threads) and the LDS-tiled kernel ({128, 64} tiles x {BK32 vec, BK16 vec, BK16 scalar} x 4 layouts),
with splitk_reduce_kernel behind every split product.  Each case names the path it is there for; the shapes are the
smallest that take it and have M, N and K tails.  Everything here is host code (numpy / torch on the CPU)."""
import ctypes
from collections import namedtuple

import numpy as np
import torch

LIMB, SKINNY, TILED = 1, 2, 3
ACT_NONE, ACT_RELU, ACT_EXP = 0, 1, 2
PAD = 4          # floats of NaN padding behind every operand row (keeps lda % 4, so the 16-byte-load decision)
GUARD_ROWS = 3
SENTINEL = -7777.25

_Case = namedtuple("Case", "name M N K ak bk bias act mask colsum ldc dense offA offB offC expect faithful")


def case(name, M, N, K, ak, bk, expect, bias=False, act=ACT_NONE, mask=False, colsum=False, ldc=0, dense=False,
         offA=0, offB=0, offC=0, faithful=False):
    """expect = (path, tile, BK, vec, splits).  ldc: 0 = N.  dense: default leading dimensions (lda = ldb = 0) instead of
    NaN-padded operand rows.  offA / offB / offC: pointer moved by that many floats (misalignment)."""
    return _Case(name, M, N, K, ak, bk, bias, act, mask, colsum, ldc, dense, offA, offB, offC, tuple(expect), faithful)


def _layouts(name, M, N, K, expect, which=((1, 1), (1, 0), (0, 1), (0, 0)), **kw):
    return [case("%s_%d%d" % (name, ak, bk), M, N, K, ak, bk, expect, **kw) for ak, bk in which]


CASES = []
# ------------------------------------------------------------------------------------------------------------ tiled
# 128 x 128 tiles, BK 16, 16-byte loads, unsplit (klen 48): M tail 8, N tail 4, K tail 8
CASES += _layouts("t128_bk16", 520, 516, 40, (TILED, 128, 16, 1, 1), which=((1, 1), (0, 1)))
CASES += [case("t128_bk16_10_bias_relu", 520, 516, 40, 1, 0, (TILED, 128, 16, 1, 1), bias=True, act=ACT_RELU),
          case("t128_bk16_00_colsum", 520, 516, 40, 0, 0, (TILED, 128, 16, 1, 1), colsum=True)]
CASES += _layouts("t128_bk16_fin_mask_ldc", 520, 516, 40, (TILED, 128, 16, 1, 1), mask=True, ldc=520)
# 128 tiles, BK 32, split: 2 slabs, and fc7's forward product above batch 256 (8 slabs, the model's dense call)
CASES += [case("t128_bk32_s2_bias_relu", 520, 516, 64, 1, 1, (TILED, 128, 32, 1, 2), bias=True, act=ACT_RELU),
          case("t128_fc7_b260_bias_relu", 260, 1024, 256, 1, 1, (TILED, 128, 32, 1, 8), bias=True, act=ACT_RELU, dense=True)]
CASES += _layouts("t128_bk32_s2_mask_ldc", 520, 516, 64, (TILED, 128, 32, 1, 2), mask=True, ldc=520)
# column-sum partials behind the slabs
CASES += [case("t128_s2_colsum", 520, 516, 72, 0, 0, (TILED, 128, 16, 1, 2), colsum=True)]
# scalar loads: K % 4 != 0 (k-major operands), M % 4 != 0 (m-major A), a misaligned n-major B
CASES += [case("t128_scalar_11", 520, 515, 38, 1, 1, (TILED, 128, 16, 0, 1)),
          case("t128_scalar_10", 520, 515, 38, 1, 0, (TILED, 128, 16, 0, 1)),
          case("t128_scalar_01", 522, 515, 38, 0, 1, (TILED, 128, 16, 0, 1), colsum=True),
          case("t128_scalar_00_colsum", 522, 515, 38, 0, 0, (TILED, 128, 16, 0, 1), colsum=True),
          case("t128_scalar_00_offB", 520, 516, 40, 0, 0, (TILED, 128, 16, 0, 1), offB=1)]
# a misaligned C: scalar stores in the tile epilogue
CASES += [case("t128_bk16_11_offC", 520, 516, 40, 1, 1, (TILED, 128, 16, 1, 1), offC=1, ldc=520, mask=True)]
# 64 x 64 tiles, BK 16, 44 slabs: the last split is 8 long; the reduce sums 5 batches of 8 slabs and a remainder of 4
CASES += _layouts("t64_bk16_s44", 8, 200, 2072, (TILED, 64, 16, 1, 44))
CASES += [case("t64_deep_s86", 5, 64, 4100, 1, 1, (TILED, 64, 16, 1, 86))]
CASES += [case("t64_scalar_11", 70, 130, 37, 1, 1, (TILED, 64, 16, 0, 1)),
          case("t64_scalar_01", 70, 130, 37, 0, 1, (TILED, 64, 16, 0, 1), colsum=True),
          case("t64_scalar_10_s43", 70, 130, 2051, 1, 0, (TILED, 64, 16, 0, 43)),
          case("t64_scalar_00_s43_colsum", 70, 130, 2051, 0, 0, (TILED, 64, 16, 0, 43), colsum=True),
          case("t64_scalar_11_s2_offA", 70, 132, 64, 1, 1, (TILED, 64, 16, 0, 2), offA=1)]
# 64 tiles, BK 32: the "wide" plan, unsplit, klen 544 against K = 540 (K tail 28)
CASES += _layouts("t64_bk32_wide", 200, 6100, 540, (TILED, 64, 32, 1, 1), which=((1, 0), (0, 1), (0, 0)))
CASES += [case("t64_bk32_wide_11_bias_relu", 200, 6100, 540, 1, 1, (TILED, 64, 32, 1, 1), bias=True, act=ACT_RELU)]
# limb-shaped products the limb kernel declines: exp epilogue; K % 8 != 0
CASES += [case("t64_limbshape_exp", 4, 2048, 2056, 1, 1, (TILED, 64, 16, 1, 15), bias=True, act=ACT_EXP),
          case("t128_limbshape_k2052", 130, 2052, 2052, 1, 1, (TILED, 128, 16, 1, 15))]
# ----------------------------------------------------------------------------------------------------------- skinny
# (37, 52, K): 256 threads at K = 40; 512 threads at K = 516 (33 chunks: a second pass that only wave 0 takes)
CASES += [case("sk256_11_bias_relu", 37, 52, 40, 1, 1, (SKINNY, 16, 16, 1, 1), bias=True, act=ACT_RELU),
          case("sk256_10_exp", 37, 52, 40, 1, 0, (SKINNY, 16, 16, 1, 1), bias=True, act=ACT_EXP),
          case("sk256_01_mask_ldc_colsum", 37, 52, 40, 0, 1, (SKINNY, 16, 16, 1, 1), mask=True, ldc=56, colsum=True),
          case("sk256_00_colsum_bias_relu", 37, 52, 40, 0, 0, (SKINNY, 16, 16, 0, 1), colsum=True, bias=True, act=ACT_RELU),
          case("sk512_11_mask_ldc", 37, 52, 516, 1, 1, (SKINNY, 16, 16, 1, 1), mask=True, ldc=56),
          case("sk512_10_bias_relu", 37, 52, 516, 1, 0, (SKINNY, 16, 16, 1, 1), bias=True, act=ACT_RELU),
          case("sk512_01_exp_colsum", 37, 52, 516, 0, 1, (SKINNY, 16, 16, 1, 1), bias=True, act=ACT_EXP, colsum=True),
          case("sk512_00_mask_ldc_colsum", 37, 52, 516, 0, 0, (SKINNY, 16, 16, 0, 1), mask=True, ldc=56, colsum=True)]
# ------------------------------------------------------------------------------------------------------------- limb
# 128 x 64 tiles, 8 splits of 288 (the last 40 long: a partial K step), M tail 2, N tail 4; 528 items, more than the
# resident workgroups of a 256-CU part, so some workgroups take a second item of another split
CASES += _layouts("l64_s8", 130, 2052, 2056, (LIMB, 64, 32, 1, 8), which=((1, 1), (1, 0)))
# unsplit (561 tiles), the epilogue's bias + ReLU + mask with ldc > N, K = 40 inside one 64-long step
CASES += _layouts("l64_fin_bias_relu_mask_ldc", 2052, 2052, 40, (LIMB, 64, 32, 1, 1), which=((1, 1), (1, 0)),
                  bias=True, act=ACT_RELU, mask=True, ldc=2056)
# split, finished by the reduce kernel with bias + ReLU + mask and ldc > N (516 items)
CASES += [case("l64_s2_bias_relu_mask_ldc", 256, 8256, 1024, 1, 1, (LIMB, 64, 32, 1, 2), bias=True, act=ACT_RELU,
               mask=True, ldc=8260)]
CASES += [case("l64_single_row", 1, 2052, 2056, 1, 1, (LIMB, 64, 32, 1, 13))]
# 128 x 128 tiles (m-major A): K below one step, split with column sums, and the k-major-B instantiation
CASES += [case("l128_k12_colsum", 2052, 2060, 12, 0, 0, (LIMB, 128, 32, 1, 1), colsum=True),
          case("l128_k5_colsum", 2052, 2060, 5, 0, 0, (LIMB, 128, 32, 1, 1), colsum=True),
          case("l128_s8_colsum", 132, 2052, 2056, 0, 0, (LIMB, 128, 32, 1, 8), colsum=True),
          case("l128_bkmajor_s8", 2052, 132, 2056, 0, 1, (LIMB, 128, 32, 1, 8), colsum=True)]
# limb faithfulness: K = 64, where 4 x e_seq separates six limb pairs from five (test_cpu_gemm_cases.py)
CASES += [case("l64_faithful", 2048, 2052, 64, 1, 1, (LIMB, 64, 32, 1, 1), faithful=True),
          case("l128_faithful", 2052, 2060, 64, 0, 0, (LIMB, 128, 32, 1, 1), faithful=True)]

assert len({c.name for c in CASES}) == len(CASES)
BY_NAME = {c.name: c for c in CASES}

ALL_INSTANTIATIONS = (
    {("limb", 64, 1, 1), ("limb", 64, 1, 0), ("limb", 128, 0, 1), ("limb", 128, 0, 0)}
    | {("skinny", ak, bk, th) for ak in (0, 1) for bk in (0, 1) for th in (256, 512)}
    | {("tiled", bm, kind, ak, bk) for bm in (128, 64) for kind in ("bk32vec", "bk16vec", "bk16scalar")
       for ak in (0, 1) for bk in (0, 1)})
assert len(ALL_INSTANTIATIONS) == 36


def instantiation(c, path, info):
    """the kernel instantiation behind an ava_gemm_path answer"""
    tile, bk, vec, _splits, _klen, threads = info
    if path == LIMB:
        return ("limb", tile, c.ak, c.bk)
    if path == SKINNY:
        return ("skinny", c.ak, c.bk, threads)
    return ("tiled", tile, "bk32vec" if bk == 32 else ("bk16vec" if vec else "bk16scalar"), c.ak, c.bk)


def leading_dims(c):
    """(lda, ldb, ldc) as passed to ava_gemm, and the stored row lengths behind them"""
    na, nb = (c.K if c.ak else c.M), (c.K if c.bk else c.N)
    if c.dense:
        return (0, 0, c.ldc), (na, nb, c.ldc or c.N)
    return (na + PAD, nb + PAD, c.ldc), (na + PAD, nb + PAD, c.ldc or c.N)


def query(lib, c, A, B, bias, C, mask, colsum):
    """ava_gemm_path on pointer VALUES (ints or None): (path, info[6])"""
    (lda, ldb, ldc), _ = leading_dims(c)
    info = (ctypes.c_int * 6)()
    path = lib.ava_gemm_path(A, lda, B, ldb, bias, C, ldc, mask, colsum, c.M, c.N, c.K, c.ak, c.bk, c.act, info)
    return path, tuple(info)


def dummy_pointers(c):
    """aligned pointer values that are never dereferenced, moved by 4 bytes per misaligned float"""
    return dict(A=4096 + 4 * c.offA, B=(1 << 20) + 4 * c.offB, bias=(2 << 20) if c.bias else None,
                C=(3 << 20) + 4 * c.offC, mask=(4 << 20) if c.mask else None,
                colsum=(5 << 20) if c.colsum else None)


# ---------------------------------------------------------------------------------------------------- inputs, reference
def _f32(x):
    return x.astype(np.float32).astype(np.float64)


def make_inputs(c):
    """Seeded fp64 operands whose values are fp32 numbers (the device receives them unchanged): A [M,K], B [K,N],
    bias [N], mask [M,N].  exp cases are scaled so that the pre-activation stays within a few units."""
    rng = np.random.default_rng(1000 + CASES.index(c))
    A = _f32(rng.standard_normal((c.M, c.K)))
    B = _f32(rng.standard_normal((c.K, c.N)))
    if c.act == ACT_EXP:
        B = _f32(B / np.sqrt(c.K))
    bias = _f32(rng.standard_normal(c.N)) if c.bias else None
    mask = _f32(rng.standard_normal((c.M, c.N))) if c.mask else None
    return A, B, bias, mask


def reference(c, A, B, bias):
    """fp64: (pre-activation, |A| |B|).  Activation and mask are applied by `finish`."""
    pre = A @ B
    if bias is not None:
        pre = pre + bias
    return pre, np.abs(A) @ np.abs(B)


def finish(c, pre, mask):
    out = np.maximum(pre, 0.0) if c.act == ACT_RELU else (np.exp(pre) if c.act == ACT_EXP else pre)
    return np.where(mask > 0, out, 0.0) if mask is not None else out


def sample(c):
    """the fixed 16-row x 64-column sample of the output"""
    rows = np.unique(np.linspace(0, c.M - 1, 16).round().astype(np.int64))
    cols = np.unique(np.linspace(0, c.N - 1, 64).round().astype(np.int64))
    return rows, cols


def metric(c, got, pre, denom, mask=None):
    """e = max |got - want| / (|A| |B|), on the pre-activation for exp (recovered with log); masked-out elements are
    left to the caller (they must be exactly 0)."""
    got = np.asarray(got, np.float64)
    if c.act == ACT_EXP:
        with np.errstate(divide="ignore", invalid="ignore"):
            err = np.abs(np.log(got) - pre)
    elif c.act == ACT_RELU:
        err = np.abs(got - np.maximum(pre, 0.0))
    else:
        err = np.abs(got - pre)
    err = err / denom
    if mask is not None:
        err = np.where(mask > 0, err, 0.0)
    return float(np.nan_to_num(err, nan=np.inf).max())


def e_seq(c, A, B, bias, pre, denom):
    """The metric of a plain sequential fp32 accumulation on the sample: ascending k, one rounding per term (the product
    of two fp32 numbers is exact in fp64), then bias and activation in fp32.  This is the fp32 noise of the worst
    ordering a correct fp32 kernel can have."""
    rows, cols = sample(c)
    As, Bs = A[rows], B[:, cols]
    acc = np.zeros((len(rows), len(cols)), np.float32)
    for k in range(c.K):
        acc = (acc.astype(np.float64) + As[:, k:k + 1] * Bs[k:k + 1, :]).astype(np.float32)
    if bias is not None:
        acc = (acc + bias[cols].astype(np.float32)).astype(np.float32)
    if c.act == ACT_RELU:
        acc = np.maximum(acc, np.float32(0))
    elif c.act == ACT_EXP:
        acc = np.exp(acc)
    return metric(c, acc, pre[np.ix_(rows, cols)], denom[np.ix_(rows, cols)])


def limb_planes(x):
    """x (fp32 values) = x0 + x1 + x2: three bfloat16 roundings of successive remainders (gemm_limb.hip: limb_split2)"""
    r = torch.from_numpy(np.ascontiguousarray(x)).to(torch.float32)
    planes = []
    for _ in range(3):
        p = r.to(torch.bfloat16).to(torch.float32)
        planes.append(p.double().numpy())
        r = r - p                                   # exact in fp32
    return planes


def limb_product(A, B, drop_a2b0=False):
    """the limb kernel's product with exact (fp64) accumulation: the six pairs with i + j <= 2, or five of them"""
    a0, a1, a2 = limb_planes(A)
    b0, b1, b2 = limb_planes(B)
    out = a0 @ (b0 + b1 + b2) + a1 @ (b0 + b1)
    return out if drop_a2b0 else out + a2 @ b0
