"""The training step's statistics, layout and reduction kernels (csrc/bn.hip, csrc/misc.hip, csrc/bn_acc.h) against the numpy
restatement of tests/step_kernel_cases.py, at the sizes where a workgroup takes more than one tile, a reduction more than
one pass and a grid its cap.  The inputs make every sum exact (test_cpu_step_kernels.py proves that for each shape used
here), so sums, permutations and single roundings compare with ==; what goes through a square root, a logarithm or Adam's
division keeps the bound tests/test_gpu_kernels.py asserts for the same quantity.  Every output lies inside a larger
allocation filled with a sentinel that must survive on both sides."""
import ctypes

import numpy as np
import pytest
import torch

import step_kernel_cases as SC
from gpu_util import dev, p, rel, stream
from ava_amd import _lib, synthetic as syn
from oracle import vae_oracle as O

pytestmark = pytest.mark.gpu

GUARD = 256
SENT = -12345.0
SENT_LL = -(2 ** 62) + 5
SENT_H = 0x7B7B


def guarded(n, dtype=torch.float32, fill=SENT):
    """(allocation, the n elements in its middle): both sides are GUARD elements of ``fill``"""
    flat = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return flat, flat[GUARD:GUARD + n]


def intact(flat, fill=SENT):
    return bool((flat[:GUARD] == fill).all()) and bool((flat[-GUARD:] == fill).all())


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def ok(rc, what):
    _lib.check(rc, what)


def zero_slot():
    flat, slot = guarded(SC.ACC_SHARDS * SC.ACC_SHARD_LL, torch.int64, SENT_LL)
    slot.zero_()
    return flat, slot


def slot_to_device(slot_np):
    flat, slot = guarded(SC.ACC_SHARDS * SC.ACC_SHARD_LL, torch.int64, SENT_LL)
    slot.copy_(torch.from_numpy(np.ascontiguousarray(slot_np).reshape(-1)))
    return flat, slot


def slot_np(slot):
    return slot.cpu().numpy().reshape(SC.ACC_SHARDS, SC.ACC_SHARD_LL)


def test_slot_constants():
    lib = _lib.load()
    assert lib.ava_acc_shards() == SC.ACC_SHARDS and lib.ava_acc_shard_ll() == SC.ACC_SHARD_LL


# ---- nchw_to_nhwc_stats (plain and two-slab), 1024-workgroup cap -----------------------------------------------------------
def run_stats(case, acc):
    """one launch: (out as float32 values [B, P, 32], full or None, partials rows or None, slot or None, nparts)"""
    lib = _lib.load()
    B, P, bf16 = case["B"], case["P"], case["bf16"]
    n = B * 32 * P
    x, s1, bias = dev(case["in"]), None, None
    full_flat = full = None
    if case["slab1"] is not None:
        s1 = dev(case["slab1"])
        bias = dev(case["bias"]) if case["bias"] is not None else None
        full_flat, full = guarded(n)
    if bf16:
        out_flat, out = guarded(n, torch.int16, SENT_H)
    else:
        out_flat, out = guarded(n)
    part_flat, part = guarded(SC.STATS_CAP * 64)
    slot_flat, slot = zero_slot()
    nparts = ctypes.c_int(-1)
    ok(lib.ava_layout_nchw_to_nhwc_stats(p(x), p(s1), p(bias), case["relu"], p(full), p(out), p(part),
                                         p(slot) if acc else None, B, P, int(bf16), ctypes.byref(nparts), stream()), "stats")
    torch.cuda.synchronize()
    assert intact(out_flat, SENT_H if bf16 else SENT) and intact(part_flat) and intact(slot_flat, SENT_LL)
    assert full_flat is None or intact(full_flat)
    if bf16:
        got = (bits(out).astype(np.uint32) << 16).view(np.float32).reshape(B, P, 32)
    else:
        got = out.cpu().numpy().reshape(B, P, 32)
    return got, (None if full is None else full.cpu().numpy().reshape(B, 32, P)), part.cpu().numpy().reshape(-1, 64), \
        slot_np(slot), nparts.value


@pytest.mark.parametrize("variant", SC.STATS_VARIANTS)
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SC.STATS_SHAPES, ids=lambda s: "B%d_P%d" % s)
def test_nchw_to_nhwc_stats(shape, bf16, variant):
    B, P = shape
    case = SC.stats_case(B, P, bf16, variant)
    tiles = (P // 64) * B
    grid = min(tiles, 1024)
    exact = SC.stats_exact(case["stored"])
    # through partials
    out, full, part, slot, nparts = run_stats(case, acc=False)
    assert nparts == grid
    assert np.array_equal(bits(out), bits(case["stored"]))
    if variant != "plain":
        assert np.array_equal(full, case["value"])
    assert np.array_equal(part[:nparts].astype(np.float64).sum(0), exact)
    assert np.array_equal(part[nparts:], np.full_like(part[nparts:], SENT)) and not slot.any()
    # through the accumulator slot
    out, full, part, slot, nparts = run_stats(case, acc=True)
    assert nparts == grid and np.array_equal(bits(out), bits(case["stored"]))
    if variant != "plain":
        assert np.array_equal(full, case["value"])
    assert np.array_equal(part, np.full_like(part, SENT))
    assert np.array_equal(SC.read(slot), exact)
    assert np.count_nonzero(np.abs(slot).sum(1)) == min(grid, 8) and not slot[:, 192].any()
    assert np.array_equal(slot, SC.slot_of_partials(SC.stats_partials_f32_order(case["stored"], grid)))


@pytest.mark.parametrize("variant", SC.STATS_VARIANTS)
@pytest.mark.parametrize("shape", [(3, 256), (1025, 64)], ids=lambda s: "B%d_P%d" % s)
def test_nchw_to_nhwc_stats_nan_poisons_one_shard(shape, variant):
    """a NaN element in the LAST tile (the second trip of its workgroup at B = 1025): the flag of that workgroup's shard is
    set, that workgroup's two sums of the channel are left out, nothing else changes.  The two-slab form with the ReLU
    removes the NaN (fmaxf(NaN, 0) = 0) before the statistics."""
    B, P = shape
    case = SC.stats_case(B, P, False, variant)
    grid = min((P // 64) * B, 1024)
    clean = SC.slot_of_partials(SC.stats_partials_f32_order(case["stored"], grid))
    c, pix = 5, P - 3
    case["in"] = case["in"].copy()
    case["in"][B - 1, c, pix] = np.nan
    case["value"] = case["in"] if variant == "plain" else SC.slab_sum(case["in"], case["slab1"], case["bias"], case["relu"])
    case["stored"] = SC.nchw_to_nhwc(case["value"])
    wg = ((P // 64) * B - 1) % grid
    out, full, part, slot, nparts = run_stats(case, acc=True)
    assert np.array_equal(out, case["stored"], equal_nan=True)
    assert full is None or np.array_equal(full, case["value"], equal_nan=True)
    assert np.array_equal(slot, SC.slot_of_partials(SC.stats_partials_f32_order(case["stored"], grid)))
    if case["relu"]:
        assert out[B - 1, pix, c] == 0 and not slot[:, 192].any()
        assert np.array_equal(SC.read(slot), SC.stats_exact(case["stored"]))
        return
    assert np.isnan(out[B - 1, pix, c]) and np.isnan(out).sum() == 1
    if variant == "plain":
        assert np.array_equal(bits(out), bits(case["stored"]))
    assert np.flatnonzero(slot[:, 192]).tolist() == [wg % 8] and np.isnan(SC.read(slot)).all()
    changed = np.argwhere(slot != clean).tolist()
    allowed = [[wg % 8, k * 64 + which * 32 + c] for k in range(3) for which in range(2)] + [[wg % 8, 192]]
    assert [wg % 8, 192] in changed and all(i in allowed for i in changed)


# ---- the 2048-cap layout kernels ------------------------------------------------------------------------------------------
def special_mask_operand(shape, seed):
    """y of the ReLU mask: the layout values with NaN, -1 and the smallest positive float among them"""
    y = SC.layout_values(shape, seed)
    rs = np.random.RandomState(seed + 1)
    pick = rs.randint(0, 32, shape)
    y[pick == 0] = np.nan
    y[pick == 1] = np.float32(2.0 ** -149)
    return y


@pytest.mark.parametrize("shape", SC.LAYOUT_SHAPES, ids=lambda s: "B%d_P%d" % s)
def test_nhwc_to_nchw(shape):
    lib = _lib.load()
    B, P = shape
    x = special_mask_operand((B, P, 32), 300 + B)                                # a permutation: NaN and -0.0 keep their bits
    flat, out = guarded(B * 32 * P)
    xd = dev(x)
    ok(lib.ava_layout_nhwc_to_nchw(p(xd), p(out), B, P, stream()), "nhwc_to_nchw")
    torch.cuda.synchronize()
    assert intact(flat)
    assert np.array_equal(bits(out).reshape(B, 32, P), bits(SC.nhwc_to_nchw(x)))


@pytest.mark.parametrize("slab", [False, True], ids=["one", "slabs"])
@pytest.mark.parametrize("shape", SC.LAYOUT_SHAPES, ids=lambda s: "B%d_P%d" % s)
def test_relu_mask_to_nhwc(shape, slab):
    lib = _lib.load()
    B, P = shape
    dy0 = SC.layout_values((B, 32, P), 400 + B)
    dy1 = SC.layout_values((B, 32, P), 401 + B) if slab else None
    y = special_mask_operand((B, P, 32), 402 + B)
    assert np.isnan(y).any() and (y == 0).any() and (y < 0).any() and np.signbit(y[y == 0]).any()
    want = SC.relu_mask(SC.slab_sum(dy0, dy1) if slab else dy0, y)
    flat, out = guarded(B * 32 * P)
    d0, d1, yd = dev(dy0), (dev(dy1) if slab else None), dev(y)
    ok(lib.ava_layout_relu_mask_to_nhwc(p(d0), p(d1), p(yd), p(out), B, P, stream()), "relu_mask")
    torch.cuda.synchronize()
    assert intact(flat)
    got = out.cpu().numpy().reshape(B, P, 32)
    assert np.array_equal(got, want) and not got[np.isnan(y)].any()              # a NaN y gives 0
    if not slab:
        assert np.array_equal(bits(got), bits(want))                             # dy is copied: -0.0 stays -0.0


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SC.LAYOUT_SHAPES, ids=lambda s: "B%d_P%d" % s)
def test_bn_bwd_apply_to_nchw_arrays(shape, bf16):
    lib = _lib.load()
    B, P = shape
    g = SC.layout_values((B, P, 32), 500 + B)
    f8 = SC.layout_values((B, 32, P), 501 + B, bf16)
    if bf16:
        assert (SC.stored(f8, True) != f8).mean() > 0.05                         # values that the rounding changes
    A, Bc, Cc = SC.dyadic_coefficients(502 + B)
    want = SC.bn_bwd_apply(g, f8, A, Bc, Cc, bf16)
    if bf16:
        assert (want != SC.bn_bwd_apply(g, f8, A, Bc, Cc, False)).mean() > 0.01  # and the result shows it
    flat, out = guarded(B * 32 * P)
    gd, fd, Ad, Bd, Cd = dev(g), dev(f8), dev(A), dev(Bc), dev(Cc)
    ok(lib.ava_layout_bn_bwd_apply_to_nchw(p(gd), p(fd), p(Ad), p(Bd), p(Cd), p(out), B, P, int(bf16), None, None, None, None,
                                           None, None, None, 0.0, 0, 0, stream()), "bn_bwd_apply")
    torch.cuda.synchronize()
    assert intact(flat)
    assert np.array_equal(out.cpu().numpy().reshape(B, 32, P), want)


def slot_path_inputs(C, seed):
    hi, lo = SC.slot_values(seed)
    values = hi.astype(np.float64) + lo.astype(np.float64)
    rs = np.random.RandomState(seed + 50)
    gamma = (0.5 + rs.rand(32)).astype(np.float32)
    mean = rs.standard_normal(32).astype(np.float32)
    invstd = (0.5 + rs.rand(32)).astype(np.float32)
    cols = np.r_[0:C, 32:32 + C]
    return values, np.stack([hi[cols], lo[cols]]), gamma, mean, invstd


@pytest.mark.parametrize("eval_mode", [0, 1], ids=["train", "eval"])
@pytest.mark.parametrize("C", [32, 24])
@pytest.mark.parametrize("shape", [(3, 256), (2049, 64)], ids=lambda s: "B%d_P%d" % s)
def test_bn_bwd_apply_to_nchw_slot(shape, C, eval_mode):
    lib = _lib.load()
    B, P = shape
    n = float(B * P)
    values, rows, gamma, mean, invstd = slot_path_inputs(C, 600 + C)
    slot_flat, slot = slot_to_device(SC.build_slot(values, 601))
    g = SC.layout_values((B, P, 32), 602 + B)
    f8 = SC.layout_values((B, 32, P), 603 + B)
    gd, fd, gmd, mud, isd = dev(g), dev(f8), dev(gamma), dev(mean), dev(invstd)
    dg_flat, dgamma = guarded(C)
    db_flat, dbeta = guarded(C)
    abc_flat, abc = guarded(96)
    flat, out = guarded(B * 32 * P)
    before = slot_np(slot).copy()
    ok(lib.ava_layout_bn_bwd_apply_to_nchw(p(gd), p(fd), None, None, None, p(out), B, P, 0, p(slot), p(gmd), p(mud), p(isd),
                                           p(dgamma), p(dbeta), p(abc), n, C, eval_mode, stream()), "bn_bwd_apply slot")
    # the same totals through ava_bn_finalize_bwd's partial rows (eval = 0 there)
    ref = [torch.empty(C, device="cuda") for _ in range(5)]
    rd = dev(rows)
    ok(lib.ava_bn_finalize_bwd(p(rd), 2, int(n), C, p(gmd), p(mud), p(isd), *[p(o) for o in ref], stream()), "finalize_bwd")
    torch.cuda.synchronize()
    assert all(intact(f) for f in (dg_flat, db_flat, abc_flat, flat)) and intact(slot_flat, SENT_LL)
    assert np.array_equal(slot_np(slot), before)                                 # the consumer only reads
    row = abc.cpu().numpy().reshape(3, 32)
    assert np.array_equal(row[:, C:], np.full((3, 32 - C), SENT, np.float32))     # nothing published beyond C
    sums = np.concatenate([values[:C], values[32:32 + C]])
    want = SC.finalize_bwd(sums, n, C, gamma, mean, invstd, eval_mode)
    assert np.array_equal(dgamma.cpu().numpy(), ref[0].cpu().numpy()) and np.array_equal(dgamma.cpu().numpy(), want["dgamma"])
    assert np.array_equal(dbeta.cpu().numpy(), ref[1].cpu().numpy()) and np.array_equal(dbeta.cpu().numpy(), want["dbeta"])
    assert np.array_equal(row[0, :C], ref[2].cpu().numpy()) and np.array_equal(row[0, :C], want["A"][:C])
    if eval_mode:
        assert not row[1, :C].any() and not row[2, :C].any()
    else:
        assert np.array_equal(row[1, :C], ref[3].cpu().numpy()) and np.array_equal(row[1, :C], want["Bc"])
        for name, got in (("slot", row[2, :C]), ("finalize_bwd", ref[4].cpu().numpy())):
            ratio = np.abs(got.astype(np.float64) - want["Cc64"]) / want["Cc_term"]
            print("Cc (%s): max |error| / largest term = %.3g (bound 2^-22 = %.3g)" % (name, ratio.max(), 2.0 ** -22))
            assert ratio.max() <= 2.0 ** -22
    coef = np.zeros((3, 32), np.float32)
    coef[:, :C] = row[:, :C]
    assert np.array_equal(out.cpu().numpy().reshape(B, 32, P), SC.bn_bwd_apply(g, f8, coef[0], coef[1], coef[2], False))


def test_bn_bwd_apply_to_nchw_poisoned_slot():
    lib = _lib.load()
    B, P, C = 33, 4096, 32                                                       # 2112 tiles: the second trip sees the NaN too
    values, rows, gamma, mean, invstd = slot_path_inputs(C, 610)
    poisoned = SC.build_slot(values, 611)
    poisoned[6, 192] = 1
    slot_flat, slot = slot_to_device(poisoned)
    g = SC.layout_values((B, P, 32), 612)
    f8 = SC.layout_values((B, 32, P), 613)
    gd, fd, gmd, mud, isd = dev(g), dev(f8), dev(gamma), dev(mean), dev(invstd)
    outs = [guarded(C), guarded(C), guarded(96), guarded(B * 32 * P)]
    ok(lib.ava_layout_bn_bwd_apply_to_nchw(p(gd), p(fd), None, None, None, p(outs[3][1]), B, P, 0, p(slot), p(gmd), p(mud),
                                           p(isd), p(outs[0][1]), p(outs[1][1]), p(outs[2][1]), float(B * P), C, 0, stream()),
       "bn_bwd_apply poisoned")
    torch.cuda.synchronize()
    assert all(intact(f) for f, _ in outs)
    out = outs[3][1].cpu().numpy().reshape(B, 32, P)
    assert np.isnan(out[f8 > 0]).all() and not out[~(f8 > 0)].any() and (f8 > 0).any() and (~(f8 > 0)).any()
    assert np.isnan(outs[0][1].cpu().numpy()).all() and np.isnan(outs[1][1].cpu().numpy()).all()


# ---- scale_backward_roots ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nwg", [1, 256 * 256 + 3])
@pytest.mark.parametrize("n4", [1, 255 * 256 + 1, 2048 * 256, 2048 * 256 + 5])
def test_scale_backward_roots(n4, nwg):
    lib = _lib.load()
    n = 4 * n4
    rs = np.random.RandomState(n4 % 1000 + nwg)
    seed0 = rs.standard_normal(n).astype(np.float32)
    wg0 = rs.standard_normal(nwg).astype(np.float32)
    hi, lo = SC.slot_values(700)
    values = hi.astype(np.float64) + lo.astype(np.float64)
    slot0 = SC.build_slot(values, 701)
    for scale in (1.0, 0.5, 3.0):
        seed_flat, seed = guarded(n)
        wg_flat, wg = guarded(nwg)
        seed.copy_(torch.from_numpy(seed0))
        wg.copy_(torch.from_numpy(wg0))
        slot_flat, slot = slot_to_device(slot0)
        sc = torch.full((1,), scale, device="cuda")
        ok(lib.ava_layout_scale_backward_roots(p(seed), n, p(wg), nwg, p(slot), p(sc), stream()), "scale_roots")
        torch.cuda.synchronize()
        assert intact(seed_flat) and intact(wg_flat) and intact(slot_flat, SENT_LL)
        after = slot_np(slot)
        if scale == 1.0:                                                         # touches nothing, bit for bit
            assert np.array_equal(bits(seed), bits(seed0)) and np.array_equal(bits(wg), bits(wg0))
            assert np.array_equal(after, slot0)
            continue
        assert np.array_equal(bits(seed), bits(seed0 * np.float32(scale)))
        assert np.array_equal(bits(wg), bits(wg0 * np.float32(scale)))
        assert np.array_equal(SC.read(after), SC.read(slot0) * scale) and np.array_equal(SC.read(after), values * scale)
        assert not after[1:].any() and after[0].any()
        assert np.array_equal(after, SC.slot_from_values(values * scale))


def test_scale_backward_roots_poison_optional_operands_and_refusal():
    lib = _lib.load()
    hi, lo = SC.slot_values(710)
    values = hi.astype(np.float64) + lo.astype(np.float64)
    poisoned = SC.build_slot(values, 711)
    poisoned[3, 192] = 1
    seed0 = np.arange(8, dtype=np.float32) - 3
    sc = torch.full((1,), 0.5, device="cuda")
    # a poisoned slot stays poisoned; no wg
    seed_flat, seed = guarded(8)
    seed.copy_(torch.from_numpy(seed0))
    slot_flat, slot = slot_to_device(poisoned)
    ok(lib.ava_layout_scale_backward_roots(p(seed), 8, None, 0, p(slot), p(sc), stream()), "scale_roots")
    torch.cuda.synchronize()
    after = slot_np(slot)
    assert intact(seed_flat) and intact(slot_flat, SENT_LL) and np.array_equal(seed.cpu().numpy(), seed0 * 0.5)
    assert np.isnan(SC.read(after)).all() and after[0, 192] == 1 and not after[1:].any() and not after[0, :192].any()
    # no slot, no wg: the seed alone
    seed.copy_(torch.from_numpy(seed0))
    ok(lib.ava_layout_scale_backward_roots(p(seed), 8, None, 0, None, p(sc), stream()), "scale_roots")
    torch.cuda.synchronize()
    assert intact(seed_flat) and np.array_equal(seed.cpu().numpy(), seed0 * 0.5)
    # n % 4 != 0 is refused and nothing is written
    seed.copy_(torch.from_numpy(seed0))
    for n in (5, 6, 7, 2):
        assert lib.ava_layout_scale_backward_roots(p(seed), n, None, 0, p(slot), p(sc), stream()) == -1
    torch.cuda.synchronize()
    assert np.array_equal(seed.cpu().numpy(), seed0) and np.array_equal(slot_np(slot), after)


# ---- ava_bn_stats -----------------------------------------------------------------------------------------------------------
def check_bn_stats(n, C, seed):
    lib = _lib.load()
    x = SC.integer_rows(n, C, seed)
    grid = SC.bn_stats_grid(n, C)
    flat, part = guarded(1024 * 2 * C)
    nparts = ctypes.c_int(-1)
    xd = dev(x)
    ok(lib.ava_bn_stats(p(xd), n, C, p(part), ctypes.byref(nparts), stream()), "bn_stats")
    torch.cuda.synchronize()
    rows = part.cpu().numpy().reshape(1024, 2 * C)
    assert intact(flat) and nparts.value == grid
    assert np.array_equal(rows[grid:], np.full_like(rows[grid:], SENT))
    assert np.array_equal(rows[:grid].astype(np.float64).sum(0), SC.bn_stats_exact(x, C)), (n, C)


@pytest.mark.parametrize("C", [1, 8, 16, 24, 32])
def test_bn_stats(C):
    for n in [1, 2047, 2048, 2049, 3 * 2048 + 5] + ([3, 4 * 2048 + 3] if C == 1 else []):
        check_bn_stats(n, C, 50 * C + n % 97)


@pytest.mark.parametrize("C,n", [(1, 4 * (1024 * 2048 + 1) + 3), (8, 1024 * 2048 + 5)])
def test_bn_stats_at_the_grid_cap(C, n):
    assert SC.bn_stats_grid(n, C) == 1024                                        # and every thread takes a ninth element
    check_bn_stats(n, C, 77)


def test_bn_stats_refuses_other_channel_counts():
    lib = _lib.load()
    flat, part = guarded(64)
    x = torch.zeros(500, device="cuda")
    nparts = ctypes.c_int(-1)
    assert lib.ava_bn_stats(p(x), 100, 5, p(part), ctypes.byref(nparts), stream()) == -1
    torch.cuda.synchronize()
    assert nparts.value == -1 and bool((flat == SENT).all())


# ---- ava_bn_finalize / ava_bn_finalize_bwd ------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 5, 8, 16, 24, 32])
def test_bn_finalize_over_the_column_sum_edges(C):
    lib = _lib.load()
    rs = np.random.RandomState(800 + C)
    gamma, beta = (0.5 + rs.rand(C)).astype(np.float32), rs.standard_normal(C).astype(np.float32)
    rm0, rv0 = rs.standard_normal(C).astype(np.float32), (0.5 + rs.rand(C)).astype(np.float32)
    gd, bd = dev(gamma), dev(beta)
    worst = dict(invstd=0.0, scale=0.0, shift=0.0, running_mean=0.0, running_var=0.0)
    for nparts in SC.finalize_nparts(C):
        n = 16 * nparts
        partials = SC.finalize_partials(nparts, C, 900 * C + nparts)
        sums = partials.astype(np.float64).sum(0)
        want = SC.finalize(sums, n, C, gamma, beta, rm0, rv0)
        assert want["var"].min() > 1
        pd_ = dev(partials)
        bufs = [guarded(C) for _ in range(6)]                                    # running mean, var, mean, invstd, scale, shift
        bufs[0][1].copy_(torch.from_numpy(rm0))
        bufs[1][1].copy_(torch.from_numpy(rv0))
        nbt = torch.full((3,), 7, dtype=torch.int64, device="cuda")
        ok(lib.ava_bn_finalize(p(pd_), nparts, n, C, p(gd), p(bd), p(bufs[0][1]), p(bufs[1][1]), p(nbt[1:]), 1,
                               *[p(b[1]) for b in bufs[2:]], stream()), "bn_finalize")
        torch.cuda.synchronize()
        assert all(intact(f) for f, _ in bufs) and nbt.tolist() == [7, 8, 7]
        rm, rv, mean, invstd, scale, shift = [b[1].cpu().numpy() for b in bufs]
        assert np.array_equal(mean, want["mean"]), (C, nparts)
        var = want["var"]
        for key, got, ref in (("invstd", invstd, 1 / np.sqrt(var + 1e-5)),
                              ("scale", scale, gamma.astype(np.float64) / np.sqrt(var + 1e-5)),
                              ("shift", shift, beta.astype(np.float64) - want["mean64"] * gamma / np.sqrt(var + 1e-5)),
                              ("running_mean", rm, want["running_mean64"]), ("running_var", rv, want["running_var64"])):
            worst[key] = max(worst[key], rel(got, ref))
        # eval mode: running statistics in, buffers and the batch counter untouched
        kept = [b[1].clone() for b in bufs[:2]]
        ok(lib.ava_bn_finalize(None, 0, n, C, p(gd), p(bd), p(bufs[0][1]), p(bufs[1][1]), p(nbt[1:]), 0,
                               *[p(b[1]) for b in bufs[2:]], stream()), "bn_finalize eval")
        torch.cuda.synchronize()
        assert torch.equal(kept[0], bufs[0][1]) and torch.equal(kept[1], bufs[1][1]) and nbt.tolist() == [7, 8, 7]
        assert all(intact(f) for f, _ in bufs)
        assert np.array_equal(bufs[2][1].cpu().numpy(), rm)
        assert rel(bufs[3][1].cpu().numpy(), 1 / np.sqrt(rv.astype(np.float64) + 1e-5)) < 1e-6
    print("bn_finalize C=%d: max relative errors %s (bounds 1e-6, shift 2e-6)" % (C, worst))
    assert worst["invstd"] < 1e-6 and worst["scale"] < 1e-6 and worst["shift"] < 2e-6
    assert worst["running_mean"] < 1e-6 and worst["running_var"] < 1e-6


def test_bn_finalize_of_one_element():
    lib = _lib.load()
    C = 8
    x = np.arange(-3, 5, dtype=np.float32)
    partials = np.concatenate([x, x * x])[None]
    gamma, beta = np.full(C, 1.5, np.float32), np.full(C, 0.25, np.float32)
    rm0, rv0 = np.full(C, 2.0, np.float32), np.full(C, 3.0, np.float32)
    pd_, gd, bd, rm, rv = dev(partials), dev(gamma), dev(beta), dev(rm0), dev(rv0)
    outs = [guarded(C) for _ in range(4)]
    ok(lib.ava_bn_finalize(p(pd_), 1, 1, C, p(gd), p(bd), p(rm), p(rv), None, 1, *[p(o[1]) for o in outs], stream()), "n=1")
    torch.cuda.synchronize()
    want = SC.finalize(partials[0], 1, C, gamma, beta, rm0, rv0)
    assert not want["var"].any() and all(intact(f) for f, _ in outs)
    assert np.array_equal(outs[0][1].cpu().numpy(), x)
    assert np.array_equal(outs[1][1].cpu().numpy(), np.full(C, np.float32(1 / np.sqrt(1e-5))))
    assert np.array_equal(rv.cpu().numpy(), np.full(C, np.float32(0.9 * 3.0)))    # the unbiased variance is the biased one: 0
    assert np.array_equal(rm.cpu().numpy(), want["running_mean"])


@pytest.mark.parametrize("C", [1, 5, 8, 16, 24, 32])
def test_bn_finalize_bwd_over_the_column_sum_edges(C):
    lib = _lib.load()
    rs = np.random.RandomState(850 + C)
    gamma, mean, invstd = [(0.5 + rs.rand(C)).astype(np.float32) for _ in range(3)]
    gd, md, isd = dev(gamma), dev(mean), dev(invstd)
    worst = 0.0
    for nparts in SC.finalize_nparts(C):
        n = 16 * nparts
        partials = SC.integer_partials(nparts, 2 * C, 950 * C + nparts)
        want = SC.finalize_bwd(partials.astype(np.float64).sum(0), n, C, gamma, mean, invstd)
        pd_ = dev(partials)
        outs = [guarded(C) for _ in range(5)]
        ok(lib.ava_bn_finalize_bwd(p(pd_), nparts, n, C, p(gd), p(md), p(isd), *[p(o[1]) for o in outs], stream()), "bwd")
        torch.cuda.synchronize()
        assert all(intact(f) for f, _ in outs)
        dgamma, dbeta, A, Bc, Cc = [o[1].cpu().numpy() for o in outs]
        assert np.array_equal(dgamma, want["dgamma"]) and np.array_equal(dbeta, want["dbeta"]), (C, nparts)
        assert np.array_equal(A, want["A"]) and np.array_equal(Bc, want["Bc"]), (C, nparts)
        worst = max(worst, rel(Cc, want["Cc64"]))
    print("bn_finalize_bwd C=%d: Cc max relative error %.3g (bound 1e-5)" % (C, worst))
    assert worst < 1e-5


# ---- ava_adam_flat ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 1024, 4 * (4096 * 256) + 4 * 257])
def test_adam_flat_sizes(n):
    """The bound on p is absolute, 2e-7: between one and two ulps of a parameter in [1, 2), less than one ulp (2.4e-7) of one
    in [2, 4).  The kernel forms p - step_size * (m / denom) and torch p + (-step_size * m) / denom: both round correctly
    and may end one ulp of p apart, so the bound is meaningful for |p| < 2 only, and the parameters are drawn there
    (every parameter of the model is: |w| <= 1 / sqrt(fan_in), BatchNorm weights near 1).  Measured with N(0, 1)
    parameters at the largest n: 51 of 4.2 million elements one ulp apart at |p| >= 2 (2.38e-7), none above one ulp
    anywhere, and the same elements scattered over the whole range, not at a block or grid boundary."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(n % 1000)
    p0 = torch.randn(n, generator=g) * 0.35
    assert float(p0.abs().max()) < 1.95
    bufs = [guarded(n) for _ in range(3)]                                        # p, m, v
    bufs[0][1].copy_(p0)
    bufs[1][1].zero_()
    bufs[2][1].zero_()
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([ref], lr=1e-3)
    worst = [0.0, 0.0, 0.0]
    for step in range(1, 4):
        gr = torch.randn(n, generator=g) * (10.0 ** (step - 2))
        gr[::7] = 0.0
        ref.grad = gr.clone()
        opt.step()
        grd = gr.cuda()
        ok(lib.ava_adam_flat(p(bufs[0][1]), p(grd), p(bufs[1][1]), p(bufs[2][1]), n, 1e-3, 0.9, 0.999, 1e-8, step, stream()), "adam")
        torch.cuda.synchronize()
        st = opt.state[ref]
        assert all(intact(f) for f, _ in bufs)
        worst[0] = max(worst[0], float((bufs[0][1].cpu() - ref.detach()).abs().max()))
        worst[1] = max(worst[1], rel(bufs[1][1].cpu(), st["exp_avg"]))
        worst[2] = max(worst[2], rel(bufs[2][1].cpu(), st["exp_avg_sq"]))
    print("adam n=%d: max |dp| %.3g (2e-7), m %.3g, v %.3g (1e-6)" % (n, *worst))
    assert worst[0] < 2e-7 and worst[1] < 1e-6 and worst[2] < 1e-6


def test_adam_flat_refusals_write_nothing():
    lib = _lib.load()
    bufs = [guarded(16) for _ in range(4)]
    for n, step in [(6, 1), (15, 1), (0, 1), (-4, 1), (8, 0), (8, -2)]:
        assert lib.ava_adam_flat(p(bufs[0][1]), p(bufs[1][1]), p(bufs[2][1]), p(bufs[3][1]), n, 1e-3, 0.9, 0.999, 1e-8, step,
                                 stream()) == -1
    torch.cuda.synchronize()
    assert all(bool((f == SENT).all()) for f, _ in bufs)


# ---- ava_fill_normal ----------------------------------------------------------------------------------------------------------
def test_fill_normal_beyond_one_grid_pass_element_by_element():
    lib = _lib.load()
    n = 1024 * 256 + 300
    flat, out = guarded(n)
    ok(lib.ava_fill_normal(p(out), n, 2002, 0, stream()), "fill_normal")
    torch.cuda.synchronize()
    want = syn.gauss(n, 2002)
    err = rel(out.cpu().numpy(), want)
    print("fill_normal n=%d: max error / max |value| = %.3g (bound 1e-6)" % (n, err))
    assert intact(flat) and err < 1e-6
    assert rel(out[1024 * 256:].cpu().numpy(), want[1024 * 256:]) < 1e-6         # the second pass on its own
    ok(lib.ava_fill_normal(p(out), n, 2002, 1 << 20, stream()), "fill_normal offset")
    torch.cuda.synchronize()
    assert intact(flat) and rel(out.cpu().numpy(), syn.gauss((1 << 20) + n, 2002)[1 << 20:]) < 1e-6


# ---- ava_elbo_finalize ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 255, 256, 257, 1000])
def test_elbo_finalize_strided_loops(B):
    lib = _lib.load()
    z, prec = 32, 10.0
    worst = 0.0
    for nparts in (1, 256, 257, 1024):
        rs = np.random.RandomState(B + nparts)
        lat = rs.randint(-1000, 1001, (B, 2)).astype(np.float32)
        sse = rs.randint(0, 4001, (nparts, 2)).astype(np.float32)
        loss, sums = SC.elbo(lat, sse, z, prec)
        flat, out = guarded(4)
        latd, ssed = dev(lat), dev(sse)
        ok(lib.ava_elbo_finalize(p(latd), B, p(ssed), nparts, z, prec, p(out), stream()), "elbo")
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert intact(flat) and np.array_equal(got[1:], sums), (B, nparts)
        worst = max(worst, abs(float(got[0]) - loss) / abs(loss))
    print("elbo B=%d: max relative loss error %.3g (bound 1e-6)" % (B, worst))
    assert worst < 1e-6


# ---- ava_latent_fwd / ava_latent_bwd ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("z", [1, 63, 64, 65, 127, 128])
@pytest.mark.parametrize("B", [1, 4, 5])
def test_latent_block_sizes(B, z):
    lib = _lib.load()
    g = torch.Generator().manual_seed(100 * B + z)
    mu, u, a, ed, gdec = [torch.randn(B, z, generator=g, dtype=torch.float64) * 0.7 for _ in range(5)]
    mu, u, a, ed, gdec = [t.float().double() for t in (mu, u, a, ed, gdec)]
    ew = torch.randn(B, 1, generator=g, dtype=torch.float64).float().double()
    d = torch.exp(a)
    zs = O.rsample(mu, u, d, ew, ed)
    H = O.entropy(u, d)
    outs = [guarded(B * z), guarded(B * z), guarded(2 * B)]                      # d, z, sums
    status = torch.zeros(3, dtype=torch.int32, device="cuda")
    mud, ud, ad, ewd, edd = dev(mu), dev(u), dev(a), dev(ew.reshape(B)), dev(ed)
    ok(lib.ava_latent_fwd(p(mud), p(ud), p(ad), p(ewd), p(edd), *[p(o[1]) for o in outs], p(status[1:]), B, z, stream()), "lat")
    torch.cuda.synchronize()
    dd, zd, sums = outs[0][1].view(B, z), outs[1][1].view(B, z), outs[2][1].view(B, 2)
    errs = [rel(dd.cpu(), d), rel(zd.cpu(), zs), rel(sums[:, 0].cpu(), (zs * zs).sum(1)), rel(sums[:, 1].cpu(), H)]
    assert all(intact(f) for f, _ in outs) and status.tolist() == [0, 0, 0]
    dmu, du, da = O.latent_backward(zd.cpu().double() + gdec, u, dd.cpu().double(), ew, ed)
    bouts = [guarded(B * z) for _ in range(3)]
    gdd = dev(gdec)
    ok(lib.ava_latent_bwd(p(zd), p(gdd), p(ud), p(dd), p(ewd), p(edd), *[p(o[1]) for o in bouts], B, z, stream()), "latb")
    torch.cuda.synchronize()
    berrs = [rel(o[1].view(B, z).cpu(), w) for o, w in zip(bouts, (dmu, du, da))]
    print("latent B=%d z=%d: forward %s (1e-6), backward %s (1e-5)" % (B, z, errs, berrs))
    assert all(intact(f) for f, _ in bouts)
    assert max(errs) < 1e-6 and max(berrs) < 1e-5
    # d underflows to 0 in the last row, last dim: the status word is set, the other rows are what they were
    first = [o[1].clone() for o in outs]
    ad2 = ad.clone()
    ad2[B - 1, z - 1] = -200.0
    ok(lib.ava_latent_fwd(p(mud), p(ud), p(ad2), p(ewd), p(edd), *[p(o[1]) for o in outs], p(status[1:]), B, z, stream()), "lat")
    torch.cuda.synchronize()
    assert status.tolist() == [0, 1, 0] and all(intact(f) for f, _ in outs)
    for was, o, width in zip(first, outs, (z, z, 2)):
        assert torch.equal(was.view(B, width)[:B - 1], o[1].view(B, width)[:B - 1])
    assert float(outs[0][1].view(B, z)[B - 1, z - 1]) == 0.0
