"""The restatement of the training step's small kernels (tests/step_kernel_cases.py) without a GPU: the number formats, the
fixed-point accumulator of bn_acc.h, that the generated inputs make every kernel sum exact in the kernel's own order (what
lets test_gpu_step_kernels.py compare with ==), and the refusals of the C entry points, decided before any launch."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import step_kernel_cases as SC


# ---- number formats ------------------------------------------------------------------------------------------------------
def test_bf16_rounding_is_to_nearest_even():
    x = np.array([1.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -12, -(1 + 2.0 ** -7 + 2.0 ** -9), 0.0, -0.0,
                  3.0e38, np.inf], np.float32)
    want = np.array([1.0, 1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, -(1 + 2.0 ** -7), 0.0, -0.0, 3.0e38, np.inf], np.float32)
    got = SC.bf16_round(x)
    want[7] = np.float32(np.uint32(0x7F62 << 16).view(np.float32))               # 3.0e38 = 0x7F61B1E6: up to 0x7F62
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.isnan(SC.bf16_round(np.array([np.nan], np.float32))[0])
    assert np.array_equal(SC.bf16_bits(x[:3]), [0x3F80, 0x3F80, 0x3F82])
    torch = pytest.importorskip("torch")
    r = np.random.RandomState(0).standard_normal(4096).astype(np.float32) * 3
    assert np.array_equal(SC.bf16_round(r), torch.from_numpy(r).to(torch.bfloat16).float().numpy())


def test_fma32_is_one_rounding_of_the_exact_value():
    rs = np.random.RandomState(1)
    a, b = rs.standard_normal(2000).astype(np.float32), rs.standard_normal(2000).astype(np.float32)
    c = (-(a.astype(np.float64) * b) * (1 + rs.standard_normal(2000) * 1e-7)).astype(np.float32)      # heavy cancellation
    c[::3] = rs.standard_normal(len(c[::3])).astype(np.float32)
    got = SC.fma32(a, b, c)
    assert got.dtype == np.float32 and got.shape == a.shape
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        err = abs(Fraction(float(got[i])) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), i
    # the case two roundings get wrong: (2^-12 + 2^-35)(2^-12 - 2^-35) + (1 + 2^-23) = 1 + 2^-23 + 2^-24 - 2^-70.  float64
    # rounds the sum to the float32 tie 1 + 2^-23 + 2^-24, which then goes to even, 1 + 2^-22; the exact value lies below it
    x, y, z = np.float32(2.0 ** -12 + 2.0 ** -35), np.float32(2.0 ** -12 - 2.0 ** -35), np.float32(1 + 2.0 ** -23)
    assert float(x) * float(y) == 2.0 ** -24 - 2.0 ** -70
    assert np.float32(float(x) * float(y) + float(z)) == np.float32(1 + 2.0 ** -22)
    assert SC.fma32(x, y, z)[()] == z
    assert SC.fma32(x, x, z)[()] == np.float32(1 + 2.0 ** -22)                          # above the tie
    # a true tie goes to even
    assert SC.fma32(np.float32(2.0 ** -12), np.float32(2.0 ** -12), z)[()] == np.float32(1 + 2.0 ** -22)
    assert SC.fma32(np.float32(2.0 ** -12), np.float32(2.0 ** -12), np.float32(1.0))[()] == np.float32(1.0)
    assert np.isnan(SC.fma32(np.float32(np.nan), x, z)[()]) and np.isnan(SC.fma32(x, y, np.float32(np.nan))[()])


# ---- layouts -------------------------------------------------------------------------------------------------------------
def test_layout_restatement_is_the_index_map_of_the_kernels():
    B, P = 3, 128
    x = np.arange(B * 32 * P, dtype=np.float32).reshape(B, 32, P)
    y = SC.nchw_to_nhwc(x)
    assert y.shape == (B, P, 32) and y.flags["C_CONTIGUOUS"]
    flat_in, flat_out = x.ravel(), y.ravel()
    for b, c, p in [(0, 0, 0), (1, 31, 127), (2, 5, 64), (2, 17, 63)]:
        assert flat_out[b * 32 * P + p * 32 + c] == flat_in[b * 32 * P + c * P + p]
    assert np.array_equal(SC.nhwc_to_nchw(y), x)
    tiles = SC.tiles_of(y)
    assert tiles.shape == (6, 64, 32) and tiles[3, 5, 7] == y[1, 64 + 5, 7]              # tile w = b * nq + q
    assert [SC.layout_grid(b, p, SC.LAYOUT_CAP) for b, p in SC.LAYOUT_SHAPES] == [1, 12, 2048, 2048, 2048, 2048, 2048]
    assert [(p // 64) * b for b, p in SC.LAYOUT_SHAPES] == [1, 12, 2048, 2049, 2050, 2049, 4098]
    assert [SC.layout_grid(b, p, SC.STATS_CAP) for b, p in SC.STATS_SHAPES] == [1, 12, 1024, 1024, 1024, 1024]
    assert [(p // 64) * b for b, p in SC.STATS_SHAPES] == [1, 12, 1024, 1025, 2052, 2049]


def test_mask_slab_and_apply_restatements():
    dy = np.full((1, 32, 64), 7.0, np.float32)
    y = np.zeros((1, 64, 32), np.float32)
    y[0, 0, :6] = [1.0, 0.0, -0.0, -1.0, np.nan, 2.0 ** -149]
    du = SC.relu_mask(dy, y)
    assert du[0, 0, :7].tolist() == [7.0, 0.0, 0.0, 0.0, 0.0, 7.0, 0.0]
    s0 = np.array([-0.0, 1.0, -3.0, np.nan], np.float32)
    s1 = np.array([-0.0, 0.5, 1.0, 1.0], np.float32)
    plain = SC.slab_sum(s0, s1)
    assert np.array_equal(plain[:3], [0.0, 1.5, -2.0]) and not np.signbit(plain[0]) and np.isnan(plain[3])
    assert np.array_equal(SC.slab_sum(s0, s1, relu=True), [0.0, 1.5, 0.0, 0.0])          # fmaxf(NaN, 0) = 0
    g = np.full((1, 64, 32), 0.5, np.float32)
    f8 = np.zeros((1, 32, 64), np.float32)
    f8[0, 1, :4] = [1 + 2.0 ** -8, -1.0, 2.0 ** -140, 1 + 3 * 2.0 ** -8]
    A, Bc, Cc = np.full(32, 2.0, np.float32), np.full(32, 4.0, np.float32), np.full(32, -1.0, np.float32)
    out = SC.bn_bwd_apply(g, f8, A, Bc, Cc, bf16=False)
    assert out[0, 1, :5].tolist() == [4 * (1 + 2.0 ** -8), 0.0, 0.0, 4 * (1 + 3 * 2.0 ** -8), 0.0]       # 4 * 2^-140 - 1 rounds to -1
    out = SC.bn_bwd_apply(g, f8, A, Bc, Cc, bf16=True)                                   # Bc * the ROUNDED f8; 2^-140 -> 0
    assert out[0, 1, :5].tolist() == [4.0, 0.0, 0.0, 4 * (1 + 2.0 ** -6), 0.0]


# ---- bn_acc.h ------------------------------------------------------------------------------------------------------------
def test_split_truncates_keeps_signs_and_poisons_at_2_to_the_47():
    p = np.array([0.0, -0.0, 2.0 ** -48, -(2.0 ** -48), 2.0 ** -49, -(2.0 ** -49), 1.0, -1.0, 65536.0, -65536.0,
                  2.0 ** -16, 1.5 * 2.0 ** -48, 2.0 ** -149], np.float32)
    l0, l1, l2, poison = SC.split(p)
    assert not poison.any()
    assert l0.tolist() == [0, 0, 1, -1, 0, 0, 0, 0, 0, 0, 0, 1, 0]                         # below 2^-48: truncated to 0
    assert l1.tolist() == [0, 0, 0, 0, 0, 0, 65536, -65536, 0, 0, 1, 0, 0]
    assert l2.tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 1, -1, 0, 0, 0]
    big = np.float32(2.0 ** 47)
    below = np.nextafter(big, np.float32(0))
    edge = np.array([below, -below, big, -big, np.inf, -np.inf, np.nan, 3.0e38], np.float32)
    l0, l1, l2, poison = SC.split(edge)
    assert poison.tolist() == [False, False, True, True, True, True, True, True]
    assert l2[0] == 2 ** 31 - 128 and l2[1] == -(2 ** 31 - 128) and l1[0] == 0 and l0[0] == 0        # (2^24 - 1) 2^23 2^48 / 2^64
    assert not l0[2:].any() and not l1[2:].any() and not l2[2:].any()
    rs = np.random.RandomState(3)
    v = (rs.standard_normal(4096) * np.exp(rs.uniform(-40, 30, 4096))).astype(np.float32)
    l0, l1, l2, poison = SC.split(v)
    assert not poison.any() and np.abs(l0).max() < 2 ** 32 and np.abs(l1).max() < 2 ** 32 and np.abs(l2).max() < 2 ** 31
    for i in range(0, 4096, 17):
        want = int(abs(Fraction(float(v[i]))) * 2 ** 48)                                  # trunc
        got = int(l0[i]) + (int(l1[i]) << 32) + (int(l2[i]) << 64)
        assert got == (-want if v[i] < 0 else want)


def test_slot_round_trip_and_poison():
    rs = np.random.RandomState(4)
    partials = (rs.randint(-2 ** 20, 2 ** 20, (37, 64)) / 64.0).astype(np.float32)
    slot = SC.slot_of_partials(partials)
    assert np.count_nonzero(np.abs(slot).sum(1)) == 8 and (slot[:, :192] < 0).any()
    want = partials.astype(np.float64).sum(0)
    assert np.array_equal(SC.read(slot), want)
    assert SC.read_exact(slot) == [int(w * 2.0 ** 48) for w in want]
    # shard = workgroup mod 8
    one = SC.slot_add(SC.empty_slot(), 13, partials[0])
    assert np.flatnonzero(np.abs(one).sum(1)).tolist() == [5]
    # a non-finite partial sets the flag of its shard and adds nothing for that value; the reader then gives NaN
    bad = partials.copy()
    bad[10, 7] = np.nan
    poisoned = SC.slot_of_partials(bad)
    assert poisoned[2, 192] == 1 and poisoned[:, 192].sum() == 1
    # (|partial| < 2^14 in steps of 2^-6: trunc(|p| 2^48) = |k| 2^42 has its bits in the second limb alone)
    assert np.argwhere(poisoned != slot).tolist() == [[2, 64 + 7], [2, 192]]
    assert slot[2, 64 + 7] - poisoned[2, 64 + 7] == int(partials[10, 7] * 64) << 10
    assert np.isnan(SC.read(poisoned)).all()


@pytest.mark.parametrize("seed", [5, 6])
def test_built_slots_read_back_exactly(seed):
    hi, lo = SC.slot_values(seed)
    values = hi.astype(np.float64) + lo.astype(np.float64)
    assert (values < 0).any() and (values > 0).any() and np.abs(values).max() >= 2.0 ** 26 and values[0] == 0
    slot = SC.build_slot(values, seed)
    assert (slot[:, 0:64] < 0).any() and (slot[:, 64:128] != 0).any() and (slot[:, 128:192] != 0).any()
    assert (slot[:, 128:192] < 0).any() and np.abs(slot[:, 0:64]).max() >= 2 ** 32        # unnormalised limbs too
    assert not slot[:, 192].any() and np.count_nonzero(np.abs(slot).sum(1)) == 8
    assert SC.read_exact(slot) == [int(v * 2.0 ** 48) for v in values]
    assert np.array_equal(SC.read(slot), values)                                          # the kernel's float64 order is exact
    for scale in (0.5, 3.0):                                                              # scale_backward_roots' product
        after = SC.slot_from_values(SC.read(slot) * scale)
        assert not after[1:].any() and np.abs(after[0, :192]).max() < 2 ** 32
        assert SC.read_exact(after) == [int(Fraction(float(v)) * Fraction(scale) * 2 ** 48) for v in values]
        assert np.array_equal(SC.read(after), values * scale)                             # nothing truncated
    assert SC.slot_from_values([np.nan] + [0.0] * 63)[0, 192] == 1
    # the float32 partial rows with the same totals (what ava_bn_finalize_bwd is given)
    rows = np.stack([hi, lo])
    assert np.array_equal(rows.astype(np.float64).sum(0), values)
    assert np.array_equal(SC.column_sums_f64_order(rows, 64), values)


# ---- the inputs make the kernels' sums exact --------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", SC.STATS_VARIANTS)
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("shape", SC.STATS_SHAPES)
def test_stats_inputs_sum_exactly_in_the_kernel_order(shape, bf16, variant):
    B, P = shape
    case = SC.stats_case(B, P, bf16, variant)
    st = case["stored"]
    if bf16:
        assert (st != SC.nchw_to_nhwc(case["value"])).mean() > 0.02                       # storage changed values
    if variant != "plain":
        exact = case["in"].astype(np.float64) + case["slab1"] + (0 if case["bias"] is None else case["bias"][None])
        assert np.array_equal(case["value"], np.maximum(exact, 0) if case["relu"] else exact)          # the slab sum is exact
        assert (case["value"] == 0).mean() > (0.3 if case["relu"] else 0)
    grid = SC.layout_grid(B, P, SC.STATS_CAP)
    partials = SC.stats_partials_f32_order(st, grid)
    exact = SC.stats_exact(st)
    assert np.array_equal(partials.astype(np.float64).sum(0), exact)
    # and in any other order: every term is a multiple of 2^-14 and a workgroup's terms sum to less than 2^24 of them
    trips = -(-(P // 64) * B // grid)
    assert trips <= 3 and np.array_equal(st * 128, np.round(st * 128)) and np.abs(st).max() <= 2
    assert 4 * 64 * trips * 2 ** 14 < 2 ** 24
    slot = SC.slot_of_partials(partials)
    assert np.array_equal(SC.read(slot), exact) and SC.read_exact(slot) == [int(v * 2.0 ** 48) for v in exact]
    assert np.count_nonzero(np.abs(slot).sum(1)) == min(grid, 8)


def test_slab_inputs_sum_exactly():
    """the element-wise kernels (the two-slab sum of the ReLU mask, the backward apply): their inputs come from the same value
    sets at every shape, so one shape shows that no operation rounds"""
    s0, s1 = SC.layout_values((3, 32, 256), 7), SC.layout_values((3, 32, 256), 8)
    bias = SC.layout_values((32, 256), 9)
    got = SC.slab_sum(s0, s1, bias)
    assert np.array_equal(got.astype(np.float64), s0.astype(np.float64) + s1 + bias[None])
    A, Bc, Cc = SC.dyadic_coefficients(10)
    for bf16 in (False, True):
        f8 = SC.layout_values((3, 32, 256), 11, bf16)
        g = SC.layout_values((3, 256, 32), 12)
        out = SC.bn_bwd_apply(g, f8, A, Bc, Cc, bf16)
        f = SC.stored(f8, bf16).astype(np.float64)
        plain = A[None, :, None].astype(np.float64) * SC.nhwc_to_nchw(g) + (Bc[None, :, None].astype(np.float64) * f
                                                                           + Cc[None, :, None])
        assert np.array_equal(out.astype(np.float64), np.where(f > 0, plain, 0.0))        # no rounding anywhere
        if bf16:
            assert (SC.stored(f8, True) != f8).mean() > 0.05


@pytest.mark.parametrize("C", [1, 5, 8, 16, 24, 32])
def test_column_sums_of_integer_partials_are_exact_in_the_kernel_order(C):
    g = 1024 // (2 * C)
    counts = SC.finalize_nparts(C)
    assert counts == sorted({1, g - 1, g, g + 1, 7 * g, 7 * g + 1, 8 * g - 1, 8 * g, 8 * g + 1, 16 * g + 3} - {0})
    for nparts in counts:
        partials = SC.integer_partials(nparts, 2 * C, 1000 * C + nparts)
        got = SC.column_sums_f64_order(partials, 2 * C)
        assert [int(v) for v in got] == SC.column_sums_exact(partials) and np.array_equal(got, np.round(got))
        assert np.array_equal(got, partials.astype(np.float64).sum(0))
    # the eight-row loop runs exactly when nparts > 7 g
    assert 7 * g + 1 in counts and 16 * g + 3 > 15 * g


def _bn_stats_sizes(C):
    return [1, 2047, 2048, 2049, 3 * 2048 + 5] + ([3, 4 * 2048 + 3] if C == 1 else [])


@pytest.mark.parametrize("C", [1, 8, 16, 24, 32])
def test_bn_stats_rows_sum_exactly_in_the_kernel_order(C):
    for n in _bn_stats_sizes(C):
        x = SC.integer_rows(n, C, 50 * C + n % 97)
        partials = SC.bn_stats_partials_f32_order(x, C)
        assert partials.shape == (SC.bn_stats_grid(n, C), 2 * C)
        assert np.array_equal(partials.astype(np.float64).sum(0), SC.bn_stats_exact(x, C))
    assert [SC.bn_stats_grid(n, 8) for n in (1, 2047, 2048, 2049, 6149)] == [1, 1, 1, 2, 4]
    assert [SC.bn_stats_grid(n, 1) for n in (1, 3, 2049, 8192, 8195, 8196)] == [1, 1, 1, 1, 1, 2]


@pytest.mark.parametrize("C,n", [(1, 4 * (1024 * 2048 + 1) + 3), (8, 1024 * 2048 + 5)])
def test_bn_stats_cap_cases_sum_exactly(C, n):
    assert SC.bn_stats_grid(n, C) == 1024 and SC.bn_stats_grid(n - 8 * 2048 * (4 if C == 1 else 1), C) == 1017
    x = SC.integer_rows(n, C, 77)
    # order-free: every term is an integer of size <= 9 and a workgroup sees fewer than 2^24 / 9 of them
    per_workgroup = -(-n // 1024) + 4
    assert 9 * per_workgroup < 2 ** 24
    if C == 1:                                                                            # the kernel order as well (0.2 s)
        partials = SC.bn_stats_partials_f32_order(x, C)
        assert np.array_equal(partials.astype(np.float64).sum(0), SC.bn_stats_exact(x, C))


@pytest.mark.parametrize("B,nparts", [(1, 1), (255, 256), (256, 257), (257, 1024), (1000, 1024)])
def test_elbo_sums_are_exact_in_the_kernel_order(B, nparts):
    rs = np.random.RandomState(B)
    lat = rs.randint(-1000, 1001, (B, 2)).astype(np.float32)
    sse = rs.randint(0, 4001, (nparts, 2)).astype(np.float32)
    loss, sums = SC.elbo(lat, sse, 32, 10.0)
    assert SC.elbo_f64_order(lat[:, 0]) == float(sums[0]) == lat[:, 0].astype(np.int64).sum()
    assert SC.elbo_f64_order(sse[:, 0]) == float(sums[1]) == sse[:, 0].astype(np.int64).sum()
    assert SC.elbo_f64_order(lat[:, 1]) == float(sums[2]) == lat[:, 1].astype(np.int64).sum()
    assert np.isfinite(loss)


def test_finalisers_restate_the_formulas():
    C, n = 3, 10
    x = np.array([[1.0, 2.0, -3.0]] * 4 + [[2.0, 2.0, 5.0]] * 6)
    sums = np.concatenate([x.sum(0), (x * x).sum(0)])
    gamma, beta = np.array([1.0, 2.0, 0.5], np.float32), np.array([0.0, 1.0, -1.0], np.float32)
    f = SC.finalize(sums, n, C, gamma, beta, np.zeros(3, np.float32), np.ones(3, np.float32))
    assert np.allclose(f["mean"], x.mean(0)) and np.allclose(f["var"], x.var(0)) and f["var"][1] == 0.0
    assert f["invstd"][1] == np.float32(1 / np.sqrt(1e-5))
    assert np.allclose(f["running_var"], 0.9 + 0.1 * x.var(0, ddof=1)) and np.allclose(f["running_mean"], 0.1 * x.mean(0))
    assert np.allclose(f["shift"], beta - x.mean(0) * gamma * f["invstd"], rtol=1e-6)
    one = SC.finalize(np.array([4.0, 16.0]), 1, 1, gamma[:1], beta[:1], np.zeros(1, np.float32), np.ones(1, np.float32))
    assert one["var"][0] == 0.0 and one["running_var"][0] == np.float32(0.9) and one["invstd"][0] == np.float32(1 / np.sqrt(1e-5))
    b = SC.finalize_bwd(sums, n, C, gamma, f["mean"], f["invstd"])
    a64 = gamma.astype(np.float64) * f["invstd"]
    assert np.array_equal(b["A"], a64.astype(np.float32)) and np.array_equal(b["dbeta"], sums[:3].astype(np.float32))
    assert np.allclose(b["Cc64"], -a64 * sums[:3] / n + a64 * f["invstd"] * sums[3:] / n * f["mean"])
    e = SC.finalize_bwd(sums, n, C, gamma, f["mean"], f["invstd"], eval_mode=True)
    assert not e["Bc"].any() and not e["Cc64"].any() and np.array_equal(e["A"], b["A"])


# ---- the C entry points refuse before any launch ---------------------------------------------------------------------------
def test_wrappers_refuse_bad_arguments_before_any_launch():
    """none of these reaches the device: they pass on a machine without one"""
    from ava_amd import _lib
    lib = _lib.load()
    assert lib.ava_acc_shards() == SC.ACC_SHARDS and lib.ava_acc_shard_ll() == SC.ACC_SHARD_LL
    fake = 4096                                                      # never dereferenced: every call below is rejected
    nparts = ctypes.c_int(-7)
    bad_shapes = [(0, 64), (-1, 64), (1, 0), (1, 32), (1, 63), (1, 65), (1, 96), (4, -64)]

    def stats(inp=fake, slab1=None, bias=None, relu=0, full=None, out=fake, partials=fake, acc=None, B=2, P=64, bf16=0,
              np_=ctypes.byref(nparts)):
        return lib.ava_layout_nchw_to_nhwc_stats(inp, slab1, bias, relu, full, out, partials, acc, B, P, bf16, np_, None)

    def to_nchw(inp=fake, out=fake, B=2, P=64):
        return lib.ava_layout_nhwc_to_nchw(inp, out, B, P, None)

    def mask(dy=fake, slab1=None, y=fake, du=fake, B=2, P=64):
        return lib.ava_layout_relu_mask_to_nhwc(dy, slab1, y, du, B, P, None)

    def apply(g=fake, f8=fake, A=fake, Bc=fake, Cc=fake, out=fake, B=2, P=64, bf16=0, acc=None, gamma=fake, mean=fake,
              invstd=fake, dgamma=fake, dbeta=fake, abc=fake, n=128.0, C=32, eval_=0):
        return lib.ava_layout_bn_bwd_apply_to_nchw(g, f8, A, Bc, Cc, out, B, P, bf16, acc, gamma, mean, invstd, dgamma, dbeta,
                                                   abc, n, C, eval_, None)

    def roots(seed=fake, n=8, wg=None, nwg=0, slot=None, scale=fake):
        return lib.ava_layout_scale_backward_roots(seed, n, wg, nwg, slot, scale, None)

    for B, P in bad_shapes:
        assert stats(B=B, P=P) == -1 and to_nchw(B=B, P=P) == -1 and mask(B=B, P=P) == -1 and apply(B=B, P=P) == -1
        assert apply(B=B, P=P, acc=fake) == -1
    for bf16 in (-1, 2):
        assert stats(bf16=bf16) == -1 and apply(bf16=bf16) == -1 and apply(bf16=bf16, acc=fake) == -1
    assert stats(inp=None) == -1 and stats(out=None) == -1 and stats(np_=None) == -1
    assert stats(partials=None) == -1                                # neither partials nor a slot
    assert stats(bias=fake) == -1 and stats(full=fake) == -1 and stats(relu=1) == -1      # need slab1
    assert stats(slab1=fake, relu=2) == -1
    assert nparts.value == -7                                        # nothing was written
    assert to_nchw(inp=None) == -1 and to_nchw(out=None) == -1
    assert mask(dy=None) == -1 and mask(y=None) == -1 and mask(du=None) == -1
    assert apply(g=None) == -1 and apply(f8=None) == -1 and apply(out=None) == -1
    for name in ("A", "Bc", "Cc"):
        assert apply(**{name: None}) == -1
    for name in ("gamma", "mean", "invstd", "dgamma", "dbeta", "abc"):
        assert apply(acc=fake, **{name: None}) == -1
    assert apply(acc=fake, C=0) == -1 and apply(acc=fake, C=33) == -1 and apply(acc=fake, eval_=2) == -1
    assert apply(acc=fake, n=0.0) == -1 and apply(acc=fake, n=float("nan")) == -1
    assert roots(seed=None) == -1 and roots(scale=None) == -1
    for n in (0, -4, 1, 2, 3, 5, 6, 7, 4 * 2048 * 256 + 2):
        assert roots(n=n) == -1
    assert roots(wg=fake, nwg=0) == -1 and roots(nwg=-1) == -1
    # the per-op entry points of the same files
    assert lib.ava_bn_stats(fake, 100, 5, fake, None, None) == -1 and lib.ava_bn_stats(fake, 0, 8, fake, None, None) == -1
    assert lib.ava_bn_stats(None, 100, 8, fake, None, None) == -1
    for n, step in [(6, 1), (1, 1), (0, 1), (-4, 1), (8, 0), (8, -1)]:
        assert lib.ava_adam_flat(fake, fake, fake, fake, n, 1e-3, 0.9, 0.999, 1e-8, step, None) == -1
