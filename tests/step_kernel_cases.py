"""The numpy restatement of the training step's small kernels (``csrc/bn.hip``, ``csrc/misc.hip``, ``csrc/bn_acc.h``) and
the deterministic inputs of their tests (``test_cpu_step_kernels.py``, ``test_gpu_step_kernels.py``).

Tensors of the layout kernels are ``[B][32][P]`` floats: "NCHW" is ``[B, 32, P]``, "NHWC" is ``[B, P, 32]``.  One workgroup
moves tiles of 32 channels x 64 pixels; tile ``w = b * (P / 64) + q`` goes to workgroup ``w mod grid``.

The inputs are small dyadic rationals, so that every sum the kernels form is a sum of exactly representable terms whose
partial sums are exactly representable too: the result then does not depend on the order of the additions and the tests
compare with ``==``.  That is a property of the inputs, and it is checked, not assumed: the functions named ``*_f32_order``
restate the kernel's own order of float32 operations, and the CPU tests assert that they give the plain float64 sums.
"""
import numpy as np

QPIX = 64
CH = 32
STATS_CAP = 1024          # workgroups of nchw_to_nhwc_stats_kernel
LAYOUT_CAP = 2048         # workgroups of the other layout kernels
ACC_SHARDS = 8            # bn_acc.h (the library answers ava_acc_shards() / ava_acc_shard_ll())
ACC_SHARD_LL = 200
BN_EPS = 1e-5
BN_MOMENTUM = 0.1
LOG_2PI = 1.8378770664093453

# (B, P) of the layout tests; tiles = (P / 64) * B
LAYOUT_SHAPES = [(1, 64), (3, 256), (2048, 64), (2049, 64), (1025, 128), (683, 192), (1366, 192)]
STATS_SHAPES = [(1, 64), (3, 256), (1024, 64), (1025, 64), (513, 256), (683, 192)]


# ---- number formats ------------------------------------------------------------------------------------------------------
def bf16_round(x):
    """float32 -> the nearest bfloat16 (ties to even) -> float32; NaN stays NaN"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    bits = x.view(np.uint32).astype(np.uint64)
    rounded = ((bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    out = rounded.view(np.float32).copy()
    out[np.isnan(x)] = np.nan
    return out


def bf16_bits(x):
    """the 16 stored bits of ``bf16_round(x)``"""
    return (bf16_round(x).view(np.uint32) >> 16).astype(np.uint16)


def stored(x, bf16):
    """what an activation buffer holds of the float32 value"""
    return bf16_round(x) if bf16 else np.ascontiguousarray(x, dtype=np.float32)


def fma32(a, b, c):
    """float32 fma(a, b, c): one rounding of the exact a * b + c.  The product of two float32 is exact in float64; the sum
    is rounded to odd in float64 (two-sum gives the rounding error), after which the rounding to float32 is the rounding
    of the exact value (53 >= 2 * 24 + 2)."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        s = np.array(s, dtype=np.float64, ndmin=1)
        err = np.broadcast_to(err, s.shape)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s[fix] = np.nextafter(s[fix], np.where(err[fix] > 0, np.inf, -np.inf))
        return s.astype(np.float32).reshape(np.broadcast(a, b, c).shape)


# ---- layouts -------------------------------------------------------------------------------------------------------------
def nchw_to_nhwc(x):
    return np.ascontiguousarray(np.swapaxes(x, 1, 2))


def nhwc_to_nchw(x):
    return np.ascontiguousarray(np.swapaxes(x, 1, 2))


def layout_grid(B, P, cap):
    return min((P // QPIX) * B, cap)


def slab_sum(s0, s1, bias=None, relu=False):
    """0 + slab0 + slab1 (+ bias [32, P]), ReLU as fmaxf(s, 0): float32 throughout, in that order"""
    s = np.float32(0) + np.asarray(s0, np.float32)
    s = s + np.asarray(s1, np.float32)
    if bias is not None:
        s = s + np.asarray(bias, np.float32)[None]
    if relu:
        s = np.where(s > 0, s, np.float32(0))        # fmaxf: a NaN gives the other operand
    return s.astype(np.float32)


def relu_mask(dy_nchw, y_nhwc):
    """du (NHWC) = y > 0 ? dy : 0 (a NaN y gives 0)"""
    return np.where(np.asarray(y_nhwc) > 0, nchw_to_nhwc(dy_nchw), np.float32(0)).astype(np.float32)


def bn_bwd_apply(g_nhwc, f8_nchw, A, Bc, Cc, bf16):
    """out (NCHW) = f > 0 ? fma(A, g, fma(Bc, f, Cc)) : 0 with f the stored value of f8; coefficients [32]"""
    f = stored(f8_nchw, bf16)
    g = nhwc_to_nchw(g_nhwc)
    A, Bc, Cc = (np.asarray(v, np.float32)[None, :, None] for v in (A, Bc, Cc))
    du = fma32(A, g, fma32(Bc, f, Cc))
    return np.where(f > 0, du, np.float32(0)).astype(np.float32)


def tiles_of(nhwc):
    """[B, P, 32] -> [tiles, 64, 32] in the order of the tile index w = b * (P / 64) + q"""
    B, P, _ = nhwc.shape
    return nhwc.reshape(B * (P // QPIX), QPIX, CH)


def stats_partials_f32_order(stored_nhwc, grid):
    """[grid, 64] per-workgroup {sum [32], sum of squares [32]} of nchw_to_nhwc_stats_kernel in its own float32 order: thread
    (r, c) of a workgroup adds pixels r, r + 8, .. of each of its tiles (tiles ascending), the squares by fma; the eight r
    of a channel are then added ascending from zero."""
    tiles = tiles_of(np.asarray(stored_nhwc, np.float32))
    trips = -(-len(tiles) // grid)
    padded = np.zeros((trips * grid, QPIX, CH), np.float32)
    padded[:len(tiles)] = tiles
    padded = padded.reshape(trips, grid, 8, 8, CH)                  # [trip, workgroup, k, r, c]: pixel = 8 k + r
    s1 = np.zeros((grid, 8, CH), np.float32)
    s2 = np.zeros((grid, 8, CH), np.float32)
    with np.errstate(invalid="ignore"):
        for trip in range(trips):
            for k in range(8):
                v = padded[trip, :, k]
                s1 = s1 + v
                s2 = fma32(v, v, s2)
        out = np.zeros((grid, 2 * CH), np.float32)
        for r in range(8):
            out[:, :CH] = out[:, :CH] + s1[:, r]
            out[:, CH:] = out[:, CH:] + s2[:, r]
    return out


def stats_exact(stored_nhwc):
    """the plain float64 {sum [32], sum of squares [32]} over every sample and pixel"""
    v = np.asarray(stored_nhwc, np.float64).reshape(-1, CH)
    return np.concatenate([v.sum(0), (v * v).sum(0)])


# ---- bn_acc.h ------------------------------------------------------------------------------------------------------------
def split(p):
    """float32 partial(s) -> (l0, l1, l2, poison): the three signed 32-bit limbs of trunc(|p| * 2^48), limb k weighing
    2^(32 k - 48); poison for a NaN, an Inf or |p| >= 2^47 (the limbs are then 0)"""
    p = np.asarray(p, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        ad = np.abs(p.astype(np.float64)) * 2.0 ** 48
        poison = ~(ad < 2.0 ** 95)
        ad = np.where(poison, 0.0, ad)
        l2 = np.floor(ad * 2.0 ** -64)
        r1 = ad - l2 * 2.0 ** 64
        l1 = np.floor(r1 * 2.0 ** -32)
        l0 = np.floor(r1 - l1 * 2.0 ** 32)
    sg = np.where(p < 0, -1, 1).astype(np.int64)
    return sg * l0.astype(np.int64), sg * l1.astype(np.int64), sg * l2.astype(np.int64), poison


def empty_slot():
    return np.zeros((ACC_SHARDS, ACC_SHARD_LL), np.int64)


def slot_add(slot, workgroup, partial):
    """what the 64 bn_acc_add calls of one workgroup do to the slot: ``partial`` [64] float32"""
    sh = slot[workgroup % ACC_SHARDS]
    l0, l1, l2, poison = split(partial)
    sh[0:64] += l0
    sh[64:128] += l1
    sh[128:192] += l2
    if poison.any():
        sh[192] |= 1
    return slot


def slot_of_partials(partials):
    """the slot after workgroups 0 .. len(partials) - 1 added their rows to a zeroed one"""
    slot = empty_slot()
    for w, row in enumerate(np.asarray(partials, np.float32)):
        slot_add(slot, w, row)
    return slot


def read(slot):
    """bn_acc_read of the 64 values, in the kernel's float64 order (shards ascending); NaN when any flag word is set"""
    slot = np.asarray(slot, np.int64).reshape(ACC_SHARDS, ACC_SHARD_LL)
    s = np.zeros(64, np.float64)
    for sh in slot:
        s = s + ((sh[0:64].astype(np.float64) + sh[64:128].astype(np.float64) * 2.0 ** 32)
                 + sh[128:192].astype(np.float64) * 2.0 ** 64) * 2.0 ** -48
    return np.full(64, np.nan) if slot[:, 192].any() else s


def slot_from_values(values):
    """the slot scale_backward_roots leaves: the 64 float64 values as exact limbs in shard 0 (NaN: the flag of shard 0)"""
    slot = empty_slot()
    for i, v in enumerate(np.asarray(values, np.float64)):
        if not abs(v) * 2.0 ** 48 < 2.0 ** 95:
            slot[0, 192] = 1
            continue
        t = int(abs(v) * 2.0 ** 48)
        sg = -1 if v < 0 else 1
        slot[0, i], slot[0, 64 + i], slot[0, 128 + i] = sg * (t & 0xFFFFFFFF), sg * ((t >> 32) & 0xFFFFFFFF), sg * (t >> 64)
    return slot


def read_exact(slot):
    """the 64 values as exact integers, in units of 2^-48 (flags ignored)"""
    slot = np.asarray(slot, np.int64).reshape(ACC_SHARDS, ACC_SHARD_LL)
    return [sum(int(sh[i]) + (int(sh[64 + i]) << 32) + (int(sh[128 + i]) << 64) for sh in slot) for i in range(64)]


def slot_values(seed):
    """64 sums for a slot built by hand: multiples of 2^-20 up to 2^26 in size, of both signs, as the float32 pair (hi, lo)
    with value = hi + lo exact in float64 (hi a multiple of 16, |lo| < 8).  Values 0 .. 3 are fixed edge values."""
    rs = np.random.RandomState(seed)
    hi = (rs.randint(-2 ** 22, 2 ** 22, 64) * 16).astype(np.float32)
    lo = (rs.randint(-2 ** 23 + 1, 2 ** 23, 64) * 2.0 ** -20).astype(np.float32)
    hi[:4] = [0, 0, -(2.0 ** 26), 65536.0]
    lo[:4] = [0, 2.0 ** -20, 0, -(2.0 ** -20)]
    return hi, lo


def build_slot(values, seed):
    """a slot whose ``read`` is ``values`` [64] (float64 multiples of 2^-20, |v| < 2^27), spread over all shards: every shard
    holds a part of either sign with its limbs carrying the sign of the part (so limbs are negative, and the second and
    third are non-zero), and shards 1 and 5 hold theirs in the unnormalised form a sum of many arrivals has (a multiple of
    2^32 moved between limb 0 and limb 1)."""
    rs = np.random.RandomState(seed)
    slot = empty_slot()
    for i, v in enumerate(np.asarray(values, np.float64)):
        k = int(v * 2.0 ** 20)
        assert float(k) * 2.0 ** -20 == v and abs(k) < 2 ** 47
        parts = [int(x) for x in rs.randint(-2 ** 46, 2 ** 46, ACC_SHARDS - 1)]
        parts.append(k - sum(parts))
        for sh, part in enumerate(parts):
            t = abs(part) << 28                                    # units of 2^-48
            sg = -1 if part < 0 else 1
            l0, l1, l2 = sg * (t & 0xFFFFFFFF), sg * ((t >> 32) & 0xFFFFFFFF), sg * (t >> 64)
            if sh in (1, 5):
                carry = int(rs.randint(-512, 512))
                l0, l1 = l0 + (carry << 32), l1 - carry
            slot[sh, i], slot[sh, 64 + i], slot[sh, 128 + i] = l0, l1, l2
    return slot


# ---- column sums and the finalisers ----------------------------------------------------------------------------------------
def column_sums_f64_order(partials, ncols):
    """column_sums of bn.hip in its own float64 order: groups = 1024 // ncols threads per column, thread ``grp`` takes rows
    grp, grp + groups, .. (eight at a time as a balanced tree while eight remain, then one by one), and the per-group
    results are added by a binary tree over the groups that folds the upper half onto the lower."""
    partials = np.asarray(partials, np.float32).astype(np.float64)
    nparts = len(partials)
    groups = 1024 // ncols
    scratch = np.zeros((groups, ncols), np.float64)
    for grp in range(groups):
        s = np.zeros(ncols, np.float64)
        r = grp
        while r + 7 * groups < nparts:
            v = [partials[r + k * groups] for k in range(8)]
            s = s + (((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])))
            r += 8 * groups
        while r < nparts:
            s = s + partials[r]
            r += groups
        scratch[grp] = s
    cnt = groups
    while cnt > 1:
        half = (cnt + 1) >> 1
        scratch[:cnt - half] = scratch[:cnt - half] + scratch[half:cnt]
        cnt = half
    return scratch[0].copy()


def column_sums_exact(partials):
    """the exact column sums of integer-valued partials, as Python integers"""
    rows = np.asarray(partials, np.float32).astype(np.float64)
    assert np.array_equal(rows, np.round(rows))
    return [sum(int(v) for v in col) for col in rows.T]


def finalize(sums, n, C, gamma, beta, running_mean, running_var):
    """bn_finalize_kernel, training: float64 as the kernel; returns float32 mean, invstd, scale, shift and the float32
    running statistics after the momentum update, plus the float64 biased variance"""
    sums = np.asarray(sums, np.float64)
    n = float(n)
    mean = sums[:C] / n
    var = np.maximum(sums[C:2 * C] / n - mean * mean, 0.0)
    unb = var * (n / (n - 1.0)) if n > 1.0 else var
    rm = ((1.0 - BN_MOMENTUM) * np.asarray(running_mean, np.float32).astype(np.float64) + BN_MOMENTUM * mean)
    rv = ((1.0 - BN_MOMENTUM) * np.asarray(running_var, np.float32).astype(np.float64) + BN_MOMENTUM * unb)
    meanf = mean.astype(np.float32)
    invstd = (1.0 / np.sqrt(var + BN_EPS)).astype(np.float32)
    scale = np.asarray(gamma, np.float32) * invstd
    shift = np.asarray(beta, np.float32) - meanf * scale
    return dict(mean=meanf, invstd=invstd, scale=scale, shift=shift, running_mean=rm.astype(np.float32),
                running_var=rv.astype(np.float32), var=var, mean64=mean, running_mean64=rm, running_var64=rv)


def finalize_bwd(sums, n, C, gamma, mean, invstd, eval_mode=False):
    """bn_finalize_bwd_kernel / the backward side of bn_coef_from_acc: sums = {sum g [C], sum g * xhat [C]}.  Cc is given
    in float64 (its float32 value depends on whether the compiler contracts -a * dB / n - b * mu) with the larger of its two
    terms, the scale of its bound."""
    sums = np.asarray(sums, np.float64)
    n = float(n)
    dB, dG = sums[:C], sums[C:2 * C]
    inv, gm, mu = (np.asarray(v, np.float32).astype(np.float64)[:C] for v in (invstd, gamma, mean))
    a = gm * inv
    b = np.zeros(C) if eval_mode else -gm * inv * inv * dG / n
    cc = np.zeros(C) if eval_mode else -a * dB / n - b * mu
    with np.errstate(invalid="ignore"):
        term = np.maximum(np.abs(a * dB / n), np.abs(b * mu))
    return dict(dgamma=dG.astype(np.float32), dbeta=dB.astype(np.float32), A=a.astype(np.float32),
                Bc=b.astype(np.float32), Cc64=cc, Cc_term=term)


def integer_partials(nparts, ncols, seed):
    """integer-valued float32 partial rows in [-2000, 2000]: column sums of up to 16 g + 3 <= 8195 rows stay below 2^24"""
    rs = np.random.RandomState(seed)
    return rs.randint(-2000, 2001, (nparts, ncols)).astype(np.float32)


def finalize_partials(nparts, C, seed):
    """integer-valued forward partials {sum x, sum x^2} with a positive variance for n = 16 nparts elements per channel"""
    rs = np.random.RandomState(seed)
    return np.concatenate([rs.randint(-30, 31, (nparts, C)), rs.randint(1000, 2001, (nparts, C))], axis=1).astype(np.float32)


def finalize_nparts(C):
    """the row counts around the edges of column_sums' eight-row loop, g = 1024 // (2 C) rows per pass"""
    g = 1024 // (2 * C)
    return sorted({1, g - 1, g, g + 1, 7 * g, 7 * g + 1, 8 * g - 1, 8 * g, 8 * g + 1, 16 * g + 3} - {0})


# ---- ava_bn_stats ----------------------------------------------------------------------------------------------------------
def bn_stats_grid(n, C):
    work = n // 4 if C == 1 else n
    return max(1, min(1024, -(-work // 2048)))


def integer_rows(n, C, seed):
    """[n, C] float32 integers in [-3, 3]"""
    return np.random.RandomState(seed).randint(-3, 4, (n, C)).astype(np.float32)


def _wave_tree(v):
    """wave_sum over the last axis (64 lanes): v += shuffle_xor(v, o) for o = 32 .. 1"""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    return v[..., 0]


def bn_stats_partials_f32_order(x, C):
    """[grid, 2 C] partials of bn_stats_kernel in its own float32 order: per-thread strided sums (the squares by fma for
    C > 1; for C = 1 four elements at a time as (x + y) + (z + w) and (xx + yy) + (zz + ww), the n % 4 tail by thread 0),
    the xor butterfly over the lanes of a wave, then (wave 0 + wave 1) + (wave 2 + wave 3)."""
    x = np.asarray(x, np.float32).reshape(-1, C)
    n = len(x)
    grid = bn_stats_grid(n, C)
    threads = grid * 256
    if C == 1:
        n4 = n // 4
        trips = max(1, -(-n4 // threads))
        q = np.zeros((trips * threads, 4), np.float32)
        q[:n4] = x[:n4 * 4].reshape(n4, 4)
        q = q.reshape(trips, threads, 4)
        s1 = np.zeros((threads, 1), np.float32)
        s2 = np.zeros((threads, 1), np.float32)
        for t in range(trips):
            v = q[t]
            s1[:, 0] = s1[:, 0] + ((v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3]))
            s2[:, 0] = s2[:, 0] + ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + (v[:, 2] * v[:, 2] + v[:, 3] * v[:, 3]))
        for i in range(n4 * 4, n):
            s1[0, 0] = s1[0, 0] + x[i, 0]
            s2[0, 0] = s2[0, 0] + x[i, 0] * x[i, 0]
    else:
        trips = -(-n // threads)
        q = np.zeros((trips * threads, C), np.float32)
        q[:n] = x
        q = q.reshape(trips, threads, C)
        s1 = np.zeros((threads, C), np.float32)
        s2 = np.zeros((threads, C), np.float32)
        for t in range(trips):
            s1 = s1 + q[t]
            s2 = fma32(q[t], q[t], s2)
    both = np.concatenate([s1, s2], axis=1).reshape(grid, 4, 64, 2 * C)           # [workgroup, wave, lane, value]
    red = _wave_tree(np.moveaxis(both, 2, 3))                                # [workgroup, wave, value]
    return ((red[:, 0] + red[:, 1]) + (red[:, 2] + red[:, 3])).astype(np.float32)


def bn_stats_exact(x, C):
    v = np.asarray(x, np.float64).reshape(-1, C)
    return np.concatenate([v.sum(0), (v * v).sum(0)])


# ---- inputs of the layout kernels ------------------------------------------------------------------------------------------
def layout_values(shape, seed, bf16=False, span=16, base=1.0):
    """float32 multiples of 1/8 in [-span / 8, span / 8] with both zeros among them.  bf16: about one element in eight is
    instead one of the values bfloat16 storage changes: 1 + 2^-8 and 1 + 3 * 2^-8 (ties: to 1 and to 1 + 2^-6),
    1 + 2^-8 + 2^-12 (up to 1 + 2^-7), -(1 + 2^-7 + 2^-9) (down in size to -(1 + 2^-7)), with ``base`` (1 or 1.5) in the
    place of 1.  Every stored value is a multiple of 2^-7 of size <= max(span / 8, base + 2^-6)."""
    rs = np.random.RandomState(seed)
    v = (rs.randint(-span, span + 1, shape) / 8.0).astype(np.float32)
    v[rs.randint(0, 16, shape) == 0] = np.float32(-0.0)
    if bf16:
        odd = np.array([base + 2.0 ** -8, base + 3 * 2.0 ** -8, base + 2.0 ** -8 + 2.0 ** -12,
                        -(base + 2.0 ** -7 + 2.0 ** -9)], np.float32)
        pick = rs.randint(0, 8, shape) == 0
        v[pick] = odd[rs.randint(0, 4, shape)][pick]
    return v


STATS_VARIANTS = ["plain", "slabs", "slabs_bias_relu"]


def stats_case(B, P, bf16, variant, seed=0):
    """the inputs of one nchw_to_nhwc_stats launch and what it must give: ``value`` (NCHW float32, what ``full`` receives),
    ``stored`` (NHWC float32 values of what ``out`` holds).  Sizes are chosen so that |stored| <= 2 and a multiple of 2^-7:
    with at most three tiles per workgroup the squares of a channel sum to less than 2^24 units of 2^-14 in any order.
    The slabs added to a value that bfloat16 changes (1.5 + ..) are of size <= 3/8: the sum stays in [1, 2), where it is
    rounded to a multiple of 2^-7 again (in a smaller binade it would keep its low bits and the squares would not be exact)."""
    shape = (B, CH, P)
    seed = seed + 7 * B + P + (1000 if bf16 else 0)
    case = dict(B=B, P=P, bf16=bf16, variant=variant, slab1=None, bias=None, relu=0)
    if variant == "plain":
        case["in"] = layout_values(shape, seed, bf16)
        case["value"] = case["in"]
    else:
        case["in"] = layout_values(shape, seed + 1, bf16, span=8, base=1.5)
        case["slab1"] = layout_values(shape, seed + 2, span=2)
        if variant == "slabs_bias_relu":
            case["bias"] = layout_values((CH, P), seed + 3, span=1)
            case["relu"] = 1
        case["value"] = slab_sum(case["in"], case["slab1"], case["bias"], case["relu"])
    case["stored"] = stored(nchw_to_nhwc(case["value"]), bf16)
    return case


def dyadic_coefficients(seed):
    """A, Bc, Cc [32]: multiples of 1/4 in [-2, 2]: with the values of ``layout_values`` both fmas are exact"""
    rs = np.random.RandomState(seed)
    return tuple((rs.randint(-8, 9, CH) / 4.0).astype(np.float32) for _ in range(3))


# ---- ELBO ------------------------------------------------------------------------------------------------------------------
def elbo(latent_sums, sse_partials, zdim, prec, xdim=16384):
    """elbo_finalize_kernel on integer-valued sums: (loss in float64, float32 {sum z^2, SSE, sum H})"""
    lat = np.asarray(latent_sums, np.float64)
    sse = np.asarray(sse_partials, np.float64)
    sz2, sh, s = lat[:, 0].sum(), lat[:, 1].sum(), sse[:, 0].sum()
    c1 = 0.5 * zdim * LOG_2PI
    c2 = 0.5 * xdim * (LOG_2PI - np.log(float(np.float32(prec))))
    loss = 0.5 * sz2 + c1 + c2 + 0.5 * float(np.float32(prec)) * s - sh
    return loss, np.array([sz2, s, sh]).astype(np.float32)


def elbo_f64_order(values):
    """a column of elbo_finalize_kernel's sums in its own float64 order: 256 strided threads, the xor butterfly over each
    wave, the four waves ascending"""
    v = np.asarray(values, np.float64)
    trips = -(-len(v) // 256)
    padded = np.zeros(trips * 256)
    padded[:len(v)] = v
    per_thread = np.zeros(256)
    for row in padded.reshape(trips, 256):
        per_thread = per_thread + row
    waves = _wave_tree(per_thread.reshape(4, 64))
    return ((waves[0] + waves[1]) + waves[2]) + waves[3]
