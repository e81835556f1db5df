"""The k-means kernels (csrc/kmeans.hip, row f25) on the MI355X at their dispatch, relocation, scan and grid edges: the
EDGE_ cases of kmeans_cases.py against the numpy restatement.  test_cpu_kmeans.py proves without a GPU that every case
decides what it claims (which accumulator count runs, which rows a relocation picks, where the labels change, which scan
entry a threshold meets), so the comparisons here are conditions, not hopes.

Bounds are the project's: STEP = 1e-12 relative to the largest wanted entry for one step, FIT = 1e-11 for whole fits, and
== wherever the arithmetic is exact (integer lattices through one assign and one sums pass) or is additions in the
restated order followed by one correctly rounded division (the per-cluster means, the inertia of the device's own d2).
Every test prints its largest error against its bound.

Lattice cases are asserted for one iteration only, through ava_km_fit with it0 = 0, n_iters = 1 and a shift pointer:
after the division the centres are no longer exact, and on the lattice later iterations have rows exactly between two
centres (test_cpu_kmeans.py shows the assign margin of their whole fits is 0.0), so whole fits are left out there."""
import warnings

import numpy as np
import pytest
import torch

import kmeans_cases as KC
from test_gpu_kmeans import FIT, SHAPES, STEP, pair_sqdist, rows32
from ava_amd import _lib
from ava_amd import kmeans as KM

pytestmark = pytest.mark.gpu
CANARY = -12345.0
_WORST = {}


def report(group, what, got, want, bound):
    """the error of ``got`` relative to the largest wanted entry; prints it, and the group's largest so far, by the bound"""
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    err = float(np.abs(got - want).max() / max(np.abs(want).max(), np.finfo(float).tiny))
    _WORST[group] = max(_WORST.get(group, 0.0), err)
    print("group %s, %s: error %.3e, the group's largest %.3e (bound %.0e)" % (group, what, err, _WORST[group], bound))
    return err


def exact(group, what, got, want):
    """== on every entry (so the bits, zero's sign apart); prints the count of entries that differ"""
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    differ = int((got != np.asarray(want)).sum()) if got.shape == np.shape(want) else -1
    print("group %s, %s: %d of %d entries differ (bound: ==)" % (group, what, differ, got.size))
    return differ == 0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def wanted_centres(X, labels, k):
    sums, counts = KC.cluster_sums(X, labels, k)
    return np.where(counts[:, None] > 0, sums / np.maximum(counts, 1)[:, None], 0.0), counts


class Loop:
    """ava_km_fit one iteration per call, with a shift pointer: the state that _lloyd_device keeps, held here to be read"""

    def __init__(self, rows, start, tol, mean_var=None, words=8):
        self.X = dev(rows)
        self.n, self.d, self.k = int(self.X.shape[0]), int(self.X.shape[1]), len(start)
        self.centres = dev(np.asarray(start, dtype=np.float64)).clone()
        self.labels = torch.full((self.n,), -1, dtype=torch.int32, device="cuda")
        self.d2 = torch.full((self.n,), CANARY, dtype=torch.float64, device="cuda")
        self.ctl = torch.zeros(words, dtype=torch.int32, device="cuda")
        self.shift = torch.full((2,), CANARY, dtype=torch.float64, device="cuda")
        self.mean_var = KM._variance_device(self.X) if mean_var is None else dev(np.array([mean_var], dtype=np.float64))
        self.tol = float(tol)
        self.ws, self.nbytes = KM._workspace(self.n, self.d, self.k, self.X.device)
        self.it = 0

    def step(self):
        assert 2 + self.it + 1 < len(self.ctl)
        _lib.check(_lib.load().ava_km_fit(self.X.data_ptr(), _lib.dtype_code(self.X), self.n, self.d, self.k,
                                          self.centres.data_ptr(), self.labels.data_ptr(), self.d2.data_ptr(), self.tol,
                                          self.mean_var.data_ptr(), self.it, 1, self.ctl.data_ptr(), self.shift.data_ptr(),
                                          self.ws.data_ptr(), self.nbytes, _lib.stream()), "ava_km_fit")
        self.it += 1
        torch.cuda.synchronize()
        assert float(self.shift[1].item()) == CANARY
        return host(self.ctl)

    def state(self):
        return [host(t).copy() for t in (self.centres, self.labels, self.d2, self.shift)]


# ---- A, B: the dispatch of the sums and their order -------------------------------------------------------------------
@pytest.mark.parametrize("n,d,k", KC.EDGE_DISPATCH)
def test_sums_dispatch_against_the_restatement(n, d, k):
    """K = 16 | 17 (one accumulator, two), 32 | 33 (two, four with a dead slot), 48 | 49 (a dead slot, none): assign, update
    and the inertia as test_assign_and_update_against_the_restatement holds them, and the centres in bits"""
    X32, C = KC.dispatch_case(n, d, k)
    X = X32.astype(np.float64)
    want_labels, want_d2 = KC.assign(X, C)
    labels, d2 = KM.assign(X, C)
    assert np.array_equal(host(labels), want_labels)
    assert torch.equal(d2, pair_sqdist(X, C, labels))
    assert report("A", "d2 (%d, %d, %d)" % (n, d, k), d2, want_d2, STEP) <= STEP
    labels32, d232 = KM.assign(X32, C)
    assert torch.equal(labels32, labels) and torch.equal(d232, d2)
    total = KM._assign_device(dev(X), dev(C), inertia=True)[2]
    assert report("A", "inertia", total, KC.chunk_sum(want_d2), STEP) <= STEP
    assert exact("B", "inertia of the device's d2", total, [KC.chunk_sum(host(d2))])
    want_centres, counts = wanted_centres(X, want_labels, k)
    centres, cnt = KM.update(X, labels, k)
    assert cnt.dtype == torch.int64 and np.array_equal(host(cnt), counts) and counts.min() > 0
    assert report("A", "centres", centres, want_centres, STEP) <= STEP
    assert exact("B", "centres (%d, %d, %d)" % (n, d, k), centres, want_centres)
    centres32, cnt32 = KM.update(X32, host(labels).astype(np.int64), k)
    assert torch.equal(centres32, centres) and torch.equal(cnt32, cnt)


@pytest.mark.parametrize("n,d,k", SHAPES)
def test_sum_order_in_bits(n, d, k):
    """The sums are plain additions, rows ascending inside the chunks and the chunks ascending, which cluster_sums restates
    with np.cumsum; the mean is one correctly rounded division.  So the centres are the restatement's in bits, from
    float64 rows and from float32 rows against their float64 copy, and the inertia is chunk_sum of the device's own d2."""
    X32, X = rows32(n, d, 100 + n + d + k)
    rng = np.random.RandomState(k)
    C = X[rng.choice(n, size=k, replace=k > n)] + 0.25 * rng.standard_normal((k, d))
    labels, d2, total = KM._assign_device(dev(X), dev(C), inertia=True)
    want_centres, counts = wanted_centres(X, host(labels), k)
    for rows in (X, X32):
        centres, cnt = KM.update(rows, labels, k)
        assert np.array_equal(host(cnt), counts)
        assert exact("B", "centres (%d, %d, %d) %s" % (n, d, k, rows.dtype), centres, want_centres)
    assert exact("B", "inertia of the device's d2", total, [KC.chunk_sum(host(d2))])


@pytest.mark.parametrize("k,k2", KC.EDGE_BOUNDARIES)
def test_no_result_depends_on_the_accumulator_count(k, k2):
    """one label vector, all below K, through the kernels on both sides of a dispatch boundary: the same bits, and the
    extra cluster empty"""
    X32, labels = KC.boundary_case(k)
    want_centres, counts = wanted_centres(X32.astype(np.float64), labels, k)
    for rows in (X32, X32.astype(np.float64)):
        low, low_cnt = KM.update(rows, labels, k)
        high, high_cnt = KM.update(rows, labels, k2)
        assert torch.equal(high[:k], low) and torch.equal(high_cnt[:k], low_cnt)
        assert not bool(high[k:].any()) and not bool(high_cnt[k:].any())
        assert np.array_equal(host(low_cnt), counts)
        assert exact("A", "centres at K = %d and %d, %s" % (k, k2, rows.dtype), low, want_centres)


# ---- C: labels outside [0, K) -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KC.EDGE_FOREIGN_K)
@pytest.mark.parametrize("rot", [0, 3])
def test_foreign_labels_are_in_no_cluster(k, rot):
    """-1, K, K + 15, -16, INT32_MAX and INT32_MIN at the stage edges 63 | 64 and the chunk edge 2047 | 2048: centres and
    counts in the bits of the restatement, which skips those rows.  A -1 that reached slot 0 of group 15 would move centre
    15; a -16 would move centre 0."""
    X32, labels, rows = KC.foreign_case(k, rot)
    want_centres, counts = wanted_centres(X32.astype(np.float64), labels, k)
    assert counts.sum() == len(X32) - len(rows)
    for data in (X32, X32.astype(np.float64)):
        centres, cnt = KM.update(data, labels, k)
        assert np.array_equal(host(cnt), counts)
        assert exact("C", "centres K = %d, rot %d, %s" % (k, rot, data.dtype), centres, want_centres)
    centres64, cnt64 = KM.update(X32, labels.astype(np.int64), k)                 # the labels as int64: the same int32 values
    assert np.array_equal(host(centres64), want_centres) and np.array_equal(host(cnt64), counts)


# ---- D: relocation, one iteration on exact rows -----------------------------------------------------------------------
@pytest.mark.parametrize("m", KC.EDGE_RELOCATION_M)
@pytest.mark.parametrize("reverse", [False, True])
def test_relocation_picks_on_the_lattice(m, reverse):
    """K = 9 (register sums) and K = 70 (LDS sums) with m = 5 and 66 empty clusters: the picks are rows of a second pass of
    the r += 256 loop, tied inside one thread's rows, in chunk 1, and two donors are left with count 0 and keep their
    residual sum (0, 0).  One iteration through the ABI (see the module docstring); the turned-round rows must give the
    restatement's answer for their own order."""
    X, init = KC.relocation_case(m, reverse)
    want_labels, want_d2 = KC.assign(X, init)
    want_centres, want_shift = KC.update(X, want_labels, want_d2, init)
    assert np.array_equal(want_centres[4:], X[KC.relocation_picks(want_d2, m)])
    states = []
    for rows in (X, X.astype(np.float32)):
        loop = Loop(rows, init, tol=0.0, mean_var=1.0)
        ctl = loop.step()
        what = "m = %d%s, %s" % (m, ", reversed" if reverse else "", rows.dtype)
        assert exact("D", "labels " + what, loop.labels, want_labels)
        assert exact("D", "d2 " + what, loop.d2, want_d2)
        assert exact("D", "centres " + what, loop.centres, want_centres)
        assert report("D", "shift " + what, loop.shift[:1], [want_shift], STEP) <= STEP
        assert ctl[:4].tolist() == [0, 1, 0, 0]                                    # not strict, one iteration, not stopped
        states.append(loop.state())
    assert all(np.array_equal(a, b) for a, b in zip(*states))                      # float32 rows: the same bits


# ---- E: more than 256 assign tiles ------------------------------------------------------------------------------------
def test_changed_labels_are_counted_past_tile_255():
    """258 tiles, and iterations 1 to 3 change labels in tiles 256 and 257 alone: a count over 256 tiles stops at
    n_iter = 2"""
    X32, init = KC.many_tiles_case()
    X = X32.astype(np.float64)
    mine = KC.fit(X, 2, init=init, tol=0.0)
    m = KM.KMeans(2, init=init, tol=0.0).fit(X)
    print("group E: n_iter %d, the restatement's %d" % (m.n_iter_, mine["n_iter"]))
    assert m.n_iter_ == mine["n_iter"] == 5
    assert np.array_equal(m.labels_, mine["labels"])
    assert report("E", "centres", m.cluster_centers_, mine["centres"], FIT) <= FIT
    assert report("E", "inertia", [m.inertia_], [mine["inertia"]], FIT) <= FIT
    m32 = KM.KMeans(2, init=init, tol=0.0).fit(X32)
    assert m32.n_iter_ == m.n_iter_ and np.array_equal(m32.labels_, m.labels_)
    assert np.array_equal(m32.cluster_centers_, m.cluster_centers_) and m32.inertia_ == m.inertia_


# ---- F: distances to the centres --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,k", KC.EDGE_TRANSFORM)
def test_transform_at_tile_edges(n, d, k):
    """one, two and four centre tiles (grid.y) with row tails; the output in a padded buffer"""
    X32, C = KC.transform_case(n, d, k)
    X = X32.astype(np.float64)
    want_labels, want_d2 = KC.assign(X, C)
    Cd = dev(C)
    outs = []
    for rows in (X, X32):
        Xd = dev(rows)
        buf = torch.full((n * k + 64,), CANARY, dtype=torch.float64, device="cuda")
        _lib.check(_lib.load().ava_km_transform(Xd.data_ptr(), _lib.dtype_code(Xd), n, d, k, Cd.data_ptr(), buf.data_ptr(),
                                                _lib.stream()), "ava_km_transform")
        assert bool((buf[n * k:] == CANARY).all())
        out = buf[:n * k].view(n, k)
        assert torch.equal(KM._transform_device(Xd, Cd), out)
        outs.append(host(out))
    out = outs[0]
    assert np.array_equal(outs[1], out)                                            # float32 rows: the same bits
    assert report("F", "distances (%d, %d, %d)" % (n, d, k), out, np.sqrt(KC.sqd(X, C)), STEP) <= STEP
    assert np.array_equal(np.argmin(out, axis=1), want_labels)
    assert report("F", "own distance squared", out[np.arange(n), want_labels] ** 2, want_d2, STEP) <= STEP
    labels, d2 = KM.assign(X, C)
    assert np.array_equal(host(labels), want_labels)
    assert report("F", "own distance squared, the device's d2", out[np.arange(n), want_labels] ** 2, host(d2), STEP) <= STEP


# ---- G: the column variances ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", KC.EDGE_VARIANCE)
def test_variance_values(n, d):
    """out[0] = mean(var(X, axis=0)) and out[1:] the column variances in the chunk order, at one row, at the chunk edges
    and over three chunks; a constant column is exactly 0.0; the output in a padded buffer"""
    X32 = KC.variance_case(n, d)
    X = X32.astype(np.float64)
    _, want = KC.column_variances(X)
    outs = []
    for rows in (X, X32):
        Xd = dev(rows)
        ws, nbytes = KM._workspace(n, d, 1, Xd.device)
        buf = torch.full((1 + d + 16,), CANARY, dtype=torch.float64, device="cuda")
        _lib.check(_lib.load().ava_km_variance(Xd.data_ptr(), _lib.dtype_code(Xd), n, d, buf.data_ptr(), ws.data_ptr(),
                                               nbytes, _lib.stream()), "ava_km_variance")
        assert bool((buf[1 + d:] == CANARY).all())
        assert torch.equal(KM._variance_device(Xd), buf[:1 + d])
        outs.append(host(buf[:1 + d]))
    out = outs[0]
    assert np.array_equal(outs[1], out)                                            # float32 rows: the same bits
    if n == 1:
        assert not out.any() and not want.any()
        print("group G, (%d, %d): all zeros" % (n, d))
        return
    assert report("G", "column variances (%d, %d)" % (n, d), out[1:], want, STEP) <= STEP
    assert report("G", "their mean", out[:1], [KC.mean_variance(X)], STEP) <= STEP
    if d >= 2:
        assert out[1 + d // 2] == 0.0 and want[d // 2] == 0.0                     # the constant column


# ---- H: the k-means++ scan, exact -------------------------------------------------------------------------------------
def pp_trial(Xd, first, rand):
    """ava_km_pp_start from ``first`` and one ava_km_pp_step with the thresholds ``rand``: (row, potential, closest)"""
    lib = _lib.load()
    n, d = int(Xd.shape[0]), int(Xd.shape[1])
    ws, nbytes = KM._workspace(n, d, 1, Xd.device)
    rand_d = dev(np.asarray(rand, dtype=np.float64))
    closest = torch.full((n + 16,), CANARY, dtype=torch.float64, device="cuda")
    idx = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    pot = torch.full((2,), CANARY, dtype=torch.float64, device="cuda")
    code, st = _lib.dtype_code(Xd), _lib.stream()
    _lib.check(lib.ava_km_pp_start(Xd.data_ptr(), code, n, d, first, closest.data_ptr(), st), "ava_km_pp_start")
    _lib.check(lib.ava_km_pp_step(Xd.data_ptr(), code, n, d, len(rand), rand_d.data_ptr(), closest.data_ptr(),
                                  idx.data_ptr(), pot.data_ptr(), ws.data_ptr(), nbytes, st), "ava_km_pp_step")
    assert int(idx[1].item()) == -7 and float(pot[1].item()) == CANARY and bool((closest[n:] == CANARY).all())
    return int(idx[0].item()), float(pot[0].item()), host(closest[:n])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_scan_thresholds_on_chunk_ends(dtype):
    """scan[r] = r exactly: thresholds on the last scan entry of a chunk and just above it, in a last chunk of one row, at
    the potential and past it, one candidate per call (n_trials = 1); then all eight at once (n_trials = 8), where the
    least potential is shared by the rows 2047 and 2048 and the first wins"""
    X = KC.scan_case()
    Xd = dev(X.astype(dtype))
    start = KC.sqd(X, X[0:1])[:, 0]
    differ = 0
    for rand, row in zip(KC.EDGE_SCAN_RAND, KC.EDGE_SCAN_ROWS):
        cand, pots, b, closest = KC.plusplus_trial(X, start, [rand])
        got = pp_trial(Xd, 0, [rand])
        print("group H, threshold %.4f x 4096: row %d (wanted %d), potential %r (wanted %r)"
              % (rand, got[0], row, got[1], float(pots[0])))
        differ += got[0] != row
        assert got[0] == row == cand[0] and got[1] == pots[0] and np.array_equal(got[2], closest)
    cand, pots, b, closest = KC.plusplus_trial(X, start, KC.EDGE_SCAN_RAND)
    got = pp_trial(Xd, 0, KC.EDGE_SCAN_RAND)
    print("group H, eight thresholds at once: row %d (wanted %d), potential %r; %d rows differed (bound: ==)"
          % (got[0], cand[b], got[1], differ + (got[0] != cand[b])))
    assert pots[1] == pots[2] == pots.min() and cand[b] == 2047
    assert got[0] == 2047 and got[1] == pots[b] and np.array_equal(got[2], closest)


def test_scan_plateaus_across_the_chunk_boundaries():
    """from row 2047 closest is zero at every odd row: the scan is flat over 2046 | 2047 and 4094 | 4095, the last rows of
    both full chunks.  Thresholds on the plateau values and between them, one per call, against plusplus_steps."""
    X = KC.scan_case()
    rand, v = KC.plateau_thresholds()
    differ = 0
    for rows in (X, X.astype(np.float32)):
        Xd = dev(rows)
        for r, vi in zip(rand, v):
            want = KC.plusplus_steps(X, 2, 2047, np.array([[r]]))[1]
            got = pp_trial(Xd, 2047, [r])[0]
            differ += got != want
            assert got == want, (vi, got, want)
    print("group H, plateaus: %d of %d rows differ (bound: ==)" % (differ, 2 * len(rand)))


# ---- I: the loop's control words --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tol", KC.EDGE_CONTROL)
def test_control_words_and_shift_per_iteration(name, tol):
    """ava_km_fit one iteration per call: shift, ctl[1] and the flag ctl[2 + it + 1] after every call, ctl[0] after a strict
    stop alone; two more calls after the stop change nothing but the next flags, which are set"""
    X, start, tol, tol_abs = KC.control_case(name, tol)
    steps = KC.lloyd_steps(X, start, tol_abs, 300)
    loop = Loop(X, start, tol, words=len(steps) + 8)
    for it, step in enumerate(steps):
        ctl = loop.step()
        what = "%s tol %g, iteration %d" % (name, tol, it)
        assert report("I", "shift " + what, loop.shift[:1], [step["shift"]], FIT) <= FIT
        assert np.array_equal(host(loop.labels), step["labels"])
        assert report("I", "centres " + what, loop.centres, step["centres"], FIT) <= FIT
        assert ctl[1] == it + 1
        assert ctl[2 + it + 1] == (1 if step["stopped"] else 0) and not ctl[2 + it + 2:].any()
        assert ctl[0] == (1 if step["strict"] else 0)
    assert steps[-1]["stopped"] and ctl[1] == len(steps)
    kept, words = loop.state(), ctl[:2].copy()
    for more in range(2):
        ctl = loop.step()
        assert np.array_equal(ctl[:2], words) and ctl[2 + loop.it] == 1
        assert all(np.array_equal(a, b) for a, b in zip(loop.state(), kept))
    assert ctl[2:2 + len(steps)].tolist() == [0] * len(steps) and ctl[2 + len(steps):2 + len(steps) + 3].tolist() == [1, 1, 1]


def test_every_row_its_own_centre():
    """K = n = 256 lattice rows, the init the same rows permuted: one iteration (shift is 0.0, a stop by the tolerance),
    the labels the inverse permutation, an inertia of exactly 0.0 and no warning"""
    X, init, perm = KC.permuted_lattice_case()
    inverse = np.empty(256, dtype=np.int64)
    inverse[perm] = np.arange(256)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m = KM.KMeans(256, init=init).fit(X)
    print("group I, permuted lattice: n_iter %d, inertia %r" % (m.n_iter_, m.inertia_))
    assert m.n_iter_ == 1 and np.array_equal(m.labels_, inverse) and m.inertia_ == 0.0
    assert np.array_equal(m.cluster_centers_, init)
    loop = Loop(X, init, 1e-4)
    ctl = loop.step()
    assert ctl[:4].tolist() == [0, 1, 0, 1] and float(loop.shift[0].item()) == 0.0
    assert np.array_equal(host(loop.labels), inverse) and not host(loop.d2).any()
    assert np.array_equal(host(loop.centres), init)
