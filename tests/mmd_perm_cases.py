"""Cases and the numpy restatement of the MMD^2 permutation test of ava_amd.mmd (``mmd2_permutation_test``,
``mmd2_permutation_matrix``).

The model of the splits is the project's own (the reference has no test of significance); the statistic of a split is
the reference's ``term_1 + term_2 - term_3`` (ava/plotting/mmd_plots.py:277-295), computed here by the three
brute-force sums of the reference's loops over the two sets of the split -- not by the K0 S identity the kernels use
(``gemm_terms`` restates that one, for the CPU test that compares the two).  Split 0 is the caller's own and is pinned
to oracle/mmd_oracle.py by tests/test_cpu_mmdperm.py.  The inputs come from ava_amd.synthetic's hash streams.
"""
import numpy as np

from ava_amd import synthetic as syn

GOLD = np.uint64(0x9E3779B97F4A7C15)
BOUND = 1e-11               # relative to t1 + t2 + t3: what tests/test_gpu_mmd_matrix.py holds the MMD means to

MEMBER_POOLS = [(2, 3), (64, 64), (65, 129), (129, 70), (3, 1000)]
VALUE_POOLS = [(2, 3), (64, 64), (65, 129), (129, 70), (2, 129)]
VALUE_Z = [1, 32, 128]
SEED, N_PERM = 5, 199       # the p-value cases


def keys(n, seed, pair, p):
    """uint64 [n]: the key of every pool position in split p >= 1: the splitmix64 finaliser of ``synthetic.u01`` before
    its shift to a double, for element j of stream ``salt = ((seed + pair) mod 2^32) 2^32 + p``"""
    salt = np.uint64((((int(seed) + int(pair)) % (1 << 32)) << 32) + int(p))
    with np.errstate(over="ignore"):
        x = np.arange(n, dtype=np.uint64) + salt * GOLD
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return x


def membership(n1, n2, seed, pair, p, key_fn=keys):
    """uint8 [n1 + n2]: 1 where the pool position is in set 1 of split p.  Split 0 is positions 0 .. n1 - 1; otherwise
    the n1 positions with the smallest (key, j): a stable argsort of the keys"""
    n = n1 + n2
    out = np.zeros(n, dtype=np.uint8)
    if p == 0:
        out[:n1] = 1
    else:
        out[np.argsort(key_fn(n, seed, pair, p), kind='stable')[:n1]] = 1
    return out


def memberships(n1, n2, seed, pair, n_perm):
    """uint8 [n_perm + 1, n1 + n2]: splits 0 .. n_perm"""
    return np.stack([membership(n1, n2, seed, pair, p) for p in range(n_perm + 1)])


def kernel_matrix(pool, sigma):
    """exp(A d^2) of all pairs of pool rows, direct differences like the reference's loops"""
    A = -0.5 / (sigma ** 2)
    d = ((pool[:, None, :] - pool[None, :, :]) ** 2).sum(axis=2)
    return np.exp(A * d)


def split_terms(K, member):
    """(term_1, term_2, term_3, statistic) of one split by the reference's three sums (mmd_plots.py:277-295): over
    i < j inside set 1, over i < j inside set 2, over all pairs between them"""
    s1, s2 = np.flatnonzero(member), np.flatnonzero(member == 0)
    n1, n2 = len(s1), len(s2)
    t1 = np.triu(K[np.ix_(s1, s1)], k=1).sum() * (2 / (n1 * (n1 - 1)))
    t2 = np.triu(K[np.ix_(s2, s2)], k=1).sum() * (2 / (n2 * (n2 - 1)))
    t3 = K[np.ix_(s1, s2)].sum() * (2 / (n1 * n2))
    return t1, t2, t3, t1 + t2 - t3


def gemm_terms(K, member):
    """the same four numbers the way csrc/mmd_perm.hip forms them: K0 = K with a zero diagonal, S marks the SMALLER
    set, Y = K0 S, a = sum_{i in S} Y_i, cross = sum_{i not in S} Y_i, T = sum K0; the other set's sum is T - a - 2 cross"""
    K0 = K - np.diag(np.diag(K))
    n1 = int(member.sum())
    n2 = len(member) - n1
    S = (member if n1 <= n2 else 1 - member).astype(np.float64)
    Y = K0 @ S
    a, cross, T = Y[S == 1].sum(), Y[S == 0].sum(), K0.sum()
    m, M = min(n1, n2), max(n1, n2)
    tm = (0.5 * a) * (2 / (m * (m - 1)))
    tM = (0.5 * (T - a - 2 * cross)) * (2 / (M * (M - 1)))
    t3 = cross * (2 / (n1 * n2))
    t1, t2 = (tm, tM) if n1 <= n2 else (tM, tm)
    return t1, t2, t3, t1 + t2 - t3


def null_distribution(latent, i1, i2, sigma, seed, n_perm, pair=0):
    """float64 [n_perm + 1, 4]: the terms and the statistic of splits 0 .. n_perm"""
    pool = latent[np.concatenate([np.asarray(i1), np.asarray(i2)])]
    K = kernel_matrix(pool, sigma)
    return np.array([split_terms(K, membership(len(i1), len(i2), seed, pair, p)) for p in range(n_perm + 1)])


def count(stats):
    """#{p >= 1 : stat_p >= stat_0}"""
    return int((stats[1:] >= stats[0]).sum())


def pvalue(stats):
    return (1 + count(stats)) / len(stats)


def ambiguous(terms):
    """the permuted splits whose statistic lies within the tests' bound of stat_0: none may, for an exact count"""
    return int((np.abs(terms[1:, 3] - terms[0, 3]) <= BOUND * terms[:, :3].sum(axis=1).max()).sum())


def pool_case(n1, n2, z, salt=9800):
    """(latent [n1 + n2 + 7, z], i1, i2): two shifted Gaussians, the index lists interleaved and out of order"""
    n = n1 + n2 + 7
    latent = syn.gauss(n * z, salt + 31 * n1 + n2 + 1000 * z).reshape(n, z)
    order = np.argsort(syn.u01(n, salt + 1), kind='stable')
    i1, i2 = order[:n1].copy(), order[n1:n1 + n2].copy()
    latent[i2] += 0.3
    return np.ascontiguousarray(latent), i1, i2


def value_sigma(z):
    return 0.9 * np.sqrt(z)            # the bandwidth of tests/test_mmd.py's ragged sizes


def pvalue_case(name):
    """(latent [n, 8], i1, i2, sigma) of the three p-value cases: sets of unequal sizes, so no complementary split ties"""
    g = lambda n, salt, shift=0.0: syn.gauss(n * 8, salt).reshape(n, 8) + shift
    x, y = {"AB": (g(70, 9700), g(53, 9701)),
            "AC": (g(70, 9700), g(65, 9702, 0.35)),
            "DE": (g(129, 9703), g(64, 9704, 0.1))}[name]
    latent = np.ascontiguousarray(np.concatenate([x, y]))
    return latent, np.arange(len(x)), len(x) + np.arange(len(y)), value_sigma(8)


PVALUE_CASES = ["AB", "AC", "DE"]
_CACHE = {}


def cached(key, fn):
    """a reference computed once and shared by the tests that need it; callers do not write into it"""
    if key not in _CACHE:
        _CACHE[key] = fn()
        if isinstance(_CACHE[key], np.ndarray):
            _CACHE[key].setflags(write=False)
    return _CACHE[key]


def pvalue_null(name):
    latent, i1, i2, sigma = pvalue_case(name)
    return cached(("pnull", name), lambda: null_distribution(latent, i1, i2, sigma, SEED, N_PERM))
