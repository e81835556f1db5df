"""The kernels of csrc/tsne.hip and ava_amd.tsne.TSNE on the MI355X: each step against the numpy restatement of
tests/tsne_cases.py (and, for the golden cases, against scikit-learn's own values in tests/golden/tsne.npz) at tile
tails, one tile and several tiles, one and several column chunks; whole runs statistically.  tests/test_cpu_tsne.py
shows that the restatement is sklearn's arithmetic and that the cases are away from the two discontinuous rules."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import tsne_cases as TC
from conftest import ROOT, load_golden
from ava_amd import _lib
from ava_amd import mmd
from ava_amd import tsne as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_golden("tsne.npz")


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _device_p(name):
    """the device's P of a case (a fresh matrix: joint_probabilities overwrites its input)"""
    X, perplexity = TC.p_case(name)[:2]
    return T.joint_probabilities(T.squared_distances(_up(X)), perplexity)


# ---- squared distances -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TC.P_CASES))
def test_squared_distances_euclidean(name):
    X, _, raw, D2, _ = TC.p_case(name)
    n = len(X)
    got_raw = T.squared_distances(_up(X), round_float32=False)
    assert got_raw.stride(0) % 2 == 0 and got_raw.data_ptr() % 16 == 0
    # the bits of ava_pair_sqdist on the same rows, every ordered pair
    L = _up(X.astype(np.float64))
    a, b = (_up(v) for v in np.divmod(np.arange(n * n, dtype=np.int64), n))
    out = torch.empty(n * n, dtype=torch.float64, device="cuda")
    _lib.check(_lib.load().ava_pair_sqdist(L.data_ptr(), X.shape[1], a.data_ptr(), b.data_ptr(), n * n,
                                           out.data_ptr(), _lib.stream()), "ava_pair_sqdist")
    np.testing.assert_array_equal(got_raw.cpu().numpy(), out.cpu().numpy().reshape(n, n))
    np.testing.assert_array_equal(got_raw.cpu().numpy(), raw)
    got = T.squared_distances(_up(X)).cpu().numpy()
    np.testing.assert_array_equal(got, D2)
    np.testing.assert_array_equal(got, got.astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("n", [5, 40, 65, 130])
def test_squared_distances_precomputed(n):
    D = np.abs(TC.syn.gauss(n * n, 9730 + n)).reshape(n, n) * 3.0
    want = (D * D).astype(np.float32).astype(np.float64)
    np.testing.assert_array_equal(T.squared_distances(D, 'precomputed').cpu().numpy(), want)
    np.testing.assert_array_equal(T.squared_distances(_up(D), 'precomputed').cpu().numpy(), want)
    with pytest.raises(NotImplementedError):
        T.squared_distances(D, 'cosine')


# ---- probabilities ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TC.P_CASES))
def test_joint_probabilities(golden, name):
    P = TC.p_case(name)[4]
    got = _device_p(name).cpu().numpy()
    err = np.abs(got - P).max() / P.max()
    print("P %s: max err / max P %.3g" % (name, err))
    np.testing.assert_allclose(got, P, rtol=0, atol=1e-12 * P.max())
    np.testing.assert_array_equal(got, got.T)
    assert np.all(np.diag(got) == 0.0) and got[~np.eye(len(got), dtype=bool)].min() >= TC.MACHINE_EPSILON
    if name in TC.GOLDEN_P_CASES:
        want = golden["P_" + name]
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * want.max())


def test_joint_probabilities_copies_what_the_kernels_cannot_read():
    """an odd row stride goes through a padded copy; the values are those of the padded path"""
    _, perplexity, _, D2, P = TC.p_case("n65")
    got = T.joint_probabilities(_up(D2), perplexity).cpu().numpy()           # contiguous [65, 65]: stride 65
    np.testing.assert_array_equal(got, _device_p("n65").cpu().numpy())
    with pytest.raises(ValueError):
        T.joint_probabilities(_up(D2), 65.0)


# ---- gradient ----------------------------------------------------------------------------------------------------------
GRAD_PARAMS = [pytest.param(name, chunks, id="%s-c%s" % (name, chunks))
               for name in TC.DESCENT_CASES for chunks in TC.DESCENT_CHUNKS[name]]


@pytest.mark.parametrize("exaggeration", [1.0, 12.0])
@pytest.mark.parametrize("state", TC.DESCENT_STATES + ("clamp",))
@pytest.mark.parametrize("name, chunks", GRAD_PARAMS)
def test_kl_gradient(name, chunks, state, exaggeration):
    P = TC.p_case(name)[4]
    n = len(P)
    Y = TC.clamp_y(n) if state == "clamp" else TC.descent_start(name, state)
    want_kl, want = TC.kl_gradient(Y, P, exaggeration)
    kl, grad = T.kl_gradient(_up(Y), _up(P), exaggeration, col_chunks=chunks)
    grad = grad.cpu().numpy()
    print("kl_gradient %s: kl rel %.3g, grad err / max %.3g"
          % (name, abs(kl - want_kl) / abs(want_kl), np.abs(grad - want).max() / np.abs(want).max()))
    np.testing.assert_allclose(kl, want_kl, rtol=1e-11)
    np.testing.assert_allclose(grad, want, rtol=0, atol=1e-11 * np.abs(want).max())


def test_kl_gradient_against_sklearn(golden):
    for name in ("n130", "n300"):
        n = len(golden["Y_" + name])
        want = golden["grad_" + name]
        for chunks in (None, 3):
            kl, grad = T.kl_gradient(_up(golden["Y_" + name]), _up(golden["P_" + name]), col_chunks=chunks)
            np.testing.assert_allclose(kl, golden["kl_" + name], rtol=1e-11)
            np.testing.assert_allclose(grad.cpu().numpy(), want, rtol=0, atol=1e-11 * np.abs(want).max())
        assert grad.shape == (n, 2)


# ---- descent -----------------------------------------------------------------------------------------------------------
def _descend_device(name, state, momentum, exaggeration, n_iters, chunks):
    P = TC.p_case(name)[4]
    n = len(P)
    Y = _up(TC.descent_start(name, state))
    update = torch.zeros_like(Y)
    gains = torch.ones_like(Y)
    kl, grad_norm = T.descend(Y, update, gains, _up(P), n_iters, momentum, TC.descent_lr(n), exaggeration,
                              col_chunks=chunks)
    return Y.cpu().numpy(), update.cpu().numpy(), gains.cpu().numpy(), kl, grad_norm


@pytest.mark.parametrize("n_iters", [1, 5])
@pytest.mark.parametrize("momentum, exaggeration", [(0.5, 12.0), (0.8, 1.0)])
@pytest.mark.parametrize("state", TC.DESCENT_STATES)
@pytest.mark.parametrize("name, chunks", GRAD_PARAMS)
def test_descend(name, chunks, state, momentum, exaggeration, n_iters):
    want = TC.descent_reference(name, state, momentum, exaggeration, n_iters)
    got = _descend_device(name, state, momentum, exaggeration, n_iters, chunks)
    span = float(np.ptp(want[0], axis=0).max())
    for what, g, w in zip(("Y", "update", "gains"), got[:3], want[:3]):
        print("descend %s %s: err / span %.3g" % (name, what, np.abs(g - w).max() / span))
        np.testing.assert_allclose(g, w, rtol=0, atol=1e-9 * span)
    np.testing.assert_allclose(got[3], want[3], rtol=1e-9)
    np.testing.assert_allclose(got[4], want[4], rtol=1e-9)


def test_descend_reports_the_last_kl_only():
    P = _up(TC.p_case("n130")[4])
    Y = _up(TC.spread_y(130))
    ws, nbytes = T._workspace(130, 3, P.device)
    stats = T._descend(Y, torch.zeros_like(Y), torch.ones_like(Y), P, 4, 0.8, 50.0, 1.0, 3, ws, nbytes).cpu().numpy()
    assert np.all(np.isnan(stats[:3, 0])) and np.isfinite(stats[3, 0]) and np.all(np.isfinite(stats[:, 1]))


def test_descend_is_deterministic():
    for chunks in (1, 3):
        a = _descend_device("n300", "spread", 0.8, 1.0, 5, chunks)
        b = _descend_device("n300", "spread", 0.8, 1.0, 5, chunks)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)


def test_descend_checks_its_tensors():
    P = _up(TC.p_case("n5")[4])
    Y = _up(TC.spread_y(5))
    with pytest.raises(ValueError):
        T.descend(Y, torch.zeros_like(Y), torch.ones((5, 2), device="cuda"), P, 1, 0.5, 50.0, 1.0)      # float32 gains
    with pytest.raises(ValueError):
        T.descend(Y, torch.zeros_like(Y), torch.ones_like(Y), P, 0, 0.5, 50.0, 1.0)
    with pytest.raises(ValueError):
        T.kl_gradient(Y, P, col_chunks=65)


# ---- whole runs --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def whole_runs():
    """name -> (TSNE after fit_transform with random_state=42, the embedding); fitted once for the tests below"""
    out = {}
    for name in TC.RUN_CASES:
        metric, X, labels, perplexity, _, _ = TC.run_case(name)
        t = T.TSNE(n_components=2, random_state=TC.RUN_SEED, metric=metric, method='exact', perplexity=perplexity)
        out[name] = (t, t.fit_transform(np.array(X)))
    return out


@pytest.mark.parametrize("name", sorted(TC.RUN_CASES))
def test_whole_run(golden, whole_runs, name):
    metric, X, labels, perplexity, _, _ = TC.run_case(name)
    t, emb = whole_runs[name]
    n = len(labels)
    assert emb.dtype == np.float32 and emb.shape == (n, 2) and np.all(np.isfinite(emb)) and emb is t.embedding_
    assert t.n_iter_ == 999
    assert t.learning_rate_ == max(n / 12.0 / 4.0, 50.0)
    P = T.joint_probabilities(T.squared_distances(np.array(X), metric), perplexity).cpu().numpy()
    kl = TC.kl_gradient(emb.astype(np.float64), P)[0]
    bound = 1.25 * max(golden["restatement_kl_" + name].max(), float(golden["sklearn_kl_" + name]))
    frac = TC.neighbour_label_fraction(emb, labels)
    print("whole run %s: kl %.5f (restatement at the embedding %.5f, bound %.5f), neighbour fraction %.3f"
          % (name, t.kl_divergence_, kl, bound, frac))
    np.testing.assert_allclose(t.kl_divergence_, kl, rtol=1e-5)
    assert t.kl_divergence_ <= bound
    assert frac >= 0.95


def test_fit_transform_is_deterministic(whole_runs):
    for name in TC.RUN_CASES:
        metric, X, _, perplexity, _, _ = TC.run_case(name)
        t = T.TSNE(random_state=TC.RUN_SEED, metric=metric, perplexity=perplexity)
        np.testing.assert_array_equal(t.fit_transform(np.array(X)), whole_runs[name][1])
        assert t.kl_divergence_ == whole_runs[name][0].kl_divergence_


def test_early_stop_on_the_device():
    metric, X, _, perplexity, _, _ = TC.run_case("precomputed40")
    t = T.TSNE(random_state=TC.RUN_SEED, metric=metric, perplexity=perplexity, min_grad_norm=np.inf).fit(np.array(X))
    assert t.n_iter_ == 99 and np.all(np.isfinite(t.embedding_))


def test_array_init_and_learning_rate():
    metric, X, _, perplexity, _, _ = TC.run_case("precomputed40")
    Y0 = TC.random_init(40, 3)
    t = T.TSNE(metric=metric, perplexity=perplexity, init=Y0, learning_rate=80.0, max_iter=300).fit(np.array(X))
    assert t.n_iter_ == 299 and t.learning_rate_ == 80.0 and np.isfinite(t.kl_divergence_) and t.kl_divergence_ > 0.0
    again = T.TSNE(metric=metric, perplexity=perplexity, init=_up(Y0), learning_rate=80.0, max_iter=300).fit(_up(X))
    np.testing.assert_array_equal(again.embedding_, t.embedding_)                 # tensors in, the same bits out


# ---- the reference's caller ----------------------------------------------------------------------------------------------
UPSTREAM = {
    "ava/__init__.py": '__version__ = "0.3.1"\n',
    "ava/plotting/__init__.py": "",
    # the constructor call of mmd_tsne_plot_DC (mmd_plots.py:225-227) on sklearn's TSNE, as the reference imports it
    "ava/plotting/mmd_plots.py": textwrap.dedent("""\
        import numpy as np
        from sklearn.manifold import TSNE


        def layout(mmd2, perplexity=30.0):
            mmd2 = np.clip(mmd2, 0, None)
            transform = TSNE(n_components=2, random_state=42, metric='precomputed', \\
                    method='exact', perplexity=perplexity)
            embed = transform.fit_transform(mmd2)
            return embed
        """),
}


def test_the_references_caller(tmp_path):
    ref = tmp_path / "reference"
    for rel, src in UPSTREAM.items():
        path = ref / rel
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(src)
    code = textwrap.dedent("""\
        import numpy as np
        import ava.plotting.mmd_plots as mp
        from ava_amd import mmd, synthetic as syn
        from ava_amd.tsne import TSNE
        x = syn.gauss(40 * 5, 9770).reshape(40, 5)
        mmd2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(2) * 0.01
        mmd2[3, 7] = mmd2[7, 3] = -1e-4                      # an unbiased estimate may dip below zero: clipped
        try:
            mp.layout(mmd2, perplexity=10.0)
            raise SystemExit("sklearn's TSNE accepted the call")
        except ValueError as e:
            print("sklearn:", e)
        assert mmd.install(tsne=True) is mp and mp.TSNE is TSNE
        embed = mp.layout(mmd2, perplexity=10.0)
        assert embed.shape == (40, 2) and embed.dtype == np.float32 and np.all(np.isfinite(embed))
        print("ok", float(np.ptp(embed)))
        """)
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, str(ref)])
    res = subprocess.run([sys.executable, "-c", code], env=env, cwd=str(tmp_path), capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "ok" in res.stdout and 'init="pca"' in res.stdout
