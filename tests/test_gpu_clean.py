"""The correlation metric of ava_amd.projection and ava_amd.template_segmentation's ``segment_specs`` /
``clean_collected_segments`` on the MI355X: ``pj_knn_corr_kernel`` against scikit-learn's recorded indices and the
numpy restatement (tests/clean_cases.py, tests/golden/clean.npz), its edges (full lists, one query, long rows, affine
copies, ties, constant rows, chunking, the agreement with ``neighbors.nearest`` at k = 1), ``TransformableUMAP
(metric='correlation')`` from the graph to the pickle, and the spectrograms and rewritten files against the
reference's.

The kernel works in 64-query x 64-reference tiles, 16-column stages and 4-wide k steps; ``clean_cases.KNN_CASES`` says
which edge every case covers."""
import builtins
import json
import os
import pickle
import warnings

import numpy as np
import pytest
import torch

import clean_cases as CC
import projection_cases as PC
import refine_cases as RC
from conftest import load_golden
from ava_amd import _lib, neighbors as N, projection as P
from ava_amd import template_segmentation as TS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_golden("clean.npz")


def _tol(golden, key):
    return json.loads(str(golden["corr_tol"]))[key]


def _report(what, got, want, tol):
    err = float(np.abs(got - want).max())
    print("%s: max |device - restatement| %.3e (tolerance %.3e)" % (what, err, tol))
    return err


# ---- kNN ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", sorted(CC.KNN_CASES))
def test_knn_matches_sklearn_and_restatement(golden, name, dtype):
    key = "%s_%s" % (name, np.dtype(dtype).name)
    Q, X, k = CC.knn_case(name, dtype)
    if Q is None:
        idx, dist = P.knn(X, k, metric='correlation')
        want_idx, want_dist = CC.knn(X, k)
        np.testing.assert_array_equal(idx[:, 0], np.arange(len(X)))
        assert np.all(dist[:, 0] == 0.0)
    else:
        idx, dist = P.knn_query(Q, X, k, metric='correlation')
        want_idx, want_dist = CC.knn_query(Q, X, k)
    assert idx.dtype == np.int64 and dist.dtype == np.float64 and idx.shape == dist.shape == want_idx.shape
    err = _report(key, dist, want_dist, _tol(golden, key))
    np.testing.assert_array_equal(idx, golden["knn_" + key])
    np.testing.assert_array_equal(idx, want_idx)
    assert err <= _tol(golden, key)
    assert np.all(np.isfinite(dist)) and np.all(dist >= 0) and np.all(dist <= 2)


def test_affine_copies_and_ties(golden):
    Q, X, (i, j, a, neg) = CC.affine_case()
    tol = _tol(golden, "affine")
    idx, dist = P.knn_query(Q, X, len(X), metric='correlation')
    want_idx, want_dist = CC.knn_query(Q, X, len(X))
    _report("affine", dist, want_dist, tol)
    assert sorted(idx[0, :3]) == sorted([i, j, a]) and np.all(dist[0, :3] <= tol) and np.all(dist[0, :3] >= 0)
    pos = {int(r): c for c, r in enumerate(idx[0])}
    assert pos[i] < pos[j] and dist[0, pos[i]] == dist[0, pos[j]]                # equal bits: ordered by index
    assert idx[0, -1] == neg and abs(dist[0, -1] - 2.0) <= tol
    np.testing.assert_array_equal(idx[1:], want_idx[1:])
    assert np.abs(dist - want_dist).max() <= tol
    assert dist[0, 3] > 0.1


def test_zero_variance_rows(golden):
    Q, X, (qc, xc) = CC.constant_case()
    k = 20
    idx, dist = P.knn_query(Q, X, k, metric='correlation')
    want_idx, want_dist = CC.knn_query(Q, X, k)
    assert np.all(np.isfinite(dist))
    np.testing.assert_array_equal(idx, want_idx)
    assert np.abs(dist - want_dist).max() <= _tol(golden, "constant")
    assert idx[qc, 0] == xc and dist[qc, 0] == 0.0 and np.all(dist[qc, 1:] == 1.0)
    full_idx, full_dist = P.knn_query(Q, X, len(X), metric='correlation')
    others = np.delete(np.arange(len(Q)), qc)
    at = np.argmax(full_idx[others] == xc, axis=1)
    assert np.all(full_dist[others, at] == 1.0)
    # the self mode on the references with a second constant row
    X2 = X.copy()
    X2[3] = 7.0
    sidx, sdist = P.knn(X2, k, metric='correlation')
    assert np.all(np.isfinite(sdist)) and sidx[3, 1] == xc and sdist[3, 1] == 0.0 and sidx[xc, 1] == 3
    np.testing.assert_array_equal(sidx, CC.knn(X2, k)[0])
    # the kernel that consumes the table has no NaN path: finite weights from both tables
    for fn, table in ((P.smooth_knn_bipartite, (idx, dist)), (P.smooth_knn, (sidx, sdist))):
        sigma, rho, w = fn(*table)
        assert np.all(np.isfinite(sigma)) and np.all(np.isfinite(rho)) and np.all(np.isfinite(w))
        assert np.all(w >= 0) and np.all(w <= 1) and np.all(sigma > 0)


@pytest.mark.parametrize("name", ["a_query", "a_self"])
def test_chunk_rows_invariance(name):
    Q, X, k = CC.knn_case(name)
    tables = []
    for chunk_rows in (None, 1, 64, 100):
        if Q is None:
            tables.append(P.knn(X, k, chunk_rows=chunk_rows, metric='correlation'))
        else:
            tables.append(P.knn_query(Q, X, k, chunk_rows=chunk_rows, metric='correlation'))
    for idx, dist in tables[1:]:
        np.testing.assert_array_equal(idx, tables[0][0])
        np.testing.assert_array_equal(dist.view(np.int64), tables[0][1].view(np.int64))
    # device tensors in, one launch: the same bits
    args = [torch.from_numpy(a).cuda() for a in ((X,) if Q is None else (Q, X))]
    idx, dist = (P.knn if Q is None else P.knn_query)(*args, k, metric='correlation')
    np.testing.assert_array_equal(idx, tables[0][0])
    np.testing.assert_array_equal(dist.view(np.int64), tables[0][1].view(np.int64))


@pytest.mark.parametrize("case", [0, 1])
def test_k1_agrees_with_nearest(case):
    Q, X = CC.k1_cases()[case]
    idx, dist = P.knn_query(Q, X, 1, metric='correlation')
    want_idx, want_dist = N.nearest(Q, X, 'correlation')
    assert not np.any(np.isnan(want_dist))
    np.testing.assert_array_equal(idx[:, 0], want_idx)
    np.testing.assert_array_equal(dist[:, 0].view(np.int64), want_dist.view(np.int64))
    if case == 1:
        assert idx[0, 0] == 3                                    # the lowest index among the exact copies


def test_argument_checks():
    X = PC.gaussian(30, 8, 9990)
    with pytest.raises(ValueError):
        P.knn_query(X[:4], X, 31, metric='correlation')                # k > n
    with pytest.raises(ValueError):
        P.knn_query(X[:4, :5], X, 3, metric='correlation')             # other row length
    with pytest.raises(ValueError):
        P.knn_query(X[:4], X, 3, chunk_rows=0, metric='correlation')
    with pytest.raises(ValueError):
        P.knn(X, 31, metric='correlation')
    with pytest.raises(NotImplementedError):
        P.knn_query(X[:4], X, 3, metric='cosine')
    with pytest.raises(NotImplementedError):
        P.knn(X, 3, metric='manhattan')
    lib = _lib.load()
    x = torch.from_numpy(X).cuda()
    st = torch.empty((30, 2), dtype=torch.float64, device="cuda")
    idx = torch.empty((4, 3), dtype=torch.int64, device="cuda")
    dist = torch.empty((4, 3), dtype=torch.float64, device="cuda")
    good = [x.data_ptr(), 0, 30, 8, st.data_ptr(), _lib.stream()]
    assert lib.ava_pj_row_stats(*good) == 0
    for i, v in {0: None, 1: 2, 2: 0, 3: 0, 4: None}.items():
        args = list(good)
        args[i] = v
        assert lib.ava_pj_row_stats(*args) == -1, i
    assert lib.ava_pj_row_stats(x.data_ptr(), 0, 1, 65537, st.data_ptr(), _lib.stream()) == -1
    good = [x.data_ptr(), x.data_ptr(), 0, st.data_ptr(), st.data_ptr(), 4, 30, 8, 3, 0, 4, idx.data_ptr(),
            dist.data_ptr(), _lib.stream()]
    assert lib.ava_pj_knn_corr_query(*good) == 0
    for i, v in {0: None, 1: None, 2: 2, 3: None, 4: None, 8: 65, 9: 1, 10: 5, 11: None, 12: None}.items():
        args = list(good)                                               # 9: q0 + nq > m
        args[i] = v
        assert lib.ava_pj_knn_corr_query(*args) == -1, i
    good = [x.data_ptr(), 0, st.data_ptr(), 30, 8, 3, 0, 4, idx.data_ptr(), dist.data_ptr(), _lib.stream()]
    assert lib.ava_pj_knn_corr(*good) == 0
    for i, v in [(0, None), (1, 2), (2, None), (5, 31), (5, 65), (6, 27), (7, 0), (8, None), (9, None)]:
        args = list(good)                                               # 5: k > n, k > 64; 6: q0 + nq > n
        args[i] = v
        assert lib.ava_pj_knn_corr(*args) == -1, (i, v)
    torch.cuda.synchronize()


# ---- TransformableUMAP(metric='correlation') ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    X, labels = CC.profile_clusters()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)                  # four separate clusters: the random init
        model = P.TransformableUMAP(metric='correlation').fit(X[:400])
    return model, X, labels


def test_the_clusters_need_the_correlation_metric():
    X, labels = CC.profile_clusters()
    De = PC.distances(X[:400])
    Dc = CC.corr_distances(X[:400], X[:400])
    np.fill_diagonal(De, np.inf)
    np.fill_diagonal(Dc, np.inf)
    assert np.mean(labels[De.argmin(1)] == labels[:400]) < 0.6        # the offsets decide the euclidean neighbours
    assert np.all(labels[Dc.argmin(1)] == labels[:400])


def test_graph_is_built_from_the_restated_table(fitted):
    model, X, _ = fitted
    idx, dist = CC.knn(X[:400], 20)
    sigma, rho, w = PC.smooth_knn(idx, dist)
    want = P.fuzzy_union(idx, w, 400)
    got = model.graph_
    np.testing.assert_array_equal(got.indptr, want.indptr)
    np.testing.assert_array_equal(got.indices, want.indices)
    np.testing.assert_allclose(got.data, want.data, rtol=0, atol=1e-9)
    stats = model._train_stats
    assert stats.is_cuda and tuple(stats.shape) == (400, 2) and stats.dtype == torch.float64
    C, ss = CC.centred(X[:400])
    np.testing.assert_allclose(stats[:, 0].cpu().numpy(), X[:400].astype(np.float64).mean(1), rtol=0, atol=1e-10)
    np.testing.assert_allclose(stats[:, 1].cpu().numpy(), ss, rtol=1e-12)


def test_held_out_rows_land_in_their_cluster(fitted):
    model, X, labels = fitted
    Y = model.transform(X[400:])
    assert Y.shape == (40, 2) and Y.dtype == np.float32 and np.all(np.isfinite(Y))
    E = model.embedding_.astype(np.float64)
    cent = np.stack([E[labels[:400] == c].mean(0) for c in range(4)])
    np.testing.assert_array_equal(RC.query_distances(Y, cent).argmin(1), labels[400:])
    np.testing.assert_array_equal(model.transform(torch.from_numpy(X[400:]).cuda()), Y)


def test_transform_matches_restatement_on_a_few_rows(fitted):
    """the bound of test_gpu_refine's test of the same name, for the same 100 epochs"""
    model, X, _ = fitted
    got = model.transform(X[400:])
    want = CC.transform(X[400:], X[:400], model.embedding_, 20, model.a_, model.b_)
    print("transform: max |device - restatement| %.3e" % np.abs(got - want.astype(np.float32)).max())
    np.testing.assert_allclose(got, want.astype(np.float32), rtol=0, atol=1e-5)


def test_pickled_model_transforms_the_same(fitted):
    model, X, _ = fitted
    Y = model.transform(X[400:])
    loaded = pickle.loads(pickle.dumps(model))
    assert loaded._train_rows is None and loaded._train_stats is None and loaded._train_host.shape == (400, 60)
    np.testing.assert_array_equal(loaded.transform(X[400:]), Y)
    assert loaded._train_host is None and loaded._train_rows.is_cuda and loaded._train_stats.is_cuda
    np.testing.assert_array_equal(loaded._train_stats.cpu().numpy(), model._train_stats.cpu().numpy())


def test_euclidean_metric_is_unchanged():
    X, _ = PC.blobs(n=300, d=16, c=3, salt=9720)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        a = P.TransformableUMAP(n_epochs=30)
        ya = a.fit_transform(X)
        yb = P.UMAP(n_epochs=30).fit_transform(X)
    np.testing.assert_array_equal(ya, yb)
    assert a._train_stats is None and a.metric == 'euclidean'
    with pytest.raises(NotImplementedError):
        P.UMAP(metric='correlation').fit(X)
    with pytest.raises(NotImplementedError):
        P.TransformableUMAP(metric='cosine').fit(X)


# ---- segment_specs ---------------------------------------------------------------------------------------------------
def test_segment_specs_matches_reference(golden, tmp_path):
    _, _, result = CC.write_clean_dirs(str(tmp_path / "run"))
    want = golden["seg_specs"].astype(np.float64)
    specs = TS.segment_specs(result, CC.CLEAN_P)
    assert torch.is_tensor(specs) and specs.is_cuda and specs.dtype == torch.float64
    assert tuple(specs.shape) == want.shape
    host = specs.cpu().numpy()
    np.testing.assert_array_equal(host, host.astype(np.float32).astype(np.float64))      # the reference's float32 values
    err = np.abs(host - want).max()
    print("segment_specs: max |device - reference| %.3e (tolerance %.3e)" % (err, float(golden["spec_tol"])))
    assert err <= float(golden["spec_tol"])
    T = [int(np.ceil(len(a) / 128)) + 1 for a in CC.clean_slices()]
    assert len(set(T)) >= 3 and max(T) == want.shape[2]
    for row, t in zip(host, T):
        assert np.all(row[:, t:] == 0.0) and np.any(row[:, :t] != 0.0)                   # exact zeros behind the last frame
    one = TS.segment_specs(result, CC.CLEAN_P, max_chunk_bytes=1)                        # one slice per batch
    np.testing.assert_array_equal(one.cpu().numpy(), host)
    with pytest.raises(ValueError, match="fewer than nperseg"):
        TS.segment_specs({next(iter(result)): np.array([[0.1, 0.105]])}, CC.CLEAN_P)
    empty = TS.segment_specs({fn: np.zeros((0, 2)) for fn in result}, CC.CLEAN_P)
    assert tuple(empty.shape) == (0, want.shape[1], 0)


# ---- clean_collected_segments ----------------------------------------------------------------------------------------
def test_clean_collected_segments_with_the_stub_transform(golden, tmp_path, monkeypatch):
    """the device spectrograms, the reference's stub UMAP and boxes: the reference's files byte for byte"""
    audio_dirs, seg_dirs, result = CC.write_clean_dirs(str(tmp_path / "run"))
    answers = iter(CC.box_answers(json.loads(str(golden["boxes"]))))
    monkeypatch.setattr(builtins, "input", lambda prompt="": next(answers))
    monkeypatch.setattr(TS, "_new_transform", lambda: CC.StubUMAP(random_state=42, metric='correlation'))
    with pytest.warns(UserWarning, match="tooltip_plot"):
        TS.clean_collected_segments(result, audio_dirs, seg_dirs, CC.CLEAN_P, verbose=False,
                                    img_fn=str(tmp_path / "pic.pdf"))
    assert next(answers, None) is None
    assert RC.read_tree(seg_dirs) == json.loads(str(golden["files"]))


def test_clean_collected_segments_end_to_end(tmp_path, monkeypatch, capsys):
    """motif renditions and cage-noise bursts, the real device fit and transform: every motif segment is kept and every
    noise segment dropped"""
    dirs, labels = CC.e2e_dirs()
    audio_dirs, seg_dirs, result = CC.write_clean_dirs(str(tmp_path / "run"), dirs, CC.e2e_audio)
    p = CC.CLEAN_P
    # the embedding the function will compute (the fit is deterministic), to place the box
    specs = TS.segment_specs(result, p)
    assert len(specs) == len(labels) == 30
    perm = np.random.RandomState(42).permutation(30)                  # the function fits the rows in this order
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        emb = TS._new_transform().fit_transform(specs.reshape(len(specs), -1)[torch.from_numpy(perm).cuda()])
    motif = labels[perm]
    margin = 2.0
    lo, hi = emb[motif].min(0) - margin, emb[motif].max(0) + margin
    outside = np.any((emb[~motif] < lo - margin) | (emb[~motif] > hi + margin), axis=1)
    print("motif box", lo, hi, "noise", emb[~motif].min(0), emb[~motif].max(0))
    assert np.all(outside)                                            # the groups are further apart than the margin
    answers = iter(CC.box_answers([(hi[0], lo[0], lo[1], hi[1])]))    # x1 > x2
    monkeypatch.setattr(builtins, "input", lambda prompt="": next(answers))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        TS.clean_collected_segments(result, audio_dirs, seg_dirs, p, img_fn=str(tmp_path / "pic.pdf"))
    assert next(answers, None) is None and os.path.getsize(tmp_path / "pic.pdf") > 0
    out = capsys.readouterr().out
    assert "Running UMAP. n = 30" in out and "Selected 0 out of 30" in out and "\tdeleted: 15 remaining: 15" in out
    want = {}
    for d, files in enumerate(dirs):
        for name, _, segs in files:
            want["%d/%s.txt" % (d, name)] = "".join("%.5f %.5f\n" % s for s in segs[0::2])
    assert RC.read_tree(seg_dirs) == want
