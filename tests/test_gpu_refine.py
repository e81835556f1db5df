"""The out-of-sample half of ava_amd.projection (TransformableUMAP.transform) and ava_amd.refine_segments on the
MI355X: the query kNN, the bipartite memberships, the start positions and the transform layout against the numpy
restatement (tests/refine_cases.py), reproducibility, an end-to-end transform of held-out blobs, and get_specs /
update_segments / refine_segments_pre_vae against the reference's recorded outputs (tests/golden/refine.npz)."""
import builtins
import json
import os
import pickle
import warnings

import numpy as np
import pytest
import torch

import projection_cases as PC
import refine_cases as RC
from conftest import load_golden
from ava_amd import _lib, projection as P
from ava_amd import refine_segments as R

pytestmark = pytest.mark.gpu


# ---- query kNN -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_knn_query_matches_sklearn_and_restatement(dtype):
    Q, X, k = RC.knn_case(dtype)
    idx, dist = P.knn_query(Q, X, k)
    want_idx, want_dist = RC.knn_query(Q, X, k)
    assert idx.dtype == np.int64 and dist.dtype == np.float64 and idx.shape == dist.shape == (len(Q), k)
    np.testing.assert_array_equal(idx, load_golden("refine.npz")["knn_%s_idx" % np.dtype(dtype).name])
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_allclose(dist, want_dist, rtol=1e-12, atol=0)


@pytest.mark.parametrize("chunk_rows", [None, 1, 7, 100])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_knn_query_copies_ties_and_chunking(chunk_rows, dtype):
    Q, X, src = RC.copies_case(dtype)
    idx, dist = P.knn_query(Q, X, 20, chunk_rows=chunk_rows)
    want_idx, want_dist = RC.knn_query(Q, X, 20)
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_allclose(dist, want_dist, rtol=1e-12, atol=0)
    # a copy of reference row r gets (r, 0.0) first (the lowest index of the equal block), ties go by index
    assert np.all(dist[:len(src), 0] == 0)
    np.testing.assert_array_equal(idx[:len(src), 0], np.where((src >= 40) & (src < 60), 40, src))
    np.testing.assert_array_equal(idx[25], np.arange(40, 60))
    ref_idx, ref_dist = P.knn_query(torch.from_numpy(Q).cuda(), torch.from_numpy(X).cuda(), 20)   # one launch
    np.testing.assert_array_equal(idx, ref_idx)
    np.testing.assert_array_equal(dist, ref_dist)


def test_knn_query_full_k_and_single_query():
    X = PC.gaussian(70, 24, 9970)
    Q = PC.gaussian(66, 24, 9971)
    idx, dist = P.knn_query(Q, X, 64)
    want_idx, want_dist = RC.knn_query(Q, X, 64)
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_allclose(dist, want_dist, rtol=1e-12, atol=0)
    one_idx, one_dist = P.knn_query(Q[5:6], X, 64)
    assert one_idx.shape == (1, 64)
    np.testing.assert_array_equal(one_idx, idx[5:6])
    np.testing.assert_array_equal(one_dist, dist[5:6])


def test_knn_query_long_rows():
    """rows of spectrogram length: 512 column stages"""
    X = PC.gaussian(200, 16384, 9980)
    Q = PC.gaussian(50, 16384, 9981)
    Q[3] = X[150]
    idx, dist = P.knn_query(Q, X, 15)
    want_idx, want_dist = RC.knn_query(Q, X, 15)
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_allclose(dist, want_dist, rtol=1e-12, atol=0)
    assert idx[3, 0] == 150 and dist[3, 0] == 0


def test_knn_query_argument_checks():
    X = PC.gaussian(30, 8, 9990)
    with pytest.raises(ValueError):
        P.knn_query(X[:4], X, 31)                                      # k > n
    with pytest.raises(ValueError):
        P.knn_query(X[:4, :5], X, 3)                                   # other row length
    with pytest.raises(ValueError):
        P.knn_query(X[:4], X, 3, chunk_rows=0)
    lib = _lib.load()
    x = torch.from_numpy(X).cuda()
    idx = torch.empty((4, 3), dtype=torch.int64, device="cuda")
    dist = torch.empty((4, 3), dtype=torch.float64, device="cuda")
    good = [x.data_ptr(), x.data_ptr(), 0, 4, 30, 8, 3, 0, 4, idx.data_ptr(), dist.data_ptr(), _lib.stream()]
    assert lib.ava_pj_knn_query(*good) == 0
    for i, v in {0: None, 1: None, 2: 2, 6: 65, 7: 1, 8: 5, 9: None}.items():    # 7: q0 + nq > m
        args = list(good)
        args[i] = v
        assert lib.ava_pj_knn_query(*args) == -1, i
    torch.cuda.synchronize()


# ---- memberships and start positions -----------------------------------------------------------------------------
def test_bipartite_memberships_and_init():
    idx, dist, E = RC.membership_case()
    for lc in (0.0, 1.0):
        sigma, rho, w = P.smooth_knn_bipartite(idx, dist, lc)
        want_sigma, want_rho, want_w = RC.smooth_knn_bipartite(idx, dist, lc)
        np.testing.assert_allclose(rho, want_rho, rtol=1e-12, atol=0)
        np.testing.assert_allclose(sigma, want_sigma, rtol=1e-12, atol=0)
        np.testing.assert_allclose(w, want_w, rtol=0, atol=1e-12)
    _, _, w = P.smooth_knn_bipartite(idx, dist, 0.0)
    assert np.any(idx == np.arange(len(idx))[:, None]) and np.all(w > 0)        # nothing zeroed for idx == row
    assert np.all(w[25] == 1) and np.all(dist[25] == 0)                          # all k at distance 0
    # the fit's kernel on the same table still zeroes them
    assert np.any(P.smooth_knn(idx, dist, 0.0)[2] == 0)
    wn, Y0 = P.transform_init(idx, w, E)
    want_wn, want_Y0 = RC.normalize_init(idx, w, E)
    np.testing.assert_allclose(wn, want_wn, rtol=0, atol=1e-12)
    np.testing.assert_allclose(Y0, want_Y0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(wn.sum(1), 1.0, rtol=0, atol=1e-14)
    # a row of sum 0 stays 0
    w0 = w.copy()
    w0[7] = 0.0
    wn0, Y00 = P.transform_init(idx, w0, E)
    assert np.all(wn0[7] == 0) and np.all(Y00[7] == 0)
    np.testing.assert_array_equal(np.delete(wn0, 7, 0), np.delete(wn, 7, 0))
    with pytest.raises(ValueError):
        P.transform_init(idx + len(E), w, E)                                     # indices beyond the embedding


# ---- transform layout ------------------------------------------------------------------------------------------------
def _layout_case():
    idx, w, E = RC.layout_case()
    a, b = P.find_ab_params(1.0, 0.1)
    _, Y0 = RC.normalize_init(idx, w, E)
    return idx, w, E, Y0, a, b


def test_transform_layout_epochs_match_restatement():
    """1, 3 and 10 epochs of 12 at 1e-9, 1e-9, 1e-5, the bounds of test_gpu_projection's
    test_layout_epochs_match_restatement.  The tails are fixed here, and the restatement alone moves by less than
    1e-11 over 10 epochs when its start changes in the last bit (tests/test_cpu_refine.py holds it to that), so the
    bounds are upper bounds.  m = 130: three 64-row groups, the last partial."""
    idx, w, E, Y0, a, b = _layout_case()
    eps, epn = RC.schedule(w, 12)
    assert len(idx) == 130
    for epochs, atol in ((1, 1e-9), (3, 1e-9), (10, 1e-5)):
        got, flagged = P.transform_layout(Y0, E, idx, eps, epn, 12, a, b, RC.LAYOUT_SALT, epochs=epochs)
        want = RC.transform_layout(Y0, E, idx, eps, epn, 12, a, b, RC.LAYOUT_SALT, epochs=epochs)
        print("transform layout, %d epochs: max |device - restatement| %.3e" % (epochs, np.abs(got - want).max()))
        assert flagged is False
        assert np.array_equal(want, Y0) == (epochs == 1)
        np.testing.assert_allclose(got, want, rtol=0, atol=atol)
        # a row whose slots are all pruned stays at its start, to the bit
        np.testing.assert_array_equal(got[RC.LAYOUT_PRUNED_ROW], Y0[RC.LAYOUT_PRUNED_ROW])
        again, _ = P.transform_layout(Y0, E, idx, eps, epn, 12, a, b, RC.LAYOUT_SALT, epochs=epochs)
        np.testing.assert_array_equal(again, got)
    # the row that starts on a training point (g = 0 for its only slot) moves by its negative samples alone
    r = RC.LAYOUT_ON_POINT_ROW
    np.testing.assert_array_equal(Y0[r], E[idx[r, 0]])
    assert not np.array_equal(got[r], Y0[r])
    # other parameters
    kw = dict(gamma=2.0, learning_rate=0.5)
    got, _ = P.transform_layout(Y0, E, idx, eps, epn, 12, a, b, RC.LAYOUT_SALT, epochs=3, **kw)
    want = RC.transform_layout(Y0, E, idx, eps, epn, 12, a, b, RC.LAYOUT_SALT, epochs=3, **kw)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-9)


def test_transform_layout_cap():
    idx, w, E, Y0, a, b = _layout_case()
    eps, epn = RC.schedule(w, 12, negative_sample_rate=40)            # a period-1 slot is due 39 samples in epoch 1
    got, flagged = P.transform_layout(Y0, E, idx, eps, epn, 12, a, b, RC.LAYOUT_SALT, epochs=3)
    want, want_flagged = RC.transform_layout(Y0, E, idx, eps, epn, 12, a, b, RC.LAYOUT_SALT, epochs=3, cap=True)
    assert flagged is True and want_flagged is True
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-9)


# ---- end to end --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    X, labels = PC.blobs(n=1800, d=32, c=6, salt=9100)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)                  # six separate blobs: the random init
        model = P.TransformableUMAP().fit(X[:1500])
    return model, X, labels


def test_transform_of_held_out_blobs(fitted):
    """every new point lands among training points of its own blob.  The restatement alone does (checked on the host
    when this test was written: all 300 points, restated fit and restated transform)."""
    model, X, labels = fitted
    Y = model.transform(X[1500:])
    assert Y.shape == (300, 2) and Y.dtype == np.float32 and np.all(np.isfinite(Y))
    np.testing.assert_array_equal(model.transform(X[1500:]), Y)
    np.testing.assert_array_equal(model.transform(torch.from_numpy(X[1500:]).cuda()), Y)
    D = RC.query_distances(Y, model.embedding_)
    nearest = np.argsort(D, axis=1, kind="stable")[:, :5]
    assert np.all(labels[:1500][nearest] == labels[1500:, None])


def test_transform_matches_restatement_on_a_few_rows(fitted):
    """the whole host path (k, local_connectivity - 1, the schedule, the seed) against the restatement: 100 epochs of
    a well-conditioned layout, held to the 10-epoch bound of the kernel test"""
    model, X, _ = fitted
    got = model.transform(X[1500:1540])
    want = RC.transform(X[1500:1540], X[:1500], model.embedding_, 20, model.a_, model.b_)
    np.testing.assert_allclose(got, want.astype(np.float32), rtol=0, atol=1e-5)
    # n_epochs // 3 = 0: the start positions
    model.n_epochs = 2
    try:
        got0 = model.transform(X[1500:1540])
    finally:
        model.n_epochs = None
    want0 = RC.transform(X[1500:1540], X[:1500], model.embedding_, 20, model.a_, model.b_, n_epochs=2)
    np.testing.assert_allclose(got0, want0.astype(np.float32), rtol=0, atol=1e-6)


def test_pickled_model_transforms_the_same(fitted):
    model, X, _ = fitted
    Y = model.transform(X[1500:1600])
    loaded = pickle.loads(pickle.dumps(model))
    assert loaded._train_rows is None and loaded._train_host.shape == (1500, 32)
    np.testing.assert_array_equal(loaded.transform(X[1500:1600]), Y)
    assert loaded._train_host is None and loaded._train_rows.is_cuda   # uploaded again by the first transform


def test_guards(fitted):
    model, X, _ = fitted
    with pytest.raises(ValueError):
        P.TransformableUMAP().transform(X[:10])
    with pytest.raises(ValueError):
        model.transform(X[:0])
    with pytest.raises(ValueError):
        model.transform(X[:10, :20])
    with pytest.raises(NotImplementedError):
        P.UMAP(n_epochs=1).fit(X[:100]).transform(X[:100])
    # fewer training rows than n_neighbors: the truncated k of the fit
    with pytest.warns(UserWarning, match="n_neighbors"):
        small = P.TransformableUMAP(init='random').fit(X[:12])
    Y = small.transform(X[12:20])
    assert Y.shape == (8, 2) and np.all(np.isfinite(Y))


# ---- refine_segments ---------------------------------------------------------------------------------------------------
@pytest.fixture()
def refine_dirs(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    return RC.write_refine_dirs(str(tmp_path))


def _check_specs(g, prefix, got):
    specs, max_len, all_fns, segs = got
    want = g[prefix + "_specs"]
    assert torch.is_tensor(specs) and specs.is_cuda and specs.dtype == torch.float64
    assert tuple(specs.shape) == want.shape and max_len == int(g[prefix + "_max_len"])
    assert all_fns == json.loads(str(g[prefix + "_fns"]))
    np.testing.assert_array_equal(segs, g[prefix + "_segs"])
    host = specs.cpu().numpy()
    np.testing.assert_array_equal(host, host.astype(np.float32).astype(np.float64))      # the reference's float32 values
    err = np.abs(host - want.astype(np.float64)).max()
    assert err <= float(g["spec_tol"]), (prefix, err)
    return host


def test_get_specs_matches_reference(refine_dirs):
    audio_dirs, seg_dirs = refine_dirs
    g = load_golden("refine.npz")
    p = RC.REFINE_P
    whole = _check_specs(g, "all", R.get_specs(audio_dirs, seg_dirs, p, return_segs=True))
    cut = _check_specs(g, "cut", R.get_specs(audio_dirs, seg_dirs, p, max_len=RC.REFINE_MAX_LEN, return_segs=True))
    np.testing.assert_array_equal(cut, whole[:, :, :RC.REFINE_MAX_LEN])
    stop = _check_specs(g, "stop", R.get_specs(audio_dirs, seg_dirs, p, max_num_specs=5, return_segs=True))
    np.testing.assert_array_equal(stop, whole[:5])
    assert len(R.get_specs(audio_dirs, seg_dirs, p)) == 3
    # one slice per batch: the same bits
    one = R.get_specs(audio_dirs, seg_dirs, p, max_chunk_bytes=1)[0]
    np.testing.assert_array_equal(one.cpu().numpy(), whole)
    with pytest.raises(AssertionError, match="Found no spectrograms"):
        R.get_specs([audio_dirs[0]], [seg_dirs[0]], dict(p, nperseg=8192, noverlap=4096))     # no segment is longer
    with pytest.raises(AssertionError):
        R.get_specs(audio_dirs, seg_dirs[:1], p)


def test_update_segments_writes_the_reference_files(refine_dirs):
    audio_dirs, seg_dirs = refine_dirs
    g = load_golden("refine.npz")
    bounds = json.loads(str(g["bounds"]))
    out_dirs = ["out_0", "out_1"]
    for seg_dir, audio_dir, out_dir in zip(seg_dirs, audio_dirs, out_dirs):
        R.update_segments(seg_dir, audio_dir, out_dir, RC.REFINE_P, RC.REFINE_MAX_LEN, RC.StubTransform(), bounds,
                          verbose=False)
    assert RC.read_tree(out_dirs) == json.loads(str(g["files"]))


def _e2e_dirs(root):
    """two directories, three recordings of one second with nine segments each"""
    from scipy.io import wavfile
    audio_dirs, seg_dirs = [], []
    segs = np.stack([0.02 + 0.1 * np.arange(9), 0.09 + 0.1 * np.arange(9)], 1)
    for d, names in enumerate((("c_00", "c_01"), ("d_00",))):
        os.makedirs(os.path.join(root, "audio_%d" % d))
        os.makedirs(os.path.join(root, "segs_%d" % d))
        for name in names:
            wavfile.write(os.path.join(root, "audio_%d" % d, name + ".wav"), RC.REFINE_P['fs'],
                          RC.refine_audio(name, 1.0))
            np.savetxt(os.path.join(root, "segs_%d" % d, name + ".txt"), segs, fmt='%.5f', header="Onsets/offsets")
        audio_dirs.append("audio_%d" % d)
        seg_dirs.append("segs_%d" % d)
    return audio_dirs, seg_dirs, segs


def test_refine_segments_pre_vae_end_to_end(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    audio_dirs, seg_dirs, segs = _e2e_dirs(str(tmp_path))
    p = RC.REFINE_P
    # the embedding the function will compute (the fit is deterministic), to place the box and to know the answer
    specs, max_len, _ = R.get_specs(audio_dirs, seg_dirs, p, max_num_specs=10000)
    assert len(specs) == 27
    transform, emb = R.embed(specs)
    x_cut = float(np.median(emb[:, 0]))
    box = [float(emb[:, 0].min() - 1.0), x_cut, float(emb[:, 1].min() - 1.0), float(emb[:, 1].max() + 1.0)]
    bounds = {'x1': [box[0]], 'x2': [box[1]], 'y1': [box[2]], 'y2': [box[3]]}
    want, kept = {}, 0
    for d, (audio_dir, seg_dir) in enumerate(zip(audio_dirs, seg_dirs)):
        s, _, fns = R.get_specs([audio_dir], [seg_dir], p, max_len=max_len)
        pos = transform.transform(s.reshape(len(s), -1))
        for fn in sorted(set(fns)):
            rows = [segs[i] for i, q in enumerate(pos[[f == fn for f in fns]]) if not R.in_bounds(q, bounds)]
            kept += len(rows)
            if rows:
                want["%d/%s" % (d, fn)] = "# Cleaned onsets/offsets for %s\n" % os.path.join(audio_dir, fn) + \
                    "".join("%.5f %.5f\n" % (a, b) for a, b in rows)
    assert 0 < kept < 27
    answers = iter(['', str(box[1]), str(box[0]), str(box[2]), 'oops', str(box[3]), 'q'])   # x1 > x2: sorted; a retry
    monkeypatch.setattr(builtins, "input", lambda prompt="": next(answers))
    out_dirs = ["out_0", "out_1"]
    with pytest.warns(UserWarning, match="tooltip_plot"):
        R.refine_segments_pre_vae(seg_dirs, audio_dirs, out_dirs, p, img_fn=str(tmp_path / "grid.pdf"))
    assert next(answers, None) is None and os.path.getsize(tmp_path / "grid.pdf") > 0
    out = capsys.readouterr().out
    assert "Running UMAP... n = 27" in out and "Unrecognized input!" in out and "Updating segments in: segs_1" in out
    assert RC.read_tree(out_dirs) == want
    print("kept %d of 27 segments in %d files" % (kept, len(want)))
