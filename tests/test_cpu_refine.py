"""The out-of-sample half of ava_amd.projection and ava_amd.refine_segments without a GPU: the numpy restatements
(tests/refine_cases.py) against scikit-learn and their own invariants, argument validation, pickling, install(), and the
file logic of update_segments against the reference's recorded files (tests/golden/refine.npz)."""
import json
import pickle
import types

import numpy as np
import pytest
import torch

import projection_cases as PC
import refine_cases as RC
from conftest import load_golden
from ava_amd import projection as P
from ava_amd import refine_segments as R


def test_restated_knn_query_matches_sklearn():
    from sklearn.neighbors import NearestNeighbors
    Q, X, k = RC.knn_case()
    idx, dist = RC.knn_query(Q, X, k)
    want_dist, want_idx = NearestNeighbors(n_neighbors=k, algorithm='brute').fit(X.astype(np.float64)).kneighbors(
        Q.astype(np.float64))
    assert np.all(np.diff(dist, axis=1) > 0)                          # tie-free: the order is unambiguous
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_allclose(dist, want_dist, rtol=1e-9, atol=0)


def test_restated_knn_query_copies_and_ties():
    Q, X, src = RC.copies_case()
    idx, dist = RC.knn_query(Q, X, 20)
    for q, r in enumerate(src):
        if 40 <= r < 60:                                              # the equal block: all 20 at 0, by index
            np.testing.assert_array_equal(idx[q], np.arange(40, 60))
            assert np.all(dist[q] == 0)
        else:
            assert idx[q, 0] == r and dist[q, 0] == 0 and dist[q, 1] > 0
    assert np.all(dist[len(src):, 0] > 0)


def test_restated_memberships_and_normalisation():
    idx, dist, E = RC.membership_case()
    sigma, rho, w = RC.smooth_knn_bipartite(idx, dist, 0.0)
    assert np.all(rho == 0) and np.all(sigma > 0) and np.all((w > 0) & (w <= 1))
    assert np.all(w[dist == 0] == 1)                                  # kept although idx may equal the row number
    assert np.any(idx == np.arange(len(idx))[:, None])
    wn, Y0 = RC.normalize_init(idx, w, E)
    np.testing.assert_allclose(wn.sum(1), 1.0, rtol=0, atol=1e-14)
    lo, hi = E[idx].min(1), E[idx].max(1)
    assert np.all(Y0 >= lo - 1e-12) and np.all(Y0 <= hi + 1e-12)      # a convex combination of the neighbours
    wn0, Y00 = RC.normalize_init(idx[:2], np.zeros((2, 20)), E)
    assert np.all(wn0 == 0) and np.all(Y00 == 0)


def test_restated_schedule_matches_host():
    idx, w, _ = RC.layout_case()
    eps, epn = RC.schedule(w, 12)
    got_eps, got_epn = P.transform_schedule(w, 12)
    np.testing.assert_array_equal(got_eps, eps)
    np.testing.assert_array_equal(got_epn, epn)
    assert np.all(eps[RC.LAYOUT_PRUNED_ROW] == -1) and eps[RC.LAYOUT_ON_POINT_ROW, 0] == 1.0
    assert np.all(eps[RC.LAYOUT_ON_POINT_ROW, 1:] == -1) and np.all(eps[eps > 0] >= 1.0)


def test_restated_transform_layout_edges_and_conditioning():
    """the bounds of the GPU test (1e-9, 1e-9, 1e-5) measure the kernel: the restatement alone moves by less than 1e-11
    when its start changes in the last bit (3e-13 at 3 epochs when this was written)"""
    idx, w, E = RC.layout_case()
    a, b = PC.find_ab_params()
    eps, epn = RC.schedule(w, 12)
    _, Y0 = RC.normalize_init(idx, w, E)
    np.testing.assert_array_equal(Y0[RC.LAYOUT_ON_POINT_ROW], E[idx[RC.LAYOUT_ON_POINT_ROW, 0]])
    for epochs in (1, 3, 10):
        y = RC.transform_layout(Y0, E, idx, eps, epn, 12, a, b, RC.LAYOUT_SALT, epochs=epochs)
        y2 = RC.transform_layout(Y0 * (1 + 2.0 ** -52), E, idx, eps, epn, 12, a, b, RC.LAYOUT_SALT, epochs=epochs)
        assert np.all(np.isfinite(y)) and np.abs(y - y2).max() < 1e-11
        np.testing.assert_array_equal(y[RC.LAYOUT_PRUNED_ROW], Y0[RC.LAYOUT_PRUNED_ROW])
        assert np.array_equal(y, Y0) == (epochs == 1)                 # epoch 0 samples nothing, as in the fit
    # rate 5 never trips the cap; rate 40 does (a period-1 slot is due 39 samples in epoch 1)
    y, flagged = RC.transform_layout(Y0, E, idx, eps, epn, 12, a, b, RC.LAYOUT_SALT, epochs=3, cap=True)
    assert flagged is False
    np.testing.assert_array_equal(y, RC.transform_layout(Y0, E, idx, eps, epn, 12, a, b, RC.LAYOUT_SALT, epochs=3))
    eps40, epn40 = RC.schedule(w, 12, negative_sample_rate=40)
    with pytest.raises(AssertionError):
        RC.transform_layout(Y0, E, idx, eps40, epn40, 12, a, b, RC.LAYOUT_SALT, epochs=3)
    y, flagged = RC.transform_layout(Y0, E, idx, eps40, epn40, 12, a, b, RC.LAYOUT_SALT, epochs=3, cap=True)
    assert flagged is True and np.all(np.isfinite(y))


def test_transformable_umap_arguments():
    t = P.TransformableUMAP()
    assert isinstance(t, P.UMAP) and t.transform_seed == 42 and t.n_neighbors == 20
    assert P.TransformableUMAP(transform_seed=7, n_neighbors=15).transform_seed == 7
    with pytest.raises(ValueError, match="fit"):
        t.transform(np.zeros((3, 4), dtype=np.float32))
    with pytest.raises(NotImplementedError):
        P.UMAP().transform(np.zeros((3, 4)))                           # the base class keeps no training rows
    with pytest.raises(ValueError):
        P.TransformableUMAP(n_neighbors=1).fit(np.zeros((10, 3), dtype=np.float32))
    # a fitted object (its state injected) checks the batch before any device work
    t._train_host = np.zeros((30, 4), dtype=np.float32)
    with pytest.raises(ValueError, match="at least one row"):
        t.transform(np.zeros((0, 4), dtype=np.float32))
    with pytest.raises(ValueError, match="columns"):
        t.transform(np.zeros((3, 5), dtype=np.float32))


def test_pickle_drops_the_device_rows_and_keeps_a_host_copy():
    t = P.TransformableUMAP(transform_seed=5)
    rows = torch.arange(12, dtype=torch.float32).reshape(4, 3)         # stands in for the device tensor
    t._train_rows = rows
    t.embedding_ = np.ones((4, 2), dtype=np.float32)
    t.a_, t.b_, t._n_neighbors = 1.5, 0.9, 3
    state = t.__getstate__()
    assert state['_train_rows'] is None and not any(torch.is_tensor(v) for v in state.values())
    u = pickle.loads(pickle.dumps(t))
    assert isinstance(u, P.TransformableUMAP) and u._train_rows is None and u.transform_seed == 5
    np.testing.assert_array_equal(u._train_host, rows.numpy())
    np.testing.assert_array_equal(u.embedding_, t.embedding_)
    assert (u.a_, u.b_, u._n_neighbors) == (1.5, 0.9, 3)
    assert t._train_rows is rows                                       # pickling leaves the object as it was
    v = pickle.loads(pickle.dumps(u))                                  # a loaded object pickles again
    np.testing.assert_array_equal(v._train_host, rows.numpy())
    # never fitted: nothing to drop
    w = pickle.loads(pickle.dumps(P.TransformableUMAP()))
    assert w._train_rows is None and w._train_host is None


def test_install_on_stub_module():
    module = types.SimpleNamespace(_get_specs=None, _update_segs_helper=None, refine_segments_pre_vae=None)
    assert R.install(module) is module
    assert module._get_specs is R.get_specs and module._update_segs_helper is R.update_segments
    assert module.refine_segments_pre_vae is R.refine_segments_pre_vae


def test_in_bounds_is_strict():
    bounds = {'x1': [0.0, 5.0], 'x2': [1.0, 6.0], 'y1': [0.0, 5.0], 'y2': [2.0, 6.0]}
    assert R.in_bounds((0.5, 1.0), bounds) and R.in_bounds((5.5, 5.5), bounds)
    assert not R.in_bounds((1.0, 1.0), bounds) and not R.in_bounds((0.5, 0.0), bounds)
    assert not R.in_bounds((3.0, 3.0), bounds)
    assert not R.in_bounds((0.5, 1.0), {'x1': [], 'x2': [], 'y1': [], 'y2': []})


def test_golden_holds_the_cases_the_issue_names():
    g = load_golden("refine.npz")
    all_fns = json.loads(str(g["all_fns"]))
    lines = {name + ".txt": len(segs) for files in RC.REFINE_DIRS for name, _, segs in files}
    assert len(RC.REFINE_DIRS) == 2 and 10 <= sum(lines.values()) <= 14
    assert "a_01.txt" not in all_fns and lines["a_01.txt"] == 0                      # a file with no segments
    assert all_fns.count("a_00.txt") == lines["a_00.txt"] - 1                        # one segment <= nperseg samples
    assert int(g["all_max_len"]) > RC.REFINE_MAX_LEN == int(g["cut_max_len"])        # one truncated by max_len
    stop_fns = json.loads(str(g["stop_fns"]))
    assert len(stop_fns) == 5 and stop_fns == all_fns[:5] and all_fns[5] == stop_fns[-1]   # stops inside a file
    np.testing.assert_array_equal(g["cut_specs"], g["all_specs"][:, :, :RC.REFINE_MAX_LEN])
    dt = (g["all_segs"][:, 1] - g["all_segs"][:, 0]) / int(g["all_max_len"])
    np.testing.assert_allclose(dt, (RC.REFINE_P['nperseg'] - RC.REFINE_P['noverlap']) / RC.REFINE_P['fs'], rtol=1e-12)


def test_update_segments_file_logic_matches_reference(tmp_path, monkeypatch):
    """the spectrograms injected (the golden's, per directory, as get_specs would return them): the files written are
    the reference's byte for byte, the copied line shifted by the skipped short segment included"""
    g = load_golden("refine.npz")
    fns = json.loads(str(g["cut_fns"]))
    specs = g["cut_specs"].astype(np.float64)
    bounds = json.loads(str(g["bounds"]))
    monkeypatch.chdir(tmp_path)
    audio_dirs, seg_dirs = RC.write_refine_dirs(str(tmp_path))
    calls = []

    def fake_get_specs(a_dirs, s_dirs, p, max_len=None):
        calls.append((a_dirs, s_dirs, max_len))
        prefix = "a_" if s_dirs == [seg_dirs[0]] else "b_"
        keep = [i for i, fn in enumerate(fns) if fn.startswith(prefix)]
        return torch.from_numpy(specs[keep]), max_len, [fns[i] for i in keep]
    monkeypatch.setattr(R, "get_specs", fake_get_specs)
    out_dirs = ["out_0", "out_1"]
    for seg_dir, audio_dir, out_dir in zip(seg_dirs, audio_dirs, out_dirs):
        R.update_segments(seg_dir, audio_dir, out_dir, RC.REFINE_P, RC.REFINE_MAX_LEN, RC.StubTransform(), bounds,
                          verbose=False)
    assert calls == [([a], [s], RC.REFINE_MAX_LEN) for a, s in zip(audio_dirs, seg_dirs)]
    want = json.loads(str(g["files"]))
    assert RC.read_tree(out_dirs) == want
    assert "0.18000 0.18500" in want["1/b_01.txt"]          # the line of the skipped segment, copied for the next one
