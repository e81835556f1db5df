"""The host side of the correlation metric of ava_amd.projection and of ava_amd.template_segmentation's
``clean_collected_segments``, without a GPU: the restated correlation kNN of tests/clean_cases.py against scikit-learn's
recorded indices (tests/golden/clean.npz), the zero-variance convention, ``_in_region``, ``install``, the metric
validation of both UMAP classes, the pickle of a ``TransformableUMAP`` and the file-rewriting logic of
``clean_collected_segments`` against the files the reference wrote, with the device stages replaced by the fixture's
spectrograms and the stub transform."""
import builtins
import json
import pickle
import types

import numpy as np
import pytest
import torch

import clean_cases as CC
import refine_cases as RC
from conftest import load_golden
from ava_amd import projection as P
from ava_amd import refine_segments as R
from ava_amd import template_segmentation as TS


@pytest.fixture(scope="module")
def golden():
    return load_golden("clean.npz")


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", sorted(CC.KNN_CASES))
def test_restated_knn_equals_sklearn(golden, name, dtype):
    Q, X, k = CC.knn_case(name, dtype)
    idx, dist = CC.knn(X, k) if Q is None else CC.knn_query(Q, X, k)
    np.testing.assert_array_equal(idx, golden["knn_%s_%s" % (name, np.dtype(dtype).name)])
    assert idx.shape == dist.shape == ((len(X) if Q is None else len(Q)), k)
    assert np.all(np.diff(dist, axis=1) > 0) and np.all(dist >= 0) and np.all(dist <= 2)
    tol = json.loads(str(golden["corr_tol"]))["%s_%s" % (name, np.dtype(dtype).name)]
    assert 16 * X.shape[1] * 2.0 ** -53 <= tol < 1e-10           # far below the 1e-9 gaps the indices rest on


def test_zero_variance_convention():
    Q, X, (qc, xc) = CC.constant_case()
    D = CC.corr_distances(Q, X)
    assert np.all(np.isfinite(D))
    assert D[qc, xc] == 0.0
    assert np.all(np.delete(D[qc], xc) == 1.0) and np.all(np.delete(D[:, xc], qc) == 1.0)
    rest = np.delete(np.delete(D, qc, 0), xc, 1)
    assert np.all((rest > 0) & (rest < 2))
    idx, dist = CC.knn_query(Q, X, 5)
    assert idx[qc, 0] == xc and dist[qc, 0] == 0.0 and np.all(dist[qc, 1:] == 1.0)
    np.testing.assert_array_equal(idx[qc, 1:], np.arange(4))     # ties by index


def test_affine_copies_in_the_restatement(golden):
    Q, X, (i, j, a, neg) = CC.affine_case()
    tol = json.loads(str(golden["corr_tol"]))["affine"]
    D = CC.corr_distances(Q, X)
    assert np.all(D[0, [i, j, a]] <= tol) and abs(D[0, neg] - 2.0) <= tol
    assert D[0, i] == D[0, j]
    assert np.delete(D[0], [i, j, a]).min() > 0.1


# ---- _in_region, install, validation, pickle -----------------------------------------------------------------------------
def test_in_region_is_strict_and_order_free():
    bounds = {'x1s': [2.0, 10.0], 'x2s': [1.0, 11.0], 'y1s': [0.0, 6.0], 'y2s': [-1.0, 5.0]}    # both pairs swapped
    assert TS._in_region((1.5, -0.5), bounds) and TS._in_region((10.5, 5.5), bounds)
    for pt in [(1.0, -0.5), (2.0, -0.5), (1.5, 0.0), (1.5, -1.0), (3.0, -0.5), (1.5, 5.5), (10.5, -0.5)]:
        assert not TS._in_region(pt, bounds), pt
    assert not TS._in_region((0.0, 0.0), {'x1s': [], 'x2s': [], 'y1s': [], 'y2s': []})
    assert "_in_region" in TS.__all__


def test_install_on_a_stub_module():
    mod = types.SimpleNamespace(get_template=None, segment_files=None, _segment_file=None,
                                clean_collected_segments=None, clean_collected_data=None, _get_spec="kept")
    assert TS.install(mod) is mod
    assert mod.get_template is TS.get_template and mod.segment_files is TS.segment_files
    assert mod._segment_file is TS._segment_file
    assert mod.clean_collected_segments is TS.clean_collected_segments
    assert mod.clean_collected_data is TS.clean_collected_data
    assert mod.segment_specs is TS.segment_specs and mod._get_spec == "kept"


def test_metric_validation():
    P.TransformableUMAP(metric='correlation')._validate()
    P.TransformableUMAP()._validate()
    P.UMAP()._validate()
    assert P.UMAP.METRICS == ('euclidean',) and P.TransformableUMAP.METRICS == ('euclidean', 'correlation')
    for model in (P.UMAP(metric='correlation'), P.UMAP(metric='cosine'), P.TransformableUMAP(metric='cosine'),
                  P.TransformableUMAP(metric='manhattan')):
        with pytest.raises(NotImplementedError):
            model._validate()
    X = np.zeros((4, 3), dtype=np.float32)
    with pytest.raises(NotImplementedError):                     # before anything touches the device
        P.knn(X, 2, metric='cosine')
    with pytest.raises(NotImplementedError):
        P.knn_query(X, X, 2, metric='cosine')
    t = TS._new_transform()
    assert isinstance(t, P.TransformableUMAP) and t.metric == 'correlation' and t.random_state == 42
    assert t.n_neighbors == 15 and t.min_dist == 0.1             # umap-learn's defaults
    t._validate()


def test_pickle_drops_the_statistics():
    model = P.TransformableUMAP(metric='correlation')
    rows = torch.arange(12, dtype=torch.float32).reshape(4, 3)
    model._train_rows = rows                                      # injected state: host tensors stand in
    model._train_stats = torch.ones((4, 2), dtype=torch.float64)
    model.embedding_ = np.zeros((4, 2), dtype=np.float32)
    state = model.__getstate__()
    assert state['_train_rows'] is None and state['_train_stats'] is None
    np.testing.assert_array_equal(state['_train_host'], rows.numpy())
    loaded = pickle.loads(pickle.dumps(model))
    assert loaded._train_rows is None and loaded._train_stats is None and loaded.metric == 'correlation'
    np.testing.assert_array_equal(loaded._train_host, rows.numpy())
    assert model._train_stats is not None                        # the live object keeps its own


# ---- clean_collected_segments ----------------------------------------------------------------------------------------
class _Stages:
    """the device stages of ``clean_collected_segments`` replaced by the fixture's spectrograms (found by the bytes of
    the audio slice) and the stub transform"""

    def __init__(self, golden, monkeypatch, answers):
        self.specs = golden["seg_specs"].astype(np.float64)
        self.by_slice = {a.tobytes(): i for i, a in enumerate(CC.clean_slices())}
        assert len(self.by_slice) == len(self.specs)
        self.padded_calls = []
        it = iter(answers)
        self.answers = it
        CC.StubUMAP.fitted.clear()
        monkeypatch.setattr(TS, "segment_specs", lambda result, p: torch.from_numpy(self.specs))
        monkeypatch.setattr(TS, "_padded", self.padded)
        monkeypatch.setattr(TS, "_new_transform", lambda: CC.StubUMAP(random_state=42, metric='correlation'))
        monkeypatch.setattr(builtins, "input", lambda prompt="": next(it))

    def padded(self, slices, p, max_len, device, max_chunk_bytes):
        assert max_len == self.specs.shape[2]
        self.padded_calls.append(len(slices))
        return torch.from_numpy(self.specs[[self.by_slice[a.tobytes()] for a in slices]])


def test_clean_collected_segments_rewrites_the_reference_files(golden, tmp_path, monkeypatch, capsys):
    audio_dirs, seg_dirs, result = CC.write_clean_dirs(str(tmp_path / "run"))
    boxes = json.loads(str(golden["boxes"]))
    assert boxes[1][0] > boxes[1][1]                              # x1 > x2
    answers = CC.box_answers(boxes)
    answers.insert(2, 'oops')                                     # a retry of y1
    stages = _Stages(golden, monkeypatch, answers)
    with pytest.warns(UserWarning, match="tooltip_plot"):
        out = TS.clean_collected_segments(result, audio_dirs, seg_dirs, CC.CLEAN_P, img_fn=str(tmp_path / "pic.pdf"))
    assert out is None and next(stages.answers, None) is None
    files = RC.read_tree(seg_dirs)
    assert files == json.loads(str(golden["files"]))
    assert files[CC.CLEAN_SINGLE] == "" and 0 < sum(len(t.splitlines()) for t in files.values()) < len(stages.specs)
    assert stages.padded_calls == [7, 6]                          # one transform per directory
    np.testing.assert_array_equal(np.sort(CC.StubUMAP.fitted[-1], 0), np.sort(stages.specs.reshape(13, -1), 0))
    assert (tmp_path / "pic.pdf").stat().st_size > 0
    text = capsys.readouterr().out
    for line in ("Collecting spectrograms...", "\tCollected 13 spectrograms.", "\tSpectrogram shape: (76, 34)",
                 "Running UMAP. n = 13", "Selected 0 out of 13", "Invalid input!", "Saving segments...",
                 "\tdeleted: 5 remaining: 8"):
        assert line in text, line
    assert "Randomly sampling" not in text


def test_subsample_is_the_reference_s(golden, tmp_path, monkeypatch):
    audio_dirs, seg_dirs, result = CC.write_clean_dirs(str(tmp_path / "run"))
    stages = _Stages(golden, monkeypatch, CC.box_answers(json.loads(str(golden["boxes"]))))
    monkeypatch.setattr(R, "_tooltip_plot", lambda: None)
    with pytest.warns(UserWarning, match="Found more spectrograms than `max_num_specs` \\(5\\)"):
        TS.clean_collected_segments(result, audio_dirs, seg_dirs, CC.CLEAN_P, max_num_specs=CC.CLEAN_SUBSAMPLE,
                                    verbose=False, img_fn=str(tmp_path / "pic.pdf"))
    perm = golden["perm"]
    np.testing.assert_array_equal(perm, np.random.RandomState(42).permutation(13)[:CC.CLEAN_SUBSAMPLE])
    np.testing.assert_array_equal(CC.StubUMAP.fitted[-1], stages.specs.reshape(13, -1)[perm])
    assert RC.read_tree(seg_dirs) == json.loads(str(golden["files"]))     # the stub does not depend on its fit


def test_no_segments_warns_and_returns(tmp_path, monkeypatch):
    dirs = [[("a_00", 0.3, []), ("a_01", 0.3, [])]]
    audio_dirs, seg_dirs, result = CC.write_clean_dirs(str(tmp_path / "run"), dirs)
    monkeypatch.setattr(builtins, "input", lambda prompt="": pytest.fail("no prompt is expected"))
    before = RC.read_tree(seg_dirs)
    with pytest.warns(UserWarning, match="Found no spectrograms in ava.segmenting.template_segmentation"):
        assert TS.clean_collected_segments(result, audio_dirs, seg_dirs, CC.CLEAN_P, verbose=False) is None
    assert RC.read_tree(seg_dirs) == before


def test_longer_and_shorter_segments_are_refused(golden, tmp_path, monkeypatch):
    audio_dirs, seg_dirs, result = CC.write_clean_dirs(str(tmp_path / "run"))
    # a segment file that grew a segment longer than every collected one since ``result`` was made
    with open(seg_dirs[1] + "/b_00.txt", "a") as f:
        f.write("0.30000 0.50000\n")
    _Stages(golden, monkeypatch, CC.box_answers(json.loads(str(golden["boxes"]))))
    monkeypatch.setattr(R, "_tooltip_plot", lambda: None)
    with pytest.raises(ValueError, match="more than the 34"):
        TS.clean_collected_segments(result, audio_dirs, seg_dirs, CC.CLEAN_P, verbose=False,
                                    img_fn=str(tmp_path / "pic.pdf"))
    audio = RC.refine_audio("a_00", 0.6)
    with pytest.raises(ValueError, match="fewer than nperseg"):
        TS._segment_slices(audio, np.array([[0.1, 0.105]]), 32000, CC.CLEAN_P, "a_00.wav")
    assert [len(a) for a in TS._segment_slices(audio, np.array([[0.02, 0.1], [0.15, 0.24]]), 32000, CC.CLEAN_P,
                                               "a_00.wav")] == [2560, 2880]


def test_clean_collected_data_warns_and_forwards(monkeypatch):
    seen = []
    monkeypatch.setattr(TS, "clean_collected_segments", lambda *a, **kw: seen.append((a, kw)))
    with pytest.warns(UserWarning, match="clean_collected_data has been renamed to clean_collected_segments in v0.3.0"):
        TS.clean_collected_data("r", ["a"], ["s"], {"fs": 1}, max_num_specs=7, verbose=False, img_fn="x.pdf",
                                tooltip_plot_dir="t")
    assert seen == [(("r", ["a"], ["s"], {"fs": 1}), dict(max_num_specs=7, verbose=False, img_fn="x.pdf",
                                                           tooltip_plot_dir="t"))]
