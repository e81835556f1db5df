"""Writes tests/golden/clean.npz: scikit-learn's correlation kNN of the cases of tests/clean_cases.py, and the
reference's ``_get_spec`` and ``clean_collected_segments`` (ava/segmenting/template_segmentation.py) on the synthetic
recordings and collected segments of tests/clean_cases.py.  Needs the reference package, scipy, scikit-learn, joblib
and matplotlib; run from the repository root as ``python tests/golden/make_golden_clean.py /path/to/reference``.  The
tests only read the npz.

The reference module imports affinewarp, umap, h5py and ava.plotting.tooltip_plot at load time; they are stubbed here.
``umap.UMAP`` is ``clean_cases.StubUMAP`` (a fixed linear map of the rows that accepts ``random_state`` and ``metric``
and records what it was fitted to), ``tooltip_plot`` does nothing and ``input`` is scripted.

Recorded:
  ``knn_<case>_<dtype>``  sklearn's ``NearestNeighbors(metric='correlation', algorithm='brute')`` indices (scipy's fp64
                          distances) of every case of ``clean_cases.KNN_CASES``, both dtypes.  Every gap between
                          consecutive sorted distances of a row is asserted to be >= 1e-9, so the indices are unambiguous.
  ``corr_tol``            JSON, one value per case (the kNN cases of both dtypes, ``affine``, ``constant``, ``k1_0``,
                          ``k1_1``): ``clean_cases.tolerance``, 8 x the largest deviation of the fp64 numpy restatement
                          from its ``np.longdouble`` evaluation, never below 16 d 2^-53
  ``seg_specs``           the reference's ``_get_spec`` of every segment in ``result`` order, zero-padded to the longest
                          (float64 arrays of float32 values for int16 audio, stored as float32, which loses nothing)
  ``spec_tol``            max(4 |spec - spec of the float64-cast audio|_max, 4 fp32 ulp of 1), the rule of
                          make_golden_refine.py
  ``boxes``               JSON, the two rectangles (x1, x2, y1, y2) as answered, the second with x1 > x2
  ``files``               JSON, the text of every segment file after the reference's ``clean_collected_segments`` ran
  ``perm``                the rows of ``seg_specs`` the reference fitted its UMAP to with
                          ``max_num_specs = clean_cases.CLEAN_SUBSAMPLE``, in order
"""
import builtins
import contextlib
import io
import json
import os
import shutil
import sys
import tempfile
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.append(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("AVA_REFERENCE", "../reference"))

for _name in ("affinewarp", "umap", "h5py", "ava.plotting.tooltip_plot"):
    _stub = types.ModuleType(_name)
    _stub.ShiftWarping = _stub.tooltip_plot = None
    sys.modules[_name] = _stub

import clean_cases as CC                                    # noqa: E402
import refine_cases as RC                                   # noqa: E402
import ava.segmenting.template_segmentation as TS           # noqa: E402

TS.umap.UMAP = CC.StubUMAP
TS.tooltip_plot = lambda *args, **kwargs: None

OUT = {}
MARGIN = 1e-3        # every point stays this far from every edge of the boxes


def record_knn():
    from sklearn.neighbors import NearestNeighbors
    tol = {}
    for name in CC.KNN_CASES:
        for dtype in (np.float32, np.float64):
            Q, X, k = CC.knn_case(name, dtype)
            X64 = X.astype(np.float64)
            Q64 = X64 if Q is None else Q.astype(np.float64)
            nn = NearestNeighbors(n_neighbors=k, metric='correlation', algorithm='brute').fit(X64)
            dist, idx = nn.kneighbors(Q64)
            gap = float(np.diff(dist, axis=1).min()) if k > 1 else np.inf
            assert gap >= 1e-9, (name, gap)
            if Q is None:
                assert np.array_equal(idx[:, 0], np.arange(len(X)))
            key = "%s_%s" % (name, np.dtype(dtype).name)
            OUT["knn_" + key] = idx.astype(np.int64)
            tol[key] = CC.tolerance(Q64, X64)
            want = (CC.knn(X, k) if Q is None else CC.knn_query(Q, X, k))[0]
            assert np.array_equal(want, idx), name
            print("knn %-20s smallest gap %.3g, corr_tol %.3g" % (key, gap, tol[key]))
    Q, X, _ = CC.affine_case()
    tol["affine"] = CC.tolerance(Q, X)
    Q, X, _ = CC.constant_case()
    tol["constant"] = CC.tolerance(Q, X)
    for i, (Q, X) in enumerate(CC.k1_cases()):
        tol["k1_%d" % i] = CC.tolerance(Q, X)
    OUT["corr_tol"] = np.array(json.dumps(tol))


def scripted(answers):
    it = iter(answers)
    return lambda prompt="": next(it)


def run_reference(result, audio_dirs, seg_dirs, p, answers, **kwargs):
    old = builtins.input
    builtins.input = scripted(answers)
    try:
        with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
            warnings.simplefilter("ignore")
            TS.clean_collected_segments(result, audio_dirs, seg_dirs, p, verbose=False,
                                        img_fn=os.path.join(os.path.dirname(audio_dirs[0]), "temp.pdf"), **kwargs)
    finally:
        builtins.input = old


def main():
    record_knn()
    p = dict(CC.CLEAN_P)
    fs = p['fs']
    # the reference's spectrogram of every segment, and of the float64-cast audio for the tolerance
    slices = CC.clean_slices()
    specs = [TS._get_spec(fs, a, p)[0] for a in slices]
    gap = max(float(np.abs(s.astype(np.float64) - TS._get_spec(fs, a.astype(np.float64), p)[0]).max())
              for s, a in zip(specs, slices))
    OUT["spec_tol"] = np.array(max(4.0 * gap, 4.0 * float(np.spacing(np.float32(1.0)))))
    max_t = max(s.shape[1] for s in specs)
    assert len({s.shape[1] for s in specs}) >= 3
    padded = np.zeros((len(specs), specs[0].shape[0], max_t))
    for i, s in enumerate(specs):
        padded[i, :, :s.shape[1]] = s
    assert np.array_equal(padded, padded.astype(np.float32).astype(np.float64))
    OUT["seg_specs"] = padded.astype(np.float32)
    N = len(padded)

    # two boxes in the stub's plane.  The first takes the side of a split of the x axis that does not hold the point of
    # the single-segment file; the second, answered with x1 > x2, is a small box about one more point.
    pts = RC.StubTransform().transform(padded.reshape(N, -1))
    names = [n for files in CC.CLEAN_DIRS for n, _, segs in files for _ in segs]
    single = names.index(CC.CLEAN_SINGLE.split('/')[1][:-4])
    assert names.count(names[single]) == 1
    xs = np.sort(pts[:, 0])
    mid = N // 2
    split = 0.5 * (xs[mid - 1] + xs[mid])
    lo, hi = float(pts.min() - 1.0), float(pts.max() + 1.0)
    box1 = (split, hi, lo, hi) if pts[single, 0] < split else (lo, split, lo, hi)
    outside = [i for i in range(N) if i != single and not (min(box1[:2]) < pts[i, 0] < max(box1[:2]))]
    extra = outside[0]
    r = 0.25 * min(np.abs(pts[extra] - pts[i]).max() for i in range(N) if i != extra)
    box2 = (float(pts[extra, 0] + r), float(pts[extra, 0] - r), float(pts[extra, 1] - r), float(pts[extra, 1] + r))
    boxes = [tuple(float(v) for v in box1), box2]
    for b in boxes:
        assert np.abs(pts[:, 0, None] - np.array(b[:2])[None, :]).min() > MARGIN
        assert np.abs(pts[:, 1, None] - np.array(b[2:])[None, :]).min() > MARGIN
    OUT["boxes"] = np.array(json.dumps(boxes))

    root = tempfile.mkdtemp()
    try:
        audio_dirs, seg_dirs, result = CC.write_clean_dirs(os.path.join(root, "run"))
        assert [len(v) for v in result.values()] == [len(segs) for files in CC.CLEAN_DIRS for _, _, segs in files]
        CC.StubUMAP.fitted.clear()
        run_reference(result, audio_dirs, seg_dirs, p, CC.box_answers(boxes))
        fitted = CC.StubUMAP.fitted[-1]
        assert fitted.shape == (N, padded[0].size)
        files = RC.read_tree(seg_dirs)
        OUT["files"] = np.array(json.dumps(files))
        kept = sum(len(t.splitlines()) for t in files.values())
        print("boxes", boxes)
        print("segments kept: %d of %d; empty files: %s" % (kept, N, sorted(k for k, t in files.items() if t == "")))
        assert 0 < kept < N and files[CC.CLEAN_SINGLE] == ""

        # the subsample: which rows the reference fits with max_num_specs < N
        audio_dirs, seg_dirs, result = CC.write_clean_dirs(os.path.join(root, "sub"))
        run_reference(result, audio_dirs, seg_dirs, p, CC.box_answers(boxes), max_num_specs=CC.CLEAN_SUBSAMPLE)
        sub = CC.StubUMAP.fitted[-1]
        flat = padded.reshape(N, -1)
        perm = [int(np.flatnonzero((flat == row).all(1))[0]) for row in sub]
        assert len(perm) == CC.CLEAN_SUBSAMPLE < N and len(set(perm)) == len(perm)
        OUT["perm"] = np.array(perm, dtype=np.int64)
        print("subsample", perm)
    finally:
        shutil.rmtree(root)
    path = os.path.join(HERE, "clean.npz")
    np.savez_compressed(path, **OUT)
    print("wrote", path, os.path.getsize(path), "bytes; spec_tol %.3g" % float(OUT["spec_tol"]))


if __name__ == "__main__":
    main()
