"""Writes tests/golden/refine.npz: the reference's ``_get_specs`` and ``_update_segs_helper``
(ava/segmenting/refine_segments.py) on the synthetic recordings and segment files of tests/refine_cases.py.  Needs the
reference package, scipy and joblib; umap and bokeh are not needed (stub modules stand in: nothing recorded here calls
them).  Run from the repository root as ``python tests/golden/make_golden_refine.py /path/to/reference``.  The tests
only read the npz.

Recorded, all from the reference's own functions:
  ``all_*``     ``_get_specs`` of both directories, ``max_len=None``, ``return_segs=True``
  ``cut_*``     the same at ``max_len = REFINE_MAX_LEN`` (the longest segment is truncated)
  ``stop_*``    ``max_num_specs = 5``: the loop stops in the middle of a file
  ``spec_tol``  max(4 |spec - spec of the float64-cast audio|_max, 4 fp32 ulp of 1), the rule of make_golden_segment.py
  ``bounds``    two boxes in the plane of the stub transform (tests/refine_cases.py:StubTransform)
  ``knn_*``     scikit-learn's brute-force ``kneighbors`` indices of ``refine_cases.knn_case`` (tie-free), per dtype
  ``files``     the text of every file ``_update_segs_helper`` writes for the two directories with that stub and boxes
The spectrograms are float64 arrays of float32 values (int16 audio) and are stored as float32, which loses nothing.
"""
import json
import os
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.append(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("AVA_REFERENCE", "../reference"))

for name in ("umap", "bokeh"):
    if name not in sys.modules:
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
try:
    import ava.plotting.tooltip_plot  # noqa: F401
except ImportError:
    stub = types.ModuleType("ava.plotting.tooltip_plot")
    stub.tooltip_plot = None
    sys.modules["ava.plotting.tooltip_plot"] = stub

import refine_cases as RC                                   # noqa: E402
import ava.segmenting.refine_segments as R                  # noqa: E402
import ava.segmenting.utils as U                            # noqa: E402

OUT = {}


def record(prefix, specs, max_len, all_fns, segs):
    specs = np.stack(specs)
    assert specs.dtype == np.float64 and np.array_equal(specs, specs.astype(np.float32).astype(np.float64))
    OUT[prefix + "_specs"] = specs.astype(np.float32)
    OUT[prefix + "_max_len"] = np.array(max_len)
    OUT[prefix + "_fns"] = np.array(json.dumps(list(all_fns)))
    OUT[prefix + "_segs"] = segs
    print("%-5s %d spectrograms of %s, max_len %d" % (prefix, len(specs), specs.shape[1:], max_len))
    return specs


def main():
    p = dict(RC.REFINE_P)
    root = tempfile.mkdtemp()
    cwd = os.getcwd()
    os.chdir(root)
    try:
        audio_dirs, seg_dirs = RC.write_refine_dirs(root)
        specs_all = record("all", *R._get_specs(audio_dirs, seg_dirs, p, return_segs=True))
        assert specs_all.shape[2] > RC.REFINE_MAX_LEN
        record("cut", *R._get_specs(audio_dirs, seg_dirs, p, max_len=RC.REFINE_MAX_LEN, return_segs=True))
        stop = record("stop", *R._get_specs(audio_dirs, seg_dirs, p, max_num_specs=5, return_segs=True))
        fns = json.loads(str(OUT["stop_fns"]))
        assert len(stop) == 5 and fns.count(fns[-1]) < json.loads(str(OUT["all_fns"])).count(fns[-1])

        # tolerance of a spectrogram value: the reference on the float64-cast audio
        gap = 0.0
        for files in RC.REFINE_DIRS:
            for name, seconds, _ in files:
                a = RC.refine_audio(name, seconds)
                gap = max(gap, float(np.abs(U.get_spec(a, p)[0].astype(np.float64) -
                                            U.get_spec(a.astype(np.float64), p)[0]).max()))
        OUT["spec_tol"] = np.array(max(4.0 * gap, 4.0 * float(np.spacing(np.float32(1.0)))))

        # boxes in the stub's plane: the lower-left quadrant about the medians, and a small box about the last point
        stub = RC.StubTransform()
        cut = OUT["cut_specs"].astype(np.float64)
        pts = stub.transform(cut.reshape(len(cut), -1))
        med = np.median(pts, axis=0)
        bounds = {'x1': [float(pts[:, 0].min() - 1.0), float(pts[-1, 0] - 1e-3)],
                  'x2': [float(med[0]), float(pts[-1, 0] + 1e-3)],
                  'y1': [float(pts[:, 1].min() - 1.0), float(pts[-1, 1] - 1e-3)],
                  'y2': [float(med[1]), float(pts[-1, 1] + 1e-3)]}
        OUT["bounds"] = np.array(json.dumps(bounds))
        out_dirs = ["out_%d" % d for d in range(len(seg_dirs))]
        for seg_dir, audio_dir, out_dir in zip(seg_dirs, audio_dirs, out_dirs):
            R._update_segs_helper(seg_dir, audio_dir, out_dir, p, RC.REFINE_MAX_LEN, stub, bounds, False)
        files = RC.read_tree(out_dirs)
        OUT["files"] = np.array(json.dumps(files))
        kept = sum(len(t.splitlines()) - 1 for t in files.values())
        print("boxes", bounds)
        print("files written:", sorted(files), "segments kept: %d of %d" % (kept, len(cut)))
        assert 0 < kept < len(cut)
    finally:
        os.chdir(cwd)
        shutil.rmtree(root)
    from sklearn.neighbors import NearestNeighbors
    for dtype in (np.float32, np.float64):
        Q, X, k = RC.knn_case(dtype)
        nn = NearestNeighbors(n_neighbors=k, algorithm='brute').fit(X.astype(np.float64))
        dist, idx = nn.kneighbors(Q.astype(np.float64))
        assert np.all(np.diff(dist, axis=1) > 0)
        OUT["knn_%s_idx" % np.dtype(dtype).name] = idx.astype(np.int64)
    path = os.path.join(HERE, "refine.npz")
    np.savez_compressed(path, **OUT)
    print("wrote", path, os.path.getsize(path), "bytes; spec_tol %.3g" % float(OUT["spec_tol"]))


if __name__ == "__main__":
    main()
