"""CPU-side tests of the shotgun-movie search (row f7): the golden against an fp64 numpy restatement of both metrics,
the window schedule against the reference's loop, argument validation and ``install``."""
import types

import numpy as np
import pytest

import neighbor_cases as NC
from conftest import load_golden
from ava_amd import _lib, neighbors as N, shotgun_movie as SM


@pytest.fixture(scope="module")
def golden():
    return load_golden("neighbors.npz")


@pytest.mark.parametrize("name", sorted(NC.CASES))
def test_golden_agrees_with_numpy_restatement(golden, name):
    metric = NC.CASES[name][0]
    np.testing.assert_array_equal(golden[name + "_params"], NC.params_row(name))
    q, r = NC.case_inputs(name)
    idx, dist, D = NC.numpy_nearest(q, r, metric)
    g_idx, g_dist, g_gap = golden[name + "_idx"], golden[name + "_dist"], golden[name + "_gap"]
    assert g_idx.shape == (len(q),) and g_dist.shape == (len(q),)
    clear = g_gap > 1e-9
    np.testing.assert_array_equal(idx[clear], g_idx[clear])
    # where the golden holds a tie, its pick is (within rounding) as near as the restatement's
    picked = D[np.arange(len(q)), g_idx]
    np.testing.assert_allclose(picked, dist, rtol=0, atol=1e-12)
    if metric == "correlation":
        np.testing.assert_allclose(g_dist, dist, rtol=0, atol=1e-12)
    else:
        np.testing.assert_allclose(g_dist, dist, rtol=1e-12, atol=0)


def test_restatement_tie_and_nan_rules():
    D = np.array([[0.5, 0.25, 0.25], [np.nan, 0.7, np.nan], [np.nan, np.nan, np.nan]])
    idx, dist = NC.nearest_from_distances(D, "correlation")
    np.testing.assert_array_equal(idx, [1, 1, 0])
    assert np.isnan(dist[2])
    idx, _ = NC.nearest_from_distances(D, "euclidean")
    np.testing.assert_array_equal(idx, [1, 0, 0])


def _reference_schedule(n_samples, fs, window_length, fps, shoulder):
    """shotgun_movie.py:101-111, the loop as the reference writes it (spectrograms left out)"""
    onsets = []
    dt = 1/fps
    onset = shoulder
    while onset + window_length < n_samples/fs - shoulder:
        onsets.append(onset)
        onset += dt
    return onsets


@pytest.mark.parametrize("fps,shoulder,fs", [(30, 0.01, 32000), (20, 0.05, 44100), (24, 0.0, 250000), (7, 0.3, 8000)])
def test_window_schedule_matches_reference_loop(fps, shoulder, fs):
    window_length = 0.12
    float_decided = 0
    for k in range(1, 120):
        # lengths whose last window sits right at the boundary, where the accumulated onsets decide
        base = int(round((shoulder + k / fps + window_length + shoulder) * fs))
        for n_samples in range(base - 2, base + 3):
            want = _reference_schedule(n_samples, fs, window_length, fps, shoulder)
            got = SM.window_onsets(n_samples, fs, window_length, fps, shoulder)
            assert got.dtype == np.float64
            assert got.tolist() == want
            exact = shoulder + np.arange(len(want) + 2) / fps
            float_decided += int(np.sum(exact + window_length < n_samples / fs - shoulder) != len(want))
    assert float_decided > 0, "no length where the float accumulation decides the last window"
    assert SM.window_onsets(10, fs, window_length, fps, shoulder).size == 0


def test_nearest_validates_before_any_launch():
    q = np.zeros((3, 4), dtype=np.float32)
    with pytest.raises(ValueError, match="metric"):
        N.nearest(q, q, metric="cosine")
    with pytest.raises(ValueError):
        N.nearest(q, np.zeros((2, 5)), metric="euclidean")              # 10 elements are not rows of 4
    with pytest.raises(ValueError):
        N.nearest(np.zeros((0, 4)), q)
    with pytest.raises(ValueError):
        N.nearest(q, np.zeros((0, 4)))
    with pytest.raises(ValueError, match="exceeds"):
        N.nearest(np.zeros((1, 65537)), np.zeros((1, 65537)))
    with pytest.raises(ValueError, match="chunk_rows"):
        N.nearest(q, q, chunk_rows=0)
    with pytest.raises(ValueError, match="chunk_rows"):
        N.nearest(q, q, chunk_rows=2.5)


def test_nearest_reshapes_like_the_reference():
    assert N._rows(np.zeros((5, 8, 16)), None, "x").shape == (5, 128)
    assert N._rows(np.zeros(7), None, "x").shape == (1, 7)
    assert N._rows(np.zeros((6, 4, 8)), 16, "x").shape == (12, 16)
    assert N._rows(np.zeros((2, 3), dtype=np.int16), None, "x").dtype == np.float64
    assert N._rows(np.zeros((2, 3), dtype=np.float32), None, "x").dtype == np.float32


def test_c_abi_rejects_bad_arguments():
    lib = _lib.load()
    assert lib.ava_nn_workspace_bytes(1800, 20000, 16384, 0) > 0
    assert lib.ava_nn_workspace_bytes(4, 4, 16, 1) > 0
    for args in [(0, 4, 16, 0), (4, 0, 16, 0), (4, 4, 0, 0), (4, 4, 65537, 0), (4, 4, 16, 2), (4, 4, 16, -1)]:
        assert lib.ava_nn_workspace_bytes(*args) == 0, args
    # null pointers / unknown dtype are refused before anything is launched
    assert lib.ava_nn_argmin(None, 0, 4, None, 0, 4, 16, 0, None, None, None, 0, None) == -1
    assert lib.ava_nn_merge(None, None, None, None, 4, 0, 0, None) == -1


def _dc(model_filename="model.tar"):
    return types.SimpleNamespace(model_filename=model_filename, request=lambda field: None)


def test_embedding_methods():
    with pytest.raises(NotImplementedError):
        SM.shotgun_movie_embedding(_dc(), "missing.wav", {}, method="re_umap")
    with pytest.raises(AssertionError):
        SM.shotgun_movie_embedding(_dc(), "missing.wav", {}, method="umap")
    with pytest.raises(AssertionError):
        SM.shotgun_movie_embedding(_dc(None), "missing.wav", {})


def test_ffmpeg_commands_are_the_intended_ones():
    first, second = SM.ffmpeg_commands(30, "out dir", "song 1.wav", "movie.mp4")
    assert first == ["ffmpeg", "-y", "-r", "30", "-i", "out dir/viz-%05d.jpg", "temp.mp4"]
    assert second == ["ffmpeg", "-y", "-r", "30", "-i", "temp.mp4", "-i", "song 1.wav", "-c:a", "aac", "-strict", "-2",
                      "out dir/movie.mp4"]
    assert not any("{}" in a for a in first + second)


def test_install_on_a_stand_in_module():
    mod = types.ModuleType("shotgun_movie_stand_in")
    mod.shotgun_movie_DC = lambda *a, **k: None
    assert SM.install(mod) is mod
    assert mod.shotgun_movie_DC is SM.shotgun_movie_DC
