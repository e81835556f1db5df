"""CPU-side tests of the shotgun-movie search (row f7): the golden against an fp64 numpy restatement of both metrics,
the conditions of the edge cases that test_gpu_neighbors_edges.py runs on the device (clear winners, exact planted ties,
every tile position deciding, the restatement's own floor on near-constant rows, the grid.y boundary), the window
schedule against the reference's loop, argument validation and ``install``."""
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


# ---- the edge cases (neighbor_cases.EDGE_CASES): the conditions under which the device tests compare with == --------

def test_edge_cases_cover_the_listed_sizes():
    shapes = {m: {(len(NC.edge_case(n)["q"]), len(NC.edge_case(n)["r"]), NC.edge_case(n)["q"].shape[1],
                   str(NC.edge_case(n)["q"].dtype)) for n, c in NC.EDGE_CASES.items() if c[0] == "tile" and c[1] == m}
              for m in NC.TILE}
    for metric, sizes, ds, corner in [("euclidean", (63, 64, 65), (1, 31, 32, 33, 65), (65, 65, 33)),
                                      ("correlation", (127, 128, 129), (2, 15, 16, 17, 33), (129, 129, 17))]:
        got = shapes[metric]
        assert {s[:2] for s in got} >= {(a, b) for a in sizes for b in sizes} | {(1, sizes[2]), (sizes[2], 1)}
        assert {s[2] for s in got} == set(ds)
        assert {corner + ("float32",), corner + ("float64",)} <= got
    groups = {c[0] for c in NC.EDGE_CASES.values()}
    assert groups == {"tile", "d1", "position", "tie", "reduce", "near_constant", "clip"}


@pytest.mark.parametrize("name", sorted(NC.EDGE_CASES))
def test_edge_case_decides(name):
    """no tie but the planted ones: gap > 1e-9 on every query (between bit-identical rows exactly 0, and then > 1e-9
    to the third best), and the planted winner is the restatement's"""
    case = NC.edge_case(name)
    tied = sorted({t[0] for t in case["ties"]})
    clear = np.setdiff1d(np.arange(len(case["q"])), tied)
    assert (case["gap"][clear] > 1e-9).all(), case["gap"][clear].min()
    for query, low, high in case["ties"]:
        assert low < high and np.array_equal(case["r"][low], case["r"][high])
        assert case["D"][query, low] == case["D"][query, high] == case["dist"][query]
        assert case["gap"][query] == 0.0 and case["idx"][query] == low
    assert (NC.third_gap(case["D"])[tied] > 1e-9).all()
    if case["winners"] is not None:
        np.testing.assert_array_equal(case["idx"], case["winners"])
    for query in case["same"]:
        assert np.array_equal(case["q"][query], case["r"][case["idx"][query]])
    if case["group"] == "d1" or name == "edge_corr_nan_query":
        rows = slice(None) if case["group"] == "d1" else 1
        assert np.isnan(case["D"][rows]).all() and (case["idx"][rows] == 0).all()


@pytest.mark.parametrize("name", sorted(n for n, c in NC.EDGE_CASES.items() if c[0] == "reduce"))
def test_reduce_cases_reach_the_later_passes(name):
    """more than 64 tiles, and winners planted in tile 0, tile 63, tile 64 and the last row (plain runs) or a pair of
    bit-identical rows in tiles j and j + 64 (dup runs); a spoilt row in tile 64 and one in tile 2"""
    case = NC.edge_case(name)
    metric, nr = case["metric"], len(case["r"])
    tile = NC.TILE[metric]
    assert len(case["q"]) == 5 and -(-nr // tile) in (65, 129) and case["q"].shape[1] == (5 if tile == 128 else 3)
    args = NC.EDGE_CASES[name][3]
    rows, dup, spoil = args[2], args[3], args[4]
    tiles = {row // tile for row in rows}
    if dup is None or nr == 8193 and tile == 64:
        assert {0, 63, 64} <= tiles and nr - 1 in rows
    if dup is not None:
        assert dup[0] // tile == 0 and dup[1] // tile == 64 and dup[0] in rows
    if spoil:
        assert {row // tile for row in spoil} in ({64, 2}, {64})
    if metric == "correlation" and spoil:
        assert np.isnan(case["D"][:, spoil]).all() and not np.isin(case["idx"], spoil).any()


@pytest.mark.parametrize("name", sorted(n for n, c in NC.EDGE_CASES.items() if c[0] == "position"))
def test_every_position_of_a_tile_decides(name):
    """each reference is the clear winner of exactly one query, and within the first full tile every query position
    has its winner in the tile and every reference position is a winner"""
    case = NC.edge_case(name)
    idx, tile = case["idx"], NC.TILE[case["metric"]]
    assert NC.QTILE[case["metric"]] == tile
    np.testing.assert_array_equal(np.sort(idx), np.arange(len(case["r"])))
    pairs = {(i % tile, int(idx[i]) % tile) for i in range(tile) if idx[i] < tile}
    assert {p[0] for p in pairs} == set(range(tile)) and {p[1] for p in pairs} == set(range(tile))
    # neighbouring queries do not share a winner's 16-row block: the lanes that hold the winners differ too
    assert len({int(idx[i]) // 16 for i in range(4)}) > 1


def test_near_constant_floor():
    """the fp64 restatement's own error on rows of a large mean and a small variation, against np.longdouble; far
    below the 1e-9 by which the winners are clear, so the indices of this case compare with == as well"""
    case = NC.edge_case(NC.NEAR_CONSTANT)
    assert case["q"].shape == (9, 4096) and case["r"].shape == (130, 4096) and case["q"].dtype == np.float64
    for x in (case["q"], case["r"]):
        assert np.abs(x.mean(axis=1) - 1e6).max() < 1e-2 and x.std(axis=1).max() < 1e-3
    floor, DL = NC.near_constant_floor()
    print("near-constant rows: floor of the fp64 restatement against longdouble %.3e" % floor)
    assert DL.dtype == np.longdouble and DL.shape == case["D"].shape
    assert 0.0 <= floor < 1e-10
    idx_l, _ = NC.nearest_from_distances(DL, "correlation")
    np.testing.assert_array_equal(idx_l, case["idx"])


def test_workspace_bytes_at_the_grid_y_boundary():
    """ceil_div(nq, query tile) <= 65535; a host-only query, nothing is launched"""
    lib = _lib.load()
    for metric, tile in [(0, 128), (1, 64)]:
        assert lib.ava_nn_workspace_bytes(65535 * tile, 1, 1, metric) > 0
        assert lib.ava_nn_workspace_bytes(65535 * tile + 1, 1, 1, metric) == 0
        assert lib.ava_nn_workspace_bytes(65535 * tile - 1, 1, 1, metric) > 0


def test_nn_better_restatement():
    nan = np.nan
    B = NC.nn_better
    for nan_wins in (0, 1):
        assert B(1.0, 3, 2.0, 1, nan_wins) and not B(2.0, 1, 1.0, 3, nan_wins)
        assert B(1.0, 1, 1.0, 3, nan_wins) and not B(1.0, 3, 1.0, 1, nan_wins) and not B(1.0, 3, 1.0, 3, nan_wins)
        assert B(-0.0, 1, 0.0, 3, nan_wins) and not B(-0.0, 3, 0.0, 1, nan_wins)      # -0.0 == 0.0: the index decides
        assert B(nan, 1, nan, 3, nan_wins) and not B(nan, 3, nan, 1, nan_wins)
        assert B(5.0, 0, 0.0, -1, nan_wins) and not B(0.0, -1, 5.0, 0, nan_wins) and not B(0.0, -1, 0.0, -1, nan_wins)
    assert B(nan, 9, 0.0, 1, 1) and not B(0.0, 1, nan, 9, 1)
    assert B(0.0, 9, nan, 1, 0) and not B(nan, 1, 0.0, 9, 0)
    # the restated merge on the rows of test_restatement_tie_and_nan_rules, one reference per chunk
    D = np.array([[0.5, 0.25, 0.25], [np.nan, 0.7, np.nan], [np.nan, np.nan, np.nan]])
    for metric, nan_wins in (("correlation", 0), ("euclidean", 1)):
        bi, bd = np.zeros(3, dtype=np.int64), D[:, 0].copy()
        for j in (1, 2):
            bi, bd = NC.merge(bi, bd, np.zeros(3, dtype=np.int64), D[:, j], j, nan_wins)
        want_i, want_d = NC.nearest_from_distances(D, metric)
        np.testing.assert_array_equal(bi, want_i)
        np.testing.assert_array_equal(bd, want_d)


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
