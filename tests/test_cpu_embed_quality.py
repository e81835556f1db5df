"""CPU-side tests of the embedding-quality row (f26, no GPU needed): the numpy restatement of the definitions
reproduces scikit-learn's floats of tests/golden/embed_quality.npz exactly, its ranks are the brute-force definition on
tie cases, the argument checks come before any device call, and include/ava_embed_quality.h and _lib.EQ_SIGNATURES
mirror each other."""
import ctypes
import os
import re

import numpy as np
import pytest

import embed_quality_cases as EC
from conftest import ROOT, load_golden
from ava_amd import _lib
from ava_amd import embedding_quality as EQ


@pytest.fixture(scope="module")
def golden():
    return load_golden("embed_quality.npz")


@pytest.fixture(scope="module")
def pairs(golden):
    """the restatement of every golden case, made once"""
    out = []
    for i, (n, d, k, seed) in enumerate(EC.GOLDEN_CASES):
        _, X = EC.golden_x(n, d, seed)
        out.append((X, golden["c%d_Y" % i], EC.Pair(X, golden["c%d_Y" % i], k)))
    return out


@pytest.mark.parametrize("i", range(len(EC.GOLDEN_CASES)))
def test_restatement_reproduces_sklearn_exactly(golden, pairs, i):
    n, d, k, seed = EC.GOLDEN_CASES[i]
    cur = pairs[i][2].curve([k])
    assert cur["trustworthiness"][0] == float(golden["c%d_trust" % i])
    assert cur["continuity"][0] == float(golden["c%d_cont" % i])
    assert int(cur["penalty_t"][0]) == int(golden["c%d_pen_t" % i])
    assert int(cur["penalty_c"][0]) == int(golden["c%d_pen_c" % i])
    if i < EC.GOLDEN_RANK_TABLES:
        assert np.array_equal(pairs[i][2].rank_x, golden["c%d_rank_x" % i])
        assert np.array_equal(pairs[i][2].rank_y, golden["c%d_rank_y" % i])


@pytest.mark.parametrize("i", range(len(EC.GOLDEN_CASES)))
def test_gap_condition(pairs, i):
    X, Y, _ = pairs[i]
    assert EC.min_gap(EC.sqd(X)) >= EC.MIN_GAP and EC.min_gap(EC.sqd(Y)) >= EC.MIN_GAP


def test_golden_file_is_small(golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "embed_quality.npz")) < 300 * 1024


@pytest.mark.parametrize("name", ["twins", "grid"])
def test_tie_ranks_are_the_definition(name):
    X = EC.twins(20, 3, 0) if name == "twins" else EC.grid()
    D2 = EC.sqd(X)
    r = EC.ranks_of(EC.order(D2))
    n = len(X)
    for i in range(n):
        for j in range(n):
            if i != j:
                assert r[i, j] == EC.brute_rank(D2, i, j), (i, j)
    assert sorted(r[0][1:]) == list(range(1, n))           # a strict order: every rank once
    if name == "twins":
        assert all(r[i, i + 20] == 1 and r[i + 20, i] == 1 for i in range(20))
    else:
        assert EC.min_gap(D2) == 0.0                       # the grid does tie


def test_local_values_average_to_the_scalar(pairs):
    for i, (n, d, k, seed) in enumerate(EC.GOLDEN_CASES[:3]):
        cur, loc = pairs[i][2].curve([k]), pairs[i][2].local(k)
        assert abs(loc["trustworthiness"].mean() - cur["trustworthiness"][0]) <= 1e-15
        assert abs(loc["continuity"].mean() - cur["continuity"][0]) <= 1e-15
        assert loc["overlap"].sum() == round(cur["preservation"][0] * n * k)
        assert abs(cur["lcmc"][0] - (cur["preservation"][0] - k / (n - 1.0))) <= 1e-15


def test_prefix_property_of_the_sweep(pairs):
    X, Y, pair = pairs[1]
    k = EC.GOLDEN_CASES[1][2]
    cur = pair.curve([1, 5, k])
    for a, kk in enumerate([1, 5]):
        one = EC.Pair(X, Y, kk).curve([kk])
        for key in ("trustworthiness", "continuity", "preservation", "lcmc"):
            assert one[key][0] == cur[key][a]


def test_errors_come_before_any_device_call():
    X, Y = EC.rows(20, 4, 0), EC.rows(20, 2, 1)
    for k in (10, 11, 64):
        with pytest.raises(ValueError, match="n_neighbors"):
            EQ.trustworthiness(X, Y, n_neighbors=k)
    with pytest.raises(ValueError, match=r"n_neighbors \(10\) should be less than n_samples / 2 \(10.0\)"):
        EQ.trustworthiness(X, Y, n_neighbors=10)
    for fn in (EQ.continuity, EQ.neighborhood_preservation, EQ.local_quality):
        with pytest.raises(ValueError, match="n_neighbors"):
            fn(X, Y, n_neighbors=10)
    with pytest.raises(ValueError, match="n_neighbors"):
        EQ.quality_curve(X, Y, [1, 10])
    with pytest.raises(ValueError, match="n_neighbors"):
        EQ.compare_projections(X, {"a": Y}, [0])
    with pytest.raises(ValueError, match="inconsistent"):
        EQ.trustworthiness(X, Y[:19], n_neighbors=3)
    with pytest.raises(ValueError, match="inconsistent"):
        EQ.compare_projections(X, {"a": Y, "b": Y[:19]}, [3])
    with pytest.raises(ValueError, match="2D"):
        EQ.trustworthiness(X[:, 0], Y, n_neighbors=3)
    for bad in (np.nan, np.inf):
        Z = Y.copy()
        Z[3, 1] = bad
        with pytest.raises(ValueError, match="NaN|infinity"):
            EQ.trustworthiness(X, Z, n_neighbors=3)
        with pytest.raises(ValueError, match="NaN|infinity"):
            EQ.quality_curve(Z, X, [3])
    with pytest.raises(NotImplementedError):
        EQ.trustworthiness(X, Y, n_neighbors=3, metric='cosine')
    with pytest.raises(NotImplementedError):
        EQ.trustworthiness(X, Y, n_neighbors=3, metric='precomputed')
    t = np.tile(np.arange(1, 4), (20, 1))
    t[5, 1] = 5                                            # its own row
    with pytest.raises(ValueError, match="target"):
        EQ.neighbor_ranks(X, t)
    t[5, 1] = 20
    with pytest.raises(ValueError, match="target"):
        EQ.neighbor_ranks(X, t)
    with pytest.raises(ValueError, match="targets"):
        EQ.neighbor_ranks(X, np.zeros((20, 64), dtype=np.int64))


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        return                                             # with a GPU the call succeeds: test_gpu_embed_quality.py
    X, Y = EC.rows(20, 4, 0), EC.rows(20, 2, 1)
    with pytest.raises(_lib.AvaHipError):
        EQ.trustworthiness(X, Y, n_neighbors=3)


def test_header_and_signatures_mirror_each_other():
    """include/ava_embed_quality.h against _lib.EQ_SIGNATURES, by the rule of test_cpu_boundary.test_header_mirror"""
    scalar = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
              "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64}
    header = open(os.path.join(ROOT, "include", "ava_embed_quality.h")).read()
    assert set(re.findall(r"\b(ava_eq_[a-z0-9_]+)\s*\(", header)) == set(_lib.EQ_SIGNATURES)
    decls = re.findall(r"^((?:const )?\w+\s*\*?)\s*(ava_[a-z0-9_]+)\(([^;{]*)\);", header, flags=re.M)
    assert sorted(d[1] for d in decls) == sorted(_lib.EQ_SIGNATURES) and len(decls) == 6
    assert not set(_lib.EQ_SIGNATURES) & set(_lib.SIGNATURES)
    main = open(os.path.join(ROOT, "include", "ava_hip.h")).read()
    assert '#include "ava_embed_quality.h"' in main

    def mirrors(ctype, got):
        ctype = ctype.replace("const ", "").strip()
        if ctype == "ava_stream_t":
            return got is ctypes.c_void_p
        if ctype.endswith("*"):
            pointee = ctype[:-1].strip()
            return got is ctypes.c_void_p or (pointee in scalar and got is ctypes.POINTER(scalar[pointee]))
        return got is scalar[ctype]

    for res, name, args in decls:
        got_res, got_args = _lib.EQ_SIGNATURES[name]
        assert mirrors(" ".join(res.split()), got_res), name
        want = [] if args.strip() == "void" else [" ".join(a.split()) for a in args.split(",")]
        assert len(got_args) == len(want), name
        for arg, got in zip(want, got_args):
            m = re.fullmatch(r"(.*?)\s*\b\w+(\[\d*\])?", arg)
            assert mirrors(m.group(1) + ("*" if m.group(2) else ""), got), (name, arg)
    lib = _lib.load()
    for name in _lib.EQ_SIGNATURES:
        assert hasattr(lib, name), name
    assert lib.ava_eq_max_targets() == EQ.MAX_NEIGHBORS == 63
    assert lib.ava_eq_max_sweep() == EQ.MAX_SWEEP
    assert lib.ava_eq_workspace_bytes(100, 63) > 0
    assert lib.ava_eq_workspace_bytes(100, 64) == 0 and lib.ava_eq_workspace_bytes(1, 1) == 0
    assert lib.ava_eq_workspace_bytes(2 ** 31 - 64, 5) == 0 and lib.ava_eq_workspace_bytes(2 ** 31 - 65, 5) > 0
