"""The ava_gemm case table (gemm_cases.py) against the dispatcher itself, on the host: ava_gemm_path is the function
gemm_impl launches from, and it needs no device.  Every case takes the kernel it names, the table reaches all 36
instantiations and every epilogue the split and unsplit paths have, and the accuracy bound the device test asserts
(4 x e_seq) is shown to reject a limb kernel that drops one third-order pair at the K the faithfulness cases use."""
import ctypes

import numpy as np
import pytest

import gemm_cases as G
from ava_amd import _lib

AVA_EINVAL, AVA_EWORKSPACE = -1, -3


def _ask(c):
    return G.query(_lib.load(), c, **G.dummy_pointers(c))


@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c.name)
def test_case_takes_the_path_it_names(c):
    path, info = _ask(c)
    print("%s: path %d, tile %d, BK %d, vec %d, splits %d, klen %d, threads %d" % ((c.name, path) + info))
    assert (path,) + info[:4] == c.expect
    tile, bk, vec, splits, klen, threads = info
    assert splits == -(-c.K // klen) and (path == G.SKINNY or klen % bk == 0)
    assert threads == {G.LIMB: 512, G.TILED: 256}.get(path, 512 if c.K >= 512 else 256)


def test_table_reaches_all_36_instantiations():
    seen = {}
    for c in G.CASES:
        path, info = _ask(c)
        seen.setdefault(G.instantiation(c, path, info), []).append(c.name)
    for inst in sorted(G.ALL_INSTANTIATIONS, key=str):
        print(inst, "<-", ", ".join(seen.get(inst, [])))
    assert set(seen) == G.ALL_INSTANTIATIONS


def test_table_reaches_every_epilogue_of_the_split_and_unsplit_paths():
    tiled, limb = set(), set()
    for c in G.CASES:
        path, info = _ask(c)
        split = info[3] > 1
        if path == G.TILED:
            tiled |= {(split, what) for what, on in (("colsum", c.colsum), ("mask", c.mask),
                                                     ("bias+act", c.bias and c.act != G.ACT_NONE)) if on}
        elif path == G.LIMB:
            limb.add(split)
    assert tiled == {(s, w) for s in (False, True) for w in ("colsum", "mask", "bias+act")}
    assert limb == {False, True}
    # every tiled layout has a split and an unsplit case with a mask and ldc = N + 4
    for name in ("t128_bk16_fin_mask_ldc", "t128_bk32_s2_mask_ldc"):
        for ak, bk in ((1, 1), (1, 0), (0, 1), (0, 0)):
            c = G.BY_NAME["%s_%d%d" % (name, ak, bk)]
            assert c.mask and c.ldc == c.N + 4 and (_ask(c)[1][3] > 1) == ("_s2_" in name)


def test_path_query_refuses_what_ava_gemm_refuses_and_follows_pointer_alignment():
    lib = _lib.load()
    info = (ctypes.c_int * 6)()

    def ask(A=4096, B=8192, C=12288, M=256, N=1024, K=8192, bias=None, mask=None, colsum=None, ak=1, bk=1, act=0, ldc=0):
        return lib.ava_gemm_path(A, 0, B, 0, bias, C, ldc, mask, colsum, M, N, K, ak, bk, act, info)

    assert ask() == G.LIMB and tuple(info) == (64, 32, 1, 16, 512, 512)        # fc1 forward at batch 256
    for bad in (dict(A=None), dict(B=None), dict(C=None), dict(M=0), dict(N=-1), dict(K=0)):
        assert ask(**bad) == AVA_EINVAL
    # the limb kernel stores, and reads bias and mask, as 16-byte quads: a misaligned pointer sends the product elsewhere
    for off in (dict(A=4100), dict(B=8196), dict(C=12292), dict(bias=16388), dict(mask=16388), dict(ldc=1026),
                dict(act=G.ACT_EXP)):
        assert ask(**off) == G.TILED, off
    assert ask(M=256, N=64, K=32) == G.SKINNY and tuple(info) == (16, 16, 1, 1, 32, 256)
    assert ask(M=256, N=64, K=32, A=4100) == G.TILED                            # k-major A must be 16-byte aligned
    assert ask(M=64, N=256, K=192, colsum=20480) == G.TILED                     # column sums need an m-major A
    assert ask(M=192, N=256, K=64, colsum=20480, ak=0, bk=0) == G.SKINNY
    assert lib.ava_gemm_path(4096, 0, 8192, 0, None, 12288, 0, None, None, 5, 32, 64, 1, 1, 0, None) == G.SKINNY  # info may be NULL


def test_split_workspace_must_be_16_byte_aligned():
    """The split-K slabs are written and read back as 16-byte quads.  The check sits in front of every launch, so it
    answers here, on the host, before anything touches the (dummy) pointers."""
    lib = _lib.load()
    info = (ctypes.c_int * 6)()
    M, N, K = 8, 1024, 8192                                       # limb kernel, split
    nbytes = lib.ava_gemm_workspace_bytes(M, N, K)
    # every call below must be refused in front of the launch: make sure of the premise (a split product) first
    assert lib.ava_gemm_path(4096, 0, 8192, 0, None, 12288, 0, None, None, M, N, K, 1, 1, 0, info) == G.LIMB
    assert info[3] > 1 and nbytes > 0
    call = lambda ws, n: lib.ava_gemm(4096, 0, 8192, 0, None, 12288, 0, None, None, M, N, K, 1, 1, 0, ws, n, None)
    assert call(1 << 20 | 4, nbytes + 16) == AVA_EWORKSPACE
    assert call(1 << 20 | 8, nbytes + 16) == AVA_EWORKSPACE
    assert call(None, nbytes) == AVA_EWORKSPACE
    assert call(1 << 20, nbytes - 4) == AVA_EWORKSPACE
    M, N, K = 8, 200, 2072                                        # tiled kernel, 44 splits
    nbytes = lib.ava_gemm_workspace_bytes(M, N, K)
    assert lib.ava_gemm_path(4096, 0, 8192, 0, None, 12288, 0, None, None, M, N, K, 1, 1, 0, info) == G.TILED
    assert info[3] == 44
    assert lib.ava_gemm(4096, 0, 8192, 0, None, 12288, 0, None, None, M, N, K, 1, 1, 0, 1 << 20 | 4, nbytes + 16,
                        None) == AVA_EWORKSPACE


@pytest.mark.parametrize("c", [c for c in G.CASES if c.faithful], ids=lambda c: c.name)
def test_bound_accepts_six_limb_pairs_and_rejects_five(c):
    """Control for the device test's bound.  The limb split is restated in torch (three bfloat16 roundings of successive
    remainders) and the pairs are accumulated in fp64, so what is measured is the truncation of the limb scheme alone:
    the six kept pairs must pass 4 x e_seq, the six without a2 b0 must not."""
    A, B, bias, _ = G.make_inputs(c)
    pre, denom = G.reference(c, A, B, bias)
    bound = 4.0 * G.e_seq(c, A, B, bias, pre, denom)
    six = G.metric(c, G.limb_product(A, B), pre, denom)
    five = G.metric(c, G.limb_product(A, B, drop_a2b0=True), pre, denom)
    print("%s: e_seq %.3g, bound %.3g, six pairs %.3g (%.2f x e_seq), five pairs %.3g (%.2f x e_seq)"
          % (c.name, bound / 4, bound, six, 4 * six / bound, five, 4 * five / bound))
    assert six <= bound
    assert five > bound


def test_e_seq_is_the_noise_of_an_fp32_accumulation():
    """e_seq must be neither zero nor large: a few 1e-8 .. 1e-6 for K between 5 and 4100 (about sqrt(K) roundings of
    2^-24 relative to the sum of magnitudes)."""
    for name in ("l128_k5_colsum", "sk256_11_bias_relu", "t64_deep_s86"):
        c = G.BY_NAME[name]
        A, B, bias, _ = G.make_inputs(c)
        pre, denom = G.reference(c, A, B, bias)
        e = G.e_seq(c, A, B, bias, pre, denom)
        print(name, "e_seq %.3g" % e)
        assert 2.0 ** -26 < e < 2.0 ** -24 * np.sqrt(c.K) * 4
