"""Host logic of the syllable path (ava_amd.preprocess, ava_amd.syllable_dataset) against tests/golden/sylls.npz, which
holds what the reference's process_sylls / get_syllable_partition did on the files of tests/sylls_cases.py.  No GPU."""
import json
import os
import re
import warnings

import numpy as np
import pytest
import torch

import sylls_cases as SC
from conftest import ROOT, load_golden
from ava_amd import _lib
from ava_amd import preprocess as P
from ava_amd import syllable_dataset as SD

RUNS = [(name, d) for name, (_, dirs) in SC.SYLL_SETS.items() for d in dirs]


@pytest.fixture(scope="module")
def golden():
    return load_golden("sylls.npz")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """the recordings and segment files, written once; the tests run from inside it (stored names are relative)"""
    root = str(tmp_path_factory.mktemp("sylls"))
    SC.write_dirs(root)
    return root


@pytest.fixture()
def in_tree(tree, monkeypatch):
    monkeypatch.chdir(tree)
    return ["audio_0", "audio_1"], ["segs_0", "segs_1"]


def js(g, key):
    return json.loads(str(g[key]))


def test_is_audio_file():
    assert P.is_audio_file(".wav") and P.is_audio_file("a.wav")
    assert not P.is_audio_file("wav") and not P.is_audio_file("a.WAV") and not P.is_audio_file("a.wav.txt")


@pytest.mark.parametrize("d", [0, 1])
def test_file_pairing(golden, in_tree, d):
    audio_dirs, seg_dirs = in_tree
    got = P.get_audio_seg_filenames(audio_dirs[d], seg_dirs[d], SC.params("lin"))
    assert [list(got[0]), list(got[1])] == js(golden, "lin.%d.pairs.json" % d)
    assert P.get_audio_filenames(audio_dirs[d]) == [os.path.join(audio_dirs[d], n + ".wav") for n, _ in SC.SYLL_DIRS[d]]


def test_read_onsets_offsets(in_tree, tmp_path):
    on, off = P.read_onsets_offsets_from_file(os.path.join("segs_0", "s0_c.txt"), {})
    assert np.array_equal(on, [0.15, 0.52]) and np.array_equal(off, [0.3, 0.7])
    on, off = P.read_onsets_offsets_from_file(os.path.join("segs_1", "s1_c.txt"), {})
    assert on.shape == (0,) and off.shape == (0,)
    one = tmp_path / "one.txt"
    one.write_text("# header\n0.25 0.5\n")
    on, off = P.read_onsets_offsets_from_file(str(one), {})
    assert on.tolist() == [0.25] and off.tolist() == [0.5]
    odd = tmp_path / "odd.txt"
    odd.write_text("0.1 0.2 0.3\n")
    with pytest.raises(AssertionError, match="Incorrect formatting"):
        P.read_onsets_offsets_from_file(str(odd), {})


@pytest.mark.parametrize("name,d", RUNS)
def test_call_sequence_and_groups(golden, in_tree, name, d):
    """the files visited, the (t1, t2) of every get_spec call and the number of files written, from the host plan"""
    audio_dirs, seg_dirs = in_tree
    key = "%s.%d." % (name, d)
    p = SC.params(name)
    plan = P.plan_directory(audio_dirs[d], seg_dirs[d], p, shuffle=True)
    t1 = np.concatenate(plan['onsets'] + [np.zeros(0)])
    t2 = np.concatenate(plan['offsets'] + [np.zeros(0)])
    assert np.array_equal(t1, golden[key + "calls_t1"]) and np.array_equal(t2, golden[key + "calls_t2"])
    fns = [fn for fn, on in zip(plan['audio_filenames'], plan['onsets']) for _ in on]
    assert fns == js(golden, key + "calls_fn.json")
    written = js(golden, key + "written.json")
    assert plan['groups'] == len(written)
    assert [P.group_filename(k)[:-4] for k in range(plan['groups'])] == [w[:-5] for w in written]
    assert plan['stopped'] == (name == "stop" and d == 0)
    # the warnings get_spec gives, per syllable and in order
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        P._check_syllables(t1, t2, SC.FS, p)
    assert [str(w.message) for w in caught] == js(golden, key + "warnings.json")


@pytest.mark.parametrize("name,d", RUNS)
def test_grouping_of_recorded_specs(golden, in_tree, name, d):
    """iter_groups on the recorded spectrograms of the visited syllables gives the reference's files: full groups in
    order, the remainder dropped, nothing behind the max_num_syllables stop"""
    audio_dirs, seg_dirs = in_tree
    key = "%s.%d." % (name, d)
    p = SC.params(name)
    plan = P.plan_directory(audio_dirs[d], seg_dirs[d], p, shuffle=True)
    t1 = np.concatenate(plan['onsets'] + [np.zeros(0)])
    t2 = np.concatenate(plan['offsets'] + [np.zeros(0)])
    fns = np.array([os.path.join(audio_dirs[d], os.path.split(fn)[-1])
                    for fn, on in zip(plan['audio_filenames'], plan['onsets']) for _ in on])
    want_specs = golden[("lin.%d." % d if name == "stop" else key) + "specs"]
    n_written = len(golden[key + "onsets"])
    assert n_written == plan['groups'] * p['sylls_per_file'] and n_written < len(t1)      # a remainder is dropped
    # the visited syllables the reference never wrote get placeholder rows: they must not show up in any group
    specs = np.concatenate([want_specs[:n_written], np.full((len(t1) - n_written,) + want_specs.shape[1:], np.nan)])
    groups = list(P.iter_groups(specs, t1, t2, fns, p['sylls_per_file']))
    assert len(groups) == plan['groups']
    for k, g in enumerate(groups):
        rows = slice(k * p['sylls_per_file'], (k + 1) * p['sylls_per_file'])
        assert g['specs'].dtype == np.float64 and np.array_equal(g['specs'], want_specs[rows])
        assert np.array_equal(g['onsets'], golden[key + "onsets"][rows])
        assert np.array_equal(g['offsets'], golden[key + "offsets"][rows])
        assert g['audio_filenames'].dtype.kind == 'S'
        assert np.array_equal(g['audio_filenames'], golden[key + "audio_filenames"][rows])


def test_plan_groups_stop_rule():
    assert P.plan_groups([5, 4, 2], 4, None) == (3, 2, False)
    assert P.plan_groups([5, 4, 2], 4, 8) == (2, 2, True)
    assert P.plan_groups([5, 4, 2], 4, 7) == (2, 2, True)          # stops at the first multiple that reaches it
    assert P.plan_groups([9, 4], 4, 5) == (1, 2, True)             # the check sits inside the write loop
    assert P.plan_groups([0, 3], 4, 4) == (2, 0, False)
    assert P.plan_groups([], 4, 4) == (0, 0, False)


def test_get_syll_specs_asserts_before_device(in_tree):
    p = dict(SC.params("lin"), nperseg=511)
    with pytest.raises(AssertionError):
        P.get_syll_specs([0.1], [0.2], os.path.join("audio_0", "s0_a.wav"), p)
    p = SC.params("lin")
    with pytest.raises(AssertionError, match="s1: "):
        P.get_syll_specs([0.2], [0.2], os.path.join("audio_0", "s0_a.wav"), p)
    assert P.get_syll_specs([], [], os.path.join("audio_0", "s0_a.wav"), p) == ([], [])


def test_chunks_follow_their_own_longest_segment():
    """one 5 s segment among 0.1 s syllables is a chunk of few; the others are not sized by it"""
    p = SC.params("lin")
    n_samples = [3200] * 40 + [160000] + [3200] * 40
    need = _lib.load().ava_spec_workspace_bytes
    budget = need(1, 160000, 512, 256, 32, 24, 0) + 1024
    bounds = P._chunk_bounds(n_samples, p, budget)
    assert bounds[0][0] == 0 and bounds[-1][1] == len(n_samples)
    assert all(a[1] == b[0] for a, b in zip(bounds[:-1], bounds[1:]))
    for lo, hi in bounds:
        assert hi - lo == 1 or need(hi - lo, max(n_samples[lo:hi]), 512, 256, 32, 24, 0) <= budget
    sizes = [hi - lo for lo, hi in bounds]
    assert sizes[0] == 40 and max(sizes) == 40            # sized by the long segment, every chunk would hold one


def _npz_tree(root):
    for d, k in (("part_0", 4), ("part_1", 3)):
        os.makedirs(os.path.join(root, d))
        for i in range(k):
            open(os.path.join(root, d, "syllables_%04d.npz" % i), "w").close()
    open(os.path.join(root, "part_1", "notes.txt"), "w").close()


@pytest.mark.parametrize("split", [1.0, 0.8, 0.5])
@pytest.mark.parametrize("max_num_files", [None, 5])
def test_partition(golden, tmp_path, monkeypatch, split, max_num_files):
    _npz_tree(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    want = js(golden, "partition.json")["%s|%s" % (split, max_num_files)]
    got = SD.get_syllable_partition(["part_0", "part_1"], split, max_num_files=max_num_files)
    for key in ("train", "test"):
        assert got[key] == [re.sub(r"\.hdf5$", ".npz", fn) for fn in want[key]]
    assert len(got['train']) == int(round(split * (7 if max_num_files is None else 5)))


def test_partition_unshuffled(golden, tmp_path, monkeypatch):
    _npz_tree(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    want = js(golden, "partition.json")["0.5|None|noshuffle"]
    got = SD.get_syllable_partition(["part_0", "part_1"], 0.5, shuffle=False)
    assert got == {k: [re.sub(r"\.hdf5$", ".npz", fn) for fn in v] for k, v in want.items()}


def _store(n_groups_per_dir=(4, 3), spf=2):
    """a SyllableStore on the host whose row r holds the value r"""
    group_dir = [d for d, k in enumerate(n_groups_per_dir) for _ in range(k)]
    group_num = [g for k in n_groups_per_dir for g in range(k)]
    n = len(group_dir) * spf
    specs = torch.arange(n, dtype=torch.float32).reshape(n, 1, 1).repeat(1, 2, 3)
    return P.SyllableStore(specs, np.arange(n) * 0.1, np.arange(n) * 0.1 + 0.05, np.array(["f"] * n).astype('S'),
                           np.arange(n) // spf, np.array(group_dir), np.array(group_num), [False, False])


@pytest.mark.parametrize("split,max_num_files", [(1.0, None), (0.8, None), (0.5, 5)])
def test_partition_store_selects_the_files_rows(golden, split, max_num_files):
    store = _store()
    names = store.group_names(["part_0", "part_1"])
    want = js(golden, "partition.json")["%s|%s" % (split, max_num_files)]
    got = SD.partition_store(store, split, max_num_files=max_num_files, save_dirs=["part_0", "part_1"])
    for key in ("train", "test"):
        groups = [names.index(re.sub(r"\.hdf5$", ".npz", fn)) for fn in want[key]]
        rows = [r for g in groups for r in (2 * g, 2 * g + 1)]
        assert got[key][0] is store and got[key][1].tolist() == rows
    loaders_test_part = got['test'][1]
    assert (len(loaders_test_part) == 0) == (split == 1.0)


def test_loader_order_is_randperm():
    ds = SD.DeviceSyllableDataset.from_arrays(np.zeros((37, 2, 3), dtype=np.float64), device="cpu")
    assert len(ds) == 37 and ds.item_shape == (2, 3)
    loader = SD.DeviceSyllableLoader(ds, batch_size=8, shuffle=True, generator=torch.Generator().manual_seed(5))
    assert len(loader) == 5 and loader.dataset is ds and loader.batch_size == 8 and loader.device_resident
    want = torch.Generator().manual_seed(5)
    for _ in range(2):                                           # a fresh permutation per epoch, from the same generator
        assert loader.order() == torch.randperm(37, generator=want).tolist()
    assert SD.DeviceSyllableLoader(ds, batch_size=8).order() == list(range(37))


def test_rows_of_a_store_subset():
    store = _store()
    ds = SD.DeviceSyllableDataset.from_store(store, rows=[5, 3, 3, 13])
    assert len(ds) == 4 and ds.source_rows([3, 0, 1]).tolist() == [13, 5, 3]
    with pytest.raises(IndexError):
        SD.DeviceSyllableDataset.from_store(store, rows=[14])


@pytest.mark.parametrize("bad", [[37], [-1], [0, 5, 99], 37])
def test_index_error_before_any_launch(bad):
    ds = SD.DeviceSyllableDataset.from_arrays(np.zeros((37, 2, 3), dtype=np.float32), device="cpu")
    with pytest.raises(IndexError):
        ds[bad]
    with pytest.raises(TypeError):
        SD.DeviceSyllableDataset.from_arrays(np.zeros((3, 2, 3), dtype=np.int32), device="cpu")


def test_gather_refuses_bad_arguments():
    """AVA_EINVAL before any launch: needs the built library, no GPU"""
    f = _lib.load().ava_gather_rows_f32
    ok = dict(src=4096, dt=0, n_rows=4, row=8, idx=8192, n=2, dst=12288)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a['src'], a['dt'], a['n_rows'], a['row'], a['idx'], a['n'], a['dst'], None)

    for kw in (dict(src=None), dict(idx=None), dict(dst=None), dict(n=0), dict(n=-3), dict(row=0), dict(row=-1),
               dict(dt=5), dict(dt=-1), dict(n_rows=0)):
        assert call(**kw) == -1, kw


def test_exports():
    assert "ava_gather_rows_f32" in _lib.SIGNATURES
    with open(os.path.join(ROOT, "include", "ava_hip.h")) as f:
        header = f.read()
    assert re.search(r"int ava_gather_rows_f32\(const void\* src, int src_dtype, int64_t n_rows, int64_t row_elems,\s*"
                     r"const int64_t\* idx, int64_t n,\s*float\* dst, ava_stream_t s\);", header)
    for name in ("process_sylls", "get_syll_specs", "syllables_to_device", "SyllableStore", "get_audio_seg_filenames",
                 "get_audio_filenames", "read_onsets_offsets_from_file", "is_audio_file", "install"):
        assert name in P.__all__ and hasattr(P, name)
    for name in ("get_syllable_partition", "partition_store", "DeviceSyllableDataset", "DeviceSyllableLoader",
                 "get_syllable_data_loaders", "install"):
        assert name in SD.__all__ and hasattr(SD, name)
