"""The syllable path on the device: the row-gather kernel (ava_gather_rows_f32), ava_amd.preprocess against
tests/golden/sylls.npz (the reference's process_sylls on the files of tests/sylls_cases.py) and
ava_amd.syllable_dataset's loaders through the VAE's epoch loops."""
import ctypes
import json
import os
import warnings

import numpy as np
import pytest
import torch

import sylls_cases as SC
from conftest import load_golden
from ava_amd import _lib
from ava_amd import preprocess as P
from ava_amd import spec as SP
from ava_amd import syllable_dataset as SD
from ava_amd import synthetic as syn

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float64", "uint8", "float16", "bfloat16"]
CODES = {"float32": 0, "float64": 1, "uint8": 2, "float16": 3, "bfloat16": 4}
N_ROWS = 37


# ---- the gather kernel ----------------------------------------------------------------------------------------------------
def host_rows(dtype, shape, salt=7100, n=N_ROWS):
    """[n, *shape] test data as a CPU tensor of ``dtype``: float64 values that are no float32 values, halves over
    their whole exponent range, every byte value"""
    count = n * int(np.prod(shape))
    g = syn.gauss(count, salt).reshape((n,) + tuple(shape))
    if dtype == "uint8":
        return torch.from_numpy(np.minimum(syn.u01(count, salt) * 256, 255).astype(np.uint8).reshape(g.shape))
    if dtype == "float64":
        return torch.from_numpy(g * np.exp(8.0 * syn.gauss(count, salt + 1).reshape(g.shape)))
    if dtype == "float32":
        return torch.from_numpy(g.astype(np.float32))
    if dtype == "float16":
        return torch.from_numpy((g * np.exp(3.0 * syn.gauss(count, salt + 1).reshape(g.shape))).astype(np.float16))
    return torch.from_numpy(g.astype(np.float32)).to(torch.bfloat16)


def reference_rows(x, idx):
    """``torch.from_numpy(x[idx]).type(torch.FloatTensor)``; bfloat16 has no numpy form and is indexed as a tensor"""
    if x.dtype == torch.bfloat16:
        return x[torch.as_tensor(idx)].type(torch.FloatTensor)
    return torch.from_numpy(x.numpy()[np.asarray(idx)]).type(torch.FloatTensor)


def index_lists(n):
    perm = np.argsort(syn.u01(n, 7177), kind="stable")
    return {"identity": list(range(n)), "reversed": list(range(n - 1, -1, -1)), "all_equal": [n // 2] * 19,
            "single": [3], "last": [n - 1], "permutation": perm.tolist()}


def gather_raw(src_ptr, code, n_rows, row_elems, idx, dst):
    """the C ABI, called directly; ``idx`` a host list, ``dst`` a device tensor"""
    d_idx = torch.tensor(idx, dtype=torch.int64, device="cuda")
    rc = _lib.load().ava_gather_rows_f32(src_ptr, code, n_rows, row_elems, d_idx.data_ptr(), len(idx), dst.data_ptr(),
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("shape", [(128, 128), (5, 7), (3, 4)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_equals_numpy_to_tensor(dtype, shape):
    x = host_rows(dtype, shape)
    ds = SD.DeviceSyllableDataset.from_arrays(x)
    assert ds.data.dtype == x.dtype and len(ds) == N_ROWS                # uploaded raw
    for name, idx in index_lists(N_ROWS).items():
        got = ds[idx]
        assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (len(idx),) + shape
        assert torch.equal(got.cpu(), reference_rows(x, idx)), (dtype, shape, name)
    assert torch.equal(ds[N_ROWS - 1].cpu(), reference_rows(x, [N_ROWS - 1])[0])


@pytest.mark.parametrize("dtype,which", [("float32", "src"), ("uint8", "src"), ("float16", "src"), ("float64", "dst")])
def test_gather_misaligned_base_takes_the_narrow_path(dtype, which):
    """a base pointer one element off 16-byte alignment: rows of 128 x 128 would otherwise go the wide way"""
    shape = (128, 128)
    row = shape[0] * shape[1]
    x = host_rows(dtype, shape, salt=7200, n=9)
    flat = torch.empty(9 * row + 1, dtype=x.dtype, device="cuda")
    out = torch.full((5 * row + 1,), -7.0, dtype=torch.float32, device="cuda")
    src = flat[1:] if which == "src" else flat[:-1]
    dst = out[1:] if which == "dst" else out[:-1]
    src.copy_(x.reshape(-1))
    assert (src.data_ptr() % 16 != 0) == (which == "src") and (dst.data_ptr() % 16 != 0) == (which == "dst")
    idx = [8, 0, 4, 4, 1]
    assert gather_raw(src.data_ptr(), CODES[dtype], 9, row, idx, dst) == 0
    assert torch.equal(dst.cpu().reshape(5, *shape), reference_rows(x, idx))
    untouched = out[0] if which == "dst" else out[-1]
    assert float(untouched) == -7.0


def test_gather_skips_rows_outside_the_dataset():
    """an index outside [0, n_rows) is neither read nor written (the loaders refuse such lists on the host)"""
    x = host_rows("float32", (5, 7), salt=7300, n=6)
    src = x.cuda()
    dst = torch.full((4, 35), -7.0, dtype=torch.float32, device="cuda")
    assert gather_raw(src.data_ptr(), 0, 6, 35, [2, -1, 6, 5], dst) == 0
    got = dst.cpu()
    assert torch.equal(got[0], x[2].reshape(-1)) and torch.equal(got[3], x[5].reshape(-1))
    assert bool((got[1:3] == -7.0).all())


def test_gather_offsets_beyond_4_gib():
    """70 000 rows of 16 384 fp32 (4.6 GB): the byte offsets of the last rows do not fit 32 bits"""
    n_rows, row = 70000, 16384
    data = torch.empty((n_rows, 128, 128), dtype=torch.float32, device="cuda")
    rows = [0, 32768, 65536, 69999]
    fill = torch.from_numpy(syn.gauss(4 * row, 7400).astype(np.float32).reshape(4, 128, 128))
    for k, r in enumerate(rows):
        data[r] = fill[k].cuda()
    ds = SD.DeviceSyllableDataset.from_arrays(data)
    assert ds.data.data_ptr() == data.data_ptr()
    order = [3, 0, 2, 1, 3]
    got = ds[[rows[k] for k in order]]
    assert torch.equal(got.cpu(), fill[order])
    del ds, data
    torch.cuda.empty_cache()


def test_gather_is_deterministic():
    x = host_rows("float64", (128, 128), salt=7500)
    ds = SD.DeviceSyllableDataset.from_arrays(x)
    idx = index_lists(N_ROWS)["permutation"]
    a, b = ds[idx].clone(), ds[idx].clone()
    assert torch.equal(a, b)


# ---- the pipeline ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return load_golden("sylls.npz")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("sylls"))
    SC.write_dirs(root)
    return root


@pytest.fixture()
def dirs(tree, monkeypatch):
    monkeypatch.chdir(tree)
    return ["audio_0", "audio_1"], ["segs_0", "segs_1"]


def js(g, key):
    return json.loads(str(g[key]))


def golden_rows(golden, name, which):
    key = lambda d, field: ("lin" if name == "stop" and field == "specs" else name) + ".%d.%s" % (d, field)  # noqa: E731
    n = [len(golden[key(d, "onsets")]) for d in which]
    out = {f: np.concatenate([golden[key(d, f)][:k] for d, k in zip(which, n)])
           for f in ("specs", "onsets", "offsets", "audio_filenames")}
    out["groups"] = [len(js(golden, "%s.%d.written.json" % (name, d))) for d in which]
    return out


@pytest.mark.parametrize("name", list(SC.SYLL_SETS))
def test_store_matches_get_spec_and_the_reference(golden, dirs, name):
    audio_dirs, seg_dirs = dirs
    which = SC.SYLL_SETS[name][1]
    p = SC.params(name)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        # a workspace bound that forces several chunks per directory
        need = _lib.load().ava_spec_workspace_bytes(3, int(0.2 * SC.FS), p['nperseg'], p['noverlap'], p['num_freq_bins'],
                                                    p['num_time_bins'], int(p['within_syll_normalize']))
        store = P.syllables_to_device([audio_dirs[d] for d in which], [seg_dirs[d] for d in which], p,
                                      max_workspace_bytes=need)
        whole = P.syllables_to_device([audio_dirs[d] for d in which], [seg_dirs[d] for d in which], p)
    msgs = [str(w.message) for w in caught if str(w.message).startswith("Found segment longer")]
    assert msgs == 2 * [m for d in which for m in js(golden, "%s.%d.warnings.json" % (name, d))]
    want = golden_rows(golden, name, which)
    # rows, order and bookkeeping: exactly the reference's files
    assert store.specs.dtype == torch.float32 and store.specs.is_cuda
    assert tuple(store.specs.shape) == want["specs"].shape and len(store) == len(want["onsets"])
    assert np.array_equal(store.onsets, want["onsets"]) and np.array_equal(store.offsets, want["offsets"])
    assert store.audio_filenames.dtype.kind == 'S' and np.array_equal(store.audio_filenames, want["audio_filenames"])
    spf = p['sylls_per_file']
    assert store.group_dir.tolist() == [k for k, g in enumerate(want["groups"]) for _ in range(g)]
    assert store.group_num.tolist() == [i for g in want["groups"] for i in range(g)]
    assert store.group_of.tolist() == [g for g in range(sum(want["groups"])) for _ in range(spf)]
    assert store.stopped == [name == "stop" and d == 0 for d in which]
    # chunking and batch composition change no bits: get_spec, syllable by syllable
    assert torch.equal(store.specs, whole.specs)
    got = store.specs.cpu().numpy().astype(np.float64)
    for i in range(len(store)):
        fn = store.audio_filenames[i].decode()
        fs, audio = SP._read_wav(fn)
        one, flag = SP.get_spec(store.onsets[i], store.offsets[i], audio, p, fs, target_freqs=SP.target_freqs_of(p))
        assert flag and np.array_equal(one, got[i]), (name, i)
    # the reference's values
    tol = float(golden["spec_tol"])
    err = float(np.abs(got - want["specs"]).max())
    print("%s: max abs err %.3e (spec_tol %.3e)" % (name, err, tol))
    assert err <= tol
    if 0 in which:                       # the segment shorter than nperseg: an all-zero spectrogram, like the reference's
        zero = np.flatnonzero(want["specs"].reshape(len(got), -1).max(1) == 0)
        assert len(zero) == 1 and not got[zero[0]].any() and got.max() > 0.5


def test_get_syll_specs_matches_the_reference(golden, dirs):
    p = SC.params("mel_ts")
    segs = np.array(SC.SYLL_DIRS[0][0][1])
    specs, valid = P.get_syll_specs(segs[:, 0], segs[:, 1], os.path.join("audio_0", "s0_a.wav"), p)
    assert valid == golden["gss.valid"].tolist() and isinstance(specs, list) and len(specs) == len(valid)
    assert all(s.dtype == np.float64 and s.shape == (32, 24) for s in specs)
    assert float(np.abs(np.stack(specs) - golden["gss.specs"]).max()) <= float(golden["spec_tol"])
    assert not specs[1].any() and specs[4].any()               # shorter than nperseg; running past the end of the file


@pytest.mark.parametrize("name", ["lin", "stop"])
def test_process_sylls_writes_the_store_group_by_group(golden, dirs, capsys, name):
    audio_dirs, seg_dirs = dirs
    p = SC.params(name)
    save_dir = "saved_" + name
    P.process_sylls(audio_dirs[0], seg_dirs[0], save_dir, p)
    out = capsys.readouterr().out
    assert out.startswith("Processing audio files in audio_0\n")
    assert out.endswith("\tSaved max_num_syllables (8). Returning.\n" if name == "stop" else "\tDone.\n")
    written = sorted(os.listdir(save_dir))
    assert written == [w[:-5] + ".npz" for w in js(golden, "%s.0.written.json" % name)]
    store = P.syllables_to_device(audio_dirs[:1], seg_dirs[:1], p)
    specs = store.specs.cpu().numpy()
    for g, fn in enumerate(written):
        rows = store.group_of == g
        with np.load(os.path.join(save_dir, fn)) as f:
            assert sorted(f.files) == ["audio_filenames", "offsets", "onsets", "specs"]
            assert f["specs"].dtype == np.float64 and np.array_equal(f["specs"], specs[rows].astype(np.float64))
            assert np.array_equal(f["onsets"], store.onsets[rows]) and np.array_equal(f["offsets"], store.offsets[rows])
            assert np.array_equal(f["audio_filenames"], store.audio_filenames[rows])


# ---- the loaders ----------------------------------------------------------------------------------------------------------
def test_shuffled_epoch_equals_randperm_rows(dirs):
    audio_dirs, seg_dirs = dirs
    store = P.syllables_to_device(audio_dirs, seg_dirs, SC.params("lin"))
    assert len(store) == 12
    ds = SD.DeviceSyllableDataset.from_store(store)
    assert ds.data.data_ptr() == store.specs.data_ptr()
    loader = SD.DeviceSyllableLoader(ds, batch_size=5, shuffle=True, generator=torch.Generator().manual_seed(11))
    want = torch.Generator().manual_seed(11)
    for _ in range(2):
        perm = torch.randperm(12, generator=want)
        batches = [b.clone() for b in loader]
        assert [len(b) for b in batches] == [5, 5, 2] and len(loader) == 3
        assert torch.equal(torch.cat(batches), store.specs[perm.cuda()])
    with pytest.raises(IndexError):
        ds[[0, 12]]


def test_from_arrays_float64_gives_numpy_to_tensor_bits():
    x = host_rows("float64", (5, 7), salt=7600)
    ds = SD.DeviceSyllableDataset.from_arrays(x.numpy())
    assert ds.data.dtype == torch.float64
    batches = list(SD.DeviceSyllableLoader(ds, batch_size=16))
    assert [len(b) for b in batches] == [16, 16, 5]
    want = torch.from_numpy(x.numpy()).type(torch.FloatTensor)
    assert torch.equal(torch.cat([b.cpu() for b in batches]), want)


@pytest.fixture()
def trained_on(dirs):
    """the 128 x 128 set of both directories: files on disk, the store, and both partitions (2 groups : 1 group)"""
    audio_dirs, seg_dirs = dirs
    p = SC.params("train128")
    save_dirs = ["saved128_0", "saved128_1"]
    for a, s, out in zip(audio_dirs, seg_dirs, save_dirs):
        P.process_sylls(a, s, out, p, verbose=False)
    store = P.syllables_to_device(audio_dirs, seg_dirs, p)
    by_file = SD.get_syllable_partition(save_dirs, 0.67)
    by_store = SD.partition_store(store, 0.67, save_dirs=save_dirs)
    return store, by_file, by_store


def test_file_path_and_store_path_select_the_same_rows(trained_on):
    store, by_file, by_store = trained_on
    assert len(by_file['train']) == 2 and len(by_file['test']) == 1
    files = SD.get_syllable_data_loaders(by_file, batch_size=8)
    mem = SD.get_syllable_data_loaders(by_store, batch_size=8)
    for key, n in (('train', 8), ('test', 4)):
        a, b = files[key].dataset, mem[key].dataset
        assert len(a) == len(b) == n and a.data.dtype == torch.float64 and b.data.dtype == torch.float32
        assert torch.equal(a[list(range(n))], b[list(range(n))])
        assert torch.equal(b[list(range(n))], store.specs[torch.from_numpy(by_store[key][1]).cuda()])
    assert files['train'].shuffle and not files['test'].shuffle
    everything = SD.get_syllable_data_loaders(SD.partition_store(store, 1.0), batch_size=8)
    assert everything['test'] is None and len(everything['train'].dataset) == 12
    assert SD.get_syllable_data_loaders({'train': by_file['train'], 'test': []})['test'] is None


@pytest.mark.parametrize("source", ["files", "store"])
def test_vae_epochs_run_over_the_loaders(trained_on, tmp_path, source):
    from ava_amd.vae import VAE
    store, by_file, by_store = trained_on
    loaders = SD.get_syllable_data_loaders(by_file if source == "files" else by_store, batch_size=8, num_workers=3)
    model = VAE(save_dir=str(tmp_path), z_dim=32, device_name="cuda")
    train_loss = model.train_epoch(loaders['train'])
    test_loss = model.test_epoch(loaders['test'])
    assert np.isfinite(train_loss) and np.isfinite(test_loss)
    latent = model.get_latent(loaders['test'])
    assert latent.shape == (4, 32) and np.isfinite(latent).all()
    specs, rec = model.visualize(loaders['test'], num_specs=2)
    assert specs.shape == (2, 128, 128) and np.isfinite(rec).all()
