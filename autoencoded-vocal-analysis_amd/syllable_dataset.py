"""Syllable spectrograms served from HBM.

Mirror of the reference's ``ava/models/vae_dataset.py``:

  ``get_syllable_partition``     :21-59, over the ``syllables_*.npz`` files ``preprocess.process_sylls`` writes
  ``DeviceSyllableDataset``      ``SyllableDataset`` (:101-145) with every spectrogram resident on the device
  ``DeviceSyllableLoader``       what ``DataLoader(SyllableDataset(...), batch_size, shuffle)`` is to the epoch loops
  ``get_syllable_data_loaders``  :62-97, same return contract
  ``partition_store``            the same file-level split applied to the groups of a ``preprocess.SyllableStore``

The reference opens an hdf5 file per item, converts the item on the CPU (``numpy_to_tensor``), collates on the CPU and
copies the batch.  Here the dataset is one device array in the dtype it was stored in (float64 for the files the
preprocessing step writes, float32 for a ``SyllableStore``) and a batch is ONE launch: ``ava_gather_rows_f32`` reads
the rows of a shuffled index list and writes the fp32 ``[B, F, T]`` tensor the train step consumes, with the rounding
of ``numpy_to_tensor``.  The index list of a batch is validated on the host and travels through the page-locked ring
of ``spec``; nothing synchronises.

DEVIATION: the files are ``.npz``, not ``.hdf5`` (see ``preprocess``).  There is no CPU fallback.
"""
import os

import numpy as np
import torch

from . import _lib
from .feed import _CAST
from .spec import _index_list, _staging

__all__ = ["get_syllable_partition", "partition_store", "DeviceSyllableDataset", "DeviceSyllableLoader",
           "get_syllable_data_loaders", "get_npzs_from_dir", "install"]


def _is_npz_file(filename):
    """the reference's ``_is_hdf5_file`` (models/utils.py:449-451) for the other suffix"""
    return len(filename) > 4 and filename[-4:] == '.npz'


def get_npzs_from_dir(dir):
    """models/utils.py:421-430: the sorted syllable files of a directory"""
    return [os.path.join(dir, f) for f in sorted(os.listdir(dir)) if _is_npz_file(f)]


def _split(filenames, split, shuffle, max_num_files):
    """vae_dataset.py:49-59 on a list of names: (train, test)"""
    assert split > 0.0 and split <= 1.0
    filenames = sorted(filenames)
    if shuffle:
        np.random.seed(42)
        np.random.shuffle(filenames)
        np.random.seed(None)
    if max_num_files is not None:
        filenames = filenames[:max_num_files]
    index = int(round(split * len(filenames)))
    return filenames[:index], filenames[index:]


def get_syllable_partition(dirs, split, shuffle=True, max_num_files=None):
    """Mirror of vae_dataset.py:21-59: ``{'train': [...], 'test': [...]}``, a reproducible split of the
    ``.npz`` syllable files of ``dirs``."""
    assert split > 0.0 and split <= 1.0
    filenames = []
    for dir in dirs:
        filenames += get_npzs_from_dir(dir)
    train, test = _split(filenames, split, shuffle, max_num_files)
    return {'train': train, 'test': test}


def partition_store(store, split, shuffle=True, max_num_files=None, save_dirs=None):
    """``get_syllable_partition`` applied to the groups of a ``preprocess.SyllableStore``: the groups are split by the
    names their files would have (``store.group_names(save_dirs)``), so ``{'train': (store, rows), 'test': (store,
    rows)}`` holds the very syllables, in the same order, as the lists ``get_syllable_partition`` returns for the
    directories ``process_sylls`` wrote them to.  Give those directories as ``save_dirs`` (one per audio directory) when
    their names do not sort in the order of the audio directories."""
    names = store.group_names(save_dirs)
    group = {name: g for g, name in enumerate(names)}
    out = {}
    for key, part in zip(('train', 'test'), _split(names, split, shuffle, max_num_files)):
        rows = [np.flatnonzero(store.group_of == group[name]) for name in part]
        out[key] = (store, np.concatenate(rows + [np.zeros(0, dtype=np.int64)]).astype(np.int64))
    return out


class DeviceSyllableDataset:
    """``SyllableDataset`` (vae_dataset.py:101-145) with the spectrograms resident in HBM.

    ``DeviceSyllableDataset(filenames)`` reads the ``specs`` of a list of ``.npz`` files (``sylls_per_file`` and
    ``transform`` are accepted and ignored: the items already are what ``numpy_to_tensor`` + ``.to(device)`` produce);
    ``from_store`` serves rows of a ``preprocess.SyllableStore`` without a copy; ``from_arrays`` uploads an ``[N, F, T]``
    array of float32, float64, uint8, float16 or bfloat16 as it is.  ``dataset[i]`` is an fp32 device tensor ``[F, T]``,
    ``dataset[iterable]`` one fp32 device tensor ``[n, F, T]`` (the reference returns a list of CPU tensors), cast by
    the gather kernel bit for bit as ``numpy_to_tensor`` casts."""

    def __init__(self, filenames, sylls_per_file=None, transform=None, device="cuda"):
        specs = []
        for fn in filenames:
            with np.load(fn) as f:
                specs.append(f['specs'])
        if not specs:
            raise ValueError("no syllable files")
        self._setup(torch.from_numpy(np.ascontiguousarray(np.concatenate(specs))), None, device)
        self.filenames = filenames
        self.sylls_per_file = sylls_per_file
        self.transform = transform

    @classmethod
    def from_arrays(cls, specs, device="cuda"):
        self = cls.__new__(cls)
        if not torch.is_tensor(specs):
            specs = torch.from_numpy(np.ascontiguousarray(specs))
        self._setup(specs, None, device)
        return self

    @classmethod
    def from_store(cls, store, rows=None):
        self = cls.__new__(cls)
        self._setup(store.specs, rows, store.specs.device)
        self.store = store
        return self

    def _setup(self, data, rows, device):
        if data.dim() != 3:
            raise ValueError("expected [N,F,T] spectrograms, got %s" % (tuple(data.shape),))
        if data.dtype not in _CAST:
            raise TypeError("unsupported spectrogram dtype %s" % data.dtype)
        self.device = torch.device(device)
        self.data = data.contiguous().to(self.device)          # raw: no element is converted on the host
        self.code = _CAST[data.dtype][0]
        self.rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        if self.rows is not None and self.rows.size and (self.rows.min() < 0 or self.rows.max() >= data.shape[0]):
            raise IndexError("row index out of range")
        self.filenames = None
        self.sylls_per_file = None
        self.transform = None

    def __len__(self):
        return int(self.data.shape[0]) if self.rows is None else int(self.rows.size)

    @property
    def item_shape(self):
        return tuple(self.data.shape[1:])

    def source_rows(self, index):
        """the rows of ``self.data`` behind the items ``index``, as int64; ``IndexError`` for an item outside
        ``[0, len)`` (host check, before anything is launched)"""
        idx = np.ascontiguousarray(index, dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= len(self)):
            bad = idx[(idx < 0) | (idx >= len(self))][0]
            raise IndexError("syllable index %d out of range for a dataset of %d" % (int(bad), len(self)))
        return idx if self.rows is None else self.rows[idx]

    def gather(self, index, out=None):
        """fp32 ``[len(index), F, T]`` of the items ``index`` (repeats and any order allowed): one upload of the index
        list out of the page-locked ring and one ``ava_gather_rows_f32`` launch on the current stream, no
        synchronisation.  ``out``: an fp32 device tensor with room for the batch."""
        rows = self.source_rows(index)
        n = int(rows.size)
        if n == 0:
            raise ValueError("empty batch")
        F, T = self.item_shape
        if out is None:
            out = torch.empty((n, F, T), dtype=torch.float32, device=self.device)
        elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < n * F * T:
            raise ValueError("out must be a contiguous fp32 tensor with room for the batch")
        slot = _staging(self.device, 8 * n)
        slot[0][:8 * n].numpy().view(np.int64)[:] = rows
        d_idx = slot[0][:8 * n].to(self.device, non_blocking=True)
        if slot[1] is not None:
            slot[1].record()
        rc = _lib.load().ava_gather_rows_f32(self.data.data_ptr(), self.code, self.data.shape[0], F * T,
                                             d_idx.data_ptr(), n, out.data_ptr(), _lib.stream())
        _lib.check(rc, "ava_gather_rows_f32")
        return out.view(-1)[:n * F * T].view(n, F, T)

    def __getitem__(self, index):
        index, single_index = _index_list(index)
        out = self.gather(index)
        return out[0] if single_index else out


class DeviceSyllableLoader:
    """What ``DataLoader(SyllableDataset(...), batch_size, shuffle)`` is to the epoch loops (vae_dataset.py:89-96): the
    items of a ``DeviceSyllableDataset`` in batches of ``batch_size`` (ragged last batch kept), in the order of
    ``torch.randperm(n, generator=generator)`` drawn per epoch with ``shuffle`` (as ``feed.PinnedBatchLoader``), as fp32
    ``[batch, F, T]`` tensors already on the device (``device_resident``: ``VAE._feed`` hands them through).

    Every batch is one gather launch on the current stream into one of ``depth`` rotating output buffers: a batch stays
    valid until ``depth - 1`` further batches have been drawn."""
    device_resident = True

    def __init__(self, dataset, batch_size=64, shuffle=False, generator=None, depth=4):
        self.dataset = dataset
        self.batch_size = int(batch_size)
        self.shuffle = bool(shuffle)
        self.generator = generator
        self.depth = max(2, int(depth))
        self._out = None

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def order(self):
        """the item order of the next epoch (consumes the generator like an epoch does)"""
        n = len(self.dataset)
        return torch.randperm(n, generator=self.generator).tolist() if self.shuffle else list(range(n))

    def __iter__(self):
        n = len(self.dataset)
        order = self.order()
        if n == 0:
            return
        if self._out is None:
            self._out = [torch.empty((self.batch_size,) + self.dataset.item_shape, dtype=torch.float32,
                                     device=self.dataset.device) for _ in range(self.depth)]
        for k, start in enumerate(range(0, n, self.batch_size)):
            yield self.dataset.gather(order[start:start + self.batch_size], out=self._out[k % self.depth])


def _dataset_of(part, device):
    if isinstance(part, tuple):
        store, rows = part
        return DeviceSyllableDataset.from_store(store, rows)
    return DeviceSyllableDataset(part, device=device)


def get_syllable_data_loaders(partition, batch_size=64, shuffle=(True, False), num_workers=4, device="cuda"):
    """Mirror of vae_dataset.py:62-97: ``{'train': loader, 'test': loader or None}`` (``None`` when the partition's test
    part is empty).  The values of ``partition`` are lists of ``.npz`` file names (``get_syllable_partition``) or
    ``(store, row_indices)`` pairs (``partition_store``).  ``num_workers`` is accepted and ignored: there are no CPU
    workers."""
    train = DeviceSyllableLoader(_dataset_of(partition['train'], device), batch_size=batch_size, shuffle=shuffle[0])
    test_part = partition['test']
    if (isinstance(test_part, tuple) and len(test_part[1]) == 0) or (not isinstance(test_part, tuple) and not test_part):
        return {'train': train, 'test': None}
    test = DeviceSyllableLoader(_dataset_of(test_part, device), batch_size=batch_size, shuffle=shuffle[1])
    return {'train': train, 'test': test}


def install(module=None):
    """Point ``SyllableDataset``, ``get_syllable_partition`` and ``get_syllable_data_loaders`` of ``module`` (by
    default ``ava.models.vae_dataset``; the reference module imports h5py at import time, so a module object may be
    passed instead) at this module."""
    if module is None:
        import ava.models.vae_dataset as module
    module.SyllableDataset = DeviceSyllableDataset
    module.get_syllable_partition = get_syllable_partition
    module.get_syllable_data_loaders = get_syllable_data_loaders
    return module
