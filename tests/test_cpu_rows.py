"""CPU-side tests (no GPU needed) of the host path that the analysis modules share: ``_rows`` (dtype rule, finite
checks, upload) and the ABI conventions of ``_lib`` (dtype codes, workspaces)."""
import numpy as np
import pytest
import torch

from ava_amd import _lib, _rows

CPU = torch.device("cpu")
VALUES = np.array([[0.0, 1.0, -2.0], [3.0, 0.0, 1.0]])         # exact in every dtype below (bool: their truth values)


@pytest.mark.parametrize("dtype", ["float32", "float64", "float16", "int16", "bool"])
def test_native_keeps_float32_and_float64_and_converts_the_rest(dtype):
    a = VALUES.astype(dtype)
    for x in (a, torch.from_numpy(a)):
        got = _rows.native(x)
        if dtype in ("float32", "float64"):
            assert got is x
        else:
            assert type(got) is type(x) and got.dtype == (torch.float64 if torch.is_tensor(x) else np.float64)
            assert np.array_equal(np.asarray(got), a.astype(np.float64))
    assert _rows.native(a.tolist()).dtype == (np.float64)                 # a nested list is an array first


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_finite_checks_agree_between_numpy_and_tensor(dtype):
    clean = VALUES.astype(dtype)
    with_nan, with_inf = clean.copy(), clean.copy()
    with_nan[1, 2], with_inf[0, 1] = np.nan, -np.inf
    for a, finite, nan in ((clean, True, False), (with_nan, False, True), (with_inf, False, False)):
        for x in (a, torch.from_numpy(a)):
            assert _rows.is_finite(x) is finite and _rows.has_nan(x) is nan


def test_upload_gives_contiguous_rows_of_equal_values():
    a = np.arange(24, dtype=np.float64).reshape(4, 6)
    forms = [np.asfortranarray(a), torch.from_numpy(a.T.copy()).t(), a[::2, 1::2], torch.from_numpy(a)[::2, 1::2]]
    wants = [a, a, a[::2, 1::2], a[::2, 1::2]]
    assert not any(f.is_contiguous() if torch.is_tensor(f) else f.flags.c_contiguous for f in forms)
    for form, want in zip(forms, wants):
        got = _rows.upload(form, CPU)
        assert torch.is_tensor(got) and got.is_contiguous() and got.dtype == torch.float64 and got.device == CPU
        assert np.array_equal(got.numpy(), want)
    t = torch.from_numpy(a)
    assert _rows.upload(t, CPU) is t                                      # nothing to do: nothing is copied
    got = _rows.upload(np.asfortranarray(a), CPU, torch.float32)
    assert got.dtype == torch.float32 and got.is_contiguous() and np.array_equal(got.numpy(), a.astype(np.float32))


def test_dtype_code():
    for dtype, code in ((torch.float32, 0), (torch.float64, 1), (np.dtype(np.float32), 0), (np.dtype(np.float64), 1)):
        assert _lib.dtype_code(dtype) == code
    assert _lib.dtype_code(torch.zeros(2, dtype=torch.float32)) == 0 and _lib.dtype_code(torch.zeros(2).double()) == 1
    assert _lib.dtype_code(np.zeros(2, dtype=np.float32)) == 0 and _lib.dtype_code(np.zeros(2)) == 1
    for other in (torch.float16, torch.bfloat16, torch.int64, torch.bool, np.dtype(np.float16), np.dtype(np.int32),
                  torch.zeros(2, dtype=torch.int16), np.zeros(2, dtype=np.uint8)):
        with pytest.raises(_lib.AvaHipError, match="float32 or float64"):
            _lib.dtype_code(other)


def test_workspace():
    with pytest.raises(ValueError, match=r"^unsupported shape: N = 3, d = 0$"):
        _lib.workspace(0, CPU, "N = 3, d = 0")
    ws = _lib.workspace(256, CPU, "N = 3, d = 1")
    assert ws.dtype == torch.uint8 and ws.numel() == 256 and ws.device == CPU
