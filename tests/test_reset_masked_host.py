"""CPU-side checks of the per-environment reset (dynenv_reset_masked / BatchedDynEnv.reset_envs): the header declares the entry point,
the library exports it and the binding lists it; its arguments are checked before any device is looked for; and the helper that turns
reset_envs' argument into the device mask (vec_env.reset_mask) does so on CPU tensors."""
import ctypes as C

import numpy as np
import pytest

from host_common import ERR_ARG, built_capi, header_without_comments


@pytest.fixture(scope="module")
def capi():
    return built_capi()


def test_header_declares_the_entry_point_and_the_library_exports_it(capi):
    h = header_without_comments()
    assert "int dynenv_reset_masked(dynenv_t* h, const uint8_t* mask_dev, float* obs_dev, void* stream);" in h
    assert "#define DYNENV_ABI_VERSION 3" in h, "an addition only: the ABI version stays"
    assert "dynenv_reset_masked" in capi.EXPORTS
    lib = capi.load()
    assert hasattr(lib, "dynenv_reset_masked"), "libdynenv_hip.so does not export dynenv_reset_masked"
    assert lib.dynenv_reset_masked.argtypes == [C.c_void_p] * 4


def test_null_handle_and_null_mask_are_argument_errors(capi):
    """both are refused before the handle is looked at or a device is selected: with or without a GPU"""
    lib = capi.load()
    mask = (C.c_uint8 * 4)(1, 0, 1, 0)
    assert lib.dynenv_reset_masked(None, C.cast(mask, C.c_void_p), None, None) == ERR_ARG
    assert lib.dynenv_reset_masked(None, None, None, None) == ERR_ARG
    not_a_handle = (C.c_uint8 * 64)()   # never dereferenced: the NULL mask is refused first
    assert lib.dynenv_reset_masked(C.cast(not_a_handle, C.c_void_p), None, None, None) == ERR_ARG
    assert b"null" in lib.dynenv_last_error()


def test_ids_become_a_mask():
    import torch
    from dynenv_amd.vec_env import reset_mask
    for ids in ([3, 0, 4], (3, 0, 4), np.array([3, 0, 4]), np.array([3, 0, 4], np.int32), torch.tensor([3, 0, 4]),
                torch.tensor([3, 0, 4], dtype=torch.int32), [3, 0, 4, 3, 3, 0]):   # (listed more than once: reset once)
        m = reset_mask(ids, 5)
        assert m.dtype == torch.uint8 and m.is_contiguous() and m.tolist() == [1, 0, 0, 1, 1], ids
    assert reset_mask([], 3).tolist() == [0, 0, 0]
    assert reset_mask(np.zeros((0,), np.int64), 3).tolist() == [0, 0, 0]
    assert reset_mask(range(70), 70).tolist() == [1] * 70
    assert reset_mask([69, 63, 64], 70).nonzero().flatten().tolist() == [63, 64, 69]


def test_a_mask_is_taken_as_it_is():
    import torch
    from dynenv_amd.vec_env import reset_mask
    b = torch.tensor([True, False, False, True, True])
    m = reset_mask(b, 5)
    assert m.dtype == torch.uint8 and m.data_ptr() == b.data_ptr() and m.tolist() == [1, 0, 0, 1, 1], "bool is viewed as uint8: no copy"
    assert reset_mask(np.array([True, False, True]), 3).tolist() == [1, 0, 1]
    strided = torch.zeros((5, 2), dtype=torch.bool)[:, 0]
    assert reset_mask(strided, 5).is_contiguous()


def test_uint8_on_the_host_is_an_id_list_never_a_mask():
    """a uint8 mask is taken from the DEVICE only (`dones`); on the host small integers are ids, whatever their width - a uint8 id list
    of length E must not be read as a mask"""
    import torch
    from dynenv_amd._capi import DynEnvError
    from dynenv_amd.vec_env import reset_mask
    assert reset_mask(np.array([3, 0, 4], np.uint8), 5).tolist() == [1, 0, 0, 1, 1]
    assert reset_mask(np.array([1, 0, 1, 0, 0], np.uint8), 5).tolist() == [1, 1, 0, 0, 0]
    assert reset_mask(torch.tensor([1, 0, 1, 0, 0], dtype=torch.uint8), 5).tolist() == [1, 1, 0, 0, 0]
    with pytest.raises(DynEnvError, match="outside"):
        reset_mask(torch.tensor([1, 0, 7, 0, 0], dtype=torch.uint8), 5)


@pytest.mark.parametrize("bad", [
    [5], [-1], [0, 1, 70], np.array([2 ** 40]),                      # ids outside [0, E)
    "float_ids", "float_mask", "bool_short", "bool_long", "bool_2d", "ids_2d", "int_mask_len",
])
def test_what_is_not_a_mask_or_an_id_list_raises(bad):
    import torch
    from dynenv_amd._capi import DynEnvError
    from dynenv_amd.vec_env import reset_mask
    E = 5
    arg = {"float_ids": [0.5, 1.0], "float_mask": torch.zeros(E), "bool_short": torch.zeros(E - 1, dtype=torch.bool),
           "bool_long": torch.zeros(E + 1, dtype=torch.bool), "bool_2d": torch.zeros((E, 1), dtype=torch.bool),
           "ids_2d": [[0, 1], [2, 3]], "int_mask_len": np.zeros((E + 1,), np.bool_)}.get(bad, bad) if isinstance(bad, str) else bad
    with pytest.raises(DynEnvError, match="reset_envs"):
        reset_mask(arg, E)
