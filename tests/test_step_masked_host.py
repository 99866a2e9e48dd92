"""CPU-side checks of the masked step (dynenv_step_masked / BatchedDynEnv.step_flat(active=...)): the header declares the entry point,
the library exports it and the binding lists it; a NULL handle or mask is refused before any device is looked for; vec_env.reset_mask
names its caller in its errors and reset_envs' messages are what they were; and `active` on a lock-step handle raises before anything
is touched."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from host_common import ERR_ARG, built_capi, comment_before, header_without_comments

PROTOTYPE = """int dynenv_step_masked(dynenv_t* h, const uint8_t* mask_dev, const int32_t* actions_dev, const double* head_dev,
                       float* obs_dev, double* rewards_dev, uint8_t* dones_dev, void* stream);"""


@pytest.fixture(scope="module")
def capi():
    return built_capi()


def test_header_declares_the_entry_point_and_the_library_exports_it(capi):
    h = header_without_comments()
    assert re.sub(r"\s+", " ", PROTOTYPE) in h
    assert "#define DYNENV_ABI_VERSION 3" in h, "an addition only: the ABI version stays"
    assert capi.DYNENV_ABI_VERSION == 3
    assert "dynenv_step_masked" in capi.EXPORTS
    lib = capi.load()
    assert hasattr(lib, "dynenv_step_masked"), "libdynenv_hip.so does not export dynenv_step_masked"
    assert lib.dynenv_step_masked.argtypes == [C.c_void_p] * 8
    assert lib.dynenv_abi_version() == 3
    # its comment says what the issue asks of it
    comment = comment_before("dynenv_step_masked")
    for phrase in ("LISTED", "UNLISTED", "not read", "no host synchronisation, no allocation, no host copy", "Capturable", "replay"):
        assert phrase in comment, phrase


def test_null_handle_and_null_mask_are_argument_errors(capi):
    """both are refused before the handle is looked at or a device is selected: with or without a GPU"""
    lib = capi.load()
    mask = (C.c_uint8 * 4)(1, 0, 1, 0)
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.dynenv_step_masked(None, C.cast(mask, C.c_void_p), p, None, p, p, p, None) == ERR_ARG
    assert lib.dynenv_step_masked(None, None, None, None, None, None, None, None) == ERR_ARG
    not_a_handle = (C.c_uint8 * 64)()   # never dereferenced: the NULL mask is refused first
    assert lib.dynenv_step_masked(C.cast(not_a_handle, C.c_void_p), None, p, None, p, p, p, None) == ERR_ARG
    assert b"null" in lib.dynenv_last_error()
    # the unmasked calls are the same call without a mask: their NULL checks are what they were
    assert lib.dynenv_step(None, p, p, p, p, None) == ERR_ARG
    assert lib.dynenv_step_head(None, p, None, p, p, p, None) == ERR_ARG


BAD = {"outside": [5], "float_ids": [0.5, 1.0], "ids_2d": [[0, 1], [2, 3]], "bool_short": np.zeros((4,), np.bool_)}


@pytest.mark.parametrize("bad", sorted(BAD))
def test_reset_mask_names_its_caller(bad):
    from dynenv_amd._capi import DynEnvError
    from dynenv_amd.vec_env import reset_mask
    with pytest.raises(DynEnvError) as step_err:
        reset_mask(BAD[bad], 5, what="step_flat")
    with pytest.raises(DynEnvError) as reset_err:
        reset_mask(BAD[bad], 5)
    assert str(step_err.value).startswith("step_flat: ") and "reset_envs" not in str(step_err.value)
    assert str(reset_err.value).startswith("reset_envs: "), "reset_envs' messages are unchanged"
    assert str(step_err.value)[len("step_flat: "):] == str(reset_err.value)[len("reset_envs: "):]
    assert inspect.signature(reset_mask).parameters["what"].default == "reset_envs"
    assert reset_mask([3, 0, 4], 5, what="step_flat").tolist() == [1, 0, 0, 1, 1]


def test_reset_envs_messages_are_what_they_were():
    from dynenv_amd._capi import DynEnvError
    from dynenv_amd.vec_env import reset_mask
    for arg, text in (([5], "reset_envs: environment id 5 outside [0, 5)"), ([0.5], "reset_envs: environment ids must be integers, got float64"),
                      ([[0, 1], [2, 3]], "reset_envs: expected a list of environment ids, got shape (2, 2)"),
                      (np.zeros((4,), np.bool_), "reset_envs: the mask must be [5], got shape (4,)")):
        with pytest.raises(DynEnvError) as err:
            reset_mask(arg, 5)
        assert str(err.value) == text


def test_active_on_a_lock_step_handle_raises_before_anything_is_touched():
    """(as far as it goes without a device: a handle object that was never created - the check comes before the first use of it;
    tests/test_gpu_step_masked.py has the real handle)"""
    import torch
    from dynenv_amd import BatchedDynEnv
    from dynenv_amd._capi import DynEnvError
    sig = inspect.signature(BatchedDynEnv.step_flat)
    assert list(sig.parameters) == ["self", "actions", "auto_reset", "validate", "active"] and sig.parameters["active"].default is None
    env = object.__new__(BatchedDynEnv)
    env.closed, env._h = True, None
    env._needs_reset, env.per_env, env._torch = False, False, torch
    with pytest.raises(DynEnvError, match="per_env"):
        env.step_flat(None, auto_reset=False, active=[0])
    assert "stale" in re.sub(r"\s+", " ", BatchedDynEnv.step_flat.__doc__).lower(), "the docstring states the stale-rows contract"
