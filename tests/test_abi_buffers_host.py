"""CPU-side checks of the alignment rule of the observation buffers (include/dynenv.h at dynenv_reset, dynenv_step and dynenv_full_obs):
a non-NULL obs_dev / full_dev that is not 16-byte aligned is an argument error of every call that takes one - refused before the
handle is looked at and before a device is looked for, so with or without a GPU -, the error text names the pointer and the rule, and the
header and INTEGRATION.md state it.  tests/test_gpu_abi_buffers.py has the real handle."""
import ctypes as C
import os

import pytest

from host_common import ERR_ARG, ROOT, built_capi, comment_before


@pytest.fixture(scope="module")
def capi():
    return built_capi()


def _calls(lib, h, obs, p):
    """every call that takes an observation buffer, with `obs` in that place and valid-looking pointers everywhere else"""
    return {"dynenv_step": lambda: lib.dynenv_step(h, p, obs, p, p, None),
            "dynenv_step_head": lambda: lib.dynenv_step_head(h, p, None, obs, p, p, None),
            "dynenv_step_masked": lambda: lib.dynenv_step_masked(h, p, p, None, obs, p, p, None),
            "dynenv_reset": lambda: lib.dynenv_reset(h, obs, None),
            "dynenv_reset_masked": lambda: lib.dynenv_reset_masked(h, p, obs, None),
            "dynenv_full_obs": lambda: lib.dynenv_full_obs(h, obs, None)}


CALLS = ("dynenv_step", "dynenv_step_head", "dynenv_step_masked", "dynenv_reset", "dynenv_reset_masked", "dynenv_full_obs")


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("off", [4, 8, 12, 1])
def test_a_misaligned_observation_pointer_is_an_argument_error(capi, call, off):
    """the handle is 4 KiB of zeros that is no handle: the check comes before it is dereferenced (a zeroed handle that WAS looked at would
    send the call on to a device, or crash)"""
    lib = capi.load()
    not_a_handle = (C.c_uint8 * 4096)()
    buf = (C.c_uint8 * 4096)()
    base = (C.addressof(buf) + 255) & ~255
    h, p = C.c_void_p(C.addressof(not_a_handle)), C.c_void_p(base)
    lib.dynenv_step(None, None, None, None, None, None)   # (leaves another text in dynenv_last_error)
    assert b"align" not in lib.dynenv_last_error()
    assert _calls(lib, h, C.c_void_p(base + off), p)[call]() == ERR_ARG
    text = lib.dynenv_last_error().decode()
    assert "16-byte aligned" in text, text
    assert ("full_dev" if call == "dynenv_full_obs" else "obs_dev") in text, text


def test_null_arguments_are_still_refused_first(capi):
    """the NULL checks are what they were: a NULL handle with a misaligned pointer is the NULL handle's error"""
    lib = capi.load()
    buf = (C.c_uint8 * 512)()
    base = (C.addressof(buf) + 255) & ~255
    for name, call in _calls(lib, None, C.c_void_p(base + 4), C.c_void_p(base)).items():
        assert call() == ERR_ARG, name
        assert b"null" in lib.dynenv_last_error(), name


def test_the_header_and_the_integration_guide_state_the_rule():
    for name in ("dynenv_reset", "dynenv_step", "dynenv_full_obs"):
        comment = comment_before(name)
        assert "16-byte aligned" in comment and "DYNENV_ERR_ARG" in comment, name
        assert "nothing is launched" in comment or "nothing launched" in comment, name
    assert "obs_dev" in comment_before("dynenv_step") and "full_dev" in comment_before("dynenv_full_obs")
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "16-byte" in guide and "full_dev" in guide and "DYNENV_ERR_ARG" in guide
    assert "#define DYNENV_ABI_VERSION 3" in open(os.path.join(ROOT, "include", "dynenv.h")).read(), "no struct or signature changed"
