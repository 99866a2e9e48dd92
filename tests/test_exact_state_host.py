"""CPU-side checks of the exact state transfer (dynenv_exact_size / dynenv_get_exact / dynenv_set_exact): the header declares the three
entry points, the binding lists them and the library exports them, the ABI version is what it was, and a NULL handle is refused before
any device is looked for."""
import ctypes as C
import re

import pytest

from host_common import ERR_ARG, built_capi, comment_before, header_text, header_without_comments

PROTOTYPES = (
    "size_t dynenv_exact_size(const dynenv_t* h);",
    "int dynenv_get_exact(dynenv_t* h, const int32_t* env_idx_dev, int32_t n, void* blobs_dev, void* stream);",
    "int dynenv_set_exact(dynenv_t* h, const int32_t* env_idx_dev, int32_t n, const void* blobs_dev, int32_t* status_dev, void* stream);",
)
NAMES = ("dynenv_exact_size", "dynenv_get_exact", "dynenv_set_exact")


@pytest.fixture(scope="module")
def capi():
    return built_capi()


def test_header_declares_the_entry_points_and_the_abi_version_stays():
    txt, h = header_text(), header_without_comments()
    for p in PROTOTYPES:
        assert re.sub(r"\s+", " ", p) in h, p
    assert "#define DYNENV_ABI_VERSION 3" in h, "additions only: the ABI version stays"
    # like dynenv_get_state, the entries say that the reference has nothing of the kind
    assert re.search(r"dynenv_get/set_exact\s*<-\s*\(no reference equivalent", txt)
    comment = comment_before("dynenv_exact_size")
    for phrase in ("no reference equivalent", "16-byte aligned", "no host synchronisation, no allocation, no host copy", "captured", "replay",
                   "error bit 6", "0 written, 1 blob rejected, 2 index outside [0, E)"):
        assert phrase in comment, phrase


def test_binding_lists_them_and_the_library_exports_them(capi):
    assert capi.DYNENV_ABI_VERSION == 3
    for name in NAMES:
        assert name in capi.EXPORTS, name
    lib = capi.load()
    for name in NAMES:
        assert hasattr(lib, name), "libdynenv_hip.so does not export " + name
    assert lib.dynenv_abi_version() == 3
    assert lib.dynenv_exact_size.restype == C.c_size_t and lib.dynenv_exact_size.argtypes == [C.c_void_p]
    assert lib.dynenv_get_exact.argtypes == [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    assert lib.dynenv_set_exact.argtypes == [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]


def test_a_null_handle_is_an_argument_error_before_a_device_is_looked_for(capi):
    """with or without a GPU"""
    lib = capi.load()
    assert lib.dynenv_get_exact(None, None, 1, None, None) == ERR_ARG
    assert b"null" in lib.dynenv_last_error()
    assert lib.dynenv_set_exact(None, None, 1, None, None, None) == ERR_ARG
    assert b"null" in lib.dynenv_last_error()
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.dynenv_get_exact(None, None, 0, p, None) == ERR_ARG and lib.dynenv_set_exact(None, p, 4, p, p, None) == ERR_ARG
    assert lib.dynenv_exact_size(None) == 0


def test_the_python_surface_is_there():
    import inspect
    from dynenv_amd import BatchedDynEnv
    assert isinstance(BatchedDynEnv.exact_size, property)
    assert list(inspect.signature(BatchedDynEnv.get_exact).parameters) == ["self", "env_ids", "out"]
    assert list(inspect.signature(BatchedDynEnv.set_exact).parameters) == ["self", "env_ids", "blobs", "episode_step"]
    sig = inspect.signature(BatchedDynEnv.fork)
    assert list(sig.parameters) == ["self", "src_ids", "dst_ids", "exact"] and sig.parameters["exact"].default is False
    assert "contact cache" in BatchedDynEnv.fork.__doc__ and "error word" in BatchedDynEnv.fork.__doc__
