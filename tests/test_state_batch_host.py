"""CPU-side checks of the batched state transfer (dynenv_get_states / dynenv_set_states / dynenv_error_flags_env): the header declares
the three entry points and the binding lists them, and the numpy view of a state blob (`_capi.state_dtype`, `blobs_as_states`,
`states_as_blobs`) is the C struct byte for byte - every field, pads included, in both directions."""
import ctypes as C

import numpy as np
import pytest

from host_common import built_capi, header_without_comments

NEW = ("dynenv_get_states", "dynenv_set_states", "dynenv_error_flags_env")


@pytest.fixture(scope="module")
def capi():
    return built_capi()


def test_header_declares_the_three_entry_points_and_the_binding_lists_them(capi):
    h = header_without_comments()
    want = {
        "dynenv_get_states": "int dynenv_get_states(dynenv_t* h, const int32_t* env_idx_dev, int32_t n, void* blobs_dev, void* stream);",
        "dynenv_set_states": "int dynenv_set_states(dynenv_t* h, const int32_t* env_idx_dev, int32_t n, const void* blobs_dev, "
                             "int32_t* status_dev, void* stream);",
        "dynenv_error_flags_env": "int dynenv_error_flags_env(dynenv_t* h, int32_t* flags_dev, void* stream);",
    }
    for name in NEW:
        assert want[name] in h, "include/dynenv.h does not declare %s as the issue spells it" % name
        assert name in capi.EXPORTS
    assert "#define DYNENV_ABI_VERSION 3" in h, "additions only: the ABI version stays"
    lib = capi.load()
    for name in NEW:
        assert hasattr(lib, name), "libdynenv_hip.so does not export " + name
    # arguments are checked before any device is looked for: a null handle is an argument error, with or without a GPU
    assert lib.dynenv_get_states(None, None, 1, None, None) == -1
    assert lib.dynenv_set_states(None, None, 1, None, None, None) == -1
    assert lib.dynenv_error_flags_env(None, None, None) == -1


@pytest.mark.parametrize("env_type", [0, 1])
def test_state_dtype_is_the_struct(capi, env_type):
    struct = capi.RoboCupState if env_type == 0 else capi.DrivingState
    dt = capi.state_dtype(env_type)
    assert capi.state_struct(env_type) is struct
    assert dt.itemsize == C.sizeof(struct) == (2552 if env_type == 0 else 3072)
    assert dt == np.dtype(struct)
    for name, _ in struct._fields_:
        assert dt.fields[name][1] == getattr(struct, name).offset, name
    from dynenv_amd import DynEnvType
    assert capi.state_dtype(DynEnvType.DRIVE).itemsize == 3072 and capi.state_dtype(DynEnvType.ROBO_CUP).itemsize == 2552


def _leaves_ctypes(obj, path=()):
    """(path, container, key) of every scalar of a ctypes struct, arrays and nested structs walked in declaration order"""
    if isinstance(obj, C.Structure):
        for name, _ in obj._fields_:
            v = getattr(obj, name)
            if isinstance(v, (C.Structure, C.Array)):
                yield from _leaves_ctypes(v, path + (name,))
            else:
                yield path + (name,), obj, name
    else:
        for i in range(len(obj)):
            v = obj[i]
            if isinstance(v, (C.Structure, C.Array)):
                yield from _leaves_ctypes(v, path + (i,))
            else:
                yield path + (i,), obj, i


def _np_at(rec, path):
    """the element of a numpy structured scalar / array a ctypes path names"""
    v = rec
    for p in path:
        v = v[p]
    return v


def _value(k, sample):
    # distinct per field, exactly representable in either type; doubles get a fraction and a sign so that no int could stand in
    return (k * 7 + 3) * (-1 if k % 3 == 0 else 1) if isinstance(sample, int) else (k + 0.5) * (-1.0 if k % 2 else 1.0)


@pytest.mark.parametrize("env_type", [0, 1])
def test_ctypes_blob_reads_back_through_the_numpy_view_and_back(capi, env_type):
    struct = capi.state_struct(env_type)
    # ctypes -> numpy: every scalar of the struct (pads included) set to its own value
    sts = [struct(), struct()]
    n_leaves = 0
    for s_i, st in enumerate(sts):
        for k, (path, box, key) in enumerate(_leaves_ctypes(st)):
            if isinstance(box, C.Structure):
                setattr(box, key, _value(k + 1000 * s_i, getattr(box, key)))
            else:
                box[key] = _value(k + 1000 * s_i, box[key])
            n_leaves += 1
    assert n_leaves == 2 * (508 if env_type == 1 else 397), "walked %d scalars" % n_leaves
    blobs = capi.states_as_blobs(sts)
    assert blobs.dtype == np.uint8 and blobs.shape == (2, C.sizeof(struct))
    assert blobs[0].tobytes() == bytes(sts[0]) and blobs[1].tobytes() == bytes(sts[1])
    view = capi.blobs_as_states(blobs, env_type)
    assert view.shape == (2,) and view.dtype == capi.state_dtype(env_type) and np.shares_memory(view, blobs)
    for s_i, st in enumerate(sts):
        for k, (path, box, key) in enumerate(_leaves_ctypes(st)):
            got = _np_at(view[s_i], path)
            assert got == _value(k + 1000 * s_i, getattr(box, key) if isinstance(box, C.Structure) else box[key]), (s_i, path)
    assert view.tobytes() == bytes(sts[0]) + bytes(sts[1])
    # one blob, not a batch
    assert capi.blobs_as_states(blobs[1], env_type).tobytes() == bytes(sts[1])
    assert capi.states_as_blobs(sts[0]).tobytes() == bytes(sts[0])
    # numpy -> ctypes: fields edited with numpy land in the bytes the C struct reads
    arr = np.zeros((3,), capi.state_dtype(env_type))
    probe = struct()
    paths = [p for p, _, _ in _leaves_ctypes(probe)]
    for i in range(3):
        for k, path in enumerate(paths):
            box = arr[i]
            for p in path[:-1]:
                box = box[p]
            box[path[-1]] = _value(k + 77 * i, 0 if np.issubdtype(np.asarray(box[path[-1]]).dtype, np.integer) else 0.0)
    back = capi.states_as_blobs(arr)
    assert back.shape == (3, C.sizeof(struct)) and np.shares_memory(back, arr)
    for i in range(3):
        st = struct.from_buffer_copy(back[i].tobytes())
        for k, (path, box, key) in enumerate(_leaves_ctypes(st)):
            v = getattr(box, key) if isinstance(box, C.Structure) else box[key]
            assert v == _value(k + 77 * i, v), (i, path)
        assert bytes(st) == arr[i].tobytes()
    with pytest.raises(ValueError):
        capi.blobs_as_states(np.zeros((2, 100), np.uint8), env_type)
