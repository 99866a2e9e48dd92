"""numpy statement of the arranger's 16-bit CONVERSIONS (include/dynenv.h, dynenv_arrange_*_as: the conversion contract).  A helper module:
no test in here.  16-bit values travel as their bit patterns, uint16 arrays: numpy has no bfloat16, and a bit comparison wants bits.

    float32 -> bf16   round to nearest, ties to even, on the float32's bits u:  (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    float32 -> fp16   numpy's astype(np.float16): IEEE round to nearest even, overflow to infinity, subnormal results, signed zeros
    bf16 -> float32   the bits shifted up by 16: exact
    fp16 -> float32   astype(np.float32): exact, subnormals included
NaN inputs are outside the bit contract (a NaN stays a NaN, its payload is the hardware's): the bf16 formula would even carry a NaN with an
all-ones low mantissa into an infinity.  Callers keep NaN out of what they compare bit for bit.
Held to torch's CPU `.to(torch.bfloat16)` / `.to(torch.float16)` by tests/test_arranger_dtype_ref.py."""
import numpy as np

KINDS = ("bf16", "f16")


def narrow(x, kind):
    """float32 array -> uint16 bits of the same shape"""
    x = np.ascontiguousarray(x, np.float32)
    if kind == "bf16":
        u = x.view(np.uint32).astype(np.uint64)
        return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    assert kind == "f16", kind
    with np.errstate(over="ignore", under="ignore"):
        return x.astype(np.float16).view(np.uint16)


def widen(bits, kind):
    """uint16 bits -> float32 array of the same shape, exact"""
    bits = np.ascontiguousarray(bits, np.uint16)
    if kind == "bf16":
        return (bits.astype(np.uint32) << 16).view(np.float32)
    assert kind == "f16", kind
    return bits.view(np.float16).astype(np.float32)


def is_nan_bits(bits, kind):
    """which 16-bit patterns are NaNs"""
    bits = np.asarray(bits, np.uint16)
    if kind == "bf16":
        return ((bits & 0x7F80) == 0x7F80) & ((bits & 0x007F) != 0)
    return ((bits & 0x7C00) == 0x7C00) & ((bits & 0x03FF) != 0)


def non_nan_patterns(kind):
    """every 16-bit pattern that is not a NaN, ascending: 65536 - 254 for bf16, 65536 - 2046 for fp16"""
    allb = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    return allb[~is_nan_bits(allb, kind)]


def f32(*bit_patterns):
    return np.array(bit_patterns, np.uint32).view(np.float32)


def edge_table():
    """float32 inputs at which a conversion can go wrong, none a NaN: the exact halfway patterns 0x3F808000 (tie, even below: down) and
    0x3F818000 (tie, odd below: up) with their neighbours, the carry of 0x3F7FFFFF into 1.0, the largest finite values and the first to
    overflow in either type (fp16: 65519.99 -> 65504, 65520 -> inf), fp16 subnormal results and their ties, underflow to a signed zero
    (-1e-9 -> -0 in fp16), float32 subnormals (bf16 subnormals), signed zeros and infinities."""
    bits = [0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001, 0x3F7FFFFF, 0x3F7F8000, 0x3F7F7FFF,
            0xBF808000, 0xBF818000, 0xBF7FFFFF,
            0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0x7F7F8000, 0x7F7F0000,                    # float32 max -> bf16 inf; bf16's largest finite
            0x00000001, 0x80000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x00400000, 0x00800000,  # float32 subnormals and the smallest normal
            0x00000000, 0x80000000, 0x7F800000, 0xFF800000,
            0x3F801000, 0x3F803000, 0x3F800FFF, 0x3F801001, 0x3F802FFF, 0x3F803001]        # fp16's halfway patterns around 1.0
    vals = [65504.0, 65519.99, 65520.0, 65536.0, -65519.99, -65520.0, 1e5, -1e5,
            6.103515625e-05, 6.0975551605224609375e-05, 5.9604644775390625e-08, 2.98023223876953125e-08, 2.9802325940409414e-08,
            8.94069671630859375e-08, 1.5e-07, 1e-9, -1e-9, -2.98023223876953125e-08, 3.0e-05, 1.0, -1.0, 0.1, 1.0 / 3.0, 3.14159274101257324]
    t = np.concatenate([f32(*bits), np.array(vals, np.float32)])
    assert not np.isnan(t).any()
    return t
