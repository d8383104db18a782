"""bf16 rounding oracle of the bf16 inference tests: round to nearest even, as usc_cast_bf16 and
usc_spconv_pack_w_bf16 round (csrc/spconv_bf16.hip)."""
import numpy as np


def bf16_bits(a) -> np.ndarray:
    """float32 values -> the uint16 bf16 bit patterns (round to nearest even; a NaN stays a quiet NaN)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    r = np.where(nan, (u >> 16) | 0x40, r)
    return r.astype(np.uint16)


def bf16_round(a) -> np.ndarray:
    """float32 values -> float32 values that are exactly the bf16-rounded ones."""
    return (bf16_bits(a).astype(np.uint32) << 16).view(np.float32)
