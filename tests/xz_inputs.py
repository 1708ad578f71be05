"""Payloads of the xz tests (numpy, seeded) and the sizes at which each part
of the decoder can go wrong."""
import numpy as np

from tests import lzo_inputs

WINDOW = 2048  # zc_xz.hip's input window of a wave

KINDS = ("random", "zeros", "text", "halfdup", "period1", "period2", "period3", "period63", "period64", "period65",
         "period300", "alphabet4")

# 0: no block; 63..65: the 64-lane copy step; 272..274: the longest match;
# the input window; the stored chunk's limit
SIZES = (0, 1, 2, 63, 64, 65, 272, 273, 274, WINDOW - 1, WINDOW, WINDOW + 1, 65535, 65536, 65537)

PROPS = ((3, 0, 2), (0, 0, 0), (2, 2, 4), (4, 0, 2), (0, 4, 0), (3, 1, 2))  # the last three need the wide form


def payload(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "zeros":
        return np.zeros(n, dtype=np.uint8)
    if kind == "text":
        return lzo_inputs.text(n, rng)
    if kind == "halfdup":  # random, then the same again: matches at distance n / 2
        h = rng.integers(0, 256, (n + 1) // 2, dtype=np.uint8)
        return np.concatenate([h, h])[:n].copy()
    if kind.startswith("period"):
        p = int(kind[6:])
        unit = rng.integers(0, 256, p, dtype=np.uint8)
        return np.tile(unit, n // p + 1)[:n].copy()
    if kind == "alphabet4":
        return (97 + rng.integers(0, 4, n)).astype(np.uint8)
    raise ValueError(kind)
