"""Placed MXFP4 quantiser cases shared by test_mxfp4_cpu.py and test_mxfp4_decode_gpu.py. Expected
codes and scale bytes are written out by hand from the format (e2m1 magnitudes 0, .5, 1, 1.5, 2, 3,
4, 6 = codes 0..7, sign = 8; E8M0 byte b = e + 127, e = clamp(floor(log2 amax) - 2, +-120))."""
import torch

# (value, code) per 32-block, zero-padded; then the block's scale byte
TIES = [(0.0, 0), (0.5, 1), (1.0, 2), (1.5, 3), (2.0, 4), (3.0, 5), (4.0, 6), (6.0, 7),           # every magnitude
        (0.25, 0), (0.75, 2), (1.25, 2), (1.75, 4), (2.5, 4), (3.5, 6), (5.0, 6),                  # every tie: even code
        (-1.5, 11), (-0.25, 8), (-5.0, 14), (0.3125, 1), (5.5, 7)]
PLACED = [
    (TIES, 127),                                           # amax 6 = 1.5 * 2^2: e = 0
    ([(60.0, 7), (-60.0, 15), (8.0, 2)], 130),             # amax 60: e = 3, 60 / 8 = 7.5 in (6, 8) saturates
    ([], 127),                                             # all-zero block
    ([(0.125, 6), (-0.0625, 12)], 122),                    # amax 2^-3, an exact power of two: e = -5
    ([(2.0 ** -125, 0)], 7),                               # e = -127 clamps to -120: 2^-5 rounds to 0
    ([(2.0 ** 125, 7), (2.0 ** 120, 2)], 247),             # e = 123 clamps to 120: 2^5 saturates
]


def placed_row():
    x, codes = torch.zeros(32 * len(PLACED)), torch.zeros(32 * len(PLACED), dtype=torch.uint8)
    for b, (vals, _) in enumerate(PLACED):
        for i, (v, c) in enumerate(vals):
            x[32 * b + i], codes[32 * b + i] = v, c
    packed = codes.view(-1, 2)[:, 0] | (codes.view(-1, 2)[:, 1] << 4)  # element 2j in the low nibble
    return x, packed, torch.tensor([b for _, b in PLACED], dtype=torch.uint8)
