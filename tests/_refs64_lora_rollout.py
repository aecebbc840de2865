"""Input builders and the fp64 formula for the LoRA-merged decode weight tests
(test_lora_rollout_cpu.py, test_lora_rollout_gpu.py). Nothing here imports the package.

    m = bf16(w + s b a)        w [N, K], a [R, K], b [N, R]        (fp64 here, un-rounded)
    v = nw ? bf16(m * nw) : m

Exact-integer builder (on the builders of _refs64_lora): w in [-64, 64], b in [-2, 2], a the
asymmetric {-1, 0, 1} pattern, nw in {1, 2, 0.5, -1}. Every partial sum of b a is an integer of
magnitude <= 2 R <= 128, exact in fp32 whatever the summation order; s b a (s = 2 or 0.5) and
w + s b a are then exact in fp32 too (integers or half-integers far below 2^24), so the one bf16
rounding of m is the rounding of the exact value, the same in the kernel and in fp64 -> bf16.
"""
import torch

import _refs64_lora as RL

F64 = torch.float64
BF16 = torch.bfloat16
NW_VALUES = (1.0, 2.0, 0.5, -1.0)


def merged64(w, a, b, scale):
    return RL.d(w) + float(scale) * (RL.d(b) @ RL.d(a))


def exact_case(N, K, R, seed=0, with_nw=False):
    w = RL._ints((N, K), -64, 64, seed + 11).to(BF16)
    b = RL._ints((N, R), -2, 2, seed + 12).to(BF16)
    a = RL._pattern(R, K).to(BF16)
    nw = None
    if with_nw:
        idx = torch.randint(0, len(NW_VALUES), (K,), generator=RL.gen(seed + 13))
        nw = torch.tensor(NW_VALUES)[idx].to(BF16)
    return w, a, b, nw


def random_case(N, K, R, seed=0, with_nw=False):
    w = RL.rand_bf16((N, K), seed * 13 + 1)
    a = RL.rand_bf16((R, K), seed * 13 + 2, amp=K ** -0.5)
    b = RL.rand_bf16((N, R), seed * 13 + 3, amp=R ** -0.5)
    nw = (1.0 + 0.25 * torch.randn(K, generator=RL.gen(seed * 13 + 4))).to(BF16) if with_nw else None
    return w, a, b, nw


def untile(t):
    """[N/16, K/32, 4, 16, 8] (tile, k-block, 8-column group, row, column) -> [N, K]."""
    T, KB = t.shape[0], t.shape[1]
    return t.permute(0, 3, 1, 2, 4).reshape(T * 16, KB * 32)
