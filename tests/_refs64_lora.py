"""Plain fp64 references and input builders for the LoRA adapter tests (test_lora_cpu.py,
test_lora_gpu.py). Nothing here imports the package.

    shrink:  t = bf16(s * x A^T)                      x [M, K], A [R, K]
    expand:  y = bf16(y0 + t B^T)                     y0 [M, N], t [M, R], B [N, R]
    full:    y = y0 + s (x A^T) B^T,  y0 = x W^T + bias | resid + x W^T

The references return un-rounded fp64 (the check adds one bf16 ulp for a bf16 output). In the
gradients the bf16 rounding of t and of dts = s dy B is the identity, as in the kernels' autograd
function, so they are the plain derivatives of the full formula with a frozen W:

    dx = dy W + dts A,   dA = dts^T x,   dB = dy^T t,   d resid = dy,   dts = s dy B,   t = s x A^T

Exact-integer builder: x, t in {-2..2}, A, B in {-1, 0, 1}, y0 in {-64..64}, K, R <= 64. Every
partial sum is an integer of magnitude <= 2 * 64 = 128 and every result of magnitude
<= 64 + 128 = 192 < 256, so each value is exact in fp32 and in bf16 (8 significand bits hold every
integer up to 256) whatever the summation order. The A / B patterns are asymmetric in (row, k):
a row/column swap or a permuted k changes the result.
"""
import torch

F64 = torch.float64
BF16 = torch.bfloat16
EPS32 = 2.0 ** -23


def gen(seed):
    return torch.Generator().manual_seed(int(seed))


def d(x):
    return x.detach().to(F64)


# ------------------------------------------------------------------------------ formulas
def shrink64(x, a, scale):
    return float(scale) * (d(x) @ d(a).t())


def expand64(y0, t, b, scale=1.0):
    """b as [N, R]."""
    return d(y0) + float(scale) * (d(t) @ d(b).t())


def full64(x, w, a, b, scale, bias=None, resid=None):
    y0 = d(x) @ d(w).t()
    if bias is not None:
        y0 = y0 + d(bias)
    if resid is not None:
        y0 = y0 + d(resid)
    return y0 + (float(scale) * (d(x) @ d(a).t())) @ d(b).t()


def full_grads64(x, w, a, b, scale, dy):
    """Gradients of full64 for the output gradient dy (all 2-D); W frozen."""
    x, w, a, b, dy = d(x), d(w), d(a), d(b), d(dy)
    t = float(scale) * (x @ a.t())
    dts = float(scale) * (dy @ b)
    return {"dx": dy @ w + dts @ a, "dA": dts.t() @ x, "dB": dy.t() @ t, "dresid": dy, "dbias": dy.sum(0)}


# ------------------------------------------------------------------------------ random inputs
def rand_bf16(shape, seed, amp=1.0):
    return (torch.randn(shape, generator=gen(seed), dtype=torch.float32) * amp).to(BF16)


def shrink_case(M, K, R, seed=0):
    x = rand_bf16((M, K), seed * 7 + 1)
    a = rand_bf16((R, K), seed * 7 + 2, amp=K ** -0.5)
    return x, a


def expand_case(M, N, R, seed=0):
    y0 = rand_bf16((M, N), seed * 7 + 3)
    t = rand_bf16((M, R), seed * 7 + 4)
    b = rand_bf16((N, R), seed * 7 + 5, amp=R ** -0.5)
    return y0, t, b


def full_case(M, K, N, R, seed=0, with_bias=False, with_resid=False):
    x = rand_bf16((M, K), seed * 11 + 1)
    w = rand_bf16((N, K), seed * 11 + 2, amp=K ** -0.5)
    a = rand_bf16((R, K), seed * 11 + 3, amp=K ** -0.5)
    b = rand_bf16((N, R), seed * 11 + 4, amp=R ** -0.5)
    dy = rand_bf16((M, N), seed * 11 + 5)
    bias = rand_bf16((N,), seed * 11 + 6) if with_bias else None
    resid = rand_bf16((M, N), seed * 11 + 7) if with_resid else None
    return {"x": x, "w": w, "a": a, "b": b, "dy": dy, "bias": bias, "resid": resid}


def dot_extra(K, abs_dot_max):
    """The standard fp32 bound for one dot product of K terms summed in a different order:
    |fl(sum) - sum| <= gamma_K * sum |x_k| |a_k| with gamma_K = K eps / (1 - K eps) (Higham,
    Accuracy and Stability of Numerical Algorithms, section 3.1); eps = 2^-24 is the unit
    round-off of fp32. `abs_dot_max` = max over outputs of sum_k |x_k| |a_k|."""
    u = 2.0 ** -24
    return K * u / (1.0 - K * u) * float(abs_dot_max)


def abs_dot_max(p, q):
    """max_{i, j} sum_k |p[i, k]| |q[j, k]| in fp64."""
    return (d(p).abs() @ d(q).abs().t()).max().item()


# ------------------------------------------------------------------------------ exact integers
def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=gen(seed)).to(torch.float32)


def _pattern(rows, cols):
    """{-1, 0, 1} entries depending asymmetrically on (row, col):
    (2 row + 3 col + row * col // 3 + col // 8) % 3 - 1 (the col // 8 term differs between the 8-element
    fragments of a k-step), then the first row set to 1 and the first column to -1, so a transposed
    or permuted read changes the sums."""
    r = torch.arange(rows).view(-1, 1)
    c = torch.arange(cols).view(1, -1)
    p = ((2 * r + 3 * c + (r * c) // 3 + (c // 8)) % 3 - 1).to(torch.float32)
    p[0, :] = 1.0
    p[:, 0] = -1.0
    return p


def exact_shrink_case(M, K, R, seed=0):
    assert K <= 64 and R <= 64
    return _ints((M, K), -2, 2, seed + 1).to(BF16), _pattern(R, K).to(BF16)


def exact_expand_case(M, N, R, seed=0):
    assert R <= 64
    y0 = _ints((M, N), -64, 64, seed + 2).to(BF16)
    t = _ints((M, R), -2, 2, seed + 3).to(BF16)
    return y0, t, _pattern(N, R).to(BF16)
