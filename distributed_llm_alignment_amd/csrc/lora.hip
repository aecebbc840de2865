// LoRA adapter kernels: y = x W^T + s (x A^T) B^T with rank r in {8, 16, 32, 64}.
//
// Both products are skinny (one dimension is r) and bandwidth-bound: the shrink streams x once,
// the expand reads and writes y once. bf16 in and out, fp32 accumulate on
// mfma_f32_16x16x32_bf16, no LDS staging of operands, no float atomics (two launches give
// equal bits), no host sync.
//
// Fragment maps of the instruction (lane l, fr = l & 15, fq = l >> 4):
//   A operand: A[row fr][k = 8 fq + i]      B operand: B[k = 8 fq + i][col fr]      i = 0..7
//   C/D:       D[row 4 fq + reg][col fr]     reg = 0..3
//
// Tails are zero-filled in registers: every load address is clamped to an element inside the
// tensor and the loaded fragment is replaced by zero with a select, so no load is predicated
// (no branch in the k-loop) and nothing is read past a tensor.
#include "common.h"

namespace dla {

namespace {

constexpr int kShrinkWaves = 8;  // K is split across the waves of a block

__device__ __forceinline__ s16x8 load_frag(const bf16_t* p, bool ok) {
  const s16x8 v = *reinterpret_cast<const s16x8*>(p);
  const s16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  return ok ? v : z;
}

// t[m, j] = bf16(scale * sum_k x[m, k] a[j, k]); x [M, K], a [R, K], t [M, R]; R <= 16 CT.
// One block per 16 rows of x. The A fragment is 8 consecutive k of one x row, the B fragment 8
// consecutive k of one a row (16-byte global loads both); one x fragment feeds all CT column
// tiles. Wave w owns the contiguous k-steps [w per, (w + 1) per); the partial tiles meet in LDS
// and are summed in wave order.
template <int CT>
__global__ __launch_bounds__(kShrinkWaves * 64) void lora_shrink_kernel(
    const bf16_t* __restrict__ x, int64_t ldx, const bf16_t* __restrict__ a, int64_t lda,
    bf16_t* __restrict__ t, int64_t ldt, int64_t M, int K, int R, float scale) {
  __shared__ float red[kShrinkWaves][CT][4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int64_t m0 = (int64_t)blockIdx.x * 16;
  const bool mok = m0 + fr < M;
  const bf16_t* xp = x + (mok ? m0 + fr : 0) * ldx;
  const bf16_t* ap[CT];
  bool aok[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    aok[c] = c * 16 + fr < R;
    ap[c] = a + (int64_t)(aok[c] ? c * 16 + fr : 0) * lda;
  }
  f32x4 acc[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nks = (K + 31) / 32;
  const int per = (nks + kShrinkWaves - 1) / kShrinkWaves;
  const int ks0 = min(w * per, nks), ks1 = min(ks0 + per, nks);
  const int full = min(ks1, K / 32);  // k-steps with all 32 k inside the row
  int ks = ks0;
  for (; ks + 4 <= full; ks += 4) {  // four k-steps of loads in flight ahead of their MFMAs
    s16x8 xa[4], ab[4][CT];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = (ks + u) * 32 + fq * 8;
      xa[u] = load_frag(xp + k, mok);
#pragma unroll
      for (int c = 0; c < CT; ++c) ab[u][c] = load_frag(ap[c] + k, aok[c]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int c = 0; c < CT; ++c)
        acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa[u], ab[u][c], acc[c], 0, 0, 0);
  }
  for (; ks < full; ++ks) {
    const int k = ks * 32 + fq * 8;
    const s16x8 xa = load_frag(xp + k, mok);
#pragma unroll
    for (int c = 0; c < CT; ++c)
      acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa, load_frag(ap[c] + k, aok[c]), acc[c], 0, 0, 0);
  }
  if (ks < ks1) {  // the one partial k-step (K % 32 != 0; K % 8 == 0, so a lane is all in or out)
    const int k = ks * 32 + fq * 8;
    const bool kok = k < K;
    const int kc = kok ? k : 0;
    const s16x8 xa = load_frag(xp + kc, mok && kok);
#pragma unroll
    for (int c = 0; c < CT; ++c)
      acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa, load_frag(ap[c] + kc, aok[c] && kok), acc[c], 0, 0, 0);
  }
#pragma unroll
  for (int c = 0; c < CT; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[w][c][r][lane] = acc[c][r];
  __syncthreads();
  // 16 rows x (2 CT) chunks of 8 columns; element (row, col) sits in lane 16 (row / 4) + col % 16,
  // register row % 4 of column tile col / 16
  const int tid = threadIdx.x;
  if (tid < 16 * 2 * CT) {
    const int row = tid / (2 * CT), col0 = (tid % (2 * CT)) * 8;
    if (m0 + row < M && col0 < R) {
      const float* src = &red[0][col0 >> 4][row & 3][(row >> 2) * 16 + (col0 & 15)];
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = 0.f;
#pragma unroll
      for (int ww = 0; ww < kShrinkWaves; ++ww)
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] += src[ww * (CT * 4 * 64) + i];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] *= scale;
      store_bf16x8(t + (m0 + row) * ldt + col0, pack_bf16x8(v));
    }
  }
}

constexpr int kExpandMI = 4;  // 16-token tiles per wave; a block covers 16 * 4 * kExpandMI tokens x 64 n

// y[m, n] = bf16(float(y[m, n]) + scale * sum_j t[m, j] b(n, j)), in place; y [M, N], t [M, R].
// RN = false: b is [N, R] (b(n, j) = b[n ldb + j]); RN = true: b is [R, N] (b(n, j) = b[j ldb + n]).
// The MFMA computes the y^T tile (A operand = b, rows n; B operand = t, columns m), so a lane's
// four accumulator registers are consecutive n of one token. Two tiles are interleaved by rows
// (A row r of tile h holds n = 8 (r / 4) + 4 h + r % 4): lane (fr, fq) then owns n = 8 fq .. 8 fq + 7
// of token fr, one 16-byte access to y. A wave keeps the b fragments of its 64 n in registers and
// walks kExpandMI token tiles, so the small operand (strided 2-byte loads in the RN layout) is
// loaded once per block. KS = ceil(R / 32) k-steps.
template <int KS, bool RN>
__global__ __launch_bounds__(256) void lora_expand_kernel(
    bf16_t* __restrict__ y, int64_t ldy, const bf16_t* __restrict__ t, int64_t ldt,
    const bf16_t* __restrict__ b, int64_t ldb, int64_t M, int N, int R, float scale) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int n_base = blockIdx.y * 64;
  s16x8 bf[2][2][KS];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int n = n_base + 32 * p + 8 * (fr >> 2) + 4 * h + (fr & 3);
        const int j0 = 32 * s + 8 * fq;
        const bool ok = n < N && j0 < R;
        const int nc = ok ? n : 0, jc = ok ? j0 : 0;
        if (RN) {
          s16x8 v;
#pragma unroll
          for (int i = 0; i < 8; ++i) v[i] = (short)b[(int64_t)(jc + i) * ldb + nc];
          const s16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
          bf[p][h][s] = ok ? v : z;
        } else {
          bf[p][h][s] = load_frag(b + (int64_t)nc * ldb + jc, ok);
        }
      }
#pragma unroll
  for (int i = 0; i < kExpandMI; ++i) {
    const int64_t m = (((int64_t)blockIdx.x * kExpandMI + i) * 4 + w) * 16 + fr;
    const bool mok = m < M;
    const int64_t mc = mok ? m : 0;
    f32x4 acc[2][2];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int h = 0; h < 2; ++h) acc[p][h] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int j0 = 32 * s + 8 * fq;
      const bool ok = mok && j0 < R;
      const s16x8 tf = load_frag(t + mc * ldt + (j0 < R ? j0 : 0), ok);
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int h = 0; h < 2; ++h)
          acc[p][h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[p][h][s], tf, acc[p][h], 0, 0, 0);
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int n = n_base + 32 * p + 8 * fq;
      const bool ok = mok && n < N;  // N % 8 == 0: the 8 columns are all in or all out
      bf16_t* yp = y + mc * ldy + (n < N ? n : 0);
      const bf16x8 yv = load_bf16x8(yp);
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = fmaf(scale, acc[p][e >> 2][e & 3], bf2f(yv[e]));
      if (ok) store_bf16x8(yp, pack_bf16x8(o));
    }
  }
}

}  // namespace

void launch_lora_shrink(const bf16_t* x, int64_t ldx, const bf16_t* a, int64_t lda, bf16_t* t,
                        int64_t ldt, int64_t M, int K, int R, float scale, hipStream_t st) {
  if (M == 0) return;
  const unsigned grid = (unsigned)((M + 15) / 16);
  const int th = kShrinkWaves * 64;
  if (R <= 16)
    lora_shrink_kernel<1><<<grid, th, 0, st>>>(x, ldx, a, lda, t, ldt, M, K, R, scale);
  else if (R <= 32)
    lora_shrink_kernel<2><<<grid, th, 0, st>>>(x, ldx, a, lda, t, ldt, M, K, R, scale);
  else
    lora_shrink_kernel<4><<<grid, th, 0, st>>>(x, ldx, a, lda, t, ldt, M, K, R, scale);
}

void launch_lora_expand_add(bf16_t* y, int64_t ldy, const bf16_t* t, int64_t ldt, const bf16_t* b,
                            int64_t ldb, bool rn, int64_t M, int N, int R, float scale,
                            hipStream_t st) {
  if (M == 0 || N == 0) return;
  const int64_t mper = 16 * 4 * kExpandMI;
  dim3 grid((unsigned)((M + mper - 1) / mper), (unsigned)((N + 63) / 64));
  if (R <= 32) {
    if (rn)
      lora_expand_kernel<1, true><<<grid, 256, 0, st>>>(y, ldy, t, ldt, b, ldb, M, N, R, scale);
    else
      lora_expand_kernel<1, false><<<grid, 256, 0, st>>>(y, ldy, t, ldt, b, ldb, M, N, R, scale);
  } else {
    if (rn)
      lora_expand_kernel<2, true><<<grid, 256, 0, st>>>(y, ldy, t, ldt, b, ldb, M, N, R, scale);
    else
      lora_expand_kernel<2, false><<<grid, 256, 0, st>>>(y, ldy, t, ldt, b, ldb, M, N, R, scale);
  }
}

}  // namespace dla
