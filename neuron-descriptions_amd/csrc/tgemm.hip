// The strided exact-fp32 GEMM (v_mfma_f32_16x16x4_f32) of tgemm.h and the ordered column
// sums.  Determinism: every output element is reduced in a fixed order.  A split-K GEMM
// writes its partial sums to the caller's scratch and a combine kernel adds them in split
// order; the column sums are ordered loops.  No float atomics.
#include "tgemm.h"

namespace milan {
namespace tgemm {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// C(m, n) = sum_k A(m, k) B(k, n) [+ D(m, n)] [+ bias1[n]] [+ bias2[n]]
//   ta = 0: A(m, k) = a(m, k);  ta = 1: A(m, k) = a(k, m)
//   tb = 0: B(k, n) = b(k, n);  tb = 1: B(k, n) = b(n, k)
struct GemmArgs {
  View a, b, c, d;  // d.p == nullptr: no addend (d may alias c)
  int ta, tb;
  int M, N, K;
  int kchunk;   // K range of one split (multiple of BK)
  float* part;  // splits > 1: partial sums [split][M][N]
  const float* bias1;
  const float* bias2;
};

constexpr int BM = 64, BN = 64, BK = 32, LDP = 68;

// One K-tile of an operand, OP(x0 + xx, k0 + kk) for xx < 64, kk < BK, zero outside
// [0, xlim) x [k0, klim): fetched into 8 registers per lane, then stored to LDS as T[kk][xx].
// kmajor: OP(x, k) = v(k, x) (64 lanes walk x); else OP(x, k) = v(x, k) (32 lanes walk k).
__device__ __forceinline__ void fetch_tile(const View& v, int kmajor, int x0, int xlim, int k0,
                                           int klim, float (&r)[8], int tid) {
  if (kmajor) {
    const int x = x0 + (tid & 63);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = k0 + (tid >> 6) + 4 * j;
      r[j] = 0.f;
      if (x < xlim && k < klim) r[j] = v.p[voff(v, k) + x];
    }
  } else {
    const int k = k0 + (tid & 31);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int x = x0 + (tid >> 5) + 8 * j;
      r[j] = 0.f;
      if (x < xlim && k < klim) r[j] = v.p[voff(v, x) + k];
    }
  }
}
__device__ __forceinline__ void store_tile(int kmajor, const float (&r)[8], float (*T)[LDP],
                                           int tid) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (kmajor)
      T[(tid >> 6) + 4 * j][tid & 63] = r[j];
    else
      T[tid & 31][(tid >> 5) + 8 * j] = r[j];
  }
}

__device__ __forceinline__ float epilogue(const GemmArgs& g, int m, int n, float acc) {
  if (g.d.p) acc += g.d.p[voff(g.d, m) + n];
  if (g.bias1) acc += g.bias1[n];
  if (g.bias2) acc += g.bias2[n];
  return acc;
}

// 64 x 64 output tile per workgroup, four waves of 32 x 32 (2 x 2 MFMA 16x16x4 tiles).
__global__ __launch_bounds__(256) void tgemm_kernel(GemmArgs g) {
  __shared__ float As[BK][LDP], Bs[BK][LDP];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int kb = blockIdx.z * g.kchunk;
  const int ke = min(g.K, kb + g.kchunk);
  const int wm = (w & 1) * 32, wn = (w >> 1) * 32;
  const int lr = lane & 15, lk = lane >> 4;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // the next K-tile's global loads are in flight while this one's MFMAs run
  float ra[8], rb[8];
  fetch_tile(g.a, g.ta, m0, g.M, kb, ke, ra, tid);
  fetch_tile(g.b, !g.tb, n0, g.N, kb, ke, rb, tid);
  for (int k0 = kb; k0 < ke; k0 += BK) {
    store_tile(g.ta, ra, As, tid);
    store_tile(!g.tb, rb, Bs, tid);
    __syncthreads();
    if (k0 + BK < ke) {
      fetch_tile(g.a, g.ta, m0, g.M, k0 + BK, ke, ra, tid);
      fetch_tile(g.b, !g.tb, n0, g.N, k0 + BK, ke, rb, tid);
    }
#pragma unroll
    for (int ks = 0; ks < BK; ks += 4) {
      const float a0 = As[ks + lk][wm + lr], a1 = As[ks + lk][wm + 16 + lr];
      const float b0 = Bs[ks + lk][wn + lr], b1 = Bs[ks + lk][wn + 16 + lr];
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
  // C/D map of the 16x16 f32 MFMA: col = lane & 15, row = (lane >> 4) * 4 + reg
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm + 16 * i + lk * 4 + r, n = n0 + wn + 16 * j + lr;
        if (m >= g.M || n >= g.N) continue;
        if (g.part) {
          g.part[((long)blockIdx.z * g.M + m) * g.N + n] = acc[i][j][r];
        } else {
          float* c = const_cast<float*>(g.c.p);
          c[voff(g.c, m) + n] = epilogue(g, m, n, acc[i][j][r]);
        }
      }
}

// Split-K combine: the partial sums in split order, then the epilogue.
__global__ void combine_kernel(GemmArgs g, int splits) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)g.M * g.N) return;
  const int m = (int)(i / g.N), n = (int)(i % g.N);
  float s = g.part[i];
  for (int z = 1; z < splits; ++z) s += g.part[(long)z * g.M * g.N + i];
  float* c = const_cast<float*>(g.c.p);
  c[voff(g.c, m) + n] = epilogue(g, m, n, s);
}

// Splits of K: enough workgroups to cover the CUs, at least 128 of K per split.  A
// function of the shape alone, so the summation order is too.
static int plan_splits(int M, int N, int K, int* kchunk) {
  const long tiles = (long)((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  int s = 1;
  while (s < 16 && tiles * s < 512 && K / (2 * s) >= 128) s *= 2;
  int kc = (K + s - 1) / s;
  kc = (kc + BK - 1) / BK * BK;
  if (kc == 0) kc = BK;
  *kchunk = kc;
  return (K + kc - 1) / kc > 0 ? (K + kc - 1) / kc : 1;
}

size_t split_scratch_floats(int M, int N, int K) {
  int kc;
  const int s = plan_splits(M, N, K, &kc);
  return s > 1 ? (size_t)s * M * N : 0;
}

// Splits of K as a function of K alone (at least 256 of K per split, at most 8 splits): the
// bits of an output row then depend on that row of A and on B, not on how many rows the
// call has.
static int plan_splits_rows(int K, int* kchunk) {
  int s = 1;
  while (s < 8 && K / (2 * s) >= 256) s *= 2;
  int kc = (K + s - 1) / s;
  kc = (kc + BK - 1) / BK * BK;
  if (kc == 0) kc = BK;
  *kchunk = kc;
  return (K + kc - 1) / kc > 0 ? (K + kc - 1) / kc : 1;
}

size_t rows_scratch_floats(int M, int N, int K) {
  int kc;
  const int s = plan_splits_rows(K, &kc);
  return s > 1 ? (size_t)s * M * N : 0;
}

static int gemm_planned(View a, int ta, View b, int tb, View c, View d, const float* bias1,
                        const float* bias2, int M, int N, int K, bool by_rows, Scratch sc,
                        hipStream_t s);

int gemm(View a, int ta, View b, int tb, View c, View d, const float* bias1,
                const float* bias2, int M, int N, int K, Scratch sc, hipStream_t s) {
  return gemm_planned(a, ta, b, tb, c, d, bias1, bias2, M, N, K, false, sc, s);
}

int gemm_rows(View a, int ta, View b, int tb, View c, View d, const float* bias1,
              const float* bias2, int M, int N, int K, Scratch sc, hipStream_t s) {
  return gemm_planned(a, ta, b, tb, c, d, bias1, bias2, M, N, K, true, sc, s);
}

static int gemm_planned(View a, int ta, View b, int tb, View c, View d, const float* bias1,
                        const float* bias2, int M, int N, int K, bool by_rows, Scratch sc,
                        hipStream_t s) {
  if (M <= 0 || N <= 0) return 0;
  GemmArgs g{a, b, c, d, ta, tb, M, N, K, 0, nullptr, bias1, bias2};
  const int splits = K <= 0 ? 1
                            : (by_rows ? plan_splits_rows(K, &g.kchunk)
                                       : plan_splits(M, N, K, &g.kchunk));
  if (K <= 0) g.kchunk = BK;
  if (splits > 1) {
    MILAN_REQUIRE((size_t)splits * M * N <= sc.floats, MILAN_ERR_WORKSPACE,
                  "tgemm: split-K scratch too small (%d x %d x %d)", splits, M, N);
    g.part = sc.p;
  }
  dim3 grid((N + BN - 1) / BN, (M + BM - 1) / BM, splits);
  hipLaunchKernelGGL(tgemm_kernel, grid, dim3(256), 0, s, g);
  MILAN_CHECK_HIP(hipGetLastError());
  if (splits > 1) {
    const long total = (long)M * N;
    hipLaunchKernelGGL(combine_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                       g, splits);
    MILAN_CHECK_HIP(hipGetLastError());
  }
  return 0;
}

// Column sums of X [R][N], stage 1: part[c][n] = sum over the rows of chunk c, in order.
__global__ void colsum_part_kernel(const float* __restrict__ X, int R, int N, int rchunk,
                                   float* __restrict__ part) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const int r0 = blockIdx.y * rchunk, r1 = min(R, r0 + rchunk);
  float s = 0.f;
  for (int r = r0; r < r1; ++r) s += X[(long)r * N + n];
  part[(long)blockIdx.y * N + n] = s;
}
// stage 2: out1[n] (= out2[n] when given) = sum of the chunks in order
__global__ void colsum_final_kernel(const float* __restrict__ part, int chunks, int N,
                                    float* __restrict__ out1, float* __restrict__ out2) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float s = 0.f;
  for (int c = 0; c < chunks; ++c) s += part[(long)c * N + n];
  out1[n] = s;
  if (out2) out2[n] = s;
}

int colsum_chunks(int R) {
  const int c = (R + 63) / 64;
  return c < 1 ? 1 : (c > 64 ? 64 : c);
}

int colsum(const float* X, int R, int N, float* out1, float* out2, Scratch sc,
                  hipStream_t s) {
  const int chunks = colsum_chunks(R), rchunk = (R + chunks - 1) / chunks;
  MILAN_REQUIRE((size_t)chunks * N <= sc.floats, MILAN_ERR_WORKSPACE,
                "tgemm: column-sum scratch too small");
  hipLaunchKernelGGL(colsum_part_kernel, dim3((N + 255) / 256, chunks), dim3(256), 0, s, X, R,
                     N, rchunk, sc.p);
  hipLaunchKernelGGL(colsum_final_kernel, dim3((N + 255) / 256), dim3(256), 0, s, sc.p, chunks,
                     N, out1, out2);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace tgemm
}  // namespace milan
