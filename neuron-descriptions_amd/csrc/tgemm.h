// The strided exact-fp32 MFMA GEMM with deterministic split-K, and the ordered column sums:
// the contraction of the training path (lm_train.hip, decoder_train.hip) and of the
// transformer towers (clip.hip, bert.hip, vit.hip through tower_common.h).  Both operands are
// read through strided views, so X.W^T, dG^T.X and dG.W are one kernel with different views and
// no weight is ever transposed or packed.  The kernels are defined in tgemm.hip.
#pragma once
#include "common.h"

namespace milan {
namespace tgemm {

// Element (r, c) of a 2-D view is p[off(r) + c], off(r) = (r / grp) * gs + (r % grp) * rs
// (grp == 0: r * rs).  The grouped form addresses a (rows, L) slice of a (rows, L + 1)
// buffer as one row range (the h_{t-1} operand of dW_hh).
struct View {
  const float* p;
  long rs;
  int grp;
  long gs;
};
static inline View view(const float* p, long rs, int grp = 0, long gs = 0) {
  return {p, rs, grp, gs};
}

__device__ __forceinline__ long voff(const View& v, int r) {
  return v.grp ? (long)(r / v.grp) * v.gs + (long)(r % v.grp) * v.rs : (long)r * v.rs;
}

struct Scratch {
  float* p;
  size_t floats;
};

// C(m, n) = sum_k A(m, k) B(k, n) [+ D(m, n)] [+ bias1[n]] [+ bias2[n]]
//   ta = 0: A(m, k) = a(m, k);  ta = 1: A(m, k) = a(k, m)
//   tb = 0: B(k, n) = b(k, n);  tb = 1: B(k, n) = b(n, k)
// d.p == nullptr: no addend (d may alias c).  Exact fp32 MFMA; split-K partial sums go to
// `sc` and are added in split order.  The split count is a function of (M, N, K) alone.
int gemm(View a, int ta, View b, int tb, View c, View d, const float* bias1, const float* bias2,
         int M, int N, int K, Scratch sc, hipStream_t s);
// scratch floats gemm() needs for an (M, N, K) problem
size_t split_scratch_floats(int M, int N, int K);

// The same GEMM with the split count a function of K alone, so that the bits of an output
// row do not depend on M (the BERTScore tower: a sentence's embeddings must not depend on the
// batch it is encoded in).  Scratch: rows_scratch_floats.
int gemm_rows(View a, int ta, View b, int tb, View c, View d, const float* bias1,
              const float* bias2, int M, int N, int K, Scratch sc, hipStream_t s);
size_t rows_scratch_floats(int M, int N, int K);

// out1[n] (= out2[n] when given) = sum over the R rows of X [R][N], in a fixed order;
// needs colsum_chunks(R) * N scratch floats
int colsum_chunks(int R);
int colsum(const float* X, int R, int N, float* out1, float* out2, Scratch sc, hipStream_t s);

}  // namespace tgemm
}  // namespace milan
