// Pieces of the training path shared by lm_train.hip (LanguageModel.fit) and
// decoder_train.hip (Decoder.fit): the strided exact-fp32 GEMM with deterministic split-K,
// the ordered column sums, the NLL / dlogits kernels and the embedding gradient.  The
// kernels themselves live in lm_train.hip; this header declares their host launchers.
#pragma once
#include "common.h"

namespace milan {
namespace lmt {

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

// splitmix64 finaliser (the dropout masks hash (seed, tag, row, t, unit) with it)
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

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

// Per row n of logits [N][V]: lse[n], term[n] = -log p(tgt[n]) (0 for pad), valid[n].
void launch_nll_rows(const float* logits, const int64_t* tgt, int N, int V, int pad, float* lse,
                     float* term, float* valid, hipStream_t s);
// out[0] = sum of term, out[1] = sum of valid (one workgroup, fixed order)
void launch_loss_reduce(const float* term, const float* valid, int N, float* out, hipStream_t s);
// logits <- (softmax - onehot(tgt)) * valid / loss[1], in place
void launch_dlogits(float* logits, const int64_t* tgt, const float* lse, const float* valid,
                    const float* loss, int N, int V, hipStream_t s);
// dEmb[v] = sum over positions n with ids[n] == v of dX[n] (row stride E), in position order;
// row `pad` is exactly zero (pad < 0: no such row)
void launch_embed_grad(const int64_t* ids, const float* dX, int N, int E, int V, int pad,
                       float* dEmb, hipStream_t s);

}  // namespace lmt
}  // namespace milan
