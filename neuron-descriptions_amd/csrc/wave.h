// Reductions over the 64 lanes of a wave by xor butterfly: every lane ends with the result,
// and the order of the additions is fixed.  Shared by the transformer towers (tower_common.h)
// and the training path (train_common.h).
#pragma once
#include <hip/hip_runtime.h>

namespace milan {
namespace wave {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

}  // namespace wave
}  // namespace milan
