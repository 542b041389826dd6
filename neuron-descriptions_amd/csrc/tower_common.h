// Row kernels the transformer towers share (clip.hip, bert.hip, vit.hip).  Each kernel has
// one definition, in the file that first needed it; this header declares the host launchers.
#pragma once
#include "train_common.h"

namespace milan {
namespace tower {

// clip.hip.  The stride-P patches of n (3, R, R) images as the rows of conv1's im2col:
// A[(img * G + gy) * G + gx][(c * P + py) * P + px], G = R / P.  renorm_mul_add (HOST, 6
// floats: mul[3], add[3]) or nullptr: x * mul[c] + add[c] first.
int launch_patch_gather(const float* images, float* A, long n, int R, int P,
                        const float* renorm_mul_add, hipStream_t s);

// bert.hip.  dst[r][:] = LayerNorm(src[r * stride .. + W]; w, b, eps), biased variance, two
// passes (mean, then the centred second moment), one wave per row.
int launch_layernorm_rows(const float* src, long stride, float* dst, int rows, int W,
                          const float* w, const float* b, float eps, hipStream_t s);

// bert.hip.  x <- x * 0.5 * (1 + erf(x / sqrt(2))), in place.
int launch_gelu_erf(float* x, long total, hipStream_t s);

}  // namespace tower
}  // namespace milan
