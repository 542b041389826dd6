// Image sharing (milan_set_image_sharing): exemplar slots of one encoder pass
// that show the SAME uint8 image share one trunk pass.  The reference runs the trunk on the
// unmasked image and the masks enter at the pooling only (src/milan/encoders.py:295-318), so
// the features of slot i are pool(trunk(image_i), mask_i): the trunk batch holds one
// representative per class of byte-identical images and the pooling of slot i reads trunk
// slot class_of[i].
//
//   image_hash_kernel      64-bit hash of every image (candidates only)
//   image_classes_kernel   rep[i] = first slot j <= i whose bytes equal slot i's (byte compare)
//   class_flags_kernel     which classes have a member with work
//   compact_classes_kernel order[] / count / class_of[] / union bounding boxes
//   share_count_kernel     the two device-side counters of milan_image_sharing_stats
//
// Everything is enqueued on the stream; nothing is read back (the pass stays capturable).
// Integer arithmetic only: the hash is a wrapping SUM of per-block mixes (commutative and
// associative, so the reduction order cannot change it) and the class structure is decided
// by the byte comparison alone -- two different images are never merged, whatever the hash.
#include "common.h"

namespace milan {

typedef unsigned long long u64;
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

// Logical 16-byte block k of an image = its bytes [16 k, 16 k + 16), whatever the alignment
// of the image's first byte: `al` = 16 (one 16-byte load), 4 (four 4-byte loads) or 1 (bytes).
// The value does not depend on `al` (little endian).
__device__ __forceinline__ u32x4_t load_block16(const unsigned char* p, int al) {
  u32x4_t v;
  if (al == 16) {
    v = *reinterpret_cast<const u32x4_t*>(p);
  } else if (al == 4) {
    const unsigned* q = reinterpret_cast<const unsigned*>(p);
    v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      v[e] = (unsigned)p[4 * e] | ((unsigned)p[4 * e + 1] << 8) |
             ((unsigned)p[4 * e + 2] << 16) | ((unsigned)p[4 * e + 3] << 24);
  }
  return v;
}
// the last bytes % 16 bytes, zero-padded to a block
__device__ __forceinline__ u32x4_t load_tail16(const unsigned char* p, int rem) {
  u32x4_t v = {0u, 0u, 0u, 0u};
  for (int e = 0; e < rem; ++e) v[e >> 2] |= (unsigned)p[e] << (8 * (e & 3));
  return v;
}
__device__ __forceinline__ int align_of(const unsigned char* p) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  return (a & 15) == 0 ? 16 : ((a & 3) == 0 ? 4 : 1);
}

__device__ __forceinline__ u64 mix64(u64 x) {   // (the splitmix64 finaliser)
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27; x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}
// contribution of block k: depends on the position, so swapped blocks change the sum
__device__ __forceinline__ u64 block_hash(u32x4_t v, long k) {
  const u64 a = (u64)v[0] | ((u64)v[1] << 32), b = (u64)v[2] | ((u64)v[3] << 32);
  const u64 pos = (u64)(k + 1) * 0x9e3779b97f4a7c15ull;
  return mix64(a + pos) + mix64(b ^ mix64(pos));
}

// One workgroup per image: hash[i] = (sum over blocks of block_hash) & mask.
__global__ __launch_bounds__(256) void image_hash_kernel(const unsigned char* __restrict__ images,
                                                         long bytes, u64 mask,
                                                         u64* __restrict__ hash) {
  __shared__ u64 part[4];
  const int i = blockIdx.x;
  const unsigned char* p = images + (long)i * bytes;
  const int al = align_of(p);
  const long nblk = bytes >> 4;
  const int rem = (int)(bytes & 15);
  u64 h = 0;
  for (long k = threadIdx.x; k < nblk; k += 256) h += block_hash(load_block16(p + (k << 4), al), k);
  if (threadIdx.x == 0 && rem) h += block_hash(load_tail16(p + (nblk << 4), rem), nblk);
  for (int o = 32; o > 0; o >>= 1) h += __shfl_xor(h, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = h;
  __syncthreads();
  if (threadIdx.x == 0) hash[i] = (part[0] + part[1] + part[2] + part[3]) & mask;
}

// One workgroup per slot i: rep[i] = the first j < i with the same bytes, else i.  Byte equality
// is transitive and j ascends, so rep[i] is always a root (rep[rep[i]] == rep[i]).  The hash only
// selects the candidates that get the byte comparison (mask 0: every j does).
__global__ __launch_bounds__(256) void image_classes_kernel(const unsigned char* __restrict__ images,
                                                            long bytes, const u64* __restrict__ hash,
                                                            int* __restrict__ rep) {
  __shared__ u64 cand[4];
  __shared__ int differ;
  const int i = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u64 hi = hash[i];
  const unsigned char* pi = images + (long)i * bytes;
  const int ali = align_of(pi);
  const long nblk = bytes >> 4;
  const int rem = (int)(bytes & 15);
  int found = i;
  for (int j0 = 0; j0 < i && found == i; j0 += 256) {
    const int j = j0 + threadIdx.x;
    const u64 m = __ballot(j < i && hash[j] == hi);
    __syncthreads();                       // (the previous round's reads of cand / differ)
    if (lane == 0) cand[wave] = m;
    __syncthreads();
    for (int w = 0; w < 4 && found == i; ++w) {
      u64 bits = cand[w];                  // (the same for every thread: uniform control flow)
      while (bits != 0 && found == i) {
        const int b = __ffsll((long long)bits) - 1;
        bits &= bits - 1;
        const int jc = j0 + w * 64 + b;
        const unsigned char* pj = images + (long)jc * bytes;
        const int alj = align_of(pj);
        // the workgroup compares 1024 blocks (16 KiB) at a time and stops at the first difference
        bool same = true;
        for (long k0 = 0; k0 <= nblk && same; k0 += 1024) {
          int d = 0;
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const long k = k0 + u * 256 + threadIdx.x;
            u32x4_t a, c;
            if (k < nblk) {
              a = load_block16(pi + (k << 4), ali);
              c = load_block16(pj + (k << 4), alj);
            } else if (k == nblk && rem) {
              a = load_tail16(pi + (k << 4), rem);
              c = load_tail16(pj + (k << 4), rem);
            } else {
              continue;
            }
            d |= (a[0] != c[0]) | (a[1] != c[1]) | (a[2] != c[2]) | (a[3] != c[3]);
          }
          if (threadIdx.x == 0) differ = 0;
          __syncthreads();
          if (d) differ = 1;               // (every writer stores the same value)
          __syncthreads();
          same = differ == 0;
          __syncthreads();                 // (before the next round clears the flag)
        }
        if (same) found = jc;
      }
    }
  }
  if (threadIdx.x == 0) rep[i] = found;
}

// flag[root] != 0: some member of the class has a non-empty weight list at some level (or
// skip_empty is off: every class is live).  `flag` was zero-filled.
__global__ void class_flags_kernel(const int* __restrict__ rep, const int* __restrict__ list_n,
                                   int n, int skip_empty, int* __restrict__ flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int any = !skip_empty;
  for (int l = 0; l < 5; ++l) any |= list_n[i * 5 + l];
  if (any) atomicOr(&flag[rep[i]], 1);
}

// Live classes numbered in ascending order of their root: order[c] = the root image, *count =
// how many, class_of[i] = the trunk slot slot i pools from (-1: slot i's own lists are all
// empty), bbox_c[c] = the UNION of the members' level-0 boxes (the empty box 0x7fffffff / -1 is
// neutral under min / max).  One workgroup of 1024 threads, like compact_images_kernel; on
// return flag[root] = class number + 1.
__global__ __launch_bounds__(1024) void compact_classes_kernel(
    const int* __restrict__ rep, const int* __restrict__ list_n, const int* __restrict__ bbox, int n,
    int skip_empty, int* __restrict__ flag, int* __restrict__ order, int* __restrict__ bbox_c,
    int* __restrict__ count, int* __restrict__ class_of) {
  __shared__ int wsum[16];
  __shared__ int base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) base = 0;
  __syncthreads();
  for (int i0 = 0; i0 < n; i0 += 1024) {
    const int i = i0 + threadIdx.x;
    const bool live = i < n && rep[i] == i && flag[i] != 0;
    const unsigned long long m = __ballot(live);
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wave; ++w) off += wsum[w];
    if (live) {
      const int j = off + __popcll(m & ((1ull << lane) - 1ull));
      order[j] = i;
      flag[i] = j + 1;
      bbox_c[j * 4 + 0] = 0x7fffffff; bbox_c[j * 4 + 1] = -1;
      bbox_c[j * 4 + 2] = 0x7fffffff; bbox_c[j * 4 + 3] = -1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int t = 0;
      for (int w = 0; w < 16; ++w) t += wsum[w];
      base += t;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *count = base;
  __threadfence();
  __syncthreads();   // flag[] / bbox_c[] of every class are written before the members read them
  for (int i = threadIdx.x; i < n; i += 1024) {
    int any = !skip_empty;
    for (int l = 0; l < 5; ++l) any |= list_n[i * 5 + l];
    int cls = -1;
    if (any) {
      cls = flag[rep[i]] - 1;
      atomicMin(&bbox_c[cls * 4 + 0], bbox[i * 4 + 0]);
      atomicMax(&bbox_c[cls * 4 + 1], bbox[i * 4 + 1]);
      atomicMin(&bbox_c[cls * 4 + 2], bbox[i * 4 + 2]);
      atomicMax(&bbox_c[cls * 4 + 3], bbox[i * 4 + 3]);
    }
    class_of[i] = cls;
  }
}

int launch_image_classes(const ShareArgs& a, hipStream_t s) {
  const u64 mask = a.hash_bits >= 64 ? ~0ull : (a.hash_bits <= 0 ? 0ull : (1ull << a.hash_bits) - 1ull);
  hipLaunchKernelGGL(image_hash_kernel, dim3(a.n), dim3(256), 0, s, a.images, a.bytes, mask,
                     (u64*)a.hash);
  hipLaunchKernelGGL(image_classes_kernel, dim3(a.n), dim3(256), 0, s, a.images, a.bytes,
                     (const u64*)a.hash, a.rep);
  MILAN_CHECK_HIP(hipGetLastError());
  MILAN_TRY(launch_zero_fill(a.flag, sizeof(int) * (size_t)a.n, s));
  hipLaunchKernelGGL(class_flags_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a.rep, a.list_n,
                     a.n, a.skip_empty, a.flag);
  hipLaunchKernelGGL(compact_classes_kernel, dim3(1), dim3(1024), 0, s, a.rep, a.list_n, a.bbox, a.n,
                     a.skip_empty, a.flag, a.order, a.bbox_c, a.count, a.class_of);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

// stats[0] += slots of the pass; stats[1] += images its trunk ran (*live, or all of them)
__global__ void share_count_kernel(long long* __restrict__ stats, int n, const int* __restrict__ live) {
  stats[0] += n;
  stats[1] += live != nullptr ? *live : n;
}

int launch_share_count(long long* stats, int n, const int* live, hipStream_t s) {
  hipLaunchKernelGGL(share_count_kernel, dim3(1), dim3(1), 0, s, stats, n, live);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace milan
