// The last step of every split-K weight gradient: dw[e] = sum over the splits of ws[s][e], ws = [splits][n].
// One thread sums one element in a fixed order and writes it once -- no atomics -- which is what makes these gradients
// bit-repeatable.  Two orders exist, and a kernel keeps the one it was written with (they differ in the last bits, and in
// the sign of a zero sum: the first starts from ws[e], the second from 0.f):
//   dv_splitk_sum            the splits in split order;
//   dv_splitk_sum_quartered  four quarters of the split range, each in split order, then the quarters in order.
// Internal launchers (declared in dv_common.h); the caller reads dv_launch_status() behind the call.
#include "dv_common.h"

namespace {

__global__ __launch_bounds__(256) void splitk_sum_kernel(const float* __restrict__ ws, float* __restrict__ dw, long long n,
                                                         int splits) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    float s = ws[e];
    for (int k = 1; k < splits; ++k) s += ws[(size_t)k * n + e];
    dw[e] = s;
  }
}

// a block owns 64 elements, its wave q adds the splits of quarter q, the four partials meet in LDS
__global__ __launch_bounds__(256) void splitk_sum_quartered_kernel(const float* __restrict__ ws, float* __restrict__ dw,
                                                                   long long n, int splits) {
  __shared__ float part[4][64];
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
  const long long e = (long long)blockIdx.x * 64 + lane;
  const int k0 = splits * q / 4, k1 = splits * (q + 1) / 4;
  float s = 0.f;
  if (e < n)
    for (int k = k0; k < k1; ++k) s += ws[(size_t)k * n + e];
  part[q][lane] = s;
  __syncthreads();
  if (q == 0 && e < n) dw[e] = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
}

}  // namespace

void dv_splitk_sum(const float* ws, float* dw, long long n, int splits, hipStream_t s) {
  const long long nb = (n + 255) / 256;
  hipLaunchKernelGGL(splitk_sum_kernel, dim3((unsigned)(nb < 2048 ? nb : 2048)), dim3(256), 0, s, ws, dw, n, splits);
}

void dv_splitk_sum_quartered(const float* ws, float* dw, long long n, int splits, hipStream_t s) {
  hipLaunchKernelGGL(splitk_sum_quartered_kernel, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, s, ws, dw, n, splits);
}
