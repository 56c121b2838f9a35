// Bird's-eye-view rotated-box overlap / IoU and the two NMS variants of the 3-D detection branch (replaces
// TaskPrompter/detection_toolbox/iou3d/src/iou3d_kernel.cu + the host reduction of iou3d.cpp).  Box = [x1, y1, x2, y2, ry].
// The geometric algorithm (edge crossings + contained corners, angular sort about the vertex mean, fan area; margins 1e-5 / 1e-8) is the
// reference's, so degenerate configurations (identical, nested, edge-sharing boxes) resolve the same way; what is different:
//   * pairwise kernels: one lane per (a, b) pair, 64 consecutive b per wave (coalesced result rows);
//   * NMS: a 64 x 64 tile of the suppression matrix per WAVE (64-bit masks = one word per lane), only the tiles on or above the diagonal
//     (the greedy pass never reads the others), the column boxes broadcast from LDS;
//   * the greedy pass runs ON THE DEVICE in one wave (bit test on an LDS word per box, the suppressor's mask row OR-ed in by all lanes):
//     keep indices and their count stay in device memory — the reference copies the N x N/64 mask to the host and synchronises.
#include "mtt_device.h"

namespace {

#include "iou3d_dev.h"

__global__ __launch_bounds__(256) void pairwise_kernel(const float* a, int na, const float* b, int nb, float* out, int iou) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)na * nb) return;
  const int i = (int)(t / nb), j = (int)(t % nb);
  float A[5], B[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) { A[k] = a[i * 5 + k]; B[k] = b[j * 5 + k]; }
  out[t] = iou ? iou_rot(A, B) : overlap_area(A, B);
}

// one wave per 64 x 64 tile (rb <= cb): mask[(rb*64 + lane) * col_blocks + cb] bit j set when box rb*64+lane suppresses box cb*64+j
__global__ __launch_bounds__(64) void nms_mask_kernel(const float* boxes, int n, float thresh, int rotated, unsigned long long* mask) {
  const int cb = blockIdx.x, rb = blockIdx.y;
  if (rb > cb) return;
  const int col_blocks = (n + 63) / 64;
  __shared__ float cols[64 * 5];
  const int lane = threadIdx.x;
  const int cn = min(n - cb * 64, 64), rn = min(n - rb * 64, 64);
  if (lane < cn)
#pragma unroll
    for (int k = 0; k < 5; ++k) cols[lane * 5 + k] = boxes[(int64_t)(cb * 64 + lane) * 5 + k];
  __syncthreads();
  if (lane >= rn) return;
  float A[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) A[k] = boxes[(int64_t)(rb * 64 + lane) * 5 + k];
  unsigned long long m = 0;
  for (int j = (rb == cb ? lane + 1 : 0); j < cn; ++j) {
    const float v = rotated ? iou_rot(A, cols + j * 5) : iou_axis(A, cols + j * 5);
    if (v > thresh) m |= 1ull << j;
  }
  mask[(int64_t)(rb * 64 + lane) * col_blocks + cb] = m;
}

// greedy pass, one wave: remv (one 64-bit word per column block) in LDS; lanes OR the kept box's mask row in parallel
__global__ __launch_bounds__(64) void nms_reduce_kernel(const unsigned long long* mask, int n, long long* keep, int* num_out) {
  extern __shared__ unsigned long long remv[];
  const int col_blocks = (n + 63) / 64;
  const int lane = threadIdx.x;
  for (int j = lane; j < col_blocks; j += 64) remv[j] = 0ull;
  __syncthreads();
  int k = 0;
  for (int i = 0; i < n; ++i) {
    const int nb = i >> 6;
    const bool dead = (remv[nb] >> (i & 63)) & 1ull;      // wave-uniform
    if (!dead) {
      if (lane == 0) keep[k] = i;
      ++k;
      for (int j = nb + lane; j < col_blocks; j += 64) remv[j] |= mask[(int64_t)i * col_blocks + j];
    }
    __syncthreads();
  }
  if (lane == 0) *num_out = k;
}

}  // namespace

extern "C" int mtt_boxes_overlap_bev(const float* a, int na, const float* b, int nb, float* out, int iou, void* stream) {
  if (!a || !b || !out || na <= 0 || nb <= 0) return MTT_E_BADARG;
  const int64_t n = (int64_t)na * nb;
  hipLaunchKernelGGL(pairwise_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, na, b, nb, out, iou);
  return (int)hipGetLastError();
}

extern "C" size_t mtt_nms_ws_bytes(int n) { return n <= 0 ? 0 : (size_t)n * ((n + 63) / 64) * 8; }

extern "C" int mtt_nms_bev(const float* boxes, int n, float thresh, int rotated, long long* keep, int* num_out, void* ws, void* stream) {
  if (!boxes || !keep || !num_out || !ws || n <= 0) return MTT_E_BADARG;
  const int cb = (n + 63) / 64;
  if ((size_t)cb * 8 > 64 * 1024) return MTT_E_UNSUPPORTED;        /* > 524 288 boxes */
  hipLaunchKernelGGL(nms_mask_kernel, dim3(cb, cb), dim3(64), 0, (hipStream_t)stream, boxes, n, thresh, rotated, (unsigned long long*)ws);
  hipLaunchKernelGGL(nms_reduce_kernel, dim3(1), dim3(64), cb * 8, (hipStream_t)stream, (const unsigned long long*)ws, n, keep, num_out);
  return (int)hipGetLastError();
}
