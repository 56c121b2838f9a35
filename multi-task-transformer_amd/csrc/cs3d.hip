// Cityscapes-3D batch preparation on the device: the per-sample work of the reference's dataset class
// (TaskPrompter/data/cityscapes3d.py:137-241) on a batch of equally sized frames.  Two entry points (include/mtt_hip.h):
//   mtt_cs3d_image : BGR / RGB uint8 HWC -> Pillow's 8-bit bilinear resample -> ToTensor + Normalize, NCHW fp32
//   mtt_cs3d_labels: labelIds uint8 + disparity uint16 -> Pillow's nearest resample -> encode_segmap (int64), validity flags, depth (fp32)
// Pillow's resample is a two-pass fixed-point convolution whose horizontal result is rounded to 8 bits before the vertical pass.  The
// weights come from host-built tables, so everything here is 32-bit integer arithmetic up to the final two IEEE divisions: the outputs
// equal the reference's bit for bit.  A workgroup owns TH x TW output pixels; the rounded intermediate lives in LDS only.
#include "mtt_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int TH = MTT_CS3D_TILE_H, TW = MTT_CS3D_TILE_W;
constexpr int MAX_DIM = 32768;
constexpr int RAW_CAP = 16384;          // bytes of LDS for the staged source rows; a row of MTT_CS3D_MAX_COLS pixels fits
constexpr int PRECISION_BITS = 22;      // 32 - 8 - 2, Pillow's Resample.c
static_assert(TH * (TW / 4) == 256, "the vertical pass gives each of the 256 threads 4 pixels of the tile");
static_assert(((MTT_CS3D_MAX_COLS * 3 + 15 + 15) & ~15) <= RAW_CAP, "one source row has to fit the staging buffer");
static_assert(RAW_CAP + MTT_CS3D_MAX_ROWS * 3 * TW <= 65536, "LDS of one workgroup");

MTT_DEV int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
MTT_DEV int clip8(unsigned acc) { return clampi((int)acc >> PRECISION_BITS, 0, 255); }             // arithmetic shift, as clip8() of Pillow
MTT_DEV float norm8(int v, float mean, float std) { return __fdiv_rn(__fdiv_rn((float)v, 255.f) - mean, std); }
MTT_DEV int pitch_of(int cols) { return (cols * 3 + 15 + 15) & ~15; }                              // a row's bytes + its misalignment, in 16-byte vectors

// ---- image, resampled ---------------------------------------------------------------------------------------------------------------------
// grid (ceil(w / TW), ceil(h / TH), B).  LDS: raw [rb][pitch] source bytes as loaded (each row starts at its own 16-byte boundary, `shift`
// bytes before its first needed byte), then inter [span][3][TW] uint8, the horizontal pass's rounded result.  span / cols are the host's
// bounds for the largest window of any tile; what the device tables say is clamped into them.
__global__ __launch_bounds__(256) void cs3d_resample_kernel(const mtt_cs3d_desc d, int span, int cols, int rb) {
  extern __shared__ __align__(16) uint8_t lds[];
  const int pitch = pitch_of(cols);
  uint8_t* raw = lds;
  uint8_t* inter = lds + rb * pitch;
  const int tid = threadIdx.x, b = blockIdx.z, y0 = blockIdx.y * TH, x0 = blockIdx.x * TW;
  const int ny = min(TH, d.h - y0), nx = min(TW, d.w - x0);
  const int yl = y0 + ny - 1, xl = x0 + nx - 1;
  // the tile's source window [r0, r1) x [c0, c1)
  const int r0 = clampi(d.ytab[2 * y0], 0, d.H - 1);
  const int r1 = min(clampi(d.ytab[2 * yl] + d.ytab[2 * yl + 1], r0 + 1, d.H), r0 + span);
  const int c0 = clampi(d.xtab[2 * x0], 0, d.W - 1);
  const int c1 = min(clampi(d.xtab[2 * xl] + d.xtab[2 * xl + 1], c0 + 1, d.W), c0 + cols);
  const int64_t total = (int64_t)d.B * d.H * d.W * 3;
  const int nvec = pitch >> 4, nbytes = (c1 - c0) * 3;

  for (int rs = r0; rs < r1; rs += rb) {
    const int nr = min(rb, r1 - rs);
    // stage nr source rows: 16-byte loads from the aligned address below each row's first byte
    for (int idx = tid; idx < nr * nvec; idx += 256) {
      const int i = idx / nvec, v = idx - i * nvec;
      const int64_t g0 = (((int64_t)b * d.H + rs + i) * d.W + c0) * 3;
      const int64_t a = (g0 & ~(int64_t)15) + 16 * v;
      if (a >= g0 + nbytes) continue;                       // past the row's last needed byte
      u32x4 q;
      if (a + 16 <= total) {
        q = *(const u32x4*)(d.src + a);
      } else {                                              // the last vector of the buffer, byte by byte
        unsigned w4[4] = {0, 0, 0, 0};
        for (int j = 0; j < 16; ++j)
          if (a + j < total) w4[j >> 2] |= (unsigned)d.src[a + j] << (8 * (j & 3));
        q = (u32x4){w4[0], w4[1], w4[2], w4[3]};
      }
      *(u32x4*)(raw + i * pitch + 16 * v) = q;
    }
    __syncthreads();
    // horizontal pass: a wave takes the 64 columns of one staged row
    for (int idx = tid; idx < nr * TW; idx += 256) {
      const int i = idx / TW, xx = idx - i * TW;
      int o[3] = {0, 0, 0};
      if (xx < nx) {
        const int x = x0 + xx;
        const int xmin = clampi(d.xtab[2 * x], c0, c1 - 1);
        const int cnt = clampi(d.xtab[2 * x + 1], 0, min(d.xk, c1 - xmin));
        const int32_t* kx = d.xcoeff + (int64_t)x * d.xk;
        const int64_t g0 = (((int64_t)b * d.H + rs + i) * d.W + c0) * 3;
        const uint8_t* p = raw + i * pitch + (int)(g0 & 15) + (xmin - c0) * 3;
        unsigned acc[3] = {1u << (PRECISION_BITS - 1), 1u << (PRECISION_BITS - 1), 1u << (PRECISION_BITS - 1)};
        for (int k = 0; k < cnt; ++k) {
          const unsigned kk = (unsigned)kx[k];
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[c] += kk * p[3 * k + c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = clip8(acc[c]);
      }
      uint8_t* q = inter + (rs - r0 + i) * 3 * TW + xx;
#pragma unroll
      for (int c = 0; c < 3; ++c) q[c * TW] = (uint8_t)o[c];
    }
    __syncthreads();
  }

  // vertical pass + normalisation: thread -> row tid / 16, 4 columns from (tid % 16) * 4; one 32-bit LDS read per tap and channel
  const int yy = tid / (TW / 4), xq = (tid % (TW / 4)) * 4;
  if (yy >= ny || xq >= nx) return;
  const int y = y0 + yy;
  const int ymin = clampi(d.ytab[2 * y], r0, r1 - 1);
  const int cnt = clampi(d.ytab[2 * y + 1], 0, min(d.yk, r1 - ymin));
  const int32_t* ky = d.ycoeff + (int64_t)y * d.yk;
  unsigned acc[3][4];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[c][j] = 1u << (PRECISION_BITS - 1);
  for (int k = 0; k < cnt; ++k) {
    const unsigned kk = (unsigned)ky[k];
    const uint8_t* q = inter + (ymin - r0 + k) * 3 * TW + xq;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const unsigned w4 = *(const unsigned*)(q + c * TW);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[c][j] += kk * ((w4 >> (8 * j)) & 255u);
    }
  }
  const int64_t hw = (int64_t)d.h * d.w;
  float* out = d.out + (int64_t)b * 3 * hw + (int64_t)y * d.w + x0 + xq;
  const bool vec = (d.w & 3) == 0 && ((uintptr_t)d.out & 15) == 0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = norm8(clip8(d.bgr ? acc[2 - ch][j] : acc[ch][j]), d.mean[ch], d.std[ch]);      // constant indices: no scratch
    if (vec) {
      *(float4*)(out + ch * hw) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (xq + j < nx) out[ch * hw + j] = v[j];
    }
  }
}

// ---- image, same size ---------------------------------------------------------------------------------------------------------------------
// any size or alignment: one pixel per thread, grid (pixel blocks, B)
__global__ __launch_bounds__(256) void cs3d_normalise_kernel(const mtt_cs3d_desc d) {
  const int b = blockIdx.y;
  const int64_t hw = (int64_t)d.H * d.W;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= hw) return;
  const uint8_t* src = d.src + ((int64_t)b * hw + p) * 3;
  float* out = d.out + (int64_t)b * 3 * hw + p;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) out[ch * hw] = norm8(src[d.bgr ? 2 - ch : ch], d.mean[ch], d.std[ch]);
}

// grid (blocks of 4096 pixels, B), H * W % 16 == 0: a workgroup loads its 12 288 interleaved bytes with three 16-byte loads per thread
// (consecutive lanes, consecutive vectors) into LDS; each thread then takes 4 consecutive pixels (three dwords) of each quarter of the
// block, so that a wave's 16-byte stores cover 1 KiB of a channel plane without a gap.
constexpr int NORM_PX = 4096;
__global__ __launch_bounds__(256) void cs3d_normalise_lds_kernel(const mtt_cs3d_desc d) {
  __shared__ __align__(16) unsigned stage[NORM_PX * 3 / 4];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t hw = (int64_t)d.H * d.W;
  const int64_t p0 = (int64_t)blockIdx.x * NORM_PX;
  const int npx = (int)(hw - p0 < NORM_PX ? hw - p0 : NORM_PX);      // a multiple of 16
  const u32x4* src = (const u32x4*)(d.src + ((int64_t)b * hw + p0) * 3);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int v = i * 256 + tid;
    if (v * 16 < npx * 3) ((u32x4*)stage)[v] = src[v];
  }
  __syncthreads();
  const bool bgr = d.bgr != 0;
  float* out = d.out + (int64_t)b * 3 * hw + p0;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int q = g * 1024 + tid * 4;
    if (q >= npx) break;
    const unsigned w[3] = {stage[g * 768 + tid * 3], stage[g * 768 + tid * 3 + 1], stage[g * 768 + tid * 3 + 2]};
    auto byte = [&](int n) { return (int)((w[n >> 2] >> (8 * (n & 3))) & 255u); };      // n is a compile-time constant after unrolling
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = norm8(bgr ? byte(3 * j + 2 - ch) : byte(3 * j + ch), d.mean[ch], d.std[ch]);
      *(float4*)(out + ch * hw + q) = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
}

// ---- labels -------------------------------------------------------------------------------------------------------------------------------
// encode_segmap (cityscapes3d.py:92-93, 235-241) as a function of the raw id: void -> 255, valid -> its rank, anything else unchanged
MTT_DEV int encode_id(int id) {
  constexpr uint8_t valid[19] = {7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33};
  if (id > 33) return id;
  int out = 255;                                            // ids 0..33 are void unless listed (the void class -1 is no uint8 value)
#pragma unroll
  for (int k = 0; k < 19; ++k) out = id == valid[k] ? k : out;
  return out;
}

template <int V> __global__ __launch_bounds__(256) void cs3d_labels_kernel(const mtt_cs3d_desc d) {
  __shared__ uint8_t lut[256];
  lut[threadIdx.x] = (uint8_t)encode_id(threadIdx.x);
  __syncthreads();
  const int b = blockIdx.y;
  const int hw = d.h * d.w;                                 // <= 2^30
  const int p = (blockIdx.x * 256 + threadIdx.x) * V;
  bool invalid = false;
  if (p < hw) {
    const int y = p / d.w, x0 = p - y * d.w;
    const int sy = d.ytab ? clampi(d.ytab[y], 0, d.H - 1) : min(y, d.H - 1);
    const int64_t row = ((int64_t)b * d.H + sy) * d.W;
    int64_t sem[V];
    float dep[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const int x = x0 + i;
      const int sx = d.xtab ? clampi(d.xtab[x], 0, d.W - 1) : min(x, d.W - 1);
      const int id = d.src[row + sx];
      const int s = lut[id];
      sem[i] = s;
      invalid |= s != 255 && s >= 19;
      if (d.disp) {
        const int raw = d.disp[row + sx];
        float f = raw > 0 ? __fdiv_rn((float)(raw - 1), 256.f) : 0.f;
        f = f == 0.f ? -1.f : f;                            // after the decoding: d == 1 became 0 and is invalid too
        dep[i] = id == 10 ? 0.f : f;                        // the sky test reads the RAW ids (before encode_segmap), as the reference does
      }
    }
    int64_t* so = d.semseg + (int64_t)b * hw + p;
    if constexpr (V == 4) {
      typedef __attribute__((ext_vector_type(2))) long long i64x2;
      ((i64x2*)so)[0] = (i64x2){sem[0], sem[1]};
      ((i64x2*)so)[1] = (i64x2){sem[2], sem[3]};
      if (d.disp) *(float4*)(d.out + (int64_t)b * hw + p) = make_float4(dep[0], dep[1], dep[2], dep[3]);
    } else {
      so[0] = sem[0];
      if (d.disp) d.out[(int64_t)b * hw + p] = dep[0];
    }
  }
  if (__syncthreads_or(invalid) && threadIdx.x == 0) atomicOr(&d.flags[b], 1);          // every thread of the workgroup arrives
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
int check_sizes(const mtt_cs3d_desc* d) {
  if (!d || !d->src) return MTT_E_BADARG;
  if (d->B <= 0 || d->B > 65535 || d->H <= 0 || d->W <= 0 || d->h <= 0 || d->w <= 0) return MTT_E_BADARG;
  if (d->H > MAX_DIM || d->W > MAX_DIM || d->h > MAX_DIM || d->w > MAX_DIM) return MTT_E_BADARG;
  return 0;
}

// a bilinear bounds table: n rows of (first, count) inside [0, in), both ends non-decreasing.  span = the largest source window of a
// tile of `tile` consecutive outputs.
int check_bounds(const int32_t* t, int n, int n_out, int k, int in, int tile, int& span) {
  if (!t || n != n_out || k <= 0) return MTT_E_BADARG;
  for (int i = 0; i < n; ++i) {
    const int64_t first = t[2 * i], cnt = t[2 * i + 1];
    if (first < 0 || cnt <= 0 || cnt > k || first + cnt > in) return MTT_E_BADARG;
    if (i > 0 && (first < t[2 * i - 2] || first + cnt < (int64_t)t[2 * i - 2] + t[2 * i - 1])) return MTT_E_BADARG;
  }
  span = 0;
  for (int i0 = 0; i0 < n; i0 += tile) {
    const int i1 = (i0 + tile < n ? i0 + tile : n) - 1;
    const int s = t[2 * i1] + t[2 * i1 + 1] - t[2 * i0];
    span = s > span ? s : span;
  }
  return 0;
}

int check_index(const int32_t* dev, const int32_t* host, int n, int n_out, int in) {
  if (!dev != !host) return MTT_E_BADARG;
  if (!dev) return n_out == in ? 0 : MTT_E_BADARG;          // identity: the axis keeps its size
  if (n != n_out) return MTT_E_BADARG;
  for (int i = 0; i < n; ++i)
    if (host[i] < 0 || host[i] >= in) return MTT_E_BADARG;
  return 0;
}

}  // namespace

extern "C" size_t mtt_cs3d_desc_size(void) { return sizeof(mtt_cs3d_desc); }

extern "C" int mtt_cs3d_image(const mtt_cs3d_desc* d, void* stream) {
  if (const int rc = check_sizes(d)) return rc;
  if (!d->out) return MTT_E_BADARG;
  for (int c = 0; c < 3; ++c)
    if (!(d->std[c] != 0.f) || !(d->mean[c] == d->mean[c])) return MTT_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  if (!d->xtab && !d->ytab && !d->xtab_host && !d->ytab_host && !d->xcoeff && !d->ycoeff) {
    if (d->h != d->H || d->w != d->W) return MTT_E_BADARG;
    const int64_t hw = (int64_t)d->H * d->W;
    if (hw % 16 == 0 && (((uintptr_t)d->src | (uintptr_t)d->out) & 15) == 0)
      hipLaunchKernelGGL(cs3d_normalise_lds_kernel, dim3((unsigned)((hw + NORM_PX - 1) / NORM_PX), (unsigned)d->B), dim3(256), 0, s, *d);
    else
      hipLaunchKernelGGL(cs3d_normalise_kernel, dim3((unsigned)((hw + 255) / 256), (unsigned)d->B), dim3(256), 0, s, *d);
    return (int)hipGetLastError();
  }
  if (!d->xtab || !d->ytab || !d->xcoeff || !d->ycoeff) return MTT_E_BADARG;
  int span = 0, cols = 0;
  if (const int rc = check_bounds(d->ytab_host, d->yn, d->h, d->yk, d->H, TH, span)) return rc;
  if (const int rc = check_bounds(d->xtab_host, d->xn, d->w, d->xk, d->W, TW, cols)) return rc;
  if ((uintptr_t)d->src & 15) return MTT_E_ALIGN;
  if (span > MTT_CS3D_MAX_ROWS || cols > MTT_CS3D_MAX_COLS) return MTT_E_UNSUPPORTED;
  const int pitch = (cols * 3 + 15 + 15) & ~15;
  int rb = RAW_CAP / pitch;
  rb = rb < span ? rb : span;
  const size_t lds = (size_t)rb * pitch + (size_t)span * 3 * TW;
  const dim3 grid((unsigned)((d->w + TW - 1) / TW), (unsigned)((d->h + TH - 1) / TH), (unsigned)d->B);
  hipLaunchKernelGGL(cs3d_resample_kernel, grid, dim3(256), lds, s, *d, span, cols, rb);
  return (int)hipGetLastError();
}

extern "C" int mtt_cs3d_labels(const mtt_cs3d_desc* d, void* stream) {
  if (const int rc = check_sizes(d)) return rc;
  if (!d->semseg || !d->flags || (d->disp && !d->out)) return MTT_E_BADARG;
  if (const int rc = check_index(d->ytab, d->ytab_host, d->yn, d->h, d->H)) return rc;
  if (const int rc = check_index(d->xtab, d->xtab_host, d->xn, d->w, d->W)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(d->flags, 0, sizeof(int32_t) * (size_t)d->B, s);
  if (e != hipSuccess) return (int)e;
  const int64_t hw = (int64_t)d->h * d->w;
  const bool v4 = d->w % 4 == 0 && ((uintptr_t)d->semseg & 15) == 0 && (!d->disp || ((uintptr_t)d->out & 15) == 0);
  if (v4) hipLaunchKernelGGL((cs3d_labels_kernel<4>), dim3((unsigned)((hw / 4 + 255) / 256), (unsigned)d->B), dim3(256), 0, s, *d);
  else hipLaunchKernelGGL((cs3d_labels_kernel<1>), dim3((unsigned)((hw + 255) / 256), (unsigned)d->B), dim3(256), 0, s, *d);
  return (int)hipGetLastError();
}
