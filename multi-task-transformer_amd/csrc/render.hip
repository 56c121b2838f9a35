// Rendering predictions on the device: what the reference does to a prediction before it is encoded into a file
// (TaskPrompter/utils/visualization_utils.py:122-198 and evaluation/evaluate_utils.py:126-154: F.interpolate to the image size,
// get_output, .cpu(), a numpy colour-table lookup, astype(uint8)) in one pass over the fp32 NCHW logits.  Two entry points
// (include/mtt_hip.h):
//   mtt_render_map    : bilinear interpolation -> get_output's rule -> class index / table entry / truncated byte / fp32 depth
//   mtt_render_minmax : per-image minimum and maximum of the interpolated, clamped depth map (the range of its colour index)
// A wave owns consecutive x of ONE output row, so that every channel plane is read in contiguous runs; a workgroup is four such waves
// on four consecutive rows.  The taps of the row and of the thread's columns are computed once, before the loop over the channels,
// which keeps only the running maximum and its index (or the one, two or three values of the other modes) in registers.  Nothing
// wider than the output itself is written.
#include "mtt_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_DIM = 32768;
constexpr int ROWS = 4;                 // waves of a workgroup, one output row each

struct Window { int y0, x0, ho, wo; int64_t off; };

// image b's window, from the device copy of the table, checked against the grid and the output once more (the host copy was, before the launch)
MTT_DEV bool window_of(const mtt_render_desc& d, int b, bool writes, Window& win) {
  if (!d.win) {
    win = {0, 0, d.H, d.W, (int64_t)b * d.H * d.W};
    return true;
  }
  const int64_t* t = d.win + 5 * (int64_t)b;
  const int64_t y0 = t[0], x0 = t[1], ho = t[2], wo = t[3], off = t[4];
  if (y0 < 0 || x0 < 0 || ho <= 0 || wo <= 0 || y0 + ho > d.H || x0 + wo > d.W) return false;
  if (writes && (off < 0 || off + ho * wo > d.out_pixels)) return false;
  win = {(int)y0, (int)x0, (int)ho, (int)wo, off};
  return true;
}

struct Tap { int i0, i1; float w0, w1; };

// PyTorch's align_corners = False source index and weights (area_pixel_compute_source_index, guard_index_and_lambda)
MTT_DEV Tap tap_of(int dst, float scale, int in) {
  float s = scale * ((float)dst + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  const int i0 = min((int)s, in - 1);
  const float l = fminf(fmaxf(s - (float)i0, 0.f), 1.f);
  return {i0, min(i0 + 1, in - 1), 1.f - l, l};
}

// two neighbouring source pixels in one 8-byte load (4-byte aligned: the hardware takes it, the type says so)
struct __attribute__((packed, aligned(4))) Pair { float a, b; };

// the PX values of one channel plane at output row y, columns x .. x + PX - 1
template <int PX, bool IDENT> struct Fetch {
  int64_t r0, r1;                        // element offsets of the two source rows inside a plane
  float wy0, wy1;
  int i0[PX];                            // the column of the pair's first pixel: min(lower tap, w - 2)
  bool last[PX];                         // the lower tap is the last column (both taps read it): take the pair's second pixel twice
  float wx0[PX], wx1[PX];
  bool pairs;                            // w >= 2

  MTT_DEV Fetch(const mtt_render_desc& d, int x) {
    r0 = r1 = 0; wy0 = wy1 = 0.f; pairs = d.w >= 2;
    if constexpr (!IDENT) {
      const float sx = __fdiv_rn((float)d.w, (float)d.W);
#pragma unroll
      for (int j = 0; j < PX; ++j) {
        const Tap tx = tap_of(x + j, sx, d.w);
        last[j] = pairs && tx.i0 == d.w - 1;
        i0[j] = last[j] ? d.w - 2 : tx.i0;
        wx0[j] = tx.w0; wx1[j] = tx.w1;
      }
    }
  }

  MTT_DEV void row(const mtt_render_desc& d, int y, int x) {
    if constexpr (IDENT) {
      r0 = (int64_t)y * d.w + x;
    } else {
      const Tap ty = tap_of(y, __fdiv_rn((float)d.h, (float)d.H), d.h);
      r0 = (int64_t)ty.i0 * d.w; r1 = (int64_t)ty.i1 * d.w; wy0 = ty.w0; wy1 = ty.w1;
    }
  }

  MTT_DEV void get(const float* plane, float (&v)[PX]) const {
    if constexpr (IDENT) {
      if constexpr (PX == 4) {
        const float4 q = *(const float4*)(plane + r0);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      } else {
        v[0] = plane[r0];
      }
    } else {
      const float* p0 = plane + r0;
      const float* p1 = plane + r1;
#pragma unroll
      for (int j = 0; j < PX; ++j) {
        float a0, b0, a1, b1;
        if (pairs) {
          const Pair q0 = *(const Pair*)(p0 + i0[j]), q1 = *(const Pair*)(p1 + i0[j]);
          a0 = last[j] ? q0.b : q0.a; b0 = q0.b;
          a1 = last[j] ? q1.b : q1.a; b1 = q1.b;
        } else {                                            // a source of one column
          a0 = b0 = p0[0]; a1 = b1 = p1[0];
        }
        const float t0 = a0 * wx0[j] + b0 * wx1[j];         // horizontal pair first, then the vertical one
        const float t1 = a1 * wx0[j] + b1 * wx1[j];
        v[j] = t0 * wy0 + t1 * wy1;
      }
    }
  }
};

MTT_DEV unsigned trunc8(float v) { const int i = (int)v; return (unsigned)(i < 0 ? 0 : (i > 255 ? 255 : i)); }      // astype(np.uint8) on [0, 255]
MTT_DEV float clamp0(float v) { return v > 0.f ? v : 0.f; }             // -0 and NaN become +0: the bit pattern then orders as an unsigned integer

template <int PX> MTT_DEV void store_bytes(uint8_t* out, int64_t pix, const unsigned (&v)[PX]) {
  if constexpr (PX == 4) *(unsigned*)(out + pix) = v[0] | v[1] << 8 | v[2] << 16 | v[3] << 24;
  else out[pix] = (uint8_t)v[0];
}

// 3-byte pixels: a thread's 4 pixels are 12 consecutive bytes, a wave's stores 768 without a gap
template <int PX> MTT_DEV void store_rgb(uint8_t* out, int64_t pix, const unsigned (&c)[3][PX]) {
  if constexpr (PX == 4) {
    unsigned* q = (unsigned*)(out + 3 * pix);
    q[0] = c[0][0] | c[1][0] << 8 | c[2][0] << 16 | c[0][1] << 24;
    q[1] = c[1][1] | c[2][1] << 8 | c[0][2] << 16 | c[1][2] << 24;
    q[2] = c[2][2] | c[0][3] << 8 | c[1][3] << 16 | c[2][3] << 24;
  } else {
    uint8_t* q = out + 3 * pix;
    q[0] = (uint8_t)c[0][0]; q[1] = (uint8_t)c[1][0]; q[2] = (uint8_t)c[2][0];
  }
}

// grid (ceil(max W_out / (64 PX)), ceil(max H_out / ROWS), B)
template <int MODE, int PX, bool IDENT> __global__ __launch_bounds__(64 * ROWS) void render_map_kernel(const mtt_render_desc d) {
  const int b = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  Window win;
  if (!window_of(d, b, true, win)) return;
  const int oy = blockIdx.y * ROWS + wave, ox = (blockIdx.x * 64 + lane) * PX;
  if (oy >= win.ho || ox + PX > win.wo) return;
  Fetch<PX, IDENT> f(d, win.x0 + ox);
  f.row(d, win.y0 + oy, win.x0 + ox);
  const int64_t hw = (int64_t)d.h * d.w;
  const float* src = d.src + (int64_t)b * d.C * hw;
  const int64_t pix = win.off + (int64_t)oy * win.wo + ox;
  uint8_t* out = (uint8_t*)d.out;

  if constexpr (MODE == MTT_RENDER_CLASS) {
    float best[PX], v[PX];
    unsigned idx[PX];
    f.get(src, best);
#pragma unroll
    for (int j = 0; j < PX; ++j) idx[j] = 0;
    constexpr int UNROLL = IDENT ? 4 : 1;                   // with taps one channel is 4 PX loads already
#pragma unroll UNROLL
    for (int c = 1; c < d.C; ++c) {
      f.get(src + c * hw, v);
#pragma unroll
      for (int j = 0; j < PX; ++j)
        if (v[j] > best[j]) { best[j] = v[j]; idx[j] = (unsigned)c; }      // strictly greater: the first index wins ties
    }
    if (d.out_kind == MTT_RENDER_OUT_LUT3) {
      unsigned c3[3][PX];
#pragma unroll
      for (int j = 0; j < PX; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) c3[k][j] = d.table[3 * (idx[j] & 255u) + k];
      store_rgb<PX>(out, pix, c3);
    } else {
      if (d.out_kind == MTT_RENDER_OUT_LUT1) {
#pragma unroll
        for (int j = 0; j < PX; ++j) idx[j] = d.table[idx[j] & 255u];
      }
      store_bytes<PX>(out, pix, idx);
    }
  } else if constexpr (MODE == MTT_RENDER_SIGMOID255) {
    float v[PX];
    unsigned o[PX];
    f.get(src, v);
#pragma unroll
    for (int j = 0; j < PX; ++j) o[j] = trunc8(__fdiv_rn(255.f, 1.f + expf(-v[j])));
    store_bytes<PX>(out, pix, o);
  } else if constexpr (MODE == MTT_RENDER_SOFTMAX1_255) {
    float v0[PX], v1[PX];
    unsigned o[PX];
    f.get(src, v0);
    f.get(src + hw, v1);
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      const float m = fmaxf(v0[j], v1[j]);
      const float e0 = expf(v0[j] - m), e1 = expf(v1[j] - m);
      o[j] = trunc8(__fdiv_rn(e1, e0 + e1) * 255.f);
    }
    store_bytes<PX>(out, pix, o);
  } else if constexpr (MODE == MTT_RENDER_NORMALS) {
    float v[3][PX];
    unsigned c3[3][PX];
#pragma unroll
    for (int k = 0; k < 3; ++k) f.get(src + k * hw, v[k]);
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      const float n = fmaxf(__fsqrt_rn(v[0][j] * v[0][j] + v[1][j] * v[1][j] + v[2][j] * v[2][j]), 1e-12f);
#pragma unroll
      for (int k = 0; k < 3; ++k) c3[k][j] = trunc8(__fdiv_rn((__fdiv_rn(v[k][j], n) + 1.f) * 255.f, 2.f));
      if (d.swap_rb) { const unsigned t = c3[0][j]; c3[0][j] = c3[2][j]; c3[2][j] = t; }
    }
    store_rgb<PX>(out, pix, c3);
  } else {                                                  // MTT_RENDER_DEPTH
    float v[PX];
    f.get(src, v);
#pragma unroll
    for (int j = 0; j < PX; ++j) v[j] = clamp0(v[j]);
    if (d.out_kind == MTT_RENDER_OUT_F32) {
      float* o = (float*)d.out + pix;
      if constexpr (PX == 4) *(float4*)o = make_float4(v[0], v[1], v[2], v[3]);
      else o[0] = v[0];
    } else {
      const float lo = __uint_as_float(d.minmax[b]), hi = __uint_as_float(d.minmax[d.B + b]);
      const float range = hi - lo;
      unsigned idx[PX];
#pragma unroll
      for (int j = 0; j < PX; ++j) idx[j] = range > 0.f ? trunc8(__fdiv_rn(v[j] - lo, range) * 255.f) : 0u;      // a constant map: index 0
      if (d.out_kind == MTT_RENDER_OUT_LUT3) {
        unsigned c3[3][PX];
#pragma unroll
        for (int j = 0; j < PX; ++j)
#pragma unroll
          for (int k = 0; k < 3; ++k) c3[k][j] = d.table[3 * idx[j] + k];
        store_rgb<PX>(out, pix, c3);
      } else {
        store_bytes<PX>(out, pix, idx);
      }
    }
  }
}

// the same pixels as render_map_kernel<DEPTH>.  grid (as render_map_kernel, but y capped: a wave walks over rows); a wave folds its values
// with shuffles, the workgroup its four waves through LDS, and one thread issues the integer atomic pair: a few hundred per image, so that
// the atomics on the two words of an image do not queue up
template <int PX, bool IDENT> __global__ __launch_bounds__(64 * ROWS) void render_minmax_kernel(const mtt_render_desc d) {
  __shared__ unsigned part[2][ROWS];
  const int b = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  Window win;
  if (!window_of(d, b, false, win)) return;                 // the same in every thread of the workgroup
  const int ox = (blockIdx.x * 64 + lane) * PX;
  unsigned lo = 0xffffffffu, hi = 0u;
  if (ox + PX <= win.wo) {
    Fetch<PX, IDENT> f(d, win.x0 + ox);
    const float* src = d.src + (int64_t)b * d.h * d.w;
    for (int oy = blockIdx.y * ROWS + wave; oy < win.ho; oy += gridDim.y * ROWS) {
      f.row(d, win.y0 + oy, win.x0 + ox);
      float v[PX];
      f.get(src, v);
#pragma unroll
      for (int j = 0; j < PX; ++j) {
        const unsigned u = __float_as_uint(clamp0(v[j]));
        lo = min(lo, u);
        hi = max(hi, u);
      }
    }
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    lo = min(lo, (unsigned)__shfl_xor((int)lo, s, 64));
    hi = max(hi, (unsigned)__shfl_xor((int)hi, s, 64));
  }
  if (lane == 0) { part[0][wave] = lo; part[1][wave] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 1; k < ROWS; ++k) { lo = min(lo, part[0][k]); hi = max(hi, part[1][k]); }
    atomicMin(&d.minmax[b], lo);
    atomicMax(&d.minmax[d.B + b], hi);
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
struct Plan { bool vec, ident; int max_ho, max_wo; };

int check(const mtt_render_desc* d, bool map, Plan& plan) {
  if (!d || !d->src) return MTT_E_BADARG;
  if (d->B <= 0 || d->B > 65535 || d->C <= 0) return MTT_E_BADARG;
  if (d->h <= 0 || d->w <= 0 || d->H <= 0 || d->W <= 0 || d->h > MAX_DIM || d->w > MAX_DIM || d->H > MAX_DIM || d->W > MAX_DIM) return MTT_E_BADARG;
  if ((uintptr_t)d->src & 3) return MTT_E_ALIGN;
  int bytes_per_pixel = 0;                                  // of out; 0 = none (minmax)
  if (map) {
    if (!d->out) return MTT_E_BADARG;
    const int k = d->out_kind;
    switch (d->mode) {
      case MTT_RENDER_CLASS:
        if (k != MTT_RENDER_OUT_U8 && k != MTT_RENDER_OUT_LUT1 && k != MTT_RENDER_OUT_LUT3) return MTT_E_BADARG;
        if (d->C > 256) return MTT_E_UNSUPPORTED;            // the index is a byte
        break;
      case MTT_RENDER_SIGMOID255:
        if (k != MTT_RENDER_OUT_U8 || d->C != 1) return MTT_E_BADARG;
        break;
      case MTT_RENDER_SOFTMAX1_255:
        if (k != MTT_RENDER_OUT_U8 || d->C < 2) return MTT_E_BADARG;
        if (d->C > 2) return MTT_E_UNSUPPORTED;              // the two-channel saliency head only
        break;
      case MTT_RENDER_NORMALS:
        if (k != MTT_RENDER_OUT_RGB3 || d->C != 3) return MTT_E_BADARG;
        break;
      case MTT_RENDER_DEPTH:
        if ((k != MTT_RENDER_OUT_U8 && k != MTT_RENDER_OUT_LUT3 && k != MTT_RENDER_OUT_F32) || d->C != 1) return MTT_E_BADARG;
        if (k != MTT_RENDER_OUT_F32 && !d->minmax) return MTT_E_BADARG;
        break;
      default:
        return MTT_E_BADARG;
    }
    if ((k == MTT_RENDER_OUT_LUT1 || k == MTT_RENDER_OUT_LUT3) && !d->table) return MTT_E_BADARG;
    bytes_per_pixel = k == MTT_RENDER_OUT_F32 ? 4 : (k == MTT_RENDER_OUT_LUT3 || k == MTT_RENDER_OUT_RGB3 ? 3 : 1);
    if (k == MTT_RENDER_OUT_F32 && ((uintptr_t)d->out & 3)) return MTT_E_ALIGN;
  } else {
    if (d->C != 1 || !d->minmax) return MTT_E_BADARG;
  }
  if (d->minmax && ((uintptr_t)d->minmax & 3)) return MTT_E_ALIGN;
  if (!d->win != !d->win_host) return MTT_E_BADARG;
  plan.ident = d->h == d->H && d->w == d->W;
  plan.vec = d->W % 4 == 0 && (!plan.ident || ((uintptr_t)d->src & 15) == 0) && (bytes_per_pixel == 0 || ((uintptr_t)d->out & 15) == 0);
  if (!d->win_host) {
    if (map && (d->out_pixels < 0 || (int64_t)d->B * d->H * d->W > d->out_pixels)) return MTT_E_BADARG;
    plan.max_ho = d->H;
    plan.max_wo = d->W;
    return 0;
  }
  plan.max_ho = plan.max_wo = 0;
  for (int b = 0; b < d->B; ++b) {
    const int64_t* t = d->win_host + 5 * (int64_t)b;
    const int64_t y0 = t[0], x0 = t[1], ho = t[2], wo = t[3], off = t[4];
    if (y0 < 0 || x0 < 0 || ho <= 0 || wo <= 0 || y0 + ho > d->H || x0 + wo > d->W) return MTT_E_BADARG;
    if (map && (off < 0 || d->out_pixels < 0 || off + ho * wo > d->out_pixels)) return MTT_E_BADARG;
    plan.vec = plan.vec && x0 % 4 == 0 && wo % 4 == 0 && (!map || off % 4 == 0);
    plan.max_ho = ho > plan.max_ho ? (int)ho : plan.max_ho;
    plan.max_wo = wo > plan.max_wo ? (int)wo : plan.max_wo;
  }
  return 0;
}

dim3 grid_of(const Plan& p, int B) {
  const int per_wave = 64 * (p.vec ? 4 : 1);
  return dim3((unsigned)((p.max_wo + per_wave - 1) / per_wave), (unsigned)((p.max_ho + ROWS - 1) / ROWS), (unsigned)B);
}

template <int MODE> void launch_map(const mtt_render_desc& d, const Plan& p, hipStream_t s) {
  const dim3 grid = grid_of(p, d.B), block(64 * ROWS);
  if (p.vec && p.ident) hipLaunchKernelGGL((render_map_kernel<MODE, 4, true>), grid, block, 0, s, d);
  else if (p.vec) hipLaunchKernelGGL((render_map_kernel<MODE, 4, false>), grid, block, 0, s, d);
  else if (p.ident) hipLaunchKernelGGL((render_map_kernel<MODE, 1, true>), grid, block, 0, s, d);
  else hipLaunchKernelGGL((render_map_kernel<MODE, 1, false>), grid, block, 0, s, d);
}

}  // namespace

extern "C" size_t mtt_render_desc_size(void) { return sizeof(mtt_render_desc); }

extern "C" int mtt_render_map(const mtt_render_desc* d, void* stream) {
  Plan p;
  if (const int rc = check(d, true, p)) return rc;
  hipStream_t s = (hipStream_t)stream;
  switch (d->mode) {
    case MTT_RENDER_CLASS: launch_map<MTT_RENDER_CLASS>(*d, p, s); break;
    case MTT_RENDER_SIGMOID255: launch_map<MTT_RENDER_SIGMOID255>(*d, p, s); break;
    case MTT_RENDER_SOFTMAX1_255: launch_map<MTT_RENDER_SOFTMAX1_255>(*d, p, s); break;
    case MTT_RENDER_NORMALS: launch_map<MTT_RENDER_NORMALS>(*d, p, s); break;
    default: launch_map<MTT_RENDER_DEPTH>(*d, p, s); break;
  }
  return (int)hipGetLastError();
}

extern "C" int mtt_render_minmax(const mtt_render_desc* d, void* stream) {
  Plan p;
  if (const int rc = check(d, false, p)) return rc;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(d->minmax, 0xff, sizeof(uint32_t) * (size_t)d->B, s);
  if (e == hipSuccess) e = hipMemsetAsync(d->minmax + d->B, 0, sizeof(uint32_t) * (size_t)d->B, s);
  if (e != hipSuccess) return (int)e;
  dim3 grid = grid_of(p, d->B);
  const dim3 block(64 * ROWS);
  const unsigned cap = 256u / grid.x;                       // about 256 workgroups, and as many atomic pairs, per image
  grid.y = grid.y < (cap ? cap : 1u) ? grid.y : (cap ? cap : 1u);
  if (p.vec && p.ident) hipLaunchKernelGGL((render_minmax_kernel<4, true>), grid, block, 0, s, *d);
  else if (p.vec) hipLaunchKernelGGL((render_minmax_kernel<4, false>), grid, block, 0, s, *d);
  else if (p.ident) hipLaunchKernelGGL((render_minmax_kernel<1, true>), grid, block, 0, s, *d);
  else hipLaunchKernelGGL((render_minmax_kernel<1, false>), grid, block, 0, s, *d);
  return (int)hipGetLastError();
}
