// Training-batch augmentation on the device: the per-sample numpy / OpenCV pipeline of the reference's get_transformations
// (TaskPrompter/utils/common_config.py:96-124, data/transforms.py) as one gather per output pixel.  Three entry points:
//   mtt_aug_select: which of the 11 crop candidates RandomCrop(cat_max_ratio) would have settled on
//   mtt_aug_image : scale (bilinear) -> crop -> flip -> photometric distortion -> normalise -> pad, HWC uint8 / fp32 -> NCHW fp32
//   mtt_aug_labels: scale (nearest) -> crop -> flip -> pad -> ignore regions, HWC fp32 -> NCHW fp32, once per task
// The random draws come from a table (include/mtt_hip.h), one row per sample; sources are ragged and packed, addressed by element
// offsets.  grid = (pixel blocks, B): a workgroup belongs to ONE sample, so the row is wave-uniform (scalar loads) and consecutive lanes
// write consecutive output pixels (4 each with one 16-byte store per channel when w % 4 == 0).  Reads are a gather by nature: along x
// they are unit-stride up to the scale factor.  Contraction is off for the whole file: every product and sum is rounded on its own, as
// numpy does, which is what makes the outputs equal the reference's bit for bit.
#include "mtt_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_DIM = 32768;        // dx * src < 2^31 in the nearest rule

MTT_DEV int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
MTT_DEV float bits2f(int32_t u) { return __builtin_bit_cast(float, u); }

// a table row, every value forced into the range the host check admits
struct Row {
  int H, W, Sh, Sw, resized, flip;
  int oy, ox, Hc, Wc, py0, px0;
};
MTT_DEV Row load_row(const int32_t* t, int h, int w, int cand) {
  Row r;
  r.H = clampi(t[MTT_AUG_H], 1, MAX_DIM);
  r.W = clampi(t[MTT_AUG_W], 1, MAX_DIM);
  r.resized = t[MTT_AUG_RESIZED] != 0;
  r.Sh = r.resized ? clampi(t[MTT_AUG_SH], 1, MAX_DIM) : r.H;
  r.Sw = r.resized ? clampi(t[MTT_AUG_SW], 1, MAX_DIM) : r.W;
  r.flip = t[MTT_AUG_FLIP] != 0;
  const int k = cand >= 0 ? cand : clampi(t[MTT_AUG_CHOSEN], 0, MTT_AUG_CANDS - 1);
  r.oy = clampi(t[MTT_AUG_CAND_Y + k], 0, max(r.Sh - h, 0));
  r.ox = clampi(t[MTT_AUG_CAND_X + k], 0, max(r.Sw - w, 0));
  r.Hc = min(r.Sh, h);
  r.Wc = min(r.Sw, w);
  r.py0 = (h - r.Hc) >> 1;
  r.px0 = (w - r.Wc) >> 1;
  return r;
}
// output pixel -> position on the scaled grid; false = padding
MTT_DEV bool to_scaled(const Row& r, int y, int x, int& Y, int& X) {
  const int py = y - r.py0, px = x - r.px0;
  if (py < 0 || py >= r.Hc || px < 0 || px >= r.Wc) return false;
  Y = r.oy + py;
  X = r.ox + (r.flip ? r.Wc - 1 - px : px);
  return true;
}
// INTER_NEAREST
MTT_DEV int near_src(int d, int src, int dst) { return min((d * src) / dst, src - 1); }
// INTER_LINEAR on 32f: the two taps and their weights along one axis
MTT_DEV void lin_taps(int d, int src, int dst, int& s0, int& s1, float& a0, float& a1) {
  float f = (float)(((double)d + 0.5) * ((double)src / (double)dst) - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) { s = 0; f = 0.f; }
  if (s >= src - 1) { s = src - 1; f = 0.f; }
  s0 = s;
  s1 = min(s + 1, src - 1);
  a0 = 1.f - f;
  a1 = f;
}
template <bool U8> MTT_DEV float fetch(const void* src, int64_t idx, int64_t numel) {
  idx = idx < 0 ? 0 : (idx >= numel ? numel - 1 : idx);
  if constexpr (U8) return (float)((const uint8_t*)src)[idx];
  else return ((const float*)src)[idx];
}

// ---- PhotoMetricDistortion on one 8-bit RGB pixel ---------------------------------------------------------------------------------------
// convert(): img.astype(float32) * alpha + beta, clip to [0, 255], astype(uint8)
MTT_DEV int conv8(int v, float alpha, float beta) {
  const float f = (float)v * alpha + beta;
  return (int)fminf(fmaxf(f, 0.f), 255.f);
}
// cvRound(n / d) for 0 < d: the entries of OpenCV's sdiv / hdiv tables (round half to even), entry 0 = 0
MTT_DEV int rdiv_even(int n, int d) {
  if (d <= 0) return 0;
  int q = n / d;
  const int r2 = 2 * (n - q * d);
  if (r2 > d || (r2 == d && (q & 1))) ++q;
  return q;
}
// the two tables, built once per workgroup in LDS (two divisions per thread instead of four per pixel)
struct HsvTables { int sdiv[256], hdiv[256]; };
MTT_DEV void build_tables(HsvTables& tab, int tid) {
  tab.sdiv[tid] = rdiv_even(255 << 12, tid);
  tab.hdiv[tid] = rdiv_even((180 << 12) / 6, tid);
}
MTT_DEV void rgb2hsv(const HsvTables& tab, int r, int g, int b, int& h, int& s, int& v) {
  v = max(r, max(g, b));
  const int diff = v - min(r, min(g, b));
  s = (diff * tab.sdiv[v] + (1 << 11)) >> 12;
  int hh = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
  hh = (hh * tab.hdiv[diff] + (1 << 11)) >> 12;                            // arithmetic shift: floor for the negative sector
  h = hh < 0 ? hh + 180 : hh;
  s = min(s, 255);
}
MTT_DEV int sat8(float f) { return (int)fminf(fmaxf(rintf(f), 0.f), 255.f); }
MTT_DEV void hsv2rgb(int hi, int si, int vi, int& r, int& g, int& b) {
  const float s = (float)si * (1.f / 255.f), v = (float)vi * (1.f / 255.f);
  float fr, fg, fb;
  if (si == 0) {
    fr = fg = fb = v;
  } else {
    float h = (float)hi * (6.f / 180.f);
    int sector = (int)floorf(h);
    h -= (float)sector;
    if ((unsigned)sector >= 6u) { sector = 0; h = 0.f; }
    const float t0 = v, t1 = v * (1.f - s), t2 = v * (1.f - s * h), t3 = v * (1.f - s * (1.f - h));
    // sector table of (b, g, r): {1,3,0} {1,0,2} {3,0,1} {0,2,1} {0,1,3} {2,1,0}
    fb = sector == 0 || sector == 1 ? t1 : (sector == 2 ? t3 : (sector == 5 ? t2 : t0));
    fg = sector == 0 ? t3 : (sector == 1 || sector == 2 ? t0 : (sector == 3 ? t2 : t1));
    fr = sector == 0 || sector == 5 ? t0 : (sector == 1 ? t2 : (sector == 4 ? t3 : t1));
  }
  r = sat8(fr * 255.f);
  g = sat8(fg * 255.f);
  b = sat8(fb * 255.f);
}
struct Photo { int bright, fmode, contrast, sat, hue, hdelta; float beta, calpha, salpha; };
MTT_DEV Photo load_photo(const int32_t* t) {
  Photo p;
  p.bright = t[MTT_AUG_BRIGHT] != 0;
  p.fmode = t[MTT_AUG_FMODE] != 0;
  p.contrast = t[MTT_AUG_CONTRAST] != 0;
  p.sat = t[MTT_AUG_SAT] != 0;
  p.hue = t[MTT_AUG_HUE] != 0;
  p.hdelta = clampi(t[MTT_AUG_HDELTA], -18, 17);
  p.beta = bits2f(t[MTT_AUG_BETA]);
  p.calpha = bits2f(t[MTT_AUG_CALPHA]);
  p.salpha = bits2f(t[MTT_AUG_SALPHA]);
  return p;
}
MTT_DEV void photometric(const Photo& p, const HsvTables& tab, int& r, int& g, int& b) {
  if (p.bright) { r = conv8(r, 1.f, p.beta); g = conv8(g, 1.f, p.beta); b = conv8(b, 1.f, p.beta); }
  if (p.fmode && p.contrast) { r = conv8(r, p.calpha, 0.f); g = conv8(g, p.calpha, 0.f); b = conv8(b, p.calpha, 0.f); }
  int h, s, v;
  if (p.sat) {
    rgb2hsv(tab, r, g, b, h, s, v);
    s = conv8(s, p.salpha, 0.f);
    hsv2rgb(h, s, v, r, g, b);
  }
  if (p.hue) {
    rgb2hsv(tab, r, g, b, h, s, v);
    h += p.hdelta;                                                          // (h + delta) % 180 with Python's sign: h in [-18, 196]
    h = h < 0 ? h + 180 : (h >= 180 ? h - 180 : h);
    hsv2rgb(h, s, v, r, g, b);
  }
  if (!p.fmode && p.contrast) { r = conv8(r, p.calpha, 0.f); g = conv8(g, p.calpha, 0.f); b = conv8(b, p.calpha, 0.f); }
}

template <int V> MTT_DEV void store_px(float* p, const float (&v)[V]) {
  if constexpr (V == 4) *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
  else p[0] = v[0];
}

// ---- image --------------------------------------------------------------------------------------------------------------------------------
template <int V, bool U8> __global__ __launch_bounds__(256) void aug_image_kernel(const mtt_aug_desc d) {
  __shared__ HsvTables tab;
  build_tables(tab, threadIdx.x);
  __syncthreads();
  const int b = blockIdx.y, hw = d.h * d.w;
  const int p = (blockIdx.x * 256 + threadIdx.x) * V;
  if (p >= hw) return;
  const int y = p / d.w, x0 = p - y * d.w;
  const int32_t* t = d.table + (int64_t)b * MTT_AUG_COLS;
  const Row r = load_row(t, d.h, d.w, -1);
  const Photo ph = load_photo(t);
  const int64_t off = d.off[b];
  float o[3][V];
#pragma unroll
  for (int i = 0; i < V; ++i) {
    int Y, X;
    if (!to_scaled(r, y, x0 + i, Y, X)) {
      o[0][i] = o[1][i] = o[2][i] = 0.f;
      continue;
    }
    float c[3];
    if (r.resized) {
      int y0, y1, xa, xb;
      float b0, b1, a0, a1;
      lin_taps(Y, r.H, r.Sh, y0, y1, b0, b1);
      lin_taps(X, r.W, r.Sw, xa, xb, a0, a1);
      const int64_t i00 = off + ((int64_t)y0 * r.W + xa) * 3, i01 = off + ((int64_t)y0 * r.W + xb) * 3;
      const int64_t i10 = off + ((int64_t)y1 * r.W + xa) * 3, i11 = off + ((int64_t)y1 * r.W + xb) * 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float top = a0 * fetch<U8>(d.src, i00 + k, d.src_numel) + a1 * fetch<U8>(d.src, i01 + k, d.src_numel);
        const float bot = a0 * fetch<U8>(d.src, i10 + k, d.src_numel) + a1 * fetch<U8>(d.src, i11 + k, d.src_numel);
        c[k] = b0 * top + b1 * bot;
      }
    } else {
      const int64_t i0 = off + ((int64_t)Y * r.W + X) * 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) c[k] = fetch<U8>(d.src, i0 + k, d.src_numel);
    }
    if (d.photometric) {
      int R = (int)fminf(fmaxf(c[0], 0.f), 255.f), G = (int)fminf(fmaxf(c[1], 0.f), 255.f), B = (int)fminf(fmaxf(c[2], 0.f), 255.f);
      photometric(ph, tab, R, G, B);
      c[0] = (float)R; c[1] = (float)G; c[2] = (float)B;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k][i] = __fdiv_rn(__fdiv_rn(c[k], 255.f) - d.mean[k], d.std[k]);
  }
  float* out = d.out + (int64_t)b * 3 * hw + p;
#pragma unroll
  for (int k = 0; k < 3; ++k) store_px<V>(out + (int64_t)k * hw, o[k]);
}

// ---- labels -------------------------------------------------------------------------------------------------------------------------------
template <int V, int C> __global__ __launch_bounds__(256) void aug_labels_kernel(const mtt_aug_desc d) {
  const int b = blockIdx.y, hw = d.h * d.w;
  const int p = (blockIdx.x * 256 + threadIdx.x) * V;
  bool labelled = false;
  if (p < hw) {
    const int y = p / d.w, x0 = p - y * d.w;
    const int32_t* t = d.table + (int64_t)b * MTT_AUG_COLS;
    const Row r = load_row(t, d.h, d.w, -1);
    const float scale = bits2f(t[MTT_AUG_SCALE]);
    const int64_t off = d.off[b];
    float o[C][V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
      int Y, X;
      float v[C];
      if (to_scaled(r, y, x0 + i, Y, X)) {
        const int sy = r.resized ? near_src(Y, r.H, r.Sh) : Y, sx = r.resized ? near_src(X, r.W, r.Sw) : X;
        const int64_t i0 = off + ((int64_t)sy * r.W + sx) * C;
#pragma unroll
        for (int k = 0; k < C; ++k) v[k] = fetch<false>(d.src, i0 + k, d.src_numel);
        if (d.kind == MTT_AUG_DEPTH && r.resized) v[0] = __fdiv_rn(v[0], scale);
        if (d.kind == MTT_AUG_NORMALS && r.flip) v[0] = v[0] * -1.f;
      } else {
#pragma unroll
        for (int k = 0; k < C; ++k) v[k] = d.fill;
      }
      if constexpr (C == 3) {
        if (d.kind == MTT_AUG_NORMALS && v[0] * v[0] + v[1] * v[1] + v[2] * v[2] == 0.f) v[0] = v[1] = v[2] = 255.f;
      }
      if (d.kind == MTT_AUG_DEPTH && d.depth_ignore && v[0] == 0.f) v[0] = -1.f;
      labelled |= v[0] != 0.f && v[0] != 255.f;
#pragma unroll
      for (int k = 0; k < C; ++k) o[k][i] = v[k];
    }
    float* out = d.out + (int64_t)b * C * hw + p;
#pragma unroll
    for (int k = 0; k < C; ++k) store_px<V>(out + (int64_t)k * hw, o[k]);
  }
  if (d.kind == MTT_AUG_HUMAN_PARTS) {                   // wave-uniform: every thread of the workgroup arrives
    if (__syncthreads_or(labelled) && threadIdx.x == 0) atomicOr(&d.flags[b], 1);
  }
}
// AddIgnoreRegions, human_parts: an image without a single part label is ignored as a whole
template <int V> __global__ __launch_bounds__(256) void aug_fill_unlabelled_kernel(float* out, const int32_t* flags, int hw) {
  const int b = blockIdx.y;
  const int p = (blockIdx.x * 256 + threadIdx.x) * V;
  if (p >= hw || flags[b] != 0) return;
  float v[V];
#pragma unroll
  for (int i = 0; i < V; ++i) v[i] = 255.f;
  store_px<V>(out + (int64_t)b * hw + p, v);
}

// ---- crop selection -------------------------------------------------------------------------------------------------------------------------
// grid (10, B): workgroup (k, b) histograms candidate k of sample b.  Lanes of a wave that hold the label of its first active lane add
// their count with ONE LDS atomic (a failing window is mostly one class: 64 same-address atomics would serialise), the rest add singly.
__global__ __launch_bounds__(256) void aug_select_kernel(const mtt_aug_desc d) {
  __shared__ int hist[256];
  __shared__ int n_cls, c_max, c_sum;
  const int b = blockIdx.y, k = blockIdx.x, tid = threadIdx.x;
  int32_t* t = d.table + (int64_t)b * MTT_AUG_COLS;
  if (t[MTT_AUG_NTEST] != MTT_AUG_CANDS - 1) return;     // uniform over the workgroup
  const Row r = load_row(t, d.h, d.w, k);
  const int64_t off = d.off[b];
  hist[tid] = 0;
  if (tid == 0) { n_cls = 0; c_max = 0; c_sum = 0; }
  __syncthreads();
  // a thread walks down columns px = tid, tid + 256, ...: a wave reads 64 consecutive pixels of a row, and the nearest rule advances along
  // y by a quotient / remainder step (floor((Y + 1) * H / Sh) from floor(Y * H / Sh)) instead of a division per pixel.  ROWS rows'
  // loads are issued before their atomics (measured on the 126 x 512^2 batch of tools/augment_bench.py: 4 rows 389 us, 16 rows 367 us;
  // one division per pixel and axis instead of the stepping: 730 us).
  constexpr int ROWS = 16;
  const int step_q = r.H / r.Sh, step_r = r.H % r.Sh;
  auto count = [&](int label) {
    label = clampi(label, 0, 255);
    const int first = __builtin_amdgcn_readfirstlane(label);
    const unsigned long long same = __ballot(label == first);
    if (label != first) atomicAdd(&hist[label], 1);
    else if ((int)__lane_id() == __ffsll((long long)same) - 1) atomicAdd(&hist[first], (int)__popcll(same));
  };
  for (int px = tid; px < r.Wc; px += 256) {
    const int sx = near_src(r.ox + px, r.W, r.Sw);          // the identity when the sample is not resized (Sw == W)
    const int64_t col = off + sx;
    int q = (r.oy * r.H) / r.Sh, rem = (r.oy * r.H) % r.Sh;
    auto next_row = [&]() {
      const int sy = min(q, r.H - 1);
      q += step_q;
      rem += step_r;
      if (rem >= r.Sh) { rem -= r.Sh; ++q; }
      return col + (int64_t)sy * r.W;
    };
    int py = 0;
    for (; py + ROWS <= r.Hc; py += ROWS) {
      float v[ROWS];
#pragma unroll
      for (int j = 0; j < ROWS; ++j) v[j] = fetch<false>(d.src, next_row(), d.src_numel);
#pragma unroll
      for (int j = 0; j < ROWS; ++j) count((int)v[j]);
    }
    for (; py < r.Hc; ++py) count((int)fetch<false>(d.src, next_row(), d.src_numel));
  }
  __syncthreads();
  const int c = tid == 255 ? 0 : hist[tid];               // cnt[labels != 255]
  if (c > 0) {
    atomicAdd(&n_cls, 1);
    atomicMax(&c_max, c);
    atomicAdd(&c_sum, c);
  }
  __syncthreads();
  if (tid == 0 && n_cls > 1 && (double)c_max / (double)c_sum < d.cat_max_ratio) atomicMin(&t[MTT_AUG_CHOSEN], k);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
bool is01(int32_t v) { return v == 0 || v == 1; }

int check(const mtt_aug_desc* d) {
  if (!d || !d->src || !d->off || !d->off_host || !d->table || !d->table_host || d->src_numel <= 0) return MTT_E_BADARG;
  if (d->B <= 0 || d->B > 65535 || d->h <= 0 || d->w <= 0 || d->h > MAX_DIM || d->w > MAX_DIM || d->C <= 0) return MTT_E_BADARG;
  for (int b = 0; b < d->B; ++b) {
    const int32_t* t = d->table_host + (int64_t)b * MTT_AUG_COLS;
    const int64_t H = t[MTT_AUG_H], W = t[MTT_AUG_W], Sh = t[MTT_AUG_SH], Sw = t[MTT_AUG_SW], off = d->off_host[b];
    if (H < 1 || W < 1 || Sh < 1 || Sw < 1 || H > MAX_DIM || W > MAX_DIM || Sh > MAX_DIM || Sw > MAX_DIM) return MTT_E_BADARG;
    if (off < 0 || off > d->src_numel || H * W * d->C > d->src_numel - off) return MTT_E_BADARG;
    if (!is01(t[MTT_AUG_RESIZED]) || !is01(t[MTT_AUG_FLIP]) || !is01(t[MTT_AUG_BRIGHT]) || !is01(t[MTT_AUG_FMODE]) || !is01(t[MTT_AUG_CONTRAST]) ||
        !is01(t[MTT_AUG_SAT]) || !is01(t[MTT_AUG_HUE]))
      return MTT_E_BADARG;
    if (!t[MTT_AUG_RESIZED] && (Sh != H || Sw != W)) return MTT_E_BADARG;
    if (t[MTT_AUG_NTEST] != 0 && t[MTT_AUG_NTEST] != MTT_AUG_CANDS - 1) return MTT_E_BADARG;
    if (t[MTT_AUG_CHOSEN] < 0 || t[MTT_AUG_CHOSEN] >= MTT_AUG_CANDS) return MTT_E_BADARG;
    if (t[MTT_AUG_HDELTA] < -18 || t[MTT_AUG_HDELTA] > 17) return MTT_E_BADARG;
    const int64_t my = Sh > d->h ? Sh - d->h : 0, mx = Sw > d->w ? Sw - d->w : 0;
    for (int k = 0; k < MTT_AUG_CANDS; ++k)
      if (t[MTT_AUG_CAND_Y + k] < 0 || t[MTT_AUG_CAND_Y + k] > my || t[MTT_AUG_CAND_X + k] < 0 || t[MTT_AUG_CAND_X + k] > mx) return MTT_E_BADARG;
  }
  return 0;
}
bool vec4(const mtt_aug_desc* d) { return d->w % 4 == 0 && ((uintptr_t)d->out & 15) == 0; }
dim3 px_grid(const mtt_aug_desc* d, int V) { return dim3((unsigned)(((int64_t)d->h * d->w / V + 255) / 256), (unsigned)d->B); }

}  // namespace

extern "C" size_t mtt_aug_desc_size(void) { return sizeof(mtt_aug_desc); }

extern "C" int mtt_aug_select(const mtt_aug_desc* d, void* stream) {
  if (const int rc = check(d)) return rc;
  if (d->C != 1 || d->src_u8 || !(d->cat_max_ratio == d->cat_max_ratio)) return MTT_E_BADARG;
  hipLaunchKernelGGL(aug_select_kernel, dim3(MTT_AUG_CANDS - 1, (unsigned)d->B), dim3(256), 0, (hipStream_t)stream, *d);
  return (int)hipGetLastError();
}

extern "C" int mtt_aug_image(const mtt_aug_desc* d, void* stream) {
  if (const int rc = check(d)) return rc;
  if (d->C != 3 || !d->out) return MTT_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  if (vec4(d)) {
    if (d->src_u8) hipLaunchKernelGGL((aug_image_kernel<4, true>), px_grid(d, 4), dim3(256), 0, s, *d);
    else hipLaunchKernelGGL((aug_image_kernel<4, false>), px_grid(d, 4), dim3(256), 0, s, *d);
  } else {
    if (d->src_u8) hipLaunchKernelGGL((aug_image_kernel<1, true>), px_grid(d, 1), dim3(256), 0, s, *d);
    else hipLaunchKernelGGL((aug_image_kernel<1, false>), px_grid(d, 1), dim3(256), 0, s, *d);
  }
  return (int)hipGetLastError();
}

extern "C" int mtt_aug_labels(const mtt_aug_desc* d, void* stream) {
  if (const int rc = check(d)) return rc;
  if (!d->out || d->src_u8 || d->kind < MTT_AUG_PLAIN || d->kind > MTT_AUG_HUMAN_PARTS) return MTT_E_BADARG;
  if (d->C != (d->kind == MTT_AUG_NORMALS ? 3 : 1)) return MTT_E_UNSUPPORTED;
  if (d->kind == MTT_AUG_HUMAN_PARTS && !d->flags) return MTT_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  const bool v4 = vec4(d);
  if (d->kind == MTT_AUG_HUMAN_PARTS) {
    const hipError_t e = hipMemsetAsync(d->flags, 0, sizeof(int32_t) * (size_t)d->B, s);
    if (e != hipSuccess) return (int)e;
  }
  if (d->C == 3) {
    if (v4) hipLaunchKernelGGL((aug_labels_kernel<4, 3>), px_grid(d, 4), dim3(256), 0, s, *d);
    else hipLaunchKernelGGL((aug_labels_kernel<1, 3>), px_grid(d, 1), dim3(256), 0, s, *d);
  } else {
    if (v4) hipLaunchKernelGGL((aug_labels_kernel<4, 1>), px_grid(d, 4), dim3(256), 0, s, *d);
    else hipLaunchKernelGGL((aug_labels_kernel<1, 1>), px_grid(d, 1), dim3(256), 0, s, *d);
  }
  if (d->kind == MTT_AUG_HUMAN_PARTS) {
    const int hw = d->h * d->w;
    if (v4) hipLaunchKernelGGL((aug_fill_unlabelled_kernel<4>), px_grid(d, 4), dim3(256), 0, s, d->out, d->flags, hw);
    else hipLaunchKernelGGL((aug_fill_unlabelled_kernel<1>), px_grid(d, 1), dim3(256), 0, s, d->out, d->flags, hw);
  }
  return (int)hipGetLastError();
}
