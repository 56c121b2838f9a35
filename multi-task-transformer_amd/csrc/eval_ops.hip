// Evaluation of the dense tasks straight from the full-resolution logits (ABI 17): the maps of the reference's get_output
// (TaskPrompter/utils/utils.py:27-63) and the running statistics of its meters (evaluation/eval_*.py).  Two entry points:
//   mtt_eval_map  : logits -> the map get_output returns
//   mtt_eval_accum: one batch added to a meter's accumulator, from the logits (fused) or from the map mtt_eval_map wrote
// pred fp32 NCHW [B, C, HW], label fp32 [B, Cl, HW].  One thread per pixel as in loss.hip (four consecutive pixels with 16-byte loads when
// the rows are aligned): the C logits of a pixel are strided by HW, so a wave reads C coalesced 256-byte (1 KiB) rows.  The per-pixel
// value of a map is ONE device function per task, called by the map kernel and by the from-logits accumulate; the from-map accumulate
// loads what that function stored, so both sources run the same arithmetic on the same fp32 value.  Contraction is off for the whole
// file: an FMA formed across the map / meter boundary in the fused path only would break that equality, and the reference's torch ops
// round every product too.
#include "mtt_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_CLASSES = 256, MAX_THRESH = 255;
constexpr int MAX_SUMS = 5;          // fp64 partials per workgroup: the count and up to four sums

// Pixels per thread: 4 with 16-byte loads when HW is a multiple of 4 and every buffer is 16-byte aligned (rows of all channels and images
// then start aligned), else 1.  MTT_EVAL_VEC=0 compiles the one-pixel form only (tools/eval_bench.py --lib, for A/B).
#ifndef MTT_EVAL_VEC
#define MTT_EVAL_VEC 1
#endif

template <int V> struct Px { float v[V]; };
template <int V> MTT_DEV Px<V> ldv(const float* p) {
  Px<V> r;
  if constexpr (V == 4) { const float4 t = *(const float4*)p; r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w; }
  else r.v[0] = p[0];
  return r;
}
template <int V> MTT_DEV void stv(float* p, const Px<V>& r) {
  if constexpr (V == 4) *(float4*)p = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
  else p[0] = r.v[0];
}
struct alignas(16) I64x2 { int64_t a, b; };

// ---- per-pixel map values -------------------------------------------------------------------------------------------------------------
// torch.max over the class axis: the first index wins ties, a NaN wins over every number
template <int V> MTT_DEV void pix_argmax(const float* x, int C, int64_t HW, int (&arg)[V]) {
  Px<V> best = ldv<V>(x);
#pragma unroll
  for (int i = 0; i < V; ++i) arg[i] = 0;
#pragma unroll 4
  for (int c = 1; c < C; ++c) {
    const Px<V> v = ldv<V>(x + (int64_t)c * HW);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const bool take = v.v[i] > best.v[i] || (v.v[i] != v.v[i] && best.v[i] == best.v[i]);
      best.v[i] = take ? v.v[i] : best.v[i];
      arg[i] = take ? c : arg[i];
    }
  }
}
// F.softmax over two classes (subtract the max), channel 1, * 255
MTT_DEV float pix_sal(float a, float b) {
  const float m = fmaxf(a, b);
  const float ea = expf(a - m), eb = expf(b - m);
  return eb / (ea + eb) * 255.0f;
}
MTT_DEV float pix_depth(float x) { return x < 0.0f ? 0.0f : x; }               // clamp_(min=0)
MTT_DEV float pix_edge(float x) { return 255.0f / (1.0f + expf(-x)); }
// (F.normalize(x, p=2) + 1) * 255 / 2
MTT_DEV void pix_normals(float a, float b, float c, float (&m)[3]) {
  const float nrm = fmaxf(sqrtf(a * a + b * b + c * c), 1e-12f);
  m[0] = (a / nrm + 1.0f) * 255.0f / 2.0f;
  m[1] = (b / nrm + 1.0f) * 255.0f / 2.0f;
  m[2] = (c / nrm + 1.0f) * 255.0f / 2.0f;
}

// eval_normals.py:19-25: x / |x|, the zero vector where |x| == 0
MTT_DEV void normalize3(float (&v)[3]) {
  const float nrm = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  if (nrm == 0.0f) { v[0] = v[1] = v[2] = 0.0f; return; }
  v[0] = v[0] / nrm; v[1] = v[1] / nrm; v[2] = v[2] / nrm;
}

MTT_DEV double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
int eval_vec(const mtt_eval_desc* d, bool map_entry) {
  if (!MTT_EVAL_VEC || (d->HW & 3) || !aligned16(d->pred)) return 1;
  if (map_entry ? !aligned16(d->out) : !aligned16(d->label)) return 1;
  return 4;
}
// Workgroups per launch.  The integer meters end every workgroup with one 64-bit atomic per counter on the SAME few addresses, which
// the memory system serialises per address (measured: ~16 ns each, 1 536 workgroups = 25 us whatever the class count), so they run about
// two grid-striding workgroups per CU; the others write partials with plain stores and take up to 8 192.
dim3 eval_grid(const mtt_eval_desc* d, int V, bool atomics) {
  int64_t g = (d->HW / V + 255) / 256;
  const int64_t cap = ((atomics ? 512 : 8192) + d->B - 1) / d->B;
  if (g > cap) g = cap;
  return dim3((unsigned)(g < 1 ? 1 : g), (unsigned)d->B);
}
// the pixel loop of every kernel: thread-owned groups of V consecutive pixels, hw = the first pixel of the group
#define MTT_EVAL_FOR_PIXELS(hw) \
  for (int64_t hw = ((int64_t)blockIdx.x * 256 + threadIdx.x) * V; hw < d.HW; hw += (int64_t)gridDim.x * 256 * V)

// ---- maps -----------------------------------------------------------------------------------------------------------------------------
template <int KIND, int V>
__global__ __launch_bounds__(256) void eval_map_kernel(const mtt_eval_desc d) {
  const int64_t b = blockIdx.y;
  const float* xb = (const float*)d.pred + b * d.C * d.HW;
  MTT_EVAL_FOR_PIXELS(hw) {
    const float* x = xb + hw;
    if constexpr (KIND == MTT_EVAL_CONFUSION) {
      int arg[V];
      pix_argmax<V>(x, d.C, d.HW, arg);
      int64_t p[V];
#pragma unroll
      for (int i = 0; i < V; ++i) p[i] = d.class_map && arg[i] < d.n_map ? d.class_map[arg[i]] : (int64_t)arg[i];
      int64_t* o = (int64_t*)d.out + b * d.HW + hw;
      if constexpr (V == 4) { ((I64x2*)o)[0] = I64x2{p[0], p[1]}; ((I64x2*)o)[1] = I64x2{p[2], p[3]}; }
      else o[0] = p[0];
    } else if constexpr (KIND == MTT_EVAL_NORMALS) {
      const Px<V> a = ldv<V>(x), bb = ldv<V>(x + d.HW), c = ldv<V>(x + 2 * d.HW);
      float o[3 * V];
#pragma unroll
      for (int i = 0; i < V; ++i) {
        float m[3];
        pix_normals(a.v[i], bb.v[i], c.v[i], m);
        o[3 * i] = m[0]; o[3 * i + 1] = m[1]; o[3 * i + 2] = m[2];
      }
      float* dst = (float*)d.out + (b * d.HW + hw) * 3;
      if constexpr (V == 4) {
#pragma unroll
        for (int q = 0; q < 3; ++q) ((float4*)dst)[q] = make_float4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
      } else { dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2]; }
    } else {
      Px<V> r = ldv<V>(x);
      if constexpr (KIND == MTT_EVAL_SAL) {
        const Px<V> x1 = ldv<V>(x + d.HW);
#pragma unroll
        for (int i = 0; i < V; ++i) r.v[i] = pix_sal(r.v[i], x1.v[i]);
      } else {
#pragma unroll
        for (int i = 0; i < V; ++i) r.v[i] = KIND == MTT_EVAL_DEPTH ? pix_depth(r.v[i]) : pix_edge(r.v[i]);
      }
      stv<V>((float*)d.out + b * d.HW + hw, r);
    }
  }
}

// ---- integer meters: a workgroup histogram in LDS, then 64-bit integer atomics on the accumulator ---------------------------------------
template <bool FROM_MAP, int V>
__global__ __launch_bounds__(256) void eval_confusion_kernel(const mtt_eval_desc d) {
  __shared__ unsigned hist[3 * MAX_CLASSES];          // a workgroup stays inside one image, and mtt_eval_accum refuses HW >= 2^32
  const int n = d.n_classes;
  for (int i = threadIdx.x; i < 3 * n; i += 256) hist[i] = 0u;
  __syncthreads();
  const int64_t b = blockIdx.y;
  const float* xb = (const float*)d.pred + b * d.C * d.HW;
  const int64_t* mb = (const int64_t*)d.pred + b * d.HW;
  const float* lab = d.label + b * d.HW;
  MTT_EVAL_FOR_PIXELS(hw) {
    int64_t p[V];
    if constexpr (FROM_MAP) {
      if constexpr (V == 4) {
        const I64x2 lo = ((const I64x2*)(mb + hw))[0], hi = ((const I64x2*)(mb + hw))[1];
        p[0] = lo.a; p[1] = lo.b; p[2] = hi.a; p[3] = hi.b;
      } else p[0] = mb[hw];
    } else {
      int arg[V];
      pix_argmax<V>(xb + hw, d.C, d.HW, arg);
#pragma unroll
      for (int i = 0; i < V; ++i) p[i] = arg[i];
    }
    const Px<V> gv = ldv<V>(lab + hw);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float g = gv.v[i];
      if (g == d.ignore) continue;
      const bool p_in = p[i] >= 0 && p[i] < n;
      const int gi = g >= 0.0f && g < (float)n ? (int)g : -1;
      const bool g_in = gi >= 0 && (float)gi == g;
      if (p_in && g_in && gi == (int)p[i]) {
        atomicAdd(&hist[gi], 1u);
      } else {
        if (p_in) atomicAdd(&hist[n + (int)p[i]], 1u);
        if (g_in) atomicAdd(&hist[2 * n + gi], 1u);
      }
    }
  }
  __syncthreads();
  unsigned long long* acc = (unsigned long long*)d.acc;
  for (int i = threadIdx.x; i < 3 * n; i += 256)
    if (hist[i]) atomicAdd(&acc[i], (unsigned long long)hist[i]);
}

template <bool FROM_MAP, int V>
__global__ __launch_bounds__(256) void eval_sal_kernel(const mtt_eval_desc d) {
  __shared__ unsigned long long hist[2 * (MAX_THRESH + 1)];          // 64-bit: tp_hist adds the label's value, two's complement
  __shared__ unsigned long long ap_sh;
  __shared__ float th[MAX_THRESH];
  const int T = d.n_thresh, nslot = 2 * (T + 1);
  for (int i = threadIdx.x; i < nslot; i += 256) hist[i] = 0ull;
  for (int i = threadIdx.x; i < T; i += 256) th[i] = d.thresholds[i];
  if (threadIdx.x == 0) ap_sh = 0ull;
  unsigned long long ap = 0ull;                                      // every valid pixel adds to ap: kept per thread until the end
  __syncthreads();
  const int64_t b = blockIdx.y;
  const float* xb = (const float*)d.pred + b * (FROM_MAP ? 1 : d.C) * d.HW;
  const float* lab = d.label + b * d.HW;
  MTT_EVAL_FOR_PIXELS(hw) {
    Px<V> m = ldv<V>(xb + hw);
    if constexpr (!FROM_MAP) {
      const Px<V> x1 = ldv<V>(xb + d.HW + hw);
#pragma unroll
      for (int i = 0; i < V; ++i) m.v[i] = pix_sal(m.v[i], x1.v[i]);
    }
    const Px<V> gv = ldv<V>(lab + hw);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float g = gv.v[i];
      if (g == d.ignore) continue;
      const float s = 1.0f / (1.0f + expf(-(m.v[i] / 255.0f)));      // eval_sal.py:30,43: sigmoid of the probability
      int k = 0;
      for (int j = 0; j < T; ++j) k += s >= th[j] ? 1 : 0;
      const unsigned long long t = (unsigned long long)(long long)g;
      atomicAdd(&hist[k], 1ull);
      if (t) { atomicAdd(&hist[T + 1 + k], t); ap += t; }
    }
  }
  if (ap) atomicAdd(&ap_sh, ap);
  __syncthreads();
  unsigned long long* acc = (unsigned long long*)d.acc;
  for (int i = threadIdx.x; i < nslot; i += 256)
    if (hist[i]) atomicAdd(&acc[i], hist[i]);
  if (threadIdx.x == 0 && ap_sh) atomicAdd(&acc[nslot], ap_sh);
}

// ---- fp64 meters: per-workgroup partials, summed in workgroup order by eval_finish_kernel ----------------------------------------------
template <int NS>
MTT_DEV void block_partials(double (&v)[NS], double* ws) {
  __shared__ double red[4][MAX_SUMS];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const double s = wave_sum_f64(v[j]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][j] = s;
  }
  __syncthreads();
  if (threadIdx.x < NS) {
    const int64_t bi = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    ws[bi * NS + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
  }
}

template <bool FROM_MAP, int V>
__global__ __launch_bounds__(256) void eval_depth_kernel(const mtt_eval_desc d) {
  double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  const int64_t b = blockIdx.y;
  const float* xb = (const float*)d.pred + b * d.HW;
  const float* lab = d.label + b * d.HW;
  MTT_EVAL_FOR_PIXELS(hw) {
    const Px<V> xv = ldv<V>(xb + hw), gv = ldv<V>(lab + hw);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float m = FROM_MAP ? xv.v[i] : pix_depth(xv.v[i]);
      const float g = gv.v[i];
      const bool ok = d.mask_mode == 0 ? (g < d.max_depth && g > d.min_depth) : g != d.ignore;
      if (!ok) continue;
      const float gp = g <= 0.0f ? 1e-9f : g, vp = m <= 0.0f ? 1e-9f : m;        // eval_depth.py:41-42
      const float df = gp - vp, dl = logf(gp) - logf(vp);
      v[0] += 1.0;
      v[1] += (double)(df * df);
      v[2] += (double)(dl * dl);
      v[3] += (double)(fabsf(df) / gp);
      v[4] += (double)(df * df / gp);
    }
  }
  block_partials<5>(v, d.ws);
}

template <bool FROM_MAP, int V>
__global__ __launch_bounds__(256) void eval_normals_kernel(const mtt_eval_desc d) {
  double v[2] = {0.0, 0.0};
  const int64_t b = blockIdx.y;
  const float* xb = (const float*)d.pred + b * 3 * d.HW;
  const float* lab = d.label + b * 3 * d.HW;
  MTT_EVAL_FOR_PIXELS(hw) {
    float mm[3 * V];
    if constexpr (FROM_MAP) {
      const float* src = xb + hw * 3;
      if constexpr (V == 4) {
#pragma unroll
        for (int q = 0; q < 3; ++q) { const float4 t = ((const float4*)src)[q]; mm[4 * q] = t.x; mm[4 * q + 1] = t.y; mm[4 * q + 2] = t.z; mm[4 * q + 3] = t.w; }
      } else { mm[0] = src[0]; mm[1] = src[1]; mm[2] = src[2]; }
    } else {
      const Px<V> a = ldv<V>(xb + hw), bb = ldv<V>(xb + d.HW + hw), c = ldv<V>(xb + 2 * d.HW + hw);
#pragma unroll
      for (int i = 0; i < V; ++i) {
        float m[3];
        pix_normals(a.v[i], bb.v[i], c.v[i], m);
        mm[3 * i] = m[0]; mm[3 * i + 1] = m[1]; mm[3 * i + 2] = m[2];
      }
    }
    const Px<V> g0 = ldv<V>(lab + hw), g1 = ldv<V>(lab + d.HW + hw), g2 = ldv<V>(lab + 2 * d.HW + hw);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      float g[3] = {g0.v[i], g1.v[i], g2.v[i]};
      if (g[0] == d.ignore || g[1] == d.ignore || g[2] == d.ignore) continue;
      float p[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) p[c] = 2.0f * mm[3 * i + c] / 255.0f - 1.0f;     // eval_normals.py:36: reverse post-processing
      normalize3(p); normalize3(g);
      float nd = 0.0f, ns = 0.0f;
#pragma unroll
      for (int c = 0; c < 3; ++c) { const float a = p[c] - g[c], s = p[c] + g[c]; nd = nd + a * a; ns = ns + s * s; }
      const float ang = 2.0f * atan2f(sqrtf(nd), sqrtf(ns)) * 57.29577951308232f;   // rad2deg
      v[0] += 1.0;
      v[1] += (double)ang;
    }
  }
  block_partials<2>(v, d.ws);
}

template <bool FROM_MAP, int V>
__global__ __launch_bounds__(256) void eval_edge_kernel(const mtt_eval_desc d) {
  double v[2] = {0.0, 0.0};
  const float factor = 1.0f / (1.0f - d.pos_weight), pw = d.pos_weight * factor;  // loss_functions.py:80-87
  const int64_t b = blockIdx.y;
  const float* xb = (const float*)d.pred + b * d.HW;
  const float* lab = d.label + b * d.HW;
  MTT_EVAL_FOR_PIXELS(hw) {
    const Px<V> xv = ldv<V>(xb + hw), gv = ldv<V>(lab + hw);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float m = FROM_MAP ? xv.v[i] : pix_edge(xv.v[i]);
      const float y = gv.v[i];
      if (y == d.ignore) continue;
      const float z = m / 255.0f;
      // binary_cross_entropy_with_logits with pos_weight: (1 - y) z + (1 + (pw - 1) y) (log1p(exp(-|z|)) + max(-z, 0))
      const float lw = 1.0f + (pw - 1.0f) * y;
      const float term = (1.0f - y) * z + lw * (log1pf(expf(-fabsf(z))) + fmaxf(-z, 0.0f));
      v[0] += 1.0;
      v[1] += (double)(term / factor);
    }
  }
  block_partials<2>(v, d.ws);
}

// one workgroup: slot j of acc += the nblk partials of sum j in a fixed 256-way order; slot 0 is the pixel count (exact in fp64), kept int64
__global__ __launch_bounds__(256) void eval_finish_kernel(const double* ws, int nblk, int ns, void* acc) {
  __shared__ double red[256];
  for (int j = 0; j < ns; ++j) {
    double s = 0.0;
    for (int k = threadIdx.x; k < nblk; k += 256) s += ws[(int64_t)k * ns + j];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      if (j == 0) ((int64_t*)acc)[0] += (int64_t)red[0];
      else ((double*)acc)[j] += red[0];
    }
    __syncthreads();
  }
}

int n_sums(int kind) { return kind == MTT_EVAL_DEPTH ? 5 : (kind == MTT_EVAL_NORMALS || kind == MTT_EVAL_EDGE ? 2 : 0); }

int eval_check(const mtt_eval_desc* d) {
  if (!d || !d->pred || d->B <= 0 || d->B > 65535 || d->HW <= 0 || d->C <= 0 || d->kind < 0 || d->kind > MTT_EVAL_EDGE) return MTT_E_BADARG;
  if ((d->kind == MTT_EVAL_SAL && d->C != 2) || (d->kind == MTT_EVAL_NORMALS && d->C != 3) ||
      ((d->kind == MTT_EVAL_DEPTH || d->kind == MTT_EVAL_EDGE) && d->C != 1))
    return MTT_E_UNSUPPORTED;
  return 0;
}

}  // namespace

extern "C" size_t mtt_eval_desc_size(void) { return sizeof(mtt_eval_desc); }

extern "C" size_t mtt_eval_ws_floats(const mtt_eval_desc* d) {
  if (!d || d->B <= 0 || d->B > 65535 || d->HW <= 0) return 0;
  const dim3 g = eval_grid(d, 1, false);                   // the one-pixel grid is the larger one
  return (size_t)2 * n_sums(d->kind) * g.x * g.y;          // fp64 partials, counted in floats
}

extern "C" int mtt_eval_map(const mtt_eval_desc* d, void* stream) {
  if (int e = eval_check(d)) return e;
  if (!d->out || (d->class_map && (d->kind != MTT_EVAL_CONFUSION || d->n_map <= 0))) return MTT_E_BADARG;
  if (d->out == d->pred && d->kind != MTT_EVAL_DEPTH) return MTT_E_BADARG;
  const int V = eval_vec(d, true);
  const dim3 g = eval_grid(d, V, false);
  hipStream_t s = (hipStream_t)stream;
#define MTT_EVAL_MAP(K) \
  do { if (V == 4) hipLaunchKernelGGL((eval_map_kernel<K, 4>), g, dim3(256), 0, s, *d); else hipLaunchKernelGGL((eval_map_kernel<K, 1>), g, dim3(256), 0, s, *d); } while (0)
  switch (d->kind) {
    case MTT_EVAL_CONFUSION: MTT_EVAL_MAP(MTT_EVAL_CONFUSION); break;
    case MTT_EVAL_SAL: MTT_EVAL_MAP(MTT_EVAL_SAL); break;
    case MTT_EVAL_DEPTH: MTT_EVAL_MAP(MTT_EVAL_DEPTH); break;
    case MTT_EVAL_NORMALS: MTT_EVAL_MAP(MTT_EVAL_NORMALS); break;
    default: MTT_EVAL_MAP(MTT_EVAL_EDGE); break;
  }
#undef MTT_EVAL_MAP
  return (int)hipGetLastError();
}

extern "C" int mtt_eval_accum(const mtt_eval_desc* d, void* stream) {
  if (int e = eval_check(d)) return e;
  if (!d->label || !d->acc || d->source < 0 || d->source > MTT_EVAL_FROM_MAP) return MTT_E_BADARG;
  if (d->Cl != (d->kind == MTT_EVAL_NORMALS ? 3 : 1)) return MTT_E_UNSUPPORTED;
  if (d->kind == MTT_EVAL_CONFUSION && (d->n_classes <= 0 || d->n_classes > MAX_CLASSES || d->HW > 0xffffffffLL)) return MTT_E_UNSUPPORTED;   // 32-bit LDS counters per image
  if (d->kind == MTT_EVAL_SAL && (d->n_thresh <= 0 || d->n_thresh > MAX_THRESH || !d->thresholds)) return MTT_E_BADARG;
  if (d->kind == MTT_EVAL_DEPTH && (d->mask_mode < 0 || d->mask_mode > 1)) return MTT_E_BADARG;
  const int ns = n_sums(d->kind);
  if (ns && !d->ws) return MTT_E_BADARG;
  if (((uintptr_t)d->acc & 7) || (ns && ((uintptr_t)d->ws & 7))) return MTT_E_ALIGN;
  const int V = eval_vec(d, false);
  const dim3 g = eval_grid(d, V, ns == 0);
  hipStream_t s = (hipStream_t)stream;
  const bool fm = d->source == MTT_EVAL_FROM_MAP;
#define MTT_EVAL_LAUNCH(K) \
  do { \
    if (V == 4) { if (fm) hipLaunchKernelGGL((K<true, 4>), g, dim3(256), 0, s, *d); else hipLaunchKernelGGL((K<false, 4>), g, dim3(256), 0, s, *d); } \
    else { if (fm) hipLaunchKernelGGL((K<true, 1>), g, dim3(256), 0, s, *d); else hipLaunchKernelGGL((K<false, 1>), g, dim3(256), 0, s, *d); } \
  } while (0)
  switch (d->kind) {
    case MTT_EVAL_CONFUSION: MTT_EVAL_LAUNCH(eval_confusion_kernel); break;
    case MTT_EVAL_SAL: MTT_EVAL_LAUNCH(eval_sal_kernel); break;
    case MTT_EVAL_DEPTH: MTT_EVAL_LAUNCH(eval_depth_kernel); break;
    case MTT_EVAL_NORMALS: MTT_EVAL_LAUNCH(eval_normals_kernel); break;
    default: MTT_EVAL_LAUNCH(eval_edge_kernel); break;
  }
#undef MTT_EVAL_LAUNCH
  if (ns) hipLaunchKernelGGL(eval_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)d->ws, (int)(g.x * g.y), ns, d->acc);
  return (int)hipGetLastError();
}
