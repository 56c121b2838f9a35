// FCOS3D box decoding and per-class NMS of the 3ddet task at inference (ABI 16; replaces the per-level torch chain of
// TaskPrompter/detection_toolbox/det_model.py:555-681 and the per-class host loop of det_tools.py:85-210, which synchronises with the
// host once per class and once more inside every NMS call).  Four entry points on one descriptor, six launches, no host round trip:
//   select  : one workgroup per (level, image): key = max_c sigmoid(cls) sigmoid(ctr) per point, then the n largest by a 4-pass radix
//             select on the fp32 bit pattern (256-bin histogram in LDS; keys are non-negative, so the bit order is the numeric order)
//             and an ordered compaction (wave ballots + a 4-entry LDS scan): deterministic, ascending point index;
//   decode  : one thread per candidate, in the reference's fp32 operation order (this file is built without FMA contraction);
//   nms_seg : per (image, class) segment: threshold + ordered compaction + bitonic sort of (score, ~index) 64-bit keys in LDS, then the
//             64 x 64 mask tiles and the one-wave greedy pass of iou3d.hip with the grid extended over the segments (a tile or a wave
//             whose segment is shorter than the capacity returns at once);
//   collect : one thread per kept box: its output row is its rank, found by a binary search in every class's kept scores (each list
//             is already in descending order) instead of a sort of the concatenation.
#include "mtt_device.h"

namespace {

#include "iou3d_dev.h"              // corners / overlap_area / iou_rot / iou_axis; contraction stays off to the end of this file

typedef mtt_det_decode_desc Desc;
constexpr float PI_F = 3.14159265358979323846f;        // fp32(np.pi): what torch multiplies / divides an fp32 tensor by

MTT_DEV float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

MTT_DEV float map_at(const float* m, int b, int ch, int c, int64_t hw, int p) { return m[((int64_t)b * ch + c) * hw + p]; }

// exclusive prefix of `flag` over the 256 threads of the workgroup (thread order) and the workgroup's total; wtot = 4 ints of LDS.
// Every thread of the workgroup calls it; two barriers.
MTT_DEV int block_scan256(bool flag, int* wtot, int& total) {
  const unsigned long long bal = __ballot(flag);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int within = __popcll(bal & ((1ull << lane) - 1ull));
  __syncthreads();                                     // the previous call's readers are done with wtot
  if (lane == 0) wtot[wave] = __popcll(bal);
  __syncthreads();
  int before = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int v = wtot[w];
    before += w < wave ? v : 0;
    tot += v;
  }
  total = tot;
  return before + within;
}

__global__ __launch_bounds__(256) void select_kernel(const Desc d) {
  const int l = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int P = d.H[l] * d.W[l], nsel = d.cand_off[l + 1] - d.cand_off[l];
  const int64_t Ptot = d.key_off[d.nlev];
  float* keys = d.keys + (int64_t)b * Ptot + d.key_off[l];
  int32_t* sel = d.sel + (int64_t)b * d.N + d.cand_off[l];
  const float* cls = d.cls[l];
  const float* ctr = d.ctr[l];
  for (int p = tid; p < P; p += 256) {
    const float cn = sigmoid_f(map_at(ctr, b, 1, 0, P, p));
    float key = sigmoid_f(map_at(cls, b, d.C, 0, P, p)) * cn;
    for (int c = 1; c < d.C; ++c) key = fmaxf(key, sigmoid_f(map_at(cls, b, d.C, c, P, p)) * cn);
    keys[p] = key;
    if (nsel == P) sel[p] = p;
  }
  if (nsel == P) return;                               // workgroup-uniform
  __shared__ unsigned hist[256];
  __shared__ unsigned s_prefix, s_k;
  __shared__ int wtot[4];
  __syncthreads();                                     // keys[] written above are read back below by other threads
  unsigned prefix = 0u, mask = 0u, k = (unsigned)nsel;
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[tid] = 0u;
    __syncthreads();
    for (int p = tid; p < P; p += 256) {
      const unsigned kb = __float_as_uint(keys[p]);
      if ((kb & mask) == prefix) atomicAdd(&hist[(kb >> shift) & 255u], 1u);      // integer counts: order-independent
    }
    __syncthreads();
    if (tid == 0) {
      unsigned above = 0u;
      int dgt = 255;
      for (; dgt > 0; --dgt) {
        if (above + hist[dgt] >= k) break;
        above += hist[dgt];
      }
      s_prefix = prefix | ((unsigned)dgt << shift);
      s_k = k - above;
    }
    __syncthreads();
    prefix = s_prefix;
    k = s_k;
    mask |= 255u << shift;
    __syncthreads();
  }
  // prefix = bit pattern of the nsel-th largest key; k = how many of the keys equal to it are taken (the lowest point indices)
  int run_eq = 0, run_tk = 0;
  for (int base = 0; base < P; base += 256) {
    const int p = base + tid;
    const unsigned kb = p < P ? __float_as_uint(keys[p]) : 0u;
    const bool gt = p < P && kb > prefix, eq = p < P && kb == prefix;
    int tot_eq, tot_tk;
    const int rank_eq = run_eq + block_scan256(eq, wtot, tot_eq);
    const bool take = gt || (eq && rank_eq < (int)k);
    const int pos = run_tk + block_scan256(take, wtot, tot_tk);
    if (take && pos < nsel) sel[pos] = p;
    run_eq += tot_eq;
    run_tk += tot_tk;
  }
}

__global__ __launch_bounds__(256) void decode_kernel(const Desc d) {
  const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (j >= d.N) return;
  int l = 0;
  while (l + 1 < d.nlev && j >= d.cand_off[l + 1]) ++l;
  const int W = d.W[l], P = d.H[l] * W;
  const int64_t r = (int64_t)b * d.N + j;
  int p = d.sel[r];
  p = min(max(p, 0), P - 1);
  const float px = (float)(p % W) * d.stride[l] + d.half[l], py = (float)(p / W) * d.stride[l] + d.half[l];
  const float* bb = d.bbox[l];
  float v[13];
#pragma unroll
  for (int c = 0; c < 13; ++c) v[c] = map_at(bb, b, 13, c, P, p);
  const float s = d.denorm[l];
  const float u = px - v[0] * s, w = py - v[1] * s, dep = v[2];
  float* c2 = d.cen2d + r * 3;
  c2[0] = u; c2[1] = w; c2[2] = dep;
  const float* inv = d.inv + (int64_t)b * 16;
  const float h0 = u * dep, h1 = w * dep;
  float o[9];
#pragma unroll
  for (int q = 0; q < 3; ++q) o[q] = h0 * inv[q * 4] + h1 * inv[q * 4 + 1] + dep * inv[q * 4 + 2] + inv[q * 4 + 3];
  o[3] = v[3]; o[4] = v[4]; o[5] = v[5];
  const float* dr = d.dir[l];
  int32_t* dc = d.dircls + r * 3;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int cls1 = map_at(dr, b, 6, 2 * q + 1, P, p) > map_at(dr, b, 6, 2 * q, P, p) ? 1 : 0;     // argmax, the first index on a tie
    dc[q] = cls1;
    const float val = v[6 + q] - d.dir_offset;
    const float lim = val - floorf(val / PI_F + 0.0f) * PI_F;                                      // limit_period(val, 0, pi)
    o[6 + q] = lim + d.dir_offset + PI_F * (float)cls1;
  }
  float* b9 = d.box9 + r * 9;
#pragma unroll
  for (int q = 0; q < 9; ++q) b9[q] = o[q];
  const float ih = d.img_size[b * 2], iw = d.img_size[b * 2 + 1];
  float* b2 = d.box2d + r * 4;
  b2[0] = fminf(fmaxf(px - v[9] * s, 0.f), iw);
  b2[1] = fminf(fmaxf(py - v[10] * s, 0.f), ih);
  b2[2] = fminf(fmaxf(px + v[11] * s, 0.f), iw);
  b2[3] = fminf(fmaxf(py + v[12] * s, 0.f), ih);
  float* nb = d.nmsbox + r * 5;
  const float hw = o[4] / 2, hh = o[3] / 2;
  nb[0] = o[0] - hw; nb[1] = o[2] - hh; nb[2] = o[0] + hw; nb[3] = o[2] + hh; nb[4] = o[8];
  const float cn = sigmoid_f(map_at(d.ctr[l], b, 1, 0, P, p));
  float* sc = d.scores + r * d.C;
  for (int c = 0; c < d.C; ++c) sc[c] = sigmoid_f(map_at(d.cls[l], b, d.C, c, P, p)) * cn;
}

// workspace of the segmented NMS, per segment s = b * C + c (8-byte aligned parts)
struct NmsWs { float* sscore; float* sbox; float* kscore; unsigned long long* mask; };
__host__ __device__ inline size_t ws_parts(int S, int N, size_t (&off)[4]) {
  const size_t n = (size_t)S * N, cb = (size_t)(N + 63) / 64;
  off[0] = 0;                                          // sorted scores  [S, N]
  off[1] = off[0] + (n * 4 + 7) / 8 * 8;               // sorted boxes   [S, N, 5]
  off[2] = off[1] + (n * 20 + 7) / 8 * 8;              // kept scores    [S, N]
  off[3] = off[2] + (n * 4 + 7) / 8 * 8;               // masks          [S, N, cb] 64-bit words
  return off[3] + n * cb * 8;
}
MTT_DEV NmsWs ws_of(const Desc& d) {
  size_t off[4];
  ws_parts(d.B * d.C, d.N, off);
  char* w = (char*)d.ws;
  return NmsWs{(float*)(w + off[0]), (float*)(w + off[1]), (float*)(w + off[2]), (unsigned long long*)(w + off[3])};
}

// threshold + compact + sort one (image, class) segment; dynamic LDS: pow2ceil(N) 64-bit keys
__global__ __launch_bounds__(256) void seg_sort_kernel(const Desc d) {
  extern __shared__ unsigned long long skey[];
  __shared__ int wtot[4];
  const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, N = d.N;
  const int s = b * d.C + c;
  const float* scores = d.scores + (int64_t)b * N * d.C + c;
  int n = 0;
  for (int base = 0; base < N; base += 256) {
    const int j = base + tid;
    const float sc = j < N ? scores[(int64_t)j * d.C] : 0.f;
    const bool on = j < N && sc > d.score_thr;
    int tot;
    const int pos = n + block_scan256(on, wtot, tot);
    if (on) skey[pos] = ((unsigned long long)__float_as_uint(sc) << 32) | (unsigned)(~(unsigned)j);
    n += tot;
  }
  int np2 = 1;
  while (np2 < n) np2 <<= 1;
  for (int i = n + tid; i < np2; i += 256) skey[i] = 0ull;        // below every real key (their low words are ~index != 0)
  __syncthreads();
  for (int k = 2; k <= np2; k <<= 1)
    for (int jj = k >> 1; jj > 0; jj >>= 1) {
      for (int i = tid; i < np2; i += 256) {
        const int x = i ^ jj;
        if (x > i) {
          const unsigned long long a = skey[i], bq = skey[x];
          const bool desc = (i & k) == 0;
          if (desc ? a < bq : a > bq) { skey[i] = bq; skey[x] = a; }
        }
      }
      __syncthreads();
    }
  const NmsWs w = ws_of(d);
  const float* nbx = d.nmsbox + (int64_t)b * N * 5;
  for (int i = tid; i < n; i += 256) {
    const unsigned long long kq = skey[i];
    const int j = (int)(~(unsigned)kq);
    const int64_t o = (int64_t)s * N + i;
    d.seg_idx[o] = j;
    w.sscore[o] = __uint_as_float((unsigned)(kq >> 32));
#pragma unroll
    for (int q = 0; q < 5; ++q) w.sbox[o * 5 + q] = nbx[(int64_t)j * 5 + q];
  }
  if (tid == 0) d.seg_n[s] = n;
}

// nms_mask_kernel of iou3d.hip on segment blockIdx.z; row pitch of the masks = ceil(N / 64) words
__global__ __launch_bounds__(64) void seg_mask_kernel(const Desc d) {
  const int cb = blockIdx.x, rb = blockIdx.y, s = blockIdx.z;
  const int n = d.seg_n[s];
  if (rb > cb || cb * 64 >= n) return;
  const int pitch = (d.N + 63) / 64;
  const NmsWs w = ws_of(d);
  const float* boxes = w.sbox + (int64_t)s * d.N * 5;
  unsigned long long* mask = w.mask + (int64_t)s * d.N * pitch;
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
    const float v = d.rotated ? iou_rot(A, cols + j * 5) : iou_axis(A, cols + j * 5);
    if (v > d.nms_thr) m |= 1ull << j;
  }
  mask[(int64_t)(rb * 64 + lane) * pitch + cb] = m;
}

// nms_reduce_kernel of iou3d.hip on segment blockIdx.x: the kept candidates' indices and scores in score order
__global__ __launch_bounds__(64) void seg_reduce_kernel(const Desc d) {
  __shared__ unsigned long long remv[MTT_DET_MAX_CAND / 64];
  const int s = blockIdx.x, lane = threadIdx.x;
  const int n = d.seg_n[s], col_blocks = (n + 63) / 64, pitch = (d.N + 63) / 64;
  const NmsWs w = ws_of(d);
  const unsigned long long* mask = w.mask + (int64_t)s * d.N * pitch;
  const int64_t so = (int64_t)s * d.N;
  for (int j = lane; j < col_blocks; j += 64) remv[j] = 0ull;
  __syncthreads();
  int k = 0;
  for (int i = 0; i < n; ++i) {
    const int nb = i >> 6;
    const bool dead = (remv[nb] >> (i & 63)) & 1ull;      // wave-uniform
    if (!dead) {
      if (lane == 0) { d.kept[so + k] = d.seg_idx[so + i]; w.kscore[so + k] = w.sscore[so + i]; }
      ++k;
      for (int j = nb + lane; j < col_blocks; j += 64) remv[j] |= mask[(int64_t)i * pitch + j];
    }
    __syncthreads();
  }
  if (lane == 0) d.kept_n[s] = k;
}

// entries of the descending list ks[0, n) that are > v (strict) or >= v
MTT_DEV int count_above(const float* ks, int n, float v, bool or_equal) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const float x = ks[mid];
    if (or_equal ? x >= v : x > v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void collect_kernel(const Desc d) {
  const int i = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
  const int N = d.N, C = d.C;
  const int32_t* kn = d.kept_n + b * C;
  int K = 0, before = 0;
  for (int q = 0; q < C; ++q) { const int v = kn[q]; K += v; before += q < c ? v : 0; }
  if (i == 0 && c == 0) d.count[b] = min(K, d.max_per_img);
  if (i >= kn[c]) return;
  const NmsWs w = ws_of(d);
  const int64_t so = (int64_t)(b * C + c) * N;
  const float sc = w.kscore[so + i];
  int rank;
  if (K <= d.max_per_img) {
    rank = before + i;                                   // class order, score order inside a class
  } else {                                               // descending score; equal scores in concatenation order
    rank = i;
    for (int q = 0; q < C; ++q)
      if (q != c) rank += count_above(w.kscore + (int64_t)(b * C + q) * N, kn[q], sc, q < c);
    if (rank >= d.max_per_img) return;
  }
  const int j = d.kept[so + i];
  const int64_t r = (int64_t)b * N + j;
  float* o = d.out + ((int64_t)b * d.max_per_img + rank) * MTT_DET_OUT_COLS;
#pragma unroll
  for (int q = 0; q < 9; ++q) o[q] = d.box9[r * 9 + q];
  o[9] = sc;
#pragma unroll
  for (int q = 0; q < 3; ++q) o[10 + q] = d.cen2d[r * 3 + q];
#pragma unroll
  for (int q = 0; q < 4; ++q) o[13 + q] = d.box2d[r * 4 + q];
  o[17] = __int_as_float(c);
}

// geometry every entry point relies on for its bounds: levels, candidate and key offsets as the header defines them
int check(const Desc* d) {
  if (!d || d->nlev <= 0 || d->nlev > 8 || d->B <= 0 || d->C <= 0 || d->N <= 0) return MTT_E_BADARG;
  if (d->C > MTT_DET_MAX_CLASSES || d->N > MTT_DET_MAX_CAND) return MTT_E_UNSUPPORTED;
  int64_t co = 0, ko = 0;
  for (int l = 0; l < d->nlev; ++l) {
    if (d->H[l] <= 0 || d->W[l] <= 0 || d->cand_off[l] != co || d->key_off[l] != ko) return MTT_E_BADARG;
    const int64_t P = (int64_t)d->H[l] * d->W[l];
    co += (d->nms_pre > 0 && P > d->nms_pre) ? d->nms_pre : P;
    ko += P;
    if (ko > (1 << 30)) return MTT_E_UNSUPPORTED;
  }
  if (d->cand_off[d->nlev] != co || d->key_off[d->nlev] != ko || co != d->N) return MTT_E_BADARG;
  return 0;
}

int pow2ceil(int n) { int p = 1; while (p < n) p <<= 1; return p; }

}  // namespace

extern "C" size_t mtt_det_decode_desc_size(void) { return sizeof(mtt_det_decode_desc); }

extern "C" size_t mtt_det_nms_ws_bytes(const mtt_det_decode_desc* d) {
  if (!d || d->B <= 0 || d->C <= 0 || d->N <= 0) return 0;
  size_t off[4];
  return ws_parts(d->B * d->C, d->N, off);
}

extern "C" int mtt_det_select(const mtt_det_decode_desc* d, void* stream) {
  if (const int e = check(d)) return e;
  if (!d->keys || !d->sel) return MTT_E_BADARG;
  for (int l = 0; l < d->nlev; ++l)
    if (!d->cls[l] || !d->ctr[l]) return MTT_E_BADARG;
  hipLaunchKernelGGL(select_kernel, dim3(d->nlev, d->B), dim3(256), 0, (hipStream_t)stream, *d);
  return (int)hipGetLastError();
}

extern "C" int mtt_det_decode(const mtt_det_decode_desc* d, void* stream) {
  if (const int e = check(d)) return e;
  if (!d->sel || !d->inv || !d->img_size || !d->box9 || !d->cen2d || !d->box2d || !d->nmsbox || !d->dircls || !d->scores) return MTT_E_BADARG;
  for (int l = 0; l < d->nlev; ++l)
    if (!d->cls[l] || !d->bbox[l] || !d->dir[l] || !d->ctr[l]) return MTT_E_BADARG;
  hipLaunchKernelGGL(decode_kernel, dim3((d->N + 255) / 256, d->B), dim3(256), 0, (hipStream_t)stream, *d);
  return (int)hipGetLastError();
}

extern "C" int mtt_det_nms_seg(const mtt_det_decode_desc* d, void* stream) {
  if (!d || d->B <= 0 || d->C <= 0 || d->N <= 0) return MTT_E_BADARG;
  if (d->C > MTT_DET_MAX_CLASSES || d->N > MTT_DET_MAX_CAND || (int64_t)d->B * d->C > 65535) return MTT_E_UNSUPPORTED;
  if (!d->scores || !d->nmsbox || !d->seg_n || !d->seg_idx || !d->kept_n || !d->kept || !d->ws) return MTT_E_BADARG;
  static std::atomic<unsigned long long> done{0};
  const int lds = pow2ceil(d->N) * 8;
  if (const int e = mtt_ensure_dyn_lds((const void*)seg_sort_kernel, MTT_DET_MAX_CAND * 8, done)) return e;
  const int cb = (d->N + 63) / 64, S = d->B * d->C;
  hipLaunchKernelGGL(seg_sort_kernel, dim3(d->C, d->B), dim3(256), lds, (hipStream_t)stream, *d);
  hipLaunchKernelGGL(seg_mask_kernel, dim3(cb, cb, S), dim3(64), 0, (hipStream_t)stream, *d);
  hipLaunchKernelGGL(seg_reduce_kernel, dim3(S), dim3(64), 0, (hipStream_t)stream, *d);
  return (int)hipGetLastError();
}

extern "C" int mtt_det_collect(const mtt_det_decode_desc* d, void* stream) {
  if (!d || d->B <= 0 || d->C <= 0 || d->N <= 0 || d->max_per_img <= 0) return MTT_E_BADARG;
  if (d->C > MTT_DET_MAX_CLASSES || d->N > MTT_DET_MAX_CAND || d->B > 65535) return MTT_E_UNSUPPORTED;
  if (!d->box9 || !d->cen2d || !d->box2d || !d->kept_n || !d->kept || !d->ws || !d->out || !d->count) return MTT_E_BADARG;
  hipLaunchKernelGGL(collect_kernel, dim3((d->N + 255) / 256, d->C, d->B), dim3(256), 0, (hipStream_t)stream, *d);
  return (int)hipGetLastError();
}
