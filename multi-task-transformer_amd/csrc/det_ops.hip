// det_ops.hip — the FCOS3D head and FPN neck of the 3ddet task (ABI 14): GroupNorm (+ReLU), modulated deformable im2col / col2im,
// the FPN's nearest-neighbour top-down add and the per-level bbox tail.  See include/mtt_hip.h for the contracts.
//
// Every cross-workgroup reduction writes partials to the caller's workspace and sums them in a fixed order; the deformable col2im is a
// gather over buckets built by a stable integer radix sort.  No floating-point atomics anywhere, so every result is run-to-run
// reproducible bit for bit.
#include "mtt_device.h"
#include <rocprim/device/device_radix_sort.hpp>

#define S_ ((hipStream_t)stream)
#define LAUNCH_OK() ((int)hipGetLastError())

extern "C" size_t mtt_det_desc_size(int which) {
  switch (which) {
    case 0: return sizeof(mtt_gn_desc);
    case 1: return sizeof(mtt_dcn_desc);
    case 2: return sizeof(mtt_nearest_desc);
    case 3: return sizeof(mtt_bboxpost_desc);
    default: return 0;
  }
}

static inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

MTT_DEV void st_any(void* p, void* plo, int64_t idx, int dtype, float v) {
  if (dtype == MTT_SPLIT) {
    const bf16_t hi = f2bf(v);
    ((bf16_t*)p)[idx] = hi;
    ((bf16_t*)plo)[idx] = f2bf(v - bf2f(hi));
  } else {
    st_elem(p, idx, dtype, v);
  }
}

// =====================================================================================================================
// GroupNorm
// =====================================================================================================================
static constexpr int GN_RPB = 32;          // pixel rows per partial (per image)

static int gn_check(const mtt_gn_desc* d) {
  if (!d || d->Z <= 0 || d->B <= 0 || d->HW <= 0 || d->C <= 0 || d->G <= 0 || (d->C % d->G) || d->ld < d->C) return MTT_E_BADARG;
  if ((int64_t)d->Z * d->B > 65535) return MTT_E_UNSUPPORTED;
  return 0;
}
static int64_t gn_nchunk(const mtt_gn_desc* d) { return cdiv64(d->HW, GN_RPB); }

// partial (mean, M2) of every channel over the chunk's rows (forward), or (sum du, sum du * xhat) (backward)
template <int BWD>
__global__ void __launch_bounds__(256) gn_partial_kernel(mtt_gn_desc d, int64_t nchunk) {
  const int64_t chunk = blockIdx.x;
  const int64_t n = blockIdx.y;                          // image over all Z layers
  const int z = (int)(n / d.B);
  const int64_t r0 = chunk * GN_RPB, r1 = min<int64_t>(r0 + GN_RPB, d.HW);
  const int cpg = d.C / d.G;
  const float cnt = (float)(r1 - r0);
  for (int c = threadIdx.x; c < d.C; c += 256) {
    float a = 0.f, b = 0.f;
    const int64_t base = (n * d.HW) * d.ld + c;
    if (!BWD) {
      for (int64_t r = r0; r < r1; ++r) a += ld_elem(d.x, base + r * d.ld, d.x_dtype);
      a /= cnt;
      for (int64_t r = r0; r < r1; ++r) {
        const float t = ld_elem(d.x, base + r * d.ld, d.x_dtype) - a;
        b = fmaf(t, t, b);
      }
    } else {
      const int g = c / cpg;
      const float mu = d.mean[n * d.G + g], rs = d.rstd[n * d.G + g];
      const float ga = d.gamma[(int64_t)z * d.C + c], be = d.beta[(int64_t)z * d.C + c];
      for (int64_t r = r0; r < r1; ++r) {
        const float xh = (ld_elem(d.x, base + r * d.ld, d.x_dtype) - mu) * rs;
        float du = ld_elem(d.dy, base + r * d.ld, d.dy_dtype);
        if (d.relu && fmaf(xh, ga, be) <= 0.f) du = 0.f;
        a += du;
        b = fmaf(du, xh, b);
      }
    }
    float* w = d.ws + ((n * nchunk + chunk) * d.C + c) * 2;
    w[0] = a;
    w[1] = b;
  }
}

// forward statistics: one workgroup of 64 lanes per (image, group); lane l merges entries l, l+64, ... (chunk-major, channel-minor) with
// Chan's formula, then a fixed pairwise tree over the lanes
__global__ void __launch_bounds__(64) gn_stats_kernel(mtt_gn_desc d, int64_t nchunk) {
  const int64_t ng = blockIdx.x;                         // n * G + g
  const int64_t n = ng / d.G;
  const int g = (int)(ng % d.G);
  const int cpg = d.C / d.G;
  const int64_t ne = nchunk * cpg;
  float cnt = 0.f, mean = 0.f, m2 = 0.f;
  for (int64_t e = threadIdx.x; e < ne; e += 64) {
    const int64_t chunk = e / cpg;
    const int c = g * cpg + (int)(e % cpg);
    const float* w = d.ws + ((n * nchunk + chunk) * d.C + c) * 2;
    const float nb = (float)(min<int64_t>((chunk + 1) * GN_RPB, d.HW) - chunk * GN_RPB);
    const float tot = cnt + nb, delta = w[0] - mean;
    mean += delta * (nb / tot);
    m2 += w[1] + delta * delta * (cnt * nb / tot);
    cnt = tot;
  }
  __shared__ float sc[64], sm[64], s2[64];
  sc[threadIdx.x] = cnt; sm[threadIdx.x] = mean; s2[threadIdx.x] = m2;
  __syncthreads();
  for (int off = 32; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
      const float na = sc[threadIdx.x], nb = sc[threadIdx.x + off];
      const float tot = na + nb;
      if (nb > 0.f) {
        const float delta = sm[threadIdx.x + off] - sm[threadIdx.x];
        sm[threadIdx.x] += delta * (nb / tot);
        s2[threadIdx.x] += s2[threadIdx.x + off] + delta * delta * (na * nb / tot);
        sc[threadIdx.x] = tot;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    d.mean[ng] = sm[0];
    d.rstd[ng] = rsqrtf(s2[0] / sc[0] + d.eps);
  }
}

__global__ void __launch_bounds__(256) gn_apply_kernel(mtt_gn_desc d) {
  const int64_t row = blockIdx.x;
  const int64_t n = row / d.HW;
  const int z = (int)(n / d.B);
  const int cpg = d.C / d.G;
  for (int64_t c = threadIdx.x; c < d.ld; c += 256) {
    float v = 0.f;
    if (c < d.C) {
      const int g = (int)c / cpg;
      const float xh = (ld_elem(d.x, row * d.ld + c, d.x_dtype) - d.mean[n * d.G + g]) * d.rstd[n * d.G + g];
      v = fmaf(xh, d.gamma[z * d.C + c], d.beta[z * d.C + c]);
      if (d.relu) v = fmaxf(v, 0.f);
    }
    st_any(d.y, d.y_lo, row * d.ld + c, d.y_dtype, v);
  }
}

// backward: per (image, group) sums of gamma * s1 and gamma * s2 (fixed pairwise tree), written after the partials in ws
__global__ void __launch_bounds__(64) gn_bwd_group_kernel(mtt_gn_desc d, int64_t nchunk, float* gs) {
  const int64_t ng = blockIdx.x;
  const int64_t n = ng / d.G;
  const int z = (int)(n / d.B);
  const int g = (int)(ng % d.G);
  const int cpg = d.C / d.G;
  const int64_t ne = nchunk * cpg;
  float a = 0.f, b = 0.f;
  for (int64_t e = threadIdx.x; e < ne; e += 64) {
    const int64_t chunk = e / cpg;
    const int c = g * cpg + (int)(e % cpg);
    const float* w = d.ws + ((n * nchunk + chunk) * d.C + c) * 2;
    const float ga = d.gamma[(int64_t)z * d.C + c];
    a = fmaf(ga, w[0], a);
    b = fmaf(ga, w[1], b);
  }
  __shared__ float sa[64], sb[64];
  sa[threadIdx.x] = a; sb[threadIdx.x] = b;
  __syncthreads();
  for (int off = 32; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) { sa[threadIdx.x] += sa[threadIdx.x + off]; sb[threadIdx.x] += sb[threadIdx.x + off]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { gs[ng * 2] = sa[0]; gs[ng * 2 + 1] = sb[0]; }
}

// dgamma / dbeta: one thread per (z, c), summing its images and chunks in order
__global__ void __launch_bounds__(256) gn_bwd_param_kernel(mtt_gn_desc d, int64_t nchunk) {
  const int64_t zc = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (zc >= (int64_t)d.Z * d.C) return;
  const int64_t z = zc / d.C, c = zc % d.C;
  float a = 0.f, b = 0.f;
  for (int64_t n = z * d.B; n < (z + 1) * d.B; ++n)
    for (int64_t chunk = 0; chunk < nchunk; ++chunk) {
      const float* w = d.ws + ((n * nchunk + chunk) * d.C + c) * 2;
      a += w[0];
      b += w[1];
    }
  if (d.dbeta) d.dbeta[zc] = a;
  if (d.dgamma) d.dgamma[zc] = b;
}

__global__ void __launch_bounds__(256) gn_bwd_apply_kernel(mtt_gn_desc d, const float* gs) {
  const int64_t row = blockIdx.x;
  const int64_t n = row / d.HW;
  const int z = (int)(n / d.B);
  const int cpg = d.C / d.G;
  const float inv_cnt = 1.0f / (float)(d.HW * cpg);
  for (int64_t c = threadIdx.x; c < d.ld; c += 256) {
    float v = 0.f;
    if (c < d.C) {
      const int64_t ng = n * d.G + (int)c / cpg;
      const float rs = d.rstd[ng];
      const float xh = (ld_elem(d.x, row * d.ld + c, d.x_dtype) - d.mean[ng]) * rs;
      const float ga = d.gamma[z * d.C + c];
      float du = ld_elem(d.dy, row * d.ld + c, d.dy_dtype);
      if (d.relu && fmaf(xh, ga, d.beta[z * d.C + c]) <= 0.f) du = 0.f;
      v = rs * (du * ga - gs[ng * 2] * inv_cnt - xh * gs[ng * 2 + 1] * inv_cnt);
    }
    st_elem(d.dx, row * d.ld + c, d.dx_dtype, v);
  }
}

extern "C" size_t mtt_groupnorm_ws_floats(const mtt_gn_desc* d) {
  if (gn_check(d)) return 0;
  const int64_t nb = (int64_t)d->Z * d->B;
  return (size_t)(nb * gn_nchunk(d) * d->C * 2 + nb * d->G * 2);
}

extern "C" int mtt_groupnorm_fwd(const mtt_gn_desc* d, void* stream) {
  if (const int e = gn_check(d)) return e;
  if (!d->x || !d->y || !d->gamma || !d->beta || !d->mean || !d->rstd || !d->ws || (d->y_dtype == MTT_SPLIT && !d->y_lo)) return MTT_E_BADARG;
  if (d->x_dtype == MTT_SPLIT) return MTT_E_UNSUPPORTED;
  const int64_t nb = (int64_t)d->Z * d->B, nchunk = gn_nchunk(d), rows = nb * d->HW;
  hipLaunchKernelGGL(gn_partial_kernel<0>, dim3((unsigned)nchunk, (unsigned)nb), dim3(256), 0, S_, *d, nchunk);
  hipLaunchKernelGGL(gn_stats_kernel, dim3((unsigned)(nb * d->G)), dim3(64), 0, S_, *d, nchunk);
  hipLaunchKernelGGL(gn_apply_kernel, dim3((unsigned)rows), dim3(256), 0, S_, *d);
  return LAUNCH_OK();
}

extern "C" int mtt_groupnorm_bwd(const mtt_gn_desc* d, void* stream) {
  if (const int e = gn_check(d)) return e;
  if (!d->x || !d->dy || !d->dx || !d->gamma || !d->beta || !d->mean || !d->rstd || !d->ws) return MTT_E_BADARG;
  if (d->x_dtype == MTT_SPLIT || d->dy_dtype == MTT_SPLIT || d->dx_dtype == MTT_SPLIT) return MTT_E_UNSUPPORTED;
  const int64_t nb = (int64_t)d->Z * d->B, nchunk = gn_nchunk(d), rows = nb * d->HW;
  float* gs = d->ws + nb * nchunk * d->C * 2;
  hipLaunchKernelGGL(gn_partial_kernel<1>, dim3((unsigned)nchunk, (unsigned)nb), dim3(256), 0, S_, *d, nchunk);
  hipLaunchKernelGGL(gn_bwd_group_kernel, dim3((unsigned)(nb * d->G)), dim3(64), 0, S_, *d, nchunk, gs);
  if (d->dgamma || d->dbeta)
    hipLaunchKernelGGL(gn_bwd_param_kernel, dim3((unsigned)cdiv64((int64_t)d->Z * d->C, 256)), dim3(256), 0, S_, *d, nchunk);
  hipLaunchKernelGGL(gn_bwd_apply_kernel, dim3((unsigned)rows), dim3(256), 0, S_, *d, (const float*)gs);
  return LAUNCH_OK();
}

// =====================================================================================================================
// Modulated deformable im2col / col2im (mmcv 1.6.2 modulated_deform_conv semantics, restated: see the header)
// =====================================================================================================================
struct DcnSample {
  float h, w, m;
  bool in;                                               // inside the (-1, H) x (-1, W) box
};

MTT_DEV DcnSample dcn_sample(const mtt_dcn_desc& d, int64_t row, int k) {
  const int64_t hw = (int64_t)d.Ho * d.Wo;
  const int64_t pix = row % hw;
  const int ho = (int)(pix / d.Wo), wo = (int)(pix % d.Wo);
  const int i = k / 3, j = k % 3;
  DcnSample s;
  s.h = (float)(ho * d.stride - d.pad + i * d.dil);
  s.w = (float)(wo * d.stride - d.pad + j * d.dil);
  if (d.offset) {
    s.h += ld_elem(d.offset, row * d.ld_off + 2 * k, d.off_dtype);
    s.w += ld_elem(d.offset, row * d.ld_off + 2 * k + 1, d.off_dtype);
  }
  s.m = 1.f;
  if (d.mask) {
    const float v = ld_elem(d.mask, row * d.ld_mask + k, d.off_dtype);
    s.m = d.mask_sigmoid ? 1.f / (1.f + __expf(-v)) : v;
  }
  s.in = s.h > -1.f && s.w > -1.f && s.h < (float)d.H && s.w < (float)d.W;
  return s;
}

// columns: one thread per (row, tap, 8-channel chunk)
__global__ void __launch_bounds__(256) dcn_im2col_kernel(mtt_dcn_desc d) {
  const int c8n = d.Cp / 8;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t rows = (int64_t)d.B * d.Ho * d.Wo;
  if (t >= rows * 9 * c8n) return;
  const int c0 = (int)(t % c8n) * 8;
  const int k = (int)((t / c8n) % 9);
  const int64_t row = t / (c8n * 9);
  const int b = (int)(row / ((int64_t)d.Ho * d.Wo));
  const DcnSample s = dcn_sample(d, row, k);
  float v[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) v[q] = 0.f;
  if (s.in) {
    const float hf = floorf(s.h), wf = floorf(s.w);
    const int hl = (int)hf, wl = (int)wf, hh = hl + 1, wh = wl + 1;
    const float lh = s.h - hf, lw = s.w - wf, uh = 1.f - lh, uw = 1.f - lw;
    const int64_t img = (int64_t)b * d.H * d.W;
    const int ys[4] = {hl, hl, hh, hh}, xs[4] = {wl, wh, wl, wh};
    const float ws[4] = {uh * uw, uh * lw, lh * uw, lh * lw};
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      if (ys[q4] < 0 || ys[q4] > d.H - 1 || xs[q4] < 0 || xs[q4] > d.W - 1) continue;
      const int64_t base = (img + (int64_t)ys[q4] * d.W + xs[q4]) * d.ldx + c0;
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = fmaf(ws[q4], ld_elem(d.x, base + q, d.x_dtype), v[q]);
    }
  }
  const int64_t o = row * d.ldc + (int64_t)k * d.Cp + c0;
#pragma unroll
  for (int q = 0; q < 8; ++q) st_any(d.col, d.col_lo, o + q, d.col_dtype, v[q] * s.m);
}

// bucket key of a sample: its floor cell (b, floor(h) + 1, floor(w) + 1); samples outside the box go to the last key
__global__ void __launch_bounds__(256) dcn_keys_kernel(mtt_dcn_desc d, unsigned* keys, unsigned* vals, int64_t ns) {
  const int64_t sidx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (sidx >= ns) return;
  const int64_t row = sidx / 9;
  const int k = (int)(sidx % 9);
  const DcnSample s = dcn_sample(d, row, k);
  const unsigned nbk = (unsigned)d.B * (d.H + 1) * (d.W + 1);
  unsigned key = nbk;
  if (s.in) {
    const int b = (int)(row / ((int64_t)d.Ho * d.Wo));
    const int hl = (int)floorf(s.h), wl = (int)floorf(s.w);
    key = ((unsigned)b * (d.H + 1) + (unsigned)(hl + 1)) * (d.W + 1) + (unsigned)(wl + 1);
  }
  keys[sidx] = key;
  vals[sidx] = (unsigned)sidx;
}

MTT_DEV int64_t lower_bound_u32(const unsigned* a, int64_t n, unsigned key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// dx: one thread per (input pixel, 8-channel chunk); the four buckets whose floor cell has this pixel as a corner, in a fixed order,
// each in sample order (the radix sort is stable)
__global__ void __launch_bounds__(256) dcn_col2im_kernel(mtt_dcn_desc d, const unsigned* skeys, const unsigned* svals, int64_t ns) {
  const int c8n = d.Cp / 8;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t npix = (int64_t)d.B * d.H * d.W;
  if (t >= npix * c8n) return;
  const int c0 = (int)(t % c8n) * 8;
  const int64_t pix = t / c8n;
  const int b = (int)(pix / ((int64_t)d.H * d.W));
  const int y = (int)((pix / d.W) % d.H), x = (int)(pix % d.W);
  float acc[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) acc[q] = 0.f;
  // corner q4 of a cell (hl, wl): 0 (hl, wl), 1 (hl, wl+1), 2 (hl+1, wl), 3 (hl+1, wl+1)
  for (int q4 = 0; q4 < 4; ++q4) {
    const int hl = y - (q4 >> 1), wl = x - (q4 & 1);
    const unsigned key = ((unsigned)b * (d.H + 1) + (unsigned)(hl + 1)) * (d.W + 1) + (unsigned)(wl + 1);
    const int64_t e0 = lower_bound_u32(skeys, ns, key), e1 = lower_bound_u32(skeys, ns, key + 1);
    for (int64_t e = e0; e < e1; ++e) {
      const int64_t sidx = svals[e];
      const int64_t row = sidx / 9;
      const int k = (int)(sidx % 9);
      const DcnSample s = dcn_sample(d, row, k);
      const float lh = s.h - floorf(s.h), lw = s.w - floorf(s.w);
      const float wgt = ((q4 >> 1) ? lh : 1.f - lh) * ((q4 & 1) ? lw : 1.f - lw) * s.m;
      const int64_t o = row * d.ldc + (int64_t)k * d.Cp + c0;
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[q] = fmaf(wgt, ld_elem(d.dcol, o + q, d.dcol_dtype), acc[q]);
    }
  }
  const int64_t o = pix * d.ldx + c0;
#pragma unroll
  for (int q = 0; q < 8; ++q) st_elem(d.dx, o + q, d.dx_dtype, c0 + q < d.C ? acc[q] : 0.f);
}

// d offset / d mask: one wave per sample, lanes over channels, fixed xor-shuffle tree.  The coordinate weights are mmcv's
// dmcn_get_coordinate_weight: the derivative of the bilinear sample with respect to h / w with the floor cell held fixed.
__global__ void __launch_bounds__(256) dcn_coord_kernel(mtt_dcn_desc d, int64_t ns) {
  const int lane = threadIdx.x & 63;
  const int64_t sidx = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (sidx >= ns) return;
  const int64_t row = sidx / 9;
  const int k = (int)(sidx % 9);
  const int b = (int)(row / ((int64_t)d.Ho * d.Wo));
  const DcnSample s = dcn_sample(d, row, k);
  float gh = 0.f, gw = 0.f, gm = 0.f;
  if (s.in) {
    const float hf = floorf(s.h), wf = floorf(s.w);
    const int hl = (int)hf, wl = (int)wf, hh = hl + 1, wh = wl + 1;
    const float lh = s.h - hf, lw = s.w - wf, uh = 1.f - lh, uw = 1.f - lw;
    const bool ok1 = hl >= 0 && wl >= 0, ok2 = hl >= 0 && wh <= d.W - 1, ok3 = hh <= d.H - 1 && wl >= 0, ok4 = hh <= d.H - 1 && wh <= d.W - 1;
    const int64_t img = (int64_t)b * d.H * d.W;
    const int64_t p1 = (img + (int64_t)hl * d.W + wl) * d.ldx, p2 = (img + (int64_t)hl * d.W + wh) * d.ldx;
    const int64_t p3 = (img + (int64_t)hh * d.W + wl) * d.ldx, p4 = (img + (int64_t)hh * d.W + wh) * d.ldx;
    const int64_t o = row * d.ldc + (int64_t)k * d.Cp;
    for (int c = lane; c < d.C; c += 64) {
      const float v1 = ok1 ? ld_elem(d.x, p1 + c, d.x_dtype) : 0.f, v2 = ok2 ? ld_elem(d.x, p2 + c, d.x_dtype) : 0.f;
      const float v3 = ok3 ? ld_elem(d.x, p3 + c, d.x_dtype) : 0.f, v4 = ok4 ? ld_elem(d.x, p4 + c, d.x_dtype) : 0.f;
      const float g = ld_elem(d.dcol, o + c, d.dcol_dtype);
      gm = fmaf(g, uh * uw * v1 + uh * lw * v2 + lh * uw * v3 + lh * lw * v4, gm);
      gh = fmaf(g, -uw * v1 - lw * v2 + uw * v3 + lw * v4, gh);
      gw = fmaf(g, -uh * v1 + uh * v2 - lh * v3 + lh * v4, gw);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    gh += __shfl_xor(gh, off, 64);
    gw += __shfl_xor(gw, off, 64);
    gm += __shfl_xor(gm, off, 64);
  }
  if (lane == 0) {
    if (d.doffset) {
      st_elem(d.doffset, row * d.ld_off + 2 * k, d.off_dtype, gh * s.m);
      st_elem(d.doffset, row * d.ld_off + 2 * k + 1, d.off_dtype, gw * s.m);
    }
    if (d.dmask) st_elem(d.dmask, row * d.ld_mask + k, d.off_dtype, d.mask_sigmoid ? gm * s.m * (1.f - s.m) : gm);
  }
}

static int dcn_check(const mtt_dcn_desc* d) {
  if (!d || d->B <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0 || d->Cp < d->C || (d->Cp % 8) || d->ldx < d->Cp || (d->ldx % 8) ||
      d->Ho <= 0 || d->Wo <= 0 || d->stride <= 0 || d->dil <= 0 || d->pad < 0 || d->ldc < 9 * (int64_t)d->Cp) return MTT_E_BADARG;
  if ((d->offset && d->ld_off < 18) || (d->mask && d->ld_mask < 9)) return MTT_E_BADARG;
  if (d->x_dtype == MTT_SPLIT || d->off_dtype == MTT_SPLIT) return MTT_E_UNSUPPORTED;
  if ((int64_t)d->B * d->Ho * d->Wo * 9 >= (1ll << 31) || (int64_t)d->B * (d->H + 1) * (d->W + 1) >= (1ll << 31)) return MTT_E_UNSUPPORTED;
  return 0;
}

static unsigned dcn_key_bits(const mtt_dcn_desc* d) {
  const uint64_t nbk = (uint64_t)d->B * (d->H + 1) * (d->W + 1);
  unsigned bits = 1;
  while (bits < 32 && (1ull << bits) <= nbk) ++bits;
  return bits;
}

static size_t dcn_sort_bytes(const mtt_dcn_desc* d, int64_t ns) {
  size_t bytes = 0;
  if (rocprim::radix_sort_pairs(nullptr, bytes, (unsigned*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr,
                                (size_t)ns, 0, dcn_key_bits(d)) != hipSuccess) return 0;
  return bytes;
}

extern "C" size_t mtt_dcn_col2im_ws_floats(const mtt_dcn_desc* d) {
  if (dcn_check(d)) return 0;
  const int64_t ns = (int64_t)d->B * d->Ho * d->Wo * 9;
  const int64_t arr = (ns + 63) / 64 * 64;            // four 256-byte aligned uint32 arrays, then the sort's own storage
  return (size_t)(4 * arr) + (dcn_sort_bytes(d, ns) + 3) / 4 + 64;
}

extern "C" int mtt_dcn_im2col(const mtt_dcn_desc* d, void* stream) {
  if (const int e = dcn_check(d)) return e;
  if (!d->x || !d->col || (d->col_dtype == MTT_SPLIT && !d->col_lo)) return MTT_E_BADARG;
  const int64_t n = (int64_t)d->B * d->Ho * d->Wo * 9 * (d->Cp / 8);
  hipLaunchKernelGGL(dcn_im2col_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, S_, *d);
  return LAUNCH_OK();
}

extern "C" int mtt_dcn_col2im_bwd(const mtt_dcn_desc* d, void* stream) {
  if (const int e = dcn_check(d)) return e;
  if (!d->x || !d->dcol || !d->ws || d->dcol_dtype == MTT_SPLIT || d->dx_dtype == MTT_SPLIT) return MTT_E_BADARG;
  if ((d->doffset && !d->offset) || (d->dmask && !d->mask)) return MTT_E_BADARG;
  const int64_t ns = (int64_t)d->B * d->Ho * d->Wo * 9;
  if (d->dx) {
    const int64_t arr = (ns + 63) / 64 * 64;
    unsigned* keys = (unsigned*)d->ws;
    unsigned* vals = keys + arr;
    unsigned* skeys = vals + arr;
    unsigned* svals = skeys + arr;
    void* tmp = (void*)(svals + arr);
    size_t bytes = dcn_sort_bytes(d, ns);
    hipLaunchKernelGGL(dcn_keys_kernel, dim3((unsigned)cdiv64(ns, 256)), dim3(256), 0, S_, *d, keys, vals, ns);
    const hipError_t se = rocprim::radix_sort_pairs(tmp, bytes, keys, skeys, vals, svals, (size_t)ns, 0, dcn_key_bits(d), S_);
    if (se != hipSuccess) return (int)se;
    const int64_t n = (int64_t)d->B * d->H * d->W * (d->Cp / 8);
    hipLaunchKernelGGL(dcn_col2im_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, S_, *d, (const unsigned*)skeys,
                       (const unsigned*)svals, ns);
  }
  if (d->doffset || d->dmask)
    hipLaunchKernelGGL(dcn_coord_kernel, dim3((unsigned)cdiv64(ns, 4)), dim3(256), 0, S_, *d, ns);
  return LAUNCH_OK();
}

// =====================================================================================================================
// FPN nearest-neighbour top-down add
// =====================================================================================================================
MTT_DEV int nearest_src(int o, int in, int out) {
  const float scale = (float)in / (float)out;          // torch's nearest_idx for an explicit output size (float scale, floorf)
  return min((int)floorf((float)o * scale), in - 1);
}

__global__ void __launch_bounds__(256) nearest_add_kernel(mtt_nearest_desc d) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)d.B * d.Ho * d.Wo * d.C) return;
  const int c = (int)(t % d.C);
  const int64_t pix = t / d.C;
  const int x = (int)(pix % d.Wo), y = (int)((pix / d.Wo) % d.Ho), b = (int)(pix / ((int64_t)d.Ho * d.Wo));
  const int64_t sp = ((int64_t)b * d.Hi + nearest_src(y, d.Hi, d.Ho)) * d.Wi + nearest_src(x, d.Wi, d.Wo);
  const float v = ld_elem(d.a, pix * d.ld_a + c, d.dtype) + ld_elem(d.src, sp * d.ld_src + c, d.dtype);
  st_elem(d.out, pix * d.ld_out + c, d.dtype, v);
}

// first fine index whose source index is >= s
MTT_DEV int nearest_first(int s, int in, int out) {
  int o = max(0, (int)((float)s * (float)out / (float)in) - 2);
  while (o < out && nearest_src(o, in, out) < s) ++o;
  return o;
}

__global__ void __launch_bounds__(256) nearest_add_bwd_kernel(mtt_nearest_desc d) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)d.B * d.Hi * d.Wi * d.C) return;
  const int c = (int)(t % d.C);
  const int64_t pix = t / d.C;
  const int ix = (int)(pix % d.Wi), iy = (int)((pix / d.Wi) % d.Hi), b = (int)(pix / ((int64_t)d.Hi * d.Wi));
  const int y0 = nearest_first(iy, d.Hi, d.Ho), x0 = nearest_first(ix, d.Wi, d.Wo);
  float acc = 0.f;
  for (int y = y0; y < d.Ho && nearest_src(y, d.Hi, d.Ho) == iy; ++y)
    for (int x = x0; x < d.Wo && nearest_src(x, d.Wi, d.Wo) == ix; ++x)
      acc += ld_elem(d.a, (((int64_t)b * d.Ho + y) * d.Wo + x) * d.ld_a + c, d.dtype);
  st_elem(d.out, pix * d.ld_out + c, d.dtype, acc);
}

static int nearest_check(const mtt_nearest_desc* d) {
  if (!d || !d->a || !d->out || d->B <= 0 || d->C <= 0 || d->Ho <= 0 || d->Wo <= 0 || d->Hi <= 0 || d->Wi <= 0 ||
      d->ld_a < d->C || d->ld_out < d->C || d->dtype == MTT_SPLIT) return MTT_E_BADARG;
  return 0;
}

extern "C" int mtt_nearest_add(const mtt_nearest_desc* d, void* stream) {
  if (const int e = nearest_check(d)) return e;
  if (!d->src || d->ld_src < d->C) return MTT_E_BADARG;
  const int64_t n = (int64_t)d->B * d->Ho * d->Wo * d->C;
  hipLaunchKernelGGL(nearest_add_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, S_, *d);
  return LAUNCH_OK();
}

extern "C" int mtt_nearest_add_bwd(const mtt_nearest_desc* d, void* stream) {
  if (const int e = nearest_check(d)) return e;
  const int64_t n = (int64_t)d->B * d->Hi * d->Wi * d->C;
  hipLaunchKernelGGL(nearest_add_bwd_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, S_, *d);
  return LAUNCH_OK();
}

// =====================================================================================================================
// FCOS3D per-level bbox tail + NCHW store
// =====================================================================================================================
// kind of output channel j: 0 identity, 1 s0*x, 2 exp(s1*x), 3 exp(s2*x) + 1e-6, 4 relu(s3*x)
MTT_DEV int bbox_kind(const mtt_bboxpost_desc& d, int j, int nch) {
  if (!d.scales) return 0;
  if (d.bbox2d && j >= nch - 4) return 4;
  if (j < 2) return 1;
  if (j == 2) return 2;
  if (j < 6) return 3;
  return 0;
}

static int bbox_nch(const mtt_bboxpost_desc* d) {
  int n = 0;
  for (int g = 0; g < d->ngroups; ++g) n += d->dims[g];
  return n;
}

__global__ void __launch_bounds__(256) bbox_post_kernel(mtt_bboxpost_desc d, int nch) {
  const int64_t hw = (int64_t)d.H * d.W;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)d.B * nch * hw) return;
  const int64_t p = t % hw;
  const int j = (int)((t / hw) % nch);
  const int64_t b = t / (hw * nch);
  int g = 0, c = j;
  while (c >= d.dims[g]) c -= d.dims[g++];
  const float x = d.x[g][(b * hw + p) * d.ldx[g] + c];
  float v = x;
  switch (bbox_kind(d, j, nch)) {
    case 1: v = d.scales[0] * x; break;
    case 2: v = expf(d.scales[1] * x); break;
    case 3: v = expf(d.scales[2] * x) + 1e-6f; break;
    case 4: v = fmaxf(d.scales[3] * x, 0.f); break;
    default: break;
  }
  d.out[t] = v;
}

// one thread per pixel: dx of every channel, and the pixel's contributions to the four scale gradients (workgroup tree -> ws)
__global__ void __launch_bounds__(256) bbox_post_bwd_kernel(mtt_bboxpost_desc d, int nch) {
  const int64_t hw = (int64_t)d.H * d.W;
  const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float ds[4] = {0.f, 0.f, 0.f, 0.f};
  if (pix < d.B * hw) {
    const int64_t b = pix / hw, p = pix % hw;
    int j = 0;
    for (int g = 0; g < d.ngroups; ++g) {
      for (int c = 0; c < d.ldx[g]; ++c) {
        float gx = 0.f;
        if (c < d.dims[g]) {
          const float x = d.x[g][pix * d.ldx[g] + c];
          const float go = d.dout[(b * nch + j) * hw + p];
          switch (bbox_kind(d, j, nch)) {
            case 1: gx = go * d.scales[0]; ds[0] = fmaf(go, x, ds[0]); break;
            case 2: { const float e = expf(d.scales[1] * x); gx = go * e * d.scales[1]; ds[1] = fmaf(go * e, x, ds[1]); } break;
            case 3: { const float e = expf(d.scales[2] * x); gx = go * e * d.scales[2]; ds[2] = fmaf(go * e, x, ds[2]); } break;
            case 4: if (d.scales[3] * x > 0.f) { gx = go * d.scales[3]; ds[3] = fmaf(go, x, ds[3]); } break;
            default: gx = go; break;
          }
          ++j;
        }
        if (d.dx[g]) d.dx[g][pix * d.ldx[g] + c] = gx;
      }
    }
  }
  if (!d.scales) return;
  __shared__ float sh[4][256];
#pragma unroll
  for (int i = 0; i < 4; ++i) sh[i][threadIdx.x] = ds[i];
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off)
#pragma unroll
      for (int i = 0; i < 4; ++i) sh[i][threadIdx.x] += sh[i][threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x < 4) d.ws[(int64_t)blockIdx.x * 4 + threadIdx.x] = sh[threadIdx.x][0];
}

__global__ void __launch_bounds__(64) bbox_post_final_kernel(mtt_bboxpost_desc d, int nblk) {
  if (threadIdx.x >= 4) return;
  float a = 0.f;
  for (int i = 0; i < nblk; ++i) a += d.ws[(int64_t)i * 4 + threadIdx.x];
  d.dscales[threadIdx.x] = a;
}

static int bbox_check(const mtt_bboxpost_desc* d) {
  if (!d || d->ngroups <= 0 || d->ngroups > 8 || d->B <= 0 || d->H <= 0 || d->W <= 0) return MTT_E_BADARG;
  for (int g = 0; g < d->ngroups; ++g)
    if (!d->x[g] || d->dims[g] <= 0 || d->ldx[g] < d->dims[g]) return MTT_E_BADARG;
  const int nch = bbox_nch(d);
  if (d->scales && nch < (d->bbox2d ? 10 : 6)) return MTT_E_BADARG;
  return 0;
}

static int64_t bbox_nblk(const mtt_bboxpost_desc* d) { return cdiv64((int64_t)d->B * d->H * d->W, 256); }

extern "C" size_t mtt_fcos_bbox_post_ws_floats(const mtt_bboxpost_desc* d) {
  if (!d || d->B <= 0 || d->H <= 0 || d->W <= 0) return 0;
  return (size_t)bbox_nblk(d) * 4;
}

extern "C" int mtt_fcos_bbox_post(const mtt_bboxpost_desc* d, void* stream) {
  if (const int e = bbox_check(d)) return e;
  if (!d->out) return MTT_E_BADARG;
  const int nch = bbox_nch(d);
  const int64_t n = (int64_t)d->B * nch * d->H * d->W;
  hipLaunchKernelGGL(bbox_post_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, S_, *d, nch);
  return LAUNCH_OK();
}

extern "C" int mtt_fcos_bbox_post_bwd(const mtt_bboxpost_desc* d, void* stream) {
  if (const int e = bbox_check(d)) return e;
  if (!d->dout || (d->scales && (!d->dscales || !d->ws))) return MTT_E_BADARG;
  const int nch = bbox_nch(d);
  const int64_t nblk = bbox_nblk(d);
  hipLaunchKernelGGL(bbox_post_bwd_kernel, dim3((unsigned)nblk), dim3(256), 0, S_, *d, nch);
  if (d->scales) hipLaunchKernelGGL(bbox_post_final_kernel, dim3(1), dim3(64), 0, S_, *d, (int)nblk);
  return LAUNCH_OK();
}
