// det_loss3d.hip — the FCOS3D criterion of the 3ddet task (ABI 15): target assignment and the eight loss terms of DetModel.loss, forward
// and backward.  See include/mtt_hip.h for the contract.
//
// The assignment reproduces the reference's fp32 arithmetic operation by operation, so labels match it bit for bit: FMA contraction is
// off for this whole file.  The loss sums go through per-workgroup partials summed in workgroup order by one workgroup (no atomics):
// bitwise reproducible run to run, and num_pos / the averaging factors never leave the device.
#pragma clang fp contract(off)
#include "mtt_device.h"

#define S_ ((hipStream_t)stream)

namespace {

constexpr int TB = 256;            // threads per workgroup: one point each
constexpr int GT_CHUNK = 128;      // gt records staged in LDS per round (8 KiB)
constexpr int REC = 16;            // floats per gt record
constexpr int NREG = 13;           // regression channels (pred_bbox2d)
constexpr int NSUM = 11;           // partial sums: cls, offset, depth, size, rot, dir0, dir1, dir2, ctr, bbox2d, num_pos
constexpr int WSP = 12;            // partial stride (floats)
constexpr float BIG = 1e8f;        // det_model.py INF
constexpr float TWO_PI_F = 6.283185307179586f;   // fp32(2 * np.pi)
constexpr float PI_F = 3.141592653589793f;       // fp32(2 * np.pi / 2)

MTT_DEV float softplus_f(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }   // log(1 + e^x)
MTT_DEV float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

// sigmoid focal loss of one logit (det_losses.py py_sigmoid_focal_loss, gamma / alpha) and its derivative; the derivative follows the
// reference's autograd, which differentiates through the focal weight as well
MTT_DEV void focal(float x, bool pos, float gamma, float alpha, float& loss, float& grad) {
  const float s = sigmoid_f(x);
  if (pos) {
    const float q = 1.0f - s, bce = softplus_f(-x);
    const float m = gamma == 2.0f ? q * q : powf(q, gamma), m1 = gamma == 2.0f ? q : powf(q, gamma - 1.0f);
    loss = alpha * m * bce;
    grad = alpha * (m * (s - 1.0f) - gamma * m1 * s * q * bce);
  } else {
    const float bce = softplus_f(x);
    const float m = gamma == 2.0f ? s * s : powf(s, gamma), m1 = gamma == 2.0f ? s : powf(s, gamma - 1.0f);
    loss = (1.0f - alpha) * m * bce;
    grad = (1.0f - alpha) * (m * s + gamma * m1 * s * (1.0f - s) * bce);
  }
}

MTT_DEV int level_of(const mtt_fcos3d_desc& d, int64_t p, int64_t& q) {
  int64_t base = 0;
  int lv = 0;
  for (; lv < d.nlev - 1; ++lv) {
    const int64_t n = (int64_t)d.H[lv] * d.W[lv];
    if (p < base + n) break;
    base += n;
  }
  q = p - base;
  return lv;
}

MTT_DEV int dir_bin(float rot, float dir_offset) {
  const float v = rot - dir_offset;
  const float lp = v - floorf(v / TWO_PI_F + 0.0f) * TWO_PI_F;        // limit_period(v, 0, 2 pi)
  const float b = floorf(lp / PI_F);
  return b < 0.f ? 0 : (b > 1.f ? 1 : (int)b);
}

// smooth-L1 of the diff and its derivative
MTT_DEV void sl1(float df, float beta, float& loss, float& grad) {
  const float a = fabsf(df);
  loss = a < beta ? 0.5f * a * a / beta : a - 0.5f * beta;
  grad = a < beta ? df / beta : (df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f));
}

MTT_DEV float block_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const float r = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return r;
}

// grid (point blocks, labelled images): assignment (+ the loss partials when LOSS)
template <bool LOSS>
__global__ __launch_bounds__(TB) void fcos3d_fwd_kernel(const mtt_fcos3d_desc d) {
  __shared__ float sg[GT_CHUNK * REC];
  __shared__ float red[4];
  const int k = blockIdx.y;
  const int goff = d.img[k], gcnt = d.img[d.n_lab + k], b = d.img[2 * d.n_lab + k];
  const int64_t p = (int64_t)blockIdx.x * TB + threadIdx.x;
  const bool valid = p < d.P;
  int64_t q = 0;
  const int lv = valid ? level_of(d, p, q) : 0;
  const int W = d.W[lv];
  const float st = d.stride[lv], rad = d.radius[lv], lo = d.rr_lo[lv], hi = d.rr_hi[lv];
  const float xs = (float)(int)(q % W) * st + d.half[lv];
  const float ys = (float)(int)(q / W) * st + d.half[lv];
  float best = BIG;
  int bi = 0;
  for (int c0 = 0; c0 < gcnt; c0 += GT_CHUNK) {
    const int nc = min(GT_CHUNK, gcnt - c0);
    __syncthreads();
    for (int i = threadIdx.x; i < nc * REC; i += TB) sg[i] = d.gts[(int64_t)(goff + c0) * REC + i];
    __syncthreads();
    if (valid) {
      for (int j = 0; j < nc; ++j) {
        const float* r = sg + j * REC;
        const float cx = r[5], cy = r[6];
        const float dx = xs - cx, dy = ys - cy;
        const float left = xs - r[0], right = r[2] - xs, top = ys - r[1], bottom = r[3] - ys;
        const float cbl = xs - (cx - rad), cbr = (cx + rad) - xs, cbt = ys - (cy - rad), cbb = (cy + rad) - ys;
        const bool inside = fminf(fminf(cbl, cbt), fminf(cbr, cbb)) > 0.f;
        const float mx = fmaxf(fmaxf(left, top), fmaxf(right, bottom));
        const bool in_range = mx >= lo && mx <= hi;
        float dist = sqrtf(dx * dx + dy * dy);
        if (!inside || !in_range) dist = BIG;
        if (dist < best) { best = dist; bi = c0 + j; }
      }
    }
  }
  float t[NREG];
  int label = d.C;
  float ctr_t = 0.f;
  if (valid) {
    if (gcnt > 0) {
      const float* r = d.gts + (int64_t)(goff + bi) * REC;
      if (best != BIG) label = (int)r[4];
      const float dx = xs - r[5], dy = ys - r[6];
      t[0] = dx / st; t[1] = dy / st; t[2] = r[7];
      for (int c = 0; c < 6; ++c) t[3 + c] = r[8 + c];
      t[9] = (xs - r[0]) / st; t[10] = (ys - r[1]) / st; t[11] = (r[2] - xs) / st; t[12] = (r[3] - ys) / st;
      const float rel = sqrtf(dx * dx + dy * dy) / (1.414f * rad);
      ctr_t = expf(-d.ctr_alpha * rel);
    } else {
      for (int c = 0; c < NREG; ++c) t[c] = 0.f;
    }
    const int64_t o = (int64_t)k * d.P + p;
    d.label[o] = label;
    d.centerness[o] = ctr_t;
    for (int c = 0; c < NREG; ++c) d.target[((int64_t)k * NREG + c) * d.P + p] = t[c];
  }
  if (!LOSS) return;
  float s[NSUM];
  for (int i = 0; i < NSUM; ++i) s[i] = 0.f;
  if (valid) {
    const int64_t HW = (int64_t)d.H[lv] * W;
    const float* cls = d.cls[lv] + (int64_t)b * d.C * HW + q;
    for (int c = 0; c < d.C; ++c) {
      float l, g;
      focal(cls[c * HW], label == c, d.gamma, d.alpha, l, g);
      s[0] += l;
    }
    if (label >= 0 && label < d.C) {
      const float* bb = d.bbox[lv] + (int64_t)b * NREG * HW + q;
      for (int c = 0; c < NREG; ++c) {
        float pv = bb[c * HW], tv = t[c];
        if (c >= 6 && c < 9) {                                   // add_sin_difference
          const float pe = sinf(pv) * cosf(tv), te = cosf(pv) * sinf(tv);
          pv = pe; tv = te;
        }
        float l, g;
        sl1(pv - tv, c < 9 ? d.beta : d.beta2d, l, g);
        l = l * d.code_weight[c];
        s[c < 2 ? 1 : c < 3 ? 2 : c < 6 ? 3 : c < 9 ? 4 : 9] += l;
      }
      const float* dr = d.dir[lv] + (int64_t)b * 6 * HW + q;
      for (int r = 0; r < 3; ++r) {
        const float a0 = dr[(2 * r) * HW], a1 = dr[(2 * r + 1) * HW];
        const float m = fmaxf(a0, a1);
        const float lse = m + logf(expf(a0 - m) + expf(a1 - m));
        s[5 + r] += lse - (dir_bin(t[6 + r], d.dir_offset) ? a1 : a0);
      }
      const float x = d.ctr[lv][(int64_t)b * HW + q];
      s[8] += fmaxf(x, 0.f) - x * ctr_t + log1pf(expf(-fabsf(x)));
      s[10] = 1.f;
    }
  }
  float* part = d.ws + ((int64_t)k * gridDim.x + blockIdx.x) * WSP;
  for (int i = 0; i < NSUM; ++i) {
    const float v = block_sum(s[i], red);
    if (threadIdx.x == 0) part[i] = v;
  }
}

// one workgroup: the partials of every (image, block) in workgroup order -> out[9], stats[2]
__global__ __launch_bounds__(TB) void fcos3d_final_kernel(const mtt_fcos3d_desc d, int nparts) {
  __shared__ double red[TB];
  __shared__ double tot[NSUM];
  for (int i = 0; i < NSUM; ++i) {
    double a = 0.0;
    for (int j = threadIdx.x; j < nparts; j += TB) a += (double)d.ws[(int64_t)j * WSP + i];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int o = TB / 2; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) tot[i] = red[0];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const float np = (float)tot[10];
  const float avg = (float)(tot[10] + (double)d.n_lab);
  float o[8];
  o[0] = d.loss_weight[0] * ((float)tot[0] / avg);
  if (np > 0.f) {
    o[1] = d.loss_weight[1] * ((float)tot[1] / np);
    o[2] = d.loss_weight[1] * ((float)tot[2] / np);
    o[3] = d.loss_weight[1] * ((float)tot[3] / np);
    o[4] = d.loss_weight[1] * ((float)tot[4] / np);
    float dsum = 0.f;
    for (int r = 0; r < 3; ++r) dsum = dsum + d.loss_weight[2] * ((float)tot[5 + r] / np);
    o[5] = dsum;
    o[6] = d.loss_weight[3] * ((float)tot[8] / np);
    o[7] = d.loss_weight[4] * ((float)tot[9] / np);
  } else {
    for (int i = 1; i < 8; ++i) o[i] = 0.f;
  }
  float sum = 0.f;
  for (int i = 0; i < 8; ++i) { d.out[i] = o[i]; sum = sum + o[i]; }
  d.out[8] = sum;
  d.stats[0] = np;
  d.stats[1] = avg;
}

// grid (point blocks, batch images): every element of the four gradient maps
__global__ __launch_bounds__(TB) void fcos3d_bwd_kernel(const mtt_fcos3d_desc d) {
  const int b = blockIdx.y;
  const int64_t p = (int64_t)blockIdx.x * TB + threadIdx.x;
  if (p >= d.P) return;
  int64_t q = 0;
  const int lv = level_of(d, p, q);
  const int64_t HW = (int64_t)d.H[lv] * d.W[lv];
  const int k = d.img[3 * d.n_lab + b];
  float* dcls = d.dcls[lv] + (int64_t)b * d.C * HW + q;
  float* dbb = d.dbbox[lv] + (int64_t)b * NREG * HW + q;
  float* ddr = d.ddir[lv] + (int64_t)b * 6 * HW + q;
  float* dct = d.dctr[lv] + (int64_t)b * HW + q;
  int label = d.C;
  if (k >= 0) label = d.label[(int64_t)k * d.P + p];
  const float np = d.stats[0], avg = d.stats[1];
  if (k >= 0) {
    const float gc = (d.gout[0] + d.gout[8]) * d.loss_weight[0] / avg;
    const float* cls = d.cls[lv] + (int64_t)b * d.C * HW + q;
    for (int c = 0; c < d.C; ++c) {
      float l, g;
      focal(cls[c * HW], label == c, d.gamma, d.alpha, l, g);
      dcls[c * HW] = g * gc;
    }
  } else {
    for (int c = 0; c < d.C; ++c) dcls[c * HW] = 0.f;
  }
  if (k < 0 || !(label >= 0 && label < d.C) || !(np > 0.f)) {
    for (int c = 0; c < NREG; ++c) dbb[c * HW] = 0.f;
    for (int c = 0; c < 6; ++c) ddr[c * HW] = 0.f;
    dct[0] = 0.f;
    return;
  }
  const float* bb = d.bbox[lv] + (int64_t)b * NREG * HW + q;
  const float* tg = d.target + (int64_t)k * NREG * d.P + p;
  for (int c = 0; c < NREG; ++c) {
    const int comp = c < 2 ? 1 : c < 3 ? 2 : c < 6 ? 3 : c < 9 ? 4 : 7;
    const float gk = (d.gout[comp] + d.gout[8]) * d.loss_weight[c < 9 ? 1 : 4] / np * d.code_weight[c];
    const float pv = bb[c * HW], tv = tg[c * d.P];
    float l, g;
    if (c >= 6 && c < 9) {
      const float sp = sinf(pv), cp = cosf(pv), stv = sinf(tv), ctv = cosf(tv);
      sl1(sp * ctv - cp * stv, d.beta, l, g);
      g = g * (cp * ctv + sp * stv);
    } else {
      sl1(pv - tv, c < 9 ? d.beta : d.beta2d, l, g);
    }
    dbb[c * HW] = g * gk;
  }
  const float gd = (d.gout[5] + d.gout[8]) * d.loss_weight[2] / np;
  const float* dr = d.dir[lv] + (int64_t)b * 6 * HW + q;
  for (int r = 0; r < 3; ++r) {
    const float a0 = dr[(2 * r) * HW], a1 = dr[(2 * r + 1) * HW];
    const float m = fmaxf(a0, a1);
    const float e0 = expf(a0 - m), e1 = expf(a1 - m), z = e0 + e1;
    const int bin = dir_bin(tg[(6 + r) * d.P], d.dir_offset);
    ddr[(2 * r) * HW] = (e0 / z - (bin == 0 ? 1.f : 0.f)) * gd;
    ddr[(2 * r + 1) * HW] = (e1 / z - (bin == 1 ? 1.f : 0.f)) * gd;
  }
  const float x = d.ctr[lv][(int64_t)b * HW + q];
  const float ct = d.centerness[(int64_t)k * d.P + p];
  dct[0] = (sigmoid_f(x) - ct) * ((d.gout[6] + d.gout[8]) * d.loss_weight[3] / np);
}

int check(const mtt_fcos3d_desc* d, bool maps) {
  if (!d || d->nlev <= 0 || d->nlev > MTT_FCOS3D_MAX_LEVELS || d->B <= 0 || d->n_lab <= 0 || d->n_lab > d->B || d->n_lab > 65535 ||
      d->C <= 0 || d->P <= 0 || d->P > (int64_t)1 << 30 || !d->img || !d->gts || !d->label || !d->target || !d->centerness)
    return MTT_E_BADARG;
  int64_t P = 0;
  for (int l = 0; l < d->nlev; ++l) {
    if (d->H[l] <= 0 || d->W[l] <= 0 || !(d->stride[l] > 0.f)) return MTT_E_BADARG;
    if (maps && (!d->cls[l] || !d->bbox[l] || !d->dir[l] || !d->ctr[l])) return MTT_E_BADARG;
    P += (int64_t)d->H[l] * d->W[l];
  }
  return P == d->P ? 0 : MTT_E_BADARG;
}

unsigned nblk(const mtt_fcos3d_desc* d) { return (unsigned)((d->P + TB - 1) / TB); }

}  // namespace

extern "C" size_t mtt_fcos3d_desc_size(void) { return sizeof(mtt_fcos3d_desc); }

extern "C" size_t mtt_fcos3d_ws_floats(const mtt_fcos3d_desc* d) {
  if (!d || d->P <= 0 || d->n_lab <= 0) return 0;
  return (size_t)nblk(d) * d->n_lab * WSP;
}

extern "C" int mtt_fcos3d_targets(const mtt_fcos3d_desc* d, void* stream) {
  if (int e = check(d, false)) return e;
  hipLaunchKernelGGL(fcos3d_fwd_kernel<false>, dim3(nblk(d), d->n_lab), dim3(TB), 0, S_, *d);
  return (int)hipGetLastError();
}

extern "C" int mtt_fcos3d_loss_fwd(const mtt_fcos3d_desc* d, void* stream) {
  if (int e = check(d, true)) return e;
  if (!d->ws || !d->out || !d->stats) return MTT_E_BADARG;
  hipLaunchKernelGGL(fcos3d_fwd_kernel<true>, dim3(nblk(d), d->n_lab), dim3(TB), 0, S_, *d);
  hipLaunchKernelGGL(fcos3d_final_kernel, dim3(1), dim3(TB), 0, S_, *d, (int)(nblk(d) * d->n_lab));
  return (int)hipGetLastError();
}

extern "C" int mtt_fcos3d_loss_bwd(const mtt_fcos3d_desc* d, void* stream) {
  if (int e = check(d, true)) return e;
  if (!d->stats || !d->gout) return MTT_E_BADARG;
  for (int l = 0; l < d->nlev; ++l)
    if (!d->dcls[l] || !d->dbbox[l] || !d->ddir[l] || !d->dctr[l]) return MTT_E_BADARG;
  hipLaunchKernelGGL(fcos3d_bwd_kernel, dim3(nblk(d), d->B), dim3(TB), 0, S_, *d);
  return (int)hipGetLastError();
}
