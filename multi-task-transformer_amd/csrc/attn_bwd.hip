// mtt_attn_bwd: flash-style backward of mtt_attn_fwd (bf16 storage, head_dim 64).  The N x N probabilities are recomputed
// tile by tile from q, k and the forward's log-sum-exp; nothing of size N x N reaches HBM and no atomics are used: two
// kernels own disjoint outputs.  Both use the "swapped product" form of attn_fast.hip: a score tile comes out of the MFMA
// in the C layout that IS the B fragment of the next product (reduction index permuted consistently on the A side, whose
// fragments are two 8-byte transpose reads of the row-major LDS tile), so P and dS never go through LDS.
//
//   stat[b,h,0,i] = sum_d dO[i,d] * O[i,d],  stat[b,h,1,i] = lse[i] * log2(e)                (written by the dQ kernel for its own 128
//                 rows, read by the dK/dV kernel launched behind it on the same stream)
//   dQ kernel : workgroup = 128 query rows (32 per wave, B fragments of Q and dO in registers); per 64-key tile
//                 S^T = K Q^T, dP^T = V dO^T, dS^T = P^T o (dP^T - D),   dQ^T += K^T dS^T
//   dKV kernel: workgroup = 128 keys (32 per wave, B fragments of K and V in registers); per 64-query tile
//                 S = Q K^T, dP = dO V^T,   dV^T += dO^T P,   dK^T += Q^T dS
// The softmax scale is applied once to the dQ / dK accumulators; drawlog (gradient of the forward's UNSCALED prompt-row
// logits) is therefore added to dS divided by the scale.
//
// Three choices that each won an A/B against its plainer form (profiles/r09_attn_bwd_tiles_ab.log):
//   * the tile kind (full / ragged, with / without the drawlog add) is a compile-time argument of tile(); interior tiles run a body
//     without any end-of-sequence select;
//   * the dK/dV kernel's per-row D and lse*log2(e) values travel with the Q / dO tile by LDS-DMA (no ordinary global load, hence no
//     compiler-placed vmcnt(0), while the next tile's DMA is in flight);
//   * the dQ kernel computes D for its 128 rows and writes both stat rows (no separate statistics kernel).
// Two register-staged generations of both kernels (a transposed copy of each tile staged in LDS) and the plainer forms last existed at
// commit f779e8e; these kernels matched the register-staged ones bit for bit on the shapes of tests/golden/attn_bitwise.json.
#include "mtt_device.h"
#include <type_traits>

namespace {

constexpr int HD = 64;
constexpr int KTILE = 64 * HD * 2;   // 8 KiB per bf16 tile
constexpr float LOG2E = 1.4426950408889634f;

struct BwdP {
  const bf16_t* qkv; const bf16_t* dout; float* stat; const float* drawlog; bf16_t* dqkv;   // stat: the dQ kernel writes it, dK/dV reads it
  int B, N, nH, T, Np; float scale;
  const bf16_t* out; const float* lse;
  const float* skip_scale;                              // mtt_attn_desc.skip_scale (NULL = off)
};

// DropPath skip: are the patch rows of image b dead (dout == 0 there, out / lse possibly never written)?  Block-uniform, scalar unit.
MTT_DEV bool bwd_patches_dead(const BwdP& p, int b) { return p.skip_scale != nullptr && p.skip_scale[2 * b + 1] == 0.0f; }

// sum over one 8-element chunk of dO * O (packed bf16 pairs): the unit of the summation order of stat[.,.,0,.], which the dQ kernel fixes
// (within a chunk: the four pairs in order, lo * lo + hi * hi each; then the pairwise tree over the head's eight chunks there)
MTT_DEV float dot8_bf16(const u32x4& a, const u32x4& g) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) s += lo_of(a[j]) * lo_of(g[j]) + hi_of(a[j]) * hi_of(g[j]);
  return s;
}

// ---- staging (see attn_fast.hip): tiles go HBM -> LDS by LDS-DMA as they sit in memory ([64 rows][8 chunks of 16 B]); the transposed
// A fragments (K^T, Q^T, dO^T) come from ds_read_b64_tr_b16 on the SAME row-major image, so no transposed copy is staged at all (both
// kernels stage 16 KiB per tile).  One swizzle serves both read kinds: 16-byte chunk c of row r sits at position c ^ x(r), x(r) = ((r >> 1) & 3) << 1 | ((r >> 3) & 1): the 16 rows of a ds_read_b128 fragment read hit 16
// different (row parity, position) pairs, and the 8 rows a 32-lane half of a transpose read touches hit 8 different 32-byte units.
__device__ __attribute__((aligned(32))) const unsigned g_bwd_zero_page[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
MTT_DEV int bwd_swz(int row) { return (((row >> 1) & 3) << 1) | ((row >> 3) & 1); }
MTT_DEV void bwd_glds16(const bf16_t* src, unsigned char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}
MTT_DEV void bwd_glds4(const float* src, unsigned char* lds_wave_base) {   // 64 lanes x 4 B = 64 consecutive floats
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 4, 0, 0);
}
// tile kinds (and LDS stage) of the loops: a compile-time 0 / 1
using BwdNo = std::integral_constant<int, 0>;
using BwdYes = std::integral_constant<int, 1>;
template <int OFF>
MTT_DEV u32x2 bwd_ds_read_tr16(unsigned addr) {
  u32x2 r;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF) : "memory");
  return r;
}
template <int OFF>
MTT_DEV f32x4 bwd_ds_read_f4(unsigned addr) {
  f32x4 r;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF) : "memory");
  return r;
}
#define BWD_TRW(x) "+v"(x)
// waits for EVERY outstanding LDS read; the transpose-read destinations are in/out operands so that no use (and no register copy) of them
// can be placed above the wait — the asm loads are invisible to the compiler's own wait counting
#define BWD_WAIT_TR8(a, b)                                                                                                              \
  asm volatile("s_waitcnt lgkmcnt(0)" : BWD_TRW(a[0]), BWD_TRW(a[1]), BWD_TRW(a[2]), BWD_TRW(a[3]), BWD_TRW(b[0]), BWD_TRW(b[1]), BWD_TRW(b[2]), BWD_TRW(b[3]) :: "memory")
#define BWD_WAIT_TR16_F4(a, b, c, d, e, f)                                                                                              \
  asm volatile("s_waitcnt lgkmcnt(0)" : BWD_TRW(a[0]), BWD_TRW(a[1]), BWD_TRW(a[2]), BWD_TRW(a[3]), BWD_TRW(b[0]), BWD_TRW(b[1]), BWD_TRW(b[2]), BWD_TRW(b[3]), \
               BWD_TRW(c[0]), BWD_TRW(c[1]), BWD_TRW(c[2]), BWD_TRW(c[3]), BWD_TRW(d[0]), BWD_TRW(d[1]), BWD_TRW(d[2]), BWD_TRW(d[3]),                       \
               BWD_TRW(e[0]), BWD_TRW(e[1]), BWD_TRW(f[0]), BWD_TRW(f[1]) :: "memory")

// --------------------------------------------------------------------------------------------------------
// Both loops are unrolled by the two LDS stages (immediate stage offsets) and run their MFMA clusters at raised wave priority.
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_kernel(const BwdP p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int STAGE = 2 * KTILE;                  // K, V
  const int nqb = (p.N + 127) / 128;                // XCD-aware 1-D grid: one head's blocks share an XCD's L2
  const int wi = xcd_remap(blockIdx.x, gridDim.x);
  const int qb = wi % nqb, bh_ = wi / nqb;
  const int h = bh_ % p.nH, b = bh_ / p.nH;
  const int N = p.N, C = p.nH * HD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int64_t tok0 = (int64_t)b * N;
  const int64_t bh = (int64_t)b * p.nH + h;
  if (qb * 128 >= p.T && bwd_patches_dead(p, b)) {
    // a block of dead patch rows (the blocks the forward skipped): dS = 0 for its rows, so dq = 0.  Its stat entries stay unwritten —
    // the dK/dV kernel does not visit these rows — except the zero padding, which keeps its contract.  No barrier has been reached.
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + 256 * i, qrow = qb * 128 + (idx >> 3);
      if (qrow < N) *(u32x4*)(p.dqkv + (tok0 + qrow) * 3 * C + h * HD + (idx & 7) * 8) = (u32x4){0u, 0u, 0u, 0u};
    }
    if (qb == nqb - 1 && tid < p.Np - N) {
      p.stat[bh * 2 * p.Np + N + tid] = 0.f;
      p.stat[bh * 2 * p.Np + p.Np + N + tid] = 0.f;
    }
    return;
  }
  const int q0 = qb * 128 + wave * 32;
  const bool active = q0 < N;

  u32x4 qf[2][2], gf[2][2], dummy;
  float lse2[2], Dq[2];
#pragma unroll
  for (int sub = 0; sub < 2; ++sub) {
    const int qrow = q0 + sub * 16 + li;
    const bool ok = qrow < N;
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      Raw8<false> r;
      load8_raw<false>(p.qkv, (tok0 + qrow) * 3 * C + h * HD + kh * 32 + lg * 8, ok, r);
      cvt8<false, false>(ok, r, qf[sub][kh], dummy);
      load8_raw<false>(p.dout, (tok0 + qrow) * C + h * HD + kh * 32 + lg * 8, ok, r);
      cvt8<false, false>(ok, r, gf[sub][kh], dummy);
    }
    // D[q] = sum_d dO[q,d] O[q,d]: the 8-element chunk sums (dot8_bf16), then the pairwise tree over the head's eight chunks
    // (chunk = 4 kh + lg: partner chunk ^ 1 is lane ^ 16, chunk ^ 2 is lane ^ 32, chunk ^ 4 the other kh register)
    float c[2];
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      Raw8<false> r;
      u32x4 of;
      load8_raw<false>(p.out, (tok0 + qrow) * C + h * HD + kh * 32 + lg * 8, ok, r);
      cvt8<false, false>(ok, r, of, dummy);
      c[kh] = dot8_bf16(of, gf[sub][kh]);
      c[kh] += __shfl_xor(c[kh], 16, 64);
      c[kh] += __shfl_xor(c[kh], 32, 64);
    }
    Dq[sub] = c[0] + c[1];
    lse2[sub] = ok ? p.lse[bh * N + qrow] * LOG2E : 0.f;
    if (ok && lg == 0) {
      p.stat[bh * 2 * p.Np + qrow] = Dq[sub];
      p.stat[bh * 2 * p.Np + p.Np + qrow] = lse2[sub];
    }
  }
  if (qb == nqb - 1 && tid < p.Np - N) {               // the head's last block zeroes the padding [N, Np) of both stat rows
    p.stat[bh * 2 * p.Np + N + tid] = 0.f;
    p.stat[bh * 2 * p.Np + p.Np + N + tid] = 0.f;
  }

  // wave w moves key rows [16 w, 16 w + 16) of the K and of the V tile as two 1-KiB pieces each
  int dma_off[4], dma_row[2];
  uint64_t zpage = (uint64_t)(uintptr_t)g_bwd_zero_page;
  asm volatile("" : "+s"(zpage));
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = wave * 16 + i * 8 + (lane >> 3), pc = lane & 7;
    dma_row[i] = r;
    dma_off[i] = r * 3 * C + C + ((pc ^ bwd_swz(r)) & 7) * 8;
    dma_off[2 + i] = r * 3 * C + 2 * C + ((pc ^ bwd_swz(r)) & 7) * 8;
  }
  unsigned taddr[4];                                 // K^T transpose-read addresses per d tile (stage, 32-key half, 4-key half: immediates)
  const int trow = 4 * lg + (li >> 2);
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
    taddr[dt] = (unsigned)(uintptr_t)smem + (unsigned)(trow * 128 + (((2 * dt + ((li & 3) >> 1)) ^ bwd_swz(trow)) & 7) * 16 + (li & 1) * 8);
  const unsigned char* faddr[2];                     // row fragment (ds_read_b128) addresses per kh (key tile, stage, K / V: immediates)
#pragma unroll
  for (int kh = 0; kh < 2; ++kh) faddr[kh] = smem + li * 128 + (((kh * 4 + lg) ^ bwd_swz(li)) & 7) * 16;
  auto dma_issue = [&](unsigned char* st, int kv0) {
    const bf16_t* base = p.qkv + ((tok0 + kv0) * 3 * C + h * HD);
    unsigned char* dK = st + wave * 2048;
    unsigned char* dV = st + KTILE + wave * 2048;
    if (kv0 + 64 <= N) {
#pragma unroll
      for (int i = 0; i < 2; ++i) bwd_glds16(base + dma_off[i], dK + i * 1024);
#pragma unroll
      for (int i = 0; i < 2; ++i) bwd_glds16(base + dma_off[2 + i], dV + i * 1024);
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const bool ok = kv0 + dma_row[i] < N;
        bwd_glds16((const bf16_t*)(uintptr_t)(ok ? (uint64_t)(uintptr_t)(base + dma_off[i]) : zpage), dK + i * 1024);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const bool ok = kv0 + dma_row[i] < N;
        bwd_glds16((const bf16_t*)(uintptr_t)(ok ? (uint64_t)(uintptr_t)(base + dma_off[2 + i]) : zpage), dV + i * 1024);
      }
    }
  };

  f32x4 dq[2][4];
#pragma unroll
  for (int sub = 0; sub < 2; ++sub)
#pragma unroll
    for (int t = 0; t < 4; ++t) dq[sub][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const float sc2 = p.scale * LOG2E, inv_scale = 1.0f / p.scale;
  const bool add_raw = p.drawlog != nullptr && p.T > 0 && qb == 0 && wave == 0 && li < p.T;

  const int nkv = (N + 63) / 64;
  dma_issue(smem, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // RG: the key tile is ragged (1) / full (0); RW: the block's wave 0 adds drawlog (1) / nobody does (0)
  auto tile = [&](auto stage_tag, auto ragged_tag, auto raw_tag, int j) {
    constexpr int ST = decltype(stage_tag)::value;
    constexpr int RG = decltype(ragged_tag)::value, RW = decltype(raw_tag)::value;
    const bool more = RG != 1 && j + 1 < nkv;         // a ragged tile is the last one
    if (more) dma_issue(smem + (1 - ST) * STAGE, (j + 1) * 64);
    const int kv0 = j * 64;
    if (active) {
      constexpr bool full = RG == 0;
      const bool do_raw = RW != 0 && add_raw;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {                 // two 32-key halves: keeps the live score registers at 2 x [2][2] tiles
        if (RG != 0 && kv0 + 32 * ks >= N) continue;   // (block-uniform) nothing valid in this half of the last tile
        f32x4 s[2][2], dp[2][2];
        u32x2 ktl[4], kth[4];                          // K^T fragments of this half (transpose reads)
        u32x4 kf[2][2], vf[2][2];                      // every LDS read of the half in flight before the first MFMA
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
          for (int kh = 0; kh < 2; ++kh) {
            kf[k2][kh] = *(const u32x4*)(faddr[kh] + ST * STAGE + k2 * 2048 + (ks ? 4096 : 0));
            vf[k2][kh] = *(const u32x4*)(faddr[kh] + ST * STAGE + KTILE + k2 * 2048 + (ks ? 4096 : 0));
          }
        if (ks == 0) {
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) { ktl[dt] = bwd_ds_read_tr16<ST * STAGE>(taddr[dt]); kth[dt] = bwd_ds_read_tr16<ST * STAGE + 16 * 128>(taddr[dt]); }
        } else {
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) { ktl[dt] = bwd_ds_read_tr16<ST * STAGE + 32 * 128>(taddr[dt]); kth[dt] = bwd_ds_read_tr16<ST * STAGE + 48 * 128>(taddr[dt]); }
        }
        BWD_WAIT_TR8(ktl, kth);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
#pragma unroll
          for (int sub = 0; sub < 2; ++sub) { s[sub][k2] = (f32x4){0.f, 0.f, 0.f, 0.f}; dp[sub][k2] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
          for (int kh = 0; kh < 2; ++kh)
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
              s[sub][k2] = mfma16(kf[k2][kh], qf[sub][kh], s[sub][k2]);
              dp[sub][k2] = mfma16(vf[k2][kh], gf[sub][kh], dp[sub][k2]);
            }
        }
        __builtin_amdgcn_s_setprio(0);
        // s[sub][k2][r] = S[q = li][key = kv0 + 16 (2ks + k2) + 4 lg + r]
        u32x4 dsb[2];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
          float ds[2][4];
#pragma unroll
          for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float pv = __builtin_amdgcn_exp2f(fmaf(s[sub][k2][r], sc2, -lse2[sub]));
              ds[k2][r] = pv * (dp[sub][k2][r] - Dq[sub]);
            }
          if (!full) {
#pragma unroll
            for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
              for (int r = 0; r < 4; ++r)
                if (kv0 + (2 * ks + k2) * 16 + lg * 4 + r >= N) ds[k2][r] = 0.f;
          }
          if (sub == 0 && do_raw) {
            const float* rl = p.drawlog + (bh * p.T + li) * N;
#pragma unroll
            for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int key = kv0 + (2 * ks + k2) * 16 + lg * 4 + r;
                if (full || key < N) ds[k2][r] += rl[key] * inv_scale;
              }
          }
          dsb[sub] = (u32x4){pack2(ds[0][0], ds[0][1]), pack2(ds[0][2], ds[0][3]), pack2(ds[1][0], ds[1][1]), pack2(ds[1][2], ds[1][3])};
        }
        // dQ^T[d][q] += K^T[d][keys of this half] dS^T
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const u32x4 ka = (u32x4){ktl[dt][0], ktl[dt][1], kth[dt][0], kth[dt][1]};
          dq[0][dt] = mfma16(ka, dsb[0], dq[0][dt]);
          dq[1][dt] = mfma16(ka, dsb[1], dq[1][dt]);
        }
        __builtin_amdgcn_s_setprio(0);
      }
    }
    if (more) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  };
  // full tiles run the select-free body; the ragged last tile (if any) is peeled.  Blocks whose wave 0 adds drawlog (the prompt rows'
  // block of each head) run their own copy of the loop, so that every other block's body has no trace of the add
  const int nfull = N / 64;
  auto run = [&](auto raw_tag) {
    for (int j = 0; j < nfull; j += 2) {
      tile(BwdNo{}, BwdNo{}, raw_tag, j);
      if (j + 1 < nfull) tile(BwdYes{}, BwdNo{}, raw_tag, j + 1);
    }
    if (nfull < nkv) {
      if (nfull & 1) tile(BwdYes{}, BwdYes{}, raw_tag, nfull);
      else tile(BwdNo{}, BwdYes{}, raw_tag, nfull);
    }
  };
  if (p.drawlog != nullptr && p.T > 0 && qb == 0) run(BwdYes{});
  else run(BwdNo{});
  // dq[sub][dt][r] = dQ[q = li][d = 16 dt + 4 lg + r] / scale
#pragma unroll
  for (int sub = 0; sub < 2; ++sub) {
    const int qrow = q0 + sub * 16 + li;
    if (qrow >= N) continue;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
      *(u32x2*)(p.dqkv + (tok0 + qrow) * 3 * C + h * HD + dt * 16 + lg * 4) =
          (u32x2){pack2(dq[sub][dt][0] * p.scale, dq[sub][dt][1] * p.scale), pack2(dq[sub][dt][2] * p.scale, dq[sub][dt][3] * p.scale)};
  }
}

// --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void attn_bwd_dkv_kernel(const BwdP p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int STAGE = 2 * KTILE;                  // Q, dO
  const int nkb = (p.N + 127) / 128;
  const int wi = xcd_remap(blockIdx.x, gridDim.x);
  const int kb = wi % nkb, bh_ = wi / nkb;
  const int h = bh_ % p.nH, b = bh_ / p.nH;
  const int N = p.N, C = p.nH * HD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int64_t tok0 = (int64_t)b * N;
  const int64_t bh = (int64_t)b * p.nH + h;
  const int key0 = kb * 128 + wave * 32;
  const bool active = key0 < N;

  u32x4 kf[2][2], vf[2][2], dummy;
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    const int krow = key0 + kt * 16 + li;
    const bool ok = krow < N;
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      Raw8<false> r;
      load8_raw<false>(p.qkv, (tok0 + krow) * 3 * C + C + h * HD + kh * 32 + lg * 8, ok, r);
      cvt8<false, false>(ok, r, kf[kt][kh], dummy);
      load8_raw<false>(p.qkv, (tok0 + krow) * 3 * C + 2 * C + h * HD + kh * 32 + lg * 8, ok, r);
      cvt8<false, false>(ok, r, vf[kt][kh], dummy);
    }
  }

  // wave w moves query rows [16 w, 16 w + 16) of the Q and of the dO tile as two 1-KiB pieces each
  int dma_off[4], dma_row[2];
  uint64_t zpage = (uint64_t)(uintptr_t)g_bwd_zero_page;
  asm volatile("" : "+s"(zpage));
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = wave * 16 + i * 8 + (lane >> 3), pc = lane & 7;
    dma_row[i] = r;
    dma_off[i] = r * 3 * C + ((pc ^ bwd_swz(r)) & 7) * 8;
    dma_off[2 + i] = r * C + ((pc ^ bwd_swz(r)) & 7) * 8;
  }
  unsigned taddr[4];                                 // Q^T / dO^T transpose-read addresses per d tile
  const int trow = 4 * lg + (li >> 2);
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
    taddr[dt] = (unsigned)(uintptr_t)smem + (unsigned)(trow * 128 + (((2 * dt + ((li & 3) >> 1)) ^ bwd_swz(trow)) & 7) * 16 + (li & 1) * 8);
  const unsigned char* faddr[2];                     // row fragment addresses per kh
#pragma unroll
  for (int kh = 0; kh < 2; ++kh) faddr[kh] = smem + li * 128 + (((kh * 4 + lg) ^ bwd_swz(li)) & 7) * 16;
  const float* Drow = p.stat + bh * 2 * p.Np;
  const float* Lrow = Drow + p.Np;
  // the per-row statistics sit behind the two stages, per stage 64 D values then 64 lse*log2(e) values of the tile's query rows (wave 0 moves
  // the D piece, wave 1 the other); a lane reads the four rows 4 lg .. 4 lg + 3 of a 16-row sub-tile as one 16-byte LDS read
  constexpr int STAT_LDS = 2 * STAGE, STAT_STAGE = 2 * 64 * 4;
  const unsigned saddr = (unsigned)(uintptr_t)smem + (unsigned)(lg * 16);   // read by asm like the transposed fragments: see BWD_WAIT_TR8
  auto dma_issue = [&](unsigned char* st, unsigned char* sst, int q0) {
    if (__builtin_amdgcn_readfirstlane(wave) < 2) {
      const float* src = (wave ? Lrow : Drow) + q0 + lane;
      if (q0 + 64 > p.Np) src = q0 + lane < p.Np ? src : (const float*)(uintptr_t)zpage;   // rows past the zero padding of stat
      bwd_glds4(src, sst + wave * 256);
    }
    const bf16_t* baseQ = p.qkv + ((tok0 + q0) * 3 * C + h * HD);
    const bf16_t* baseG = p.dout + ((tok0 + q0) * C + h * HD);
    unsigned char* dQ = st + wave * 2048;
    unsigned char* dG = st + KTILE + wave * 2048;
    if (q0 + 64 <= N) {
#pragma unroll
      for (int i = 0; i < 2; ++i) bwd_glds16(baseQ + dma_off[i], dQ + i * 1024);
#pragma unroll
      for (int i = 0; i < 2; ++i) bwd_glds16(baseG + dma_off[2 + i], dG + i * 1024);
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const bool ok = q0 + dma_row[i] < N;
        bwd_glds16((const bf16_t*)(uintptr_t)(ok ? (uint64_t)(uintptr_t)(baseQ + dma_off[i]) : zpage), dQ + i * 1024);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const bool ok = q0 + dma_row[i] < N;
        bwd_glds16((const bf16_t*)(uintptr_t)(ok ? (uint64_t)(uintptr_t)(baseG + dma_off[2 + i]) : zpage), dG + i * 1024);
      }
    }
  };

  f32x4 dk[2][4], dv[2][4];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int t = 0; t < 4; ++t) { dk[kt][t] = (f32x4){0.f, 0.f, 0.f, 0.f}; dv[kt][t] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
  const float sc2 = p.scale * LOG2E, inv_scale = 1.0f / p.scale;

  const int nq = (N + 63) / 64;
  // DropPath skip: with the image's patch rows dead, the query tiles past the prompt rows' (a suffix of the loop) carry dO = 0 and add
  // nothing to dK / dV: only the trip count shrinks, to nlive tiles; the KIND of a tile still follows from the true N.  T == 0: no tile at all.
  int nlive = nq;
  if (bwd_patches_dead(p, b)) { const int np = (p.T + 63) / 64; nlive = np < nq ? np : nq; }
  if (nlive > 0) dma_issue(smem, smem + STAT_LDS, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // RG: the query tile is ragged (1) / full (0); FT: it is the first one, whose prompt rows take the drawlog add (1) / it is not (0)
  auto tile = [&](auto stage_tag, auto ragged_tag, auto first_tag, int j) {
    constexpr int ST = decltype(stage_tag)::value;
    constexpr int RG = decltype(ragged_tag)::value, FT = decltype(first_tag)::value;
    const bool more = RG != 1 && j + 1 < nlive;       // a ragged tile is the last one
    if (more) dma_issue(smem + (1 - ST) * STAGE, smem + STAT_LDS + (1 - ST) * STAT_STAGE, (j + 1) * 64);
    const int q0 = j * 64;
    if (active) {
      constexpr bool full = RG == 0;
      const bool add_raw = FT != 0 && p.drawlog != nullptr && p.T > 0;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {                 // two 32-query halves
        if (RG != 0 && q0 + 32 * ks >= N) continue;    // (block-uniform) nothing valid in this half of the last tile
        f32x4 s[2][2], dp[2][2];                       // [q sub of the half][key tile]
        f32x4 D4[2], L4[2];
        u32x2 qtl[4], qth[4], gtl[4], gth[4];          // Q^T / dO^T fragments of this half (transpose reads)
        // a peeled ragged tile (runs once per workgroup) carries row masks on top of everything else: its transposed fragments and stat
        // values are read after the S / dP MFMAs, when the row fragments are dead.  Every other tile has all LDS reads of the half in
        // flight before the first MFMA
        constexpr bool LATE = RG == 1;
        u32x4 qa[2][2], ga[2][2];
        auto read_stat = [&]() {
#pragma unroll
          for (int q2 = 0; q2 < 2; ++q2) {
            D4[q2] = bwd_ds_read_f4<STAT_LDS + ST * STAT_STAGE>(saddr + (ks ? 128 : 0) + q2 * 64);
            L4[q2] = bwd_ds_read_f4<STAT_LDS + ST * STAT_STAGE + 256>(saddr + (ks ? 128 : 0) + q2 * 64);
          }
        };
        auto read_tr = [&]() {
          if (ks == 0) {
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
              qtl[dt] = bwd_ds_read_tr16<ST * STAGE>(taddr[dt]); qth[dt] = bwd_ds_read_tr16<ST * STAGE + 16 * 128>(taddr[dt]);
              gtl[dt] = bwd_ds_read_tr16<ST * STAGE + KTILE>(taddr[dt]); gth[dt] = bwd_ds_read_tr16<ST * STAGE + KTILE + 16 * 128>(taddr[dt]);
            }
          } else {
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
              qtl[dt] = bwd_ds_read_tr16<ST * STAGE + 32 * 128>(taddr[dt]); qth[dt] = bwd_ds_read_tr16<ST * STAGE + 48 * 128>(taddr[dt]);
              gtl[dt] = bwd_ds_read_tr16<ST * STAGE + KTILE + 32 * 128>(taddr[dt]); gth[dt] = bwd_ds_read_tr16<ST * STAGE + KTILE + 48 * 128>(taddr[dt]);
            }
          }
        };
        auto wait_reads = [&]() { BWD_WAIT_TR16_F4(qtl, qth, gtl, gth, D4, L4); };
        if constexpr (!LATE) read_stat();
#pragma unroll
        for (int q2 = 0; q2 < 2; ++q2) {
#pragma unroll
          for (int kh = 0; kh < 2; ++kh) {
            qa[q2][kh] = *(const u32x4*)(faddr[kh] + ST * STAGE + q2 * 2048 + (ks ? 4096 : 0));
            ga[q2][kh] = *(const u32x4*)(faddr[kh] + ST * STAGE + KTILE + q2 * 2048 + (ks ? 4096 : 0));
          }
        }
        if constexpr (!LATE) { read_tr(); wait_reads(); }
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int q2 = 0; q2 < 2; ++q2) {
#pragma unroll
          for (int kt = 0; kt < 2; ++kt) { s[q2][kt] = (f32x4){0.f, 0.f, 0.f, 0.f}; dp[q2][kt] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
          for (int kh = 0; kh < 2; ++kh)
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
              s[q2][kt] = mfma16(qa[q2][kh], kf[kt][kh], s[q2][kt]);
              dp[q2][kt] = mfma16(ga[q2][kh], vf[kt][kh], dp[q2][kt]);
            }
        }
        __builtin_amdgcn_s_setprio(0);
        if constexpr (LATE) {
          read_stat();
          read_tr();
          wait_reads();
        }
        // s[q2][kt][r] = S[q = q0 + 16 (2ks + q2) + 4 lg + r][key = key0 + 16 kt + li]
        u32x4 pb[2], dsb[2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
          float pv[2][4], ds[2][4];
#pragma unroll
          for (int q2 = 0; q2 < 2; ++q2) {
            const float lr[4] = {L4[q2][0], L4[q2][1], L4[q2][2], L4[q2][3]};
            const float dr[4] = {D4[q2][0], D4[q2][1], D4[q2][2], D4[q2][3]};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              pv[q2][r] = __builtin_amdgcn_exp2f(fmaf(s[q2][kt][r], sc2, -lr[r]));
              if (!full && q0 + (2 * ks + q2) * 16 + lg * 4 + r >= N) pv[q2][r] = 0.f;
              ds[q2][r] = pv[q2][r] * (dp[q2][kt][r] - dr[r]);
            }
          }
          if (add_raw && ks == 0) {
            const int key = key0 + kt * 16 + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int q = lg * 4 + r;                  // query sub 0 of the first tile
              if (q < p.T && key < N) ds[0][r] += p.drawlog[(bh * p.T + q) * N + key] * inv_scale;
            }
          }
          pb[kt] = (u32x4){pack2(pv[0][0], pv[0][1]), pack2(pv[0][2], pv[0][3]), pack2(pv[1][0], pv[1][1]), pack2(pv[1][2], pv[1][3])};
          dsb[kt] = (u32x4){pack2(ds[0][0], ds[0][1]), pack2(ds[0][2], ds[0][3]), pack2(ds[1][0], ds[1][1]), pack2(ds[1][2], ds[1][3])};
        }
        // dV^T[d][key] += dO^T[d][q half] P ;  dK^T[d][key] += Q^T[d][q half] dS
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const u32x4 ga = (u32x4){gtl[dt][0], gtl[dt][1], gth[dt][0], gth[dt][1]};
          const u32x4 qa = (u32x4){qtl[dt][0], qtl[dt][1], qth[dt][0], qth[dt][1]};
#pragma unroll
          for (int kt = 0; kt < 2; ++kt) {
            dv[kt][dt] = mfma16(ga, pb[kt], dv[kt][dt]);
            dk[kt][dt] = mfma16(qa, dsb[kt], dk[kt][dt]);
          }
        }
        __builtin_amdgcn_s_setprio(0);
      }
    }
    if (more) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  };
  // the first tile (drawlog add on its prompt rows) and the ragged last tile are peeled; the tiles between run the body without selects
  const int nfull = N / 64;
  const int nlf = nfull < nlive ? nfull : nlive;       // live full tiles
  if (nlive >= 1) {
    if (nfull >= 1) tile(BwdNo{}, BwdNo{}, BwdYes{}, 0);
    else tile(BwdNo{}, BwdYes{}, BwdYes{}, 0);
  }
  for (int j = 1; j < nlf; j += 2) {
    tile(BwdYes{}, BwdNo{}, BwdNo{}, j);
    if (j + 1 < nlf) tile(BwdNo{}, BwdNo{}, BwdNo{}, j + 1);
  }
  if (nfull >= 1 && nfull < nq && nlive == nq) {
    if (nfull & 1) tile(BwdYes{}, BwdYes{}, BwdNo{}, nfull);
    else tile(BwdNo{}, BwdYes{}, BwdNo{}, nfull);
  }
  // dk[kt][dt][r] = dK[key = key0 + 16 kt + li][d = 16 dt + 4 lg + r] / scale
  int tid_e = tid;                                     // the store addresses are rebuilt from the thread index here, so that no row index or
  asm volatile("" : "+v"(tid_e));                      // offset computed for the prologue's loads stays in a register across the loop
  const int li_e = tid_e & 15, lg_e = (tid_e >> 4) & 3, key0_e = kb * 128 + (tid_e >> 6) * 32;
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    const int krow = key0_e + kt * 16 + li_e;
    if (krow >= N) continue;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      bf16_t* dst = p.dqkv + (tok0 + krow) * 3 * C + C + h * HD + dt * 16 + lg_e * 4;
      *(u32x2*)dst = (u32x2){pack2(dk[kt][dt][0] * p.scale, dk[kt][dt][1] * p.scale), pack2(dk[kt][dt][2] * p.scale, dk[kt][dt][3] * p.scale)};
      *(u32x2*)(dst + C) = (u32x2){pack2(dv[kt][dt][0], dv[kt][dt][1]), pack2(dv[kt][dt][2], dv[kt][dt][3])};
    }
  }
}

}  // namespace

extern "C" int mtt_attn_bwd(const mtt_attn_desc* d, const void* dout, const float* drawlog, void* dqkv, float* stat, void* stream) {
  if (!d || !d->qkv || !d->out || !d->lse || !dout || !dqkv || !stat) return MTT_E_BADARG;
  if (d->B <= 0 || d->N <= 0 || d->nH <= 0 || d->T < 0 || d->T > 16) return MTT_E_BADARG;
  if (d->dtype != MTT_BF16 || d->prec != MTT_PREC_BF16) return MTT_E_UNSUPPORTED;
  if (((uintptr_t)d->qkv | (uintptr_t)dout | (uintptr_t)d->out | (uintptr_t)stat | (uintptr_t)dqkv) & 15) return MTT_E_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  // two stages of two tiles; the dK/dV kernel adds D and lse*log2(e) of each stage's 64 query rows.  Both stay within the default 64 KiB
  // of dynamic LDS
  constexpr int smem_dq = 2 * 2 * KTILE, smem_dkv = smem_dq + 2 * 2 * 64 * 4;
  const int Np = (d->N + 3) & ~3;
  BwdP p{(const bf16_t*)d->qkv, (const bf16_t*)dout, stat, d->T > 0 ? drawlog : nullptr, (bf16_t*)dqkv, d->B, d->N, d->nH, d->T, Np, d->scale,
         (const bf16_t*)d->out, d->lse, d->skip_scale};
  dim3 grid((unsigned)(((d->N + 127) / 128) * d->nH * d->B));
  hipLaunchKernelGGL(attn_bwd_dq_kernel, grid, dim3(256), smem_dq, s, p);    // writes stat, ahead of the dK/dV launch on the same stream
  hipLaunchKernelGGL(attn_bwd_dkv_kernel, grid, dim3(256), smem_dkv, s, p);
  return (int)hipGetLastError();
}
