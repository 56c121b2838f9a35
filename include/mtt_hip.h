/*
 * mtt_hip.h — C ABI of libmtt_hip.so: the MI355X (gfx950) kernels behind the TaskPrompter / InvPT
 * hot path.  This is the drop-in boundary BELOW the Python nn.Module mirror of the reference
 * (SURVEY.md §8b).  Plain pointers and sizes only — no torch types.
 *
 * Conventions (all entry points):
 *   - return 0 on success, <0 = MTT_E_* argument error, >0 = hipError_t from the launch
 *   - asynchronous on the caller's stream; no allocation, no synchronisation (safe under hipGraph capture); every buffer,
 *     including kernel workspaces, is owned by the caller.  No floating-point atomics: every cross-workgroup reduction writes
 *     per-workgroup partials to a caller-owned workspace and sums them in a fixed order, so results are run-to-run reproducible.  No environment variables and no process-global switches: which
 *     kernel runs is a pure function of the descriptor.  The only process state is a per-device "already configured" bit per
 *     kernel for the one-time hipFuncSetAttribute(MaxDynamicSharedMemorySize) opt-in (idempotent, thread-safe)
 *   - reduction-contiguous GEMM operands (MTT_OP_K) are read in 8-element chunks: when K is not a multiple
 *     of 8 the elements K..pad8(K)-1 of every row must exist and be zero (ld >= pad8(K))
 *   - activations are token-major / NHWC: a feature map is a row-major [rows = B*H*W, channels]
 *     matrix with a leading dimension (ld, in elements) that is a multiple of 8; 16-byte aligned
 *   - dtype codes: MTT_F32 = 0, MTT_BF16 = 1, MTT_SPLIT = 2 (hi / lo bf16 planes, see below)
 *   - prec: MTT_PREC_BF16 = 0 (bf16 MFMA, fp32 accumulate — the throughput path; fp32 operands are rounded while staged)
 *           MTT_PREC_X3   = 1 (operands split hi+lo bf16, 3 MFMAs — fp32-class accuracy, the
 *                              1e-3 parity gate; operands MTT_F32 (split while staged) or both MTT_SPLIT (pre-split planes
 *                              streamed by LDS-DMA))
 *
 * Each entry names the reference code it replaces (paths relative to /root/reference).
 */
#ifndef MTT_HIP_H
#define MTT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTT_ABI_VERSION 17

/* MTT_SPLIT: an fp32-class value stored as TWO bf16 planes of identical layout, x = hi + lo with hi = bf16(x), lo = bf16(x - hi)
 * (~16 mantissa bits).  The main pointer of an operand addresses the hi plane, its `*_lo` companion the lo plane.  The hi plane alone is
 * an ordinary bf16 tensor — which is what lets a training step run its forward in fp32-class arithmetic (3 MFMAs per product on the
 * LDS-DMA kernel, MTT_PREC_X3) and its backward in bf16 on the very same buffers. */
enum { MTT_F32 = 0, MTT_BF16 = 1, MTT_SPLIT = 2 };
enum { MTT_PREC_BF16 = 0, MTT_PREC_X3 = 1 };
enum { MTT_E_BADARG = -1, MTT_E_ALIGN = -2, MTT_E_UNSUPPORTED = -3 };

/* operand layouts of mtt_gemm */
enum {
  MTT_OP_K = 0,     /* element(r,k) at base + r*ld + k   (reduction index contiguous)            */
  MTT_OP_R = 1,     /* element(r,k) at base + k*ld + r   (row index contiguous; transposed view) */
  MTT_OP_CONV_K = 2,/* A only: implicit im2col, r = output pixel, k = (tap, ci)                   */
  MTT_OP_CONV_R = 3 /* B only: implicit im2col^T, k = pixel (reduction), r = (tap, ci)            */
};
enum { MTT_ACT_NONE = 0, MTT_ACT_GELU = 1, MTT_ACT_RELU = 2, MTT_ACT_GELU_BWD = 3, MTT_ACT_RELU_BWD = 4,
       /* ABI 10 — the GELU of a bf16-arithmetic backward with its derivative taken in the FORWARD: the fc1 epilogue has z in registers and
        * stores GELU'(z) (instead of z) next to GELU(z); the fc2 input-gradient epilogue is then one multiply per element instead of an
        * erf + exp evaluation (that epilogue ran ~25 VALU instructions per element against a 16-step K loop).  Same bytes, same bf16
        * storage rounding class: GELU' in [-0.13, 1.13] rounded to bf16 vs GELU'(bf16(z)). */
       MTT_ACT_GELU_DAUX = 5 /* D = GELU(z), aux_out = GELU'(z)   (aux_out required) */,
       MTT_ACT_MUL_AUX = 6   /* D = epi(acc) * aux_in              (aux_in required) */ };
enum { MTT_STORE_ROWS = 0, MTT_STORE_PIXSHUF2 = 1 };
/* kernel selection of mtt_gemm / mtt_attn_fwd: AUTO = the library's policy (a pure function of the descriptor); the other values
 * force one kernel where it is applicable (tests of a kernel on small shapes, A/B measurements).  There is no process-global switch and
 * no environment variable: the library keeps no mutable state that affects results. */
enum { MTT_GEMM_AUTO = 0,
       MTT_GEMM_GENERAL = 1           /* the register-staged 128 x 128 kernel (any layout / dtype / precision) */,
       MTT_GEMM_DMA256 = 3            /* the 256 x 256 LDS-DMA kernel (or, for two MTT_OP_R operands, the token-major weight-gradient kernel) on any shape it supports */,
       MTT_GEMM_DMA128 = 4            /* the 128 x 128 LDS-DMA kernel (K-contiguous bf16 operands; narrow or mid-size outputs) */,
       MTT_GEMM_GENERAL_EPILOGUE = 11 /* policy kernel, but always the general (run-time configured) epilogue: A/B of the specialised one */ };
/* mtt_attn_desc.variant: PLAIN forces the straightforward forward kernel; every other value takes the policy's kernel (the flash kernel
 * for bf16 storage).  Values 2 and 3 once named two register-staged generations of the flash kernels (A/B only); they were removed
 * without a change to the descriptor layout, the entry points or MTT_ABI_VERSION, and now mean what every unnamed value means. */
enum { MTT_ATTN_AUTO = 0, MTT_ATTN_PLAIN = 1 };

/* 3x3 (dilated) "same" convolution geometry for MTT_OP_CONV_* operands; stride 1, pad = dil. */
typedef struct {
  int32_t H, W;     /* feature-map height/width (rows = B*H*W)                       */
  int32_t C;        /* valid input channels                                           */
  int32_t Cp;       /* channel pitch of the K ordering k = tap*Cp + ci (multiple of 8)*/
  int32_t dil;      /* dilation (1, or 2 for InvPT UpEmbed, invpt.py:33)              */
  int32_t flip;     /* 1: taps visited mirrored (dgrad)                               */
} mtt_conv_geom;

/*
 * D[z][m,n] = epilogue( alpha * sum_k A[z][m,k] * B[z][n,k] )      m<M, n<N, k<K, z<batch
 *
 * Replaces every nn.Linear / 1x1 nn.Conv2d / 3x3 nn.Conv2d / nn.ConvTranspose2d(k=s=2) matmul of
 * the hot path and their dgrad/wgrad (taskprompter.py:175-187,201,212,219,250 Linear; :362-366
 * fea_fuse / fea_decode convs; :692-709 heads; timm Mlp fc1/fc2; invpt.py:108-113; vit.py:179-181;
 * transformer_decoder.py:56-67,110).  Rows of A, D, aux and resid are addressed in groups:
 *   row m -> base + (m / mb) * bs + (m % mb) * ld          (mb = 0 means one group)
 * so a GEMM can read/write a token subset of a [B, N, C] buffer in place.
 * Batch index z = zo*batch_inner + zi adds zo*?_zo + zi*?_zi elements to each base.
 *
 * epilogue, in order:  v = alpha*acc;  v = v*colscale[n] + colshift[n];
 *   act: GELU(erf) / ReLU / GELU_BWD: v *= gelu'(aux_in[m,n]) / RELU_BWD: v *= (aux_in[m,n] > 0)
 *   aux_out[m,n] = pre-activation value (optional, training)
 *   v *= rowscale[(m / d_mb)*2 + ((m % d_mb) >= n_prompt)]   (DropPath per-sample scale, optional)
 *   v += resid[m,n] (fp32, own row mapping; may alias D)
 *   store D (dtype d_dtype; MTT_SPLIT: hi plane at D, lo plane at D_lo); columns N <= n < n_store are written as zeros (channel padding).
 * Operand dtypes: MTT_PREC_BF16 takes bf16 or fp32 operands in any mix (fp32 is rounded to bf16 while staged); MTT_PREC_X3 takes
 * fp32 operands (general kernel) or A and B both MTT_SPLIT with a_op = b_op = MTT_OP_K, K % 64 == 0 (LDS-DMA kernel).
 */
typedef struct {
  const void* A; const void* B; void* D;
  int32_t M, N, K;
  int32_t a_op, b_op;            /* MTT_OP_* */
  int32_t a_dtype, b_dtype, d_dtype;
  int32_t prec;
  int64_t lda, ldb, ldd;
  int32_t a_mb; int64_t a_bs;
  int32_t d_mb; int64_t d_bs;
  int32_t batch, batch_inner;    /* batch >= 1; batch_inner >= 1 */
  int64_t a_zo, a_zi, b_zo, b_zi, d_zo, d_zi;
  mtt_conv_geom conv;            /* used when a_op/b_op is MTT_OP_CONV_* */
  float alpha;
  const float* colscale; const float* colshift; int64_t col_zo, col_zi;   /* [N] per batch */
  int32_t act;
  const void* aux_in; void* aux_out; int32_t aux_dtype; int64_t ldaux; int64_t aux_zo, aux_zi; /* rows mapped like D */
  const float* rowscale; int32_t n_prompt;
  const float* resid; int64_t ldr; int32_t r_mb; int64_t r_bs; int64_t r_zo, r_zi;
  int32_t n_store;               /* >= N, <= ldd; 0 means N */
  int32_t store_mode;            /* MTT_STORE_PIXSHUF2: n = (dy*2+dx)*Co + co, D is [B,2H,2W,ldd] (ConvTranspose2d k=s=2, taskprompter.py:705) */
  int32_t ps_H, ps_W, ps_Co;
  int32_t variant;               /* MTT_GEMM_* (0 = AUTO) */
  const void* A_lo; const void* B_lo; void* D_lo;   /* lo planes of MTT_SPLIT operands / output (same layout, strides and batch offsets as the hi plane) */
  float* colsum_out; float* colsum_ws;   /* optional: colsum_out[n] = sum_m D[m,n] of the values AS STORED (bf16 D: the rounded values), n < N
                                            — the bias gradient when D is the gradient of a Linear's output (the fc2 input gradient with its
                                            GELU' epilogue IS fc1's output gradient), taken in the epilogue instead of re-reading D.  Per
                                            row-block partials go to colsum_ws (>= mtt_gemm_colsum_ws_floats(d) floats) and are summed in
                                            block order (deterministic).  batch == 1, MTT_STORE_ROWS only. */
  /* ABI 10 — A-operand PROLOGUE of the exact-fp32 tall GEMM (the kernel behind variant 11: fp32 operands, N <= 32 outputs, batch == 1):
   * the A element of channel k enters the product as act_a(A[m, k] * a_scale[k] + a_shift[k]) — BatchNorm (batch statistics folded into a
   * per-channel scale / shift, K floats each; padding channels: scale = shift = 0) + activation applied while the operand is loaded, so the
   * normalised + activated map of a conv head (8.7 GB in fp32 at the benchmark's batch) is never written in fp32 nor re-read: ConvHead's
   * BatchNorm + GELU + 1x1 prediction (taskprompter.py:692-694) is ONE pass over the conv output.  a_aux16 (optional): the transformed
   * operand rounded to bf16, [M, ld_a16] — what the bf16 backward of that layer reads (weight gradient of the predictions).
   * a_scale == NULL: no prologue.  Other kernels return MTT_E_UNSUPPORTED when it is set. */
  const float* a_scale; const float* a_shift; int32_t a_act; void* a_aux16; int64_t ld_a16;
  /* DropPath work skipping (optional; NULL = off, every kernel then behaves bit for bit as without these fields).  skip_scale is the [B, 2]
   * DropPath table of the branch (the `rowscale` layout): table row r belongs to sample q = r / skip_mb and class c = (r % skip_mb) >=
   * skip_prompt, and is DEAD iff skip_scale[2 q + c] == 0.0f.  The caller promises that dead rows only ever contribute exact zeros.
   *   - gemm_ring3_kernel<false> / gemm_dma_kernel<1> (a_op = b_op = MTT_OP_K): table row = A row m.  A 256-row tile whose rows are all dead
   *     skips its K loop and runs the unchanged epilogue on zero accumulators: it stores exactly what the call without skip_scale stores when
   *     the dead rows of A (both planes) are zero — bias, activation, aux_out, rowscale, resid and the colsum partials included.
   *   - skip_row0: for a_op = b_op = MTT_OP_R calls (weight gradients) reduction index k of batch member z is table row skip_row0 + z * K + k.
   *     No kernel skips reduction steps yet (gemm_tn_kernel ignores the table: finding the kept steps cost its K loop more than the dead
   *     steps saved); the field fixes the meaning for one that does.
   * Other kernels ignore the fields. */
  const float* skip_scale; int32_t skip_mb; int32_t skip_prompt; int64_t skip_row0;
} mtt_gemm_desc;
size_t mtt_gemm_colsum_ws_floats(const mtt_gemm_desc* d);

int mtt_abi_version(void);
/* sizeof(descriptor): 0 gemm, 1 attn, 2 softmax, 3 ln, 4 chanlogit, 5 modulate, 6 ctr, 7 resize, 8 bn, 9 conv_geom, (15 adam, 16 loss, 17 upconv, 18 gather, 19 winattn, 20 chanattn, 21 conv3s2)
 * 10 dwconv, 11 pool, 12 lnmt, 13 attnmsg, 14 convt, 17 upconv, 22 segcopy, 23 ctrw, 24 detloss (ABI 14's: mtt_det_desc_size) */
size_t mtt_desc_size(int which);
int mtt_gemm(const mtt_gemm_desc* d, void* stream);
/* which kernel mtt_gemm dispatches this descriptor to: 0 register-staged 128x128 (general), 3 phased LDS-DMA 256x256
 * (gemm_dma_kernel), 6 token-major weight-gradient kernel (gemm_tn_kernel: both operands MTT_OP_R, LDS-DMA + LDS transpose reads),
 * 8 gemm_dma_kernel on MTT_SPLIT operands (K-concatenated x3 product) */
int mtt_gemm_variant(const mtt_gemm_desc* d);

/*
 * Fused global attention over [T prompts || hw patches] with the prompt-row logit side channel.
 * Replaces Attention.forward's spatial part, taskprompter.py:201-210 (and vit.py:184-191 with T=0):
 *   qkv   [B, N, 3, nH, 64]  (dtype act)   ->   out [B, N, nH*64] = softmax(q k^T / 8) v
 *   rawlog[B, nH, T, N] fp32 = UNSCALED q.k of the first T query rows (what cal_task_feature reads,
 *   taskprompter.py:436-438,482); never materialises the N x N matrix.  head_dim is fixed at 64.
 */
typedef struct {
  const void* qkv; void* out; float* rawlog; float* lse;   /* lse [B,nH,N] fp32 (optional, for backward) */
  int32_t B, N, nH, T;
  int32_t dtype, prec;
  float scale;
  int32_t variant;   /* MTT_ATTN_* (0 = AUTO: the swapped-product flash kernel for bf16 storage, the plain kernel otherwise) */
  const void* qkv_lo; void* out_lo;   /* dtype == MTT_SPLIT (forward, MTT_PREC_X3): lo planes of qkv / out, same layout as the hi planes */
  /* DropPath work skipping (optional, NULL = off): the branch's [B, 2] table as in mtt_gemm_desc with mb = N, n_prompt = T.  When
   * skip_scale[2 b + 1] == 0 the patch rows of image b are dead: the caller promises dout == 0 there and reads neither out nor lse there.
   *   forward (attn_fwd_x3_kernel, attn_fwd_fast_kernel): a 128-row query block with qb * 128 >= T of such an image stores zeros to out
   *     (both planes) and 0 to lse and stages nothing; block 0 (prompt rows, rawlog) always runs.
   *   backward (attn_bwd_dq_kernel, attn_bwd_dkv_kernel): the same 128-row blocks store zero dq rows; the dK/dV kernel stops after its first ceil(T / 64) 64-row query
   *     tiles — a superset of the forward's dead rows, so every tile it processes has a forward-written out and lse.  Both store what the
   *     unskipped kernels store for dout == 0 there.  stat entries of skipped rows stay unwritten. */
  const float* skip_scale;
} mtt_attn_desc;
int mtt_attn_fwd(const mtt_attn_desc* d, void* stream);
/* Flash backward of mtt_attn_fwd (autograd of taskprompter.py:201-210 / vit.py:184-191), bf16 storage + MTT_PREC_BF16 only
 * (the x3 parity mode uses the materialised batched-GEMM backward).  Inputs: d->qkv, d->out (forward output), d->lse (forward
 * log-sum-exp), dout [B*N, nH*64] bf16, drawlog fp32 [B,nH,T,N] = gradient of the rawlog side channel (NULL if T == 0).
 * Outputs: dqkv [B*N, 3*nH*64] bf16 (every row written); stat fp32 [B,nH,2,pad4(N)] scratch (row 0: rowsum(dO*O), row 1:
 * lse*log2(e); pads zero).  No N x N tensor, no atomics. */
int mtt_attn_bwd(const mtt_attn_desc* d, const void* dout, const float* drawlog, void* dqkv, float* stat, void* stream);

/* Row softmax (+ its backward) on a materialised score matrix: used by the InvPT decoder attention
 * (invpt.py:232) and by the round-1 attention backward.  rows x cols, ld in elements.
 *   fwd : P = softmax(scale * S)                         S fp32/bf16 -> P (dtype)
 *   bwd : dS = scale * P * (dP - rowsum(dP*P)) (+ extra[r,c] for r < extra_rows, unscaled)  */
typedef struct {
  const void* S; void* P; const void* dP; void* dS; const float* extra;
  int64_t rows, cols, ld; int32_t s_dtype, p_dtype; float scale;
  int64_t rows_per_mat; int32_t extra_rows; int64_t extra_ld;
} mtt_softmax_desc;
int mtt_softmax_fwd(const mtt_softmax_desc* d, void* stream);
int mtt_softmax_bwd(const mtt_softmax_desc* d, void* stream);

/* LayerNorm over the last dim C (eps 1e-6 ViT: taskprompter.py:310; 1e-5 InvPT: invpt.py:256).
 * x fp32 [rows, C] (ldx) -> y (y_dtype) [rows, C] (ldy); mean/rstd [rows] fp32 saved for backward.
 * bwd: dx (fp32) = dx_in + dLN/dx   (dx_in: same layout as dx, e.g. the residual-stream gradient the LayerNorm branch joins;
 *      NULL = accumulate in place, dx += ...); dgamma / dbeta = the column sums of dy * xhat / dy (overwritten), reduced
 *      deterministically through the caller-owned workspace ws (>= mtt_layernorm_bwd_ws_floats(rows, C) floats; required with dgamma). */
typedef struct {
  const float* x; void* y; const float* gamma; const float* beta; float* mean; float* rstd;
  const void* dy; float* dx; float* dgamma; float* dbeta;
  int64_t rows; int32_t C; int64_t ldx, ldy; int32_t y_dtype; float eps;
  const float* dx_in;
  float* ws;
  void* y_lo;                    /* fwd, y_dtype == MTT_SPLIT: lo plane of y (same pitch ldy) */
  float* y32; int64_t ldy32;     /* fwd, optional: an additional fp32 copy of y (consumers that want the exact rows next to the split planes) */
} mtt_ln_desc;
size_t mtt_layernorm_bwd_ws_floats(int64_t rows, int32_t C);
int mtt_layernorm_fwd(const mtt_ln_desc* d, void* stream);
int mtt_layernorm_bwd(const mtt_ln_desc* d, void* stream);

/* Patchify for the k=s=16 patch-embed conv (timm PatchEmbed used at taskprompter.py:313,393):
 * img fp32 NCHW [B,3,H,W] -> cols [B*h*w, 768] (k = (c, py, px)), dtype out_dtype. */
int mtt_patchify16(const float* img, void* cols, int B, int H, int W, int out_dtype, void* stream);

/* Channel-attention logits, taskprompter.py:217-246:  rawchan[b,t,win,c] = sum_{p in win} q[b,t,p] * xn[b,p,c]
 * q [B,T,hw] (dtype), xn = norm1-ed tokens [B, N, C] (dtype; patch rows start at row T), rawchan fp32 [B,T,nwin,C]. */
typedef struct {
  const void* q; const void* xn; float* rawchan;
  int32_t B, T, N, C, h, w, nh, nw; int32_t dtype; int64_t ldq;
  float* ws;                     /* forward: workspace of mtt_chan_logits_ws_floats(d) floats (may be NULL when that is 0) */
  const void* xn_lo;             /* ABI 9, forward only: dtype == MTT_SPLIT reads the normalised tokens as hi (xn) + lo (xn_lo) bf16 planes — the
                                    LayerNorm output the split-plane GEMMs stream, so no fp32 copy of it is written for this kernel; q is then fp32 */
} mtt_chanlogit_desc;
/* rawchan is WRITTEN.  Reductions over the pixels of a window that are split across workgroups go through per-split partials in the
 * caller-owned workspace and are summed in split order (deterministic; no atomics — as every reduction of this library since ABI 6). */
size_t mtt_chan_logits_ws_floats(const mtt_chanlogit_desc* d);
int mtt_chan_logits(const mtt_chanlogit_desc* d, void* stream);
/* backward: dq[b,t,p] = sum_c drawchan*xn (written, dq_dtype, pitch ldq); dxn[b,T+p,c] += sum_t drawchan*q (fp32 [B,N,C]). */
int mtt_chan_logits_bwd(const mtt_chanlogit_desc* d, const float* drawchan, void* dq, int dq_dtype, float* dxn, void* stream);

/* Task-feature modulation, taskprompter.py:436-467: from x fp32 [B, hw, C] (row pitch/batch stride given)
 *   out[2t  ][b,p,c] = x[b,p,c] * (1 + rawlog[b, c/hg, t, T+p])          (rawlog fp32 [B, C/hg, T, N])
 *   out[2t+1][b,p,c] = x[b,p,c] * (1 + rawchan[b, t, win(p), c])            out dtype act (or MTT_SPLIT: two bf16 planes), [2T, B*hw, C] */
typedef struct {
  const float* x; int64_t x_ld, x_bs; const float* rawlog; const float* rawchan; void* out;
  int32_t B, T, N, C, h, w, nh, nw; int32_t out_dtype;
  int32_t hg;                    /* channels per attention head (a multiple of 8; 0 = 64, the ViT variants; 32 in the last Swin stage) */
  void* out_lo;                  /* ABI 8: out_dtype == MTT_SPLIT writes hi = bf16(v) at out and lo = bf16(v - hi) here (same layout): the
                                    fea_decode GEMMs of the fp32-class forward then stream pre-split planes (gemm_ring3_kernel) */
} mtt_modulate_desc;
int mtt_modulate(const mtt_modulate_desc* d, void* stream);
/* backward: dout [2T, B*hw, C] (d->out_dtype) -> dx = (fp32, same addressing as x; WRITTEN), drawlog[b,head,t,T+p] = (fp32 [B,nH,T,N],
 * caller zeroes the first T columns), drawchan = (fp32 [B,T,nwin,C], WRITTEN: per-split partials in ws, mtt_modulate_bwd_ws_floats(d)
 * floats, summed in split order). */
size_t mtt_modulate_bwd_ws_floats(const mtt_modulate_desc* d);
int mtt_modulate_bwd(const mtt_modulate_desc* d, const void* dout, float* dx, float* drawlog, float* drawchan, float* ws, void* stream);

/* Cross-task reweighting, taskprompter.py:478-485: w[b,t,s] from the per-head MLP on the prompt<->prompt
 * logits, then out[t][b,p,:] = sum_s w[b,t,s] * fea[s][b,p,:] (+= into acc when accumulate=1). */
typedef struct {
  const void* fea; void* out; const float* wmix;   /* fea [T, rows, ld]; wmix [B,T,T] fp32; out [T, rows, ld] (fp32 unless out_dtype says bf16) */
  int32_t T, B; int64_t rows_per_b, ld; int32_t C; int32_t fea_dtype; int32_t accumulate;
  int32_t out_dtype;             /* MTT_F32 (0, default) or MTT_BF16 (mtt_ctr_mix without accumulate only: the backward's gradient of bf16 features) */
} mtt_ctr_desc;
int mtt_ctr_mix(const mtt_ctr_desc* d, void* stream);
/* dwmix[b,t,s] = sum_{rows of b, c} dout[t][row,c] * fea[s][row,c]   (dout fp32 [T, rows, ld]; dwmix WRITTEN; ws: mtt_ctr_dw_ws_floats(d)
 * floats of per-workgroup partials, summed in workgroup order) */
size_t mtt_ctr_dw_ws_floats(const mtt_ctr_desc* d);
int mtt_ctr_dw(const mtt_ctr_desc* d, const float* dout, float* dwmix, float* ws, void* stream);

/* Cross-task reweighting WEIGHTS (taskprompter.py:482-484; modules defined at :364 `ctr_attn_conv`): for every image b and task pair
 * (t, s) the nH prompt<->prompt raw logits z[h] = rawlog[b, h, t, s] (the first T columns of the prompt rows' logits) go through task t's
 * 1x1-conv MLP over the head dimension:   wmix[b, t, s] = b2[t] + sum_j w2[t, j] * gelu(b0[t, j] + sum_h w0[t, j, h] * z[h])   (exact-erf GELU).
 * rawlog fp32 [B, nH, T, N] (row pitch N >= T); w0 [T, nH, nH], b0 [T, nH], w2 [T, nH], b2 [T] fp32 contiguous (ops.stack_vec packs);
 * wmix fp32 [B, T, T] written.  nH <= 32.
 * bwd: given dwmix [B, T, T]: drawlog[b, h, t, s] for s < T is WRITTEN (the other columns of drawlog are not touched: the caller zeroes
 * them), dw0 / db0 / dw2 / db2 are WRITTEN; the sums over (b, s) run inside one workgroup per (t, j) in a fixed order (deterministic,
 * no atomics, no workspace). */
typedef struct {
  const float* rawlog; const float* w0; const float* b0; const float* w2; const float* b2; float* wmix;
  int32_t B, T, nH; int64_t N;
} mtt_ctrw_desc;
int mtt_ctr_weights(const mtt_ctrw_desc* d, void* stream);
int mtt_ctr_weights_bwd(const mtt_ctrw_desc* d, const float* dwmix, float* drawlog, float* dw0, float* db0, float* dw2, float* db2, void* stream);

/* Losses of the 3-D detection branch (TaskPrompter/detection_toolbox/det_losses.py): element-wise loss on [N, C] with the
 * reference's weighting (weight_reduce_loss, :28-54) and a deterministic sum.
 *   kind 0  sigmoid focal loss (:226-345; mmcv-full 1.6.2 `sigmoid_focal_loss` on the device, py_sigmoid_focal_loss on the host, :183-224):
 *           target = int64 labels [N] in [0, C], C = background (no positive class);  p = sigmoid(x);
 *           loss[n, c] = -alpha (1 - p)^gamma log p            if c == target[n]
 *                        -(1 - alpha) p^gamma log(1 - p)        otherwise
 *   kind 1  smooth L1 (:102-123): target fp32 [N, C];  d = |x - y|;  loss = 0.5 d^2 / beta if d < beta else d - 0.5 beta
 * weight: NULL, [N] per sample (wmode 1) or [N, C] per element (wmode 2).  fwd: out[n, c] = w * loss (skipped when NULL), sum[0] = the sum of
 * out over all elements (skipped when NULL; ws: mtt_detloss_ws_floats(d) floats of per-workgroup partials summed in workgroup order).
 * bwd: dpred[n, c] = w * d loss / d x * (gelem ? gelem[n, c] : gscale[0]) * scale   (gelem: the upstream gradient of reduction 'none';
 * gscale: the upstream scalar of 'mean' / 'sum', read on the device; scale = loss_weight / avg_factor etc., a host constant). */
typedef struct {
  const float* pred; const void* target; const float* weight; float* out; float* sum; float* ws;
  int64_t N; int32_t C; int32_t kind; int32_t wmode; float gamma, alpha, beta;
} mtt_detloss_desc;
size_t mtt_detloss_ws_floats(const mtt_detloss_desc* d);
int mtt_detloss_fwd(const mtt_detloss_desc* d, void* stream);
int mtt_detloss_bwd(const mtt_detloss_desc* d, const float* gscale, const float* gelem, float scale, float* dpred, void* stream);

/* Bilinear resize, align_corners=False (F.interpolate at taskprompter.py:420, taskprompter_wrapper.py:36,
 * invpt.py:221,303,537, transformer_net.py:35-36).  NHWC in -> NHWC out or NCHW fp32 out.
 * bwd: din (fp32) += scatter of dout (atomics). */
typedef struct {
  const void* in; void* out; int32_t B, C, Hin, Win, Hout, Wout; int64_t ld_in, ld_out;
  int32_t in_dtype, out_dtype; int32_t out_nchw; int32_t accumulate;
} mtt_resize_desc;
int mtt_bilinear_fwd(const mtt_resize_desc* d, void* stream);
int mtt_bilinear_bwd(const mtt_resize_desc* d, void* stream);   /* in = dout, out = din (fp32) */

/* BatchNorm2d (+GELU/ReLU) on Z stacked NHWC maps [Z][rows, ld] (one BatchNorm per map; Z <= 1 = a single map), training mode
 * (batch statistics; nn.BatchNorm2d at taskprompter.py:362,692,705; SyncBatchNorm invpt.py:14).  Map z starts x_zs elements after
 * map z-1; its per-channel vectors (mean, rstd, gamma, beta, outputs) start p_zs floats after the previous map's.
 *   stats     : mean_out[z][c] = batch mean, m2_out[z][c] = sum_r (x - mean)^2 (centred; biased variance = m2 / rows).  Two-level
 *               deterministic reduction through the caller's workspace `ws` (mtt_bn_reduce_ws_floats(rows, C, Z) floats); no atomics,
 *               nothing to zero.  (mean, m2, rows) triplets of several ranks merge exactly (SyncBatchNorm) with Chan's update.
 *   apply     : y = act((x-mean)*rstd*gamma+beta), channels C..ld-1 written as zeros.
 *   bwd_reduce: dsum[z][c] = sum_r du, dsumxh[z][c] = sum_r du*xhat with du = dy*act'(u)   (same workspace, written not accumulated)
 *   bwd_apply : dx = gamma*rstd*(du - dsum/rows - xhat*dsumxh/rows)   (multi-rank: pass the all-reduced sums scaled by rows/rows_total) */
typedef struct {
  const void* x; void* y; const void* dy; void* dx;
  float* mean_out; float* m2_out; const float* mean; const float* rstd; const float* gamma; const float* beta;
  float* dsum; float* dsumxh;
  int64_t rows; int32_t C; int64_t ld; int32_t dtype; int32_t act;
  int32_t Z; int64_t x_zs; int64_t p_zs;
  int32_t g_dtype;   /* ABI 9, bwd_reduce / bwd_apply: storage of dy and dx = MTT_* dtype code + 1 (same pitch and map stride in ELEMENTS as
                      * x); 0 = the dtype of x.  Lets a bf16-arithmetic backward keep its gradient maps in bf16 next to an fp32-stored x */
} mtt_bn_desc;
size_t mtt_bn_reduce_ws_floats(int64_t rows, int32_t C, int32_t Z);
int mtt_bn_stats(const mtt_bn_desc* d, float* ws, void* stream);
int mtt_bn_apply(const mtt_bn_desc* d, void* stream);
int mtt_bn_bwd_reduce(const mtt_bn_desc* d, float* ws, void* stream);
int mtt_bn_bwd_apply(const mtt_bn_desc* d, void* stream);

/* fp32 [rows, cols] (pitch lds) -> MTT_SPLIT planes hi / lo [rows, ldd] (bf16; columns cols..ldd-1 zero): hi = bf16(x), lo = bf16(x - hi) */
int mtt_split_cast(const float* src, void* hi, void* lo, int64_t rows, int64_t cols, int64_t lds, int64_t ldd, void* stream);

/* Multi-segment strided copy / cast: ONE launch re-packs every weight of a model (the reference re-reads nn.Parameter tensors directly;
 * the packs are this implementation's operand layouts: [N, pad8(K)] casts, tap-major conv matrices, padded concatenations, hi/lo planes)
 * and scatters packed weight gradients back to parameter layout.  Segment g copies the logical box [n0][n1][n2] (n2 innermost):
 *     dst[i0*d0 + i1*d1 + i2*d2] = cast(src[i0*s0 + i1*s1 + i2*s2])
 * `table` is a DEVICE array of n_seg rows of MTT_SEG_WORDS int64 words:
 *     0 src address, 1 dst address, 2 dst_lo address (MTT_SPLIT destinations: hi -> dst, lo -> dst_lo; else 0), 3 total = n0*n1*n2,
 *     4 n1, 5 n2, 6..8 s0 s1 s2, 9..11 d0 d1 d2 (elements), 12 src dtype, 13 dst dtype, 14 vec (1: n2, s0, s1, d0, d1 multiples of 4,
 *     s2 = d2 = 1 and both addresses 16-byte aligned -> four elements per lane), 15 transpose (1: s1 = 1 and d2 = 1 — the source is
 *     contiguous along i1, the destination along i2; copied in 64 x 64 tiles of (i1, i2) through LDS; word 3 is then
 *     n0 * ceil(n1/64) * ceil(n2/64) * 4096 and chunk offsets count tile slots of 4096).
 * src_base / dst_base (bytes) are added to every src / dst(+dst_lo) address: 0 for tables of absolute addresses (persistent packs),
 * the buffers' addresses for tables of offsets (gradient scatter out of a fresh buffer).  Work is cut into chunks of
 * mtt_segcopy_chunk() logical elements: chunk c covers [chunk_off[c], chunk_off[c] + chunk) of segment chunk_seg[c].
 * Destination elements outside the boxes (padding) are not touched: the caller zeroes the buffers once. */
#define MTT_SEG_WORDS 16
typedef struct {
  const int64_t* table; const int32_t* chunk_seg; const int64_t* chunk_off; int32_t n_chunks;
  int64_t src_base, dst_base;
} mtt_segcopy_desc;
int mtt_segcopy_chunk(void);
int mtt_segcopy(const mtt_segcopy_desc* d, void* stream);

/* Small utilities: dtype cast / strided 2-D copy, column sums (bias gradients), axpy-style accumulate. */
int mtt_cast2d(const void* src, void* dst, int64_t rows, int64_t cols, int64_t lds, int64_t ldd,
               int src_dtype, int dst_dtype, int zero_pad_cols, void* stream);
/* ABI 12.  Pixel shuffle of nn.ConvTranspose2d(k = 2, s = 2) (taskprompter.py:705) computed as a PLAIN GEMM z = x W4^T, W4 row (dy*2+dx)*Co + co:
 *   out[((b*2H + 2y+dy)*2W + 2x+dx), co] = z[(b*H + y)*W + x, (dy*2+dx)*Co + co]   (co < Co; channels Co .. ldo-1 written as zeros)
 * z [B*H*W, ldz] (z_dtype), out [B*2H*2W, ldo] (out_dtype); ldo % 8 == 0.  (mtt_gemm's MTT_STORE_PIXSHUF2 does the same inside the general
 * kernel's epilogue; this pass lets the product run on the split-plane LDS-DMA kernel in the x3f mode.) */
int mtt_pixshuf2(const void* z, void* out, int32_t B, int32_t H, int32_t W, int32_t Co, int64_t ldz, int64_t ldo, int z_dtype, int out_dtype,
                 void* stream);
/* dst[r,:] = rowscale[(r/mb)*2 + ((r%mb) >= n_prompt)] * src[r,:] with dtype cast (DropPath scale of a branch gradient) */
int mtt_rowscale_cast(const void* src, void* dst, int64_t rows, int32_t cols, int64_t lds, int64_t ldd, int src_dtype, int dst_dtype,
                      const float* rowscale, int32_t mb, int32_t n_prompt, void* stream);
/* the same + colsum_out[c] = sum_r dst[r, c] of the values as stored (c < cols): when src is the gradient of a Linear's output (the
 * residual-stream gradient entering proj / fc2), the cast that prepares it for the bf16 GEMMs also yields that layer's bias gradient.
 * cols, lds, ldd multiples of 8; ws: mtt_rowscale_cast_colsum_ws_floats(rows, cols) floats of per-row-block partials (fixed-order sum). */
size_t mtt_rowscale_cast_colsum_ws_floats(int64_t rows, int32_t cols);
int mtt_rowscale_cast_colsum(const void* src, void* dst, int64_t rows, int32_t cols, int64_t lds, int64_t ldd, int src_dtype, int dst_dtype,
                             const float* rowscale, int32_t mb, int32_t n_prompt, float* colsum_out, float* ws, void* stream);
/* dst[c] = sum_r src[r, c] for c < cols (bias gradients; ld >= pad8(cols), columns up to pad8(cols) are read).  Deterministic two-stage
 * reduction through the caller-owned workspace ws (>= mtt_colsum_ws_floats(rows, cols) floats, contents unspecified afterwards). */
size_t mtt_colsum_ws_floats(int64_t rows, int32_t cols);
int mtt_colsum(const void* src, float* dst, int64_t rows, int32_t cols, int64_t ld, int src_dtype, float* ws, void* stream);
/* Z maps in one launch pair: map z starts src_zs elements after map z - 1, its sums dst_zs floats after those of z - 1;
 * ws >= Z * mtt_colsum_ws_floats(rows, cols) floats. */
int mtt_colsum_batched(const void* src, float* dst, int64_t rows, int32_t cols, int64_t ld, int src_dtype, int32_t Z, int64_t src_zs,
                       int64_t dst_zs, float* ws, void* stream);
int mtt_add_rows(const void* src, float* dst, int64_t rows, int32_t cols, int64_t lds, int64_t ldd, int src_dtype,
                 float alpha, void* stream);


/* ---------------------------------------------------------------------------------------------------------
 * InvPT decoder kernels (InvPT/models/transformers/invpt.py, transformer_decoder.py)
 * --------------------------------------------------------------------------------------------------------- */
/* Depthwise 3x3 stride-2 pad-1 conv, the query projection of invpt.py:124-138 (bias-free), Z tasks at once.
 * x [Z, B*H*W, ld] -> y [Z, B*Ho*Wo, ld], Ho = (H-1)/2+1; w fp32 [Z, 9, ld] (tap-major); optional per-channel
 * scale/shift [Z, ld] = eval BatchNorm folded in. */
typedef struct {
  const void* x; const float* w; void* y; const float* scale; const float* shift;
  int32_t Z, B, H, W; int64_t ld; int32_t dtype;
} mtt_dwconv_desc;
int mtt_dwconv3x3s2(const mtt_dwconv_desc* d, void* stream);
/* backward (scale/shift ignored: apply BN backward first): dx [Z, B*H*W, ld] (same dtype, optional), dw fp32 [Z, 9, ld] (optional) */
int mtt_dwconv3x3s2_bwd(const mtt_dwconv_desc* d, const void* dy, void* dx, float* dw, void* stream);

/* nn.AvgPool2d(kernel=stride=k, padding=0, ceil_mode=True) on NHWC (keys/values, invpt.py:139-149). */
typedef struct { const void* x; void* y; int32_t B, H, W, k; int64_t ld; int32_t dtype; } mtt_pool_desc;
int mtt_avgpool_ceil(const mtt_pool_desc* d, void* stream);
int mtt_avgpool_ceil_bwd(const mtt_pool_desc* d, const void* dy, void* dx, void* stream);

/* LayerNorm over the concatenated channels of all T tasks (norm_mts, invpt.py:482,526): x fp32 [T, rows, ldx],
 * gamma/beta fp32 [T*D] -> y [T, rows, ldy] (channels >= D written as zeros). */
typedef struct {
  const float* x; void* y; const float* gamma; const float* beta;
  int64_t rows; int32_t T, D; int64_t ldx, ldy; int32_t y_dtype; float eps;
} mtt_lnmt_desc;
int mtt_layernorm_mt(const mtt_lnmt_desc* d, void* stream);

/* Cross-stage attention message fusion (invpt.py:208-229): previous-stage scores upsampled x2 per task and mixed with
 * the current scores by the 1x1 conv fuse_attn [heads, 2*heads].  cur/out fp32 [B, heads, T*qh*qw, ldk],
 * prev fp32 [B, heads, T*(qh/2)*(qw/2), ldkp]; K valid key columns. */
typedef struct {
  const float* cur; const float* prev; float* out; const float* w; const float* bias;
  int32_t B, heads, T, qh, qw, K; int64_t ldk, ldkp;
} mtt_attnmsg_desc;
int mtt_attn_msg(const mtt_attnmsg_desc* d, void* stream);
/* backward of mtt_attn_msg (d->out unused): dcur, dup fp32 [B, heads, T*qh*qw, ldk] = gradients w.r.t. `cur` and w.r.t. the x2-upsampled
 * `prev` (the gradient of `prev` itself is mtt_bilinear_bwd of dup); dw [heads, 2*heads] and dbias [heads] are WRITTEN (per-workgroup
 * partials in ws, mtt_attn_msg_bwd_ws_floats(d) floats, summed in workgroup order). */
size_t mtt_attn_msg_bwd_ws_floats(const mtt_attnmsg_desc* d);
int mtt_attn_msg_bwd(const mtt_attnmsg_desc* d, const float* dout, float* dcur, float* dup, float* dw, float* dbias, float* ws, void* stream);

/* Gather half of nn.ConvTranspose2d(k=3, s=2, p=1, output_padding=1) (scale_embed[0], transformer_decoder.py:64):
 * yall [B*H*W, 9*Cop] = x @ Wall^T computed by mtt_gemm (column = tap*Cop + co) -> out [B*2H*2W, Cop] (+ bias[Cop]). */
typedef struct {
  const void* yall; void* out; const float* bias; int32_t B, H, W, Cop; int32_t dtype, out_dtype;
} mtt_convt_desc;
int mtt_convt3x3s2_gather(const mtt_convt_desc* d, void* stream);
/* backward: dyall [B*H*W, 9*Cop] (d->dtype) gathered from dout [B*2H*2W, Cop] (d->out_dtype) */
int mtt_convt3x3s2_gather_bwd(const mtt_convt_desc* d, const void* dout, void* dyall, void* stream);

/* ConvHead's first stage on the backbone's low-resolution task features: F.interpolate(x, scale_factor=4, 'bilinear') followed by
 * Conv2d(C, C, 3, padding=1)  (taskprompter.py:420 -> :692), evaluated "taps first".  Both operators are linear, so
 *   conv3x3(up4(x))(Y, X) = bias + sum over taps (ky, kx) of [ up4(W[ky,kx] x) ](Y + ky - 1, X + kx - 1)   (zero outside the 4h x 4w map):
 * the channel mixing runs as ONE GEMM on the h x w map (mtt_gemm, N = 9 * Cp: 16x fewer MACs than the conv on the upsampled map), and
 * these two entry points do what is left — an HBM-bound 36-point stencil — without materialising the upsampled features:
 *   mtt_upconv4_expand : z [Z][B*h*w][9*Cp] (column (ky*3+kx)*Cp + c holds W[ky,kx] x, channel padding zero)
 *                        -> y [Z][B*4h*4w][Cp] = act((sum of the shifted x4 bilinear expansions) * colscale + bias)
 *   mtt_upconv4_gather : the adjoint, dz [Z][B*h*w][9*Cp] from dy [Z][B*4h*4w][Cp] (the caller applies act' / BatchNorm backward first).
 * Bilinear semantics are PyTorch's align_corners=False (source index clamped at the borders); the x4 phase weights are the constants
 * 1/8, 3/8, 5/8, 7/8.  bias / colscale: fp32 [Z][C] or NULL.  z_dtype / y_dtype: MTT_F32 or MTT_BF16 (both the same). */
typedef struct {
  void* z; void* y; const float* bias; const float* colscale;
  int32_t Z, B, h, w, C, Cp; int32_t z_dtype, y_dtype, act;
} mtt_upconv_desc;
int mtt_upconv4_expand(const mtt_upconv_desc* d, void* stream);
int mtt_upconv4_gather(const mtt_upconv_desc* d, void* stream);

/* Fused multi-tensor clip_grad_norm_ + Adam (TaskPrompter/utils/train_utils.py:47-51, torch.optim.Adam semantics: L2 weight decay
 * added to the gradient, bias-corrected moments).  All n tensors are fp32; grads/params/exp_avg/exp_avg_sq/numel are DEVICE arrays
 * of n pointers / element counts; work is cut into chunks of mtt_adam_chunk() elements: chunk c covers elements
 * [chunk_off[c], chunk_off[c] + chunk) of tensor chunk_tensor[c] (device arrays of n_chunks entries, built once by the host).
 *   mtt_grad_sqnorm: *out_sq += sum of squares of all gradients (out_sq zeroed by the caller)
 *   mtt_adam_step  : g = grad * min(1, max_norm / (sqrt(*total_sq) + 1e-6))  (no clipping if max_norm <= 0 or total_sq NULL);
 *                    g += weight_decay * p; m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
 *                    p -= step_size * m / (sqrt(v) * inv_sqrt_bc2 + eps)   with step_size = lr / (1 - b1^t), inv_sqrt_bc2 = 1/sqrt(1 - b2^t) */
typedef struct {
  const void* const* grads; float* const* params; float* const* exp_avg; float* const* exp_avg_sq; const int64_t* numel;
  const int32_t* chunk_tensor; const int64_t* chunk_off; int32_t n_chunks;
  float max_norm, step_size, beta1, beta2, eps, weight_decay, inv_sqrt_bc2;
  const float* hyper;  /* optional DEVICE pair {step_size, inv_sqrt_bc2}: when non-NULL it replaces the two by-value fields, so that a step
                          captured in a hipGraph can be replayed with the next step count / learning rate (graphs.py) */
  float* ws;           /* mtt_grad_sqnorm: n_chunks floats of per-chunk partial sums (summed in chunk order: a deterministic clip norm) */
} mtt_adam_desc;
int mtt_adam_chunk(void);
int mtt_grad_sqnorm(const mtt_adam_desc* d, float* out_sq, void* stream);
int mtt_adam_step(const mtt_adam_desc* d, const float* total_sq, void* stream);

/* Per-task training losses from the full-resolution logits (TaskPrompter/losses/loss_functions.py:15-177; MultiTaskLoss,
 * loss_schemes.py:9-39, sums them with the task weights on the host side).  kind: 0 CrossEntropy(ignore) | 1 CrossEntropy with
 * 2-class label-frequency weights (`balanced`) | 2 balanced BCE-with-logits (pos_weight) | 3 L1(ignore) | 4 L1 on L2-normalised pred.
 * pred fp32 [B, C, HW] (NCHW), label fp32 [B, Cl, HW]; a pixel is valid when all its Cl label channels != ignore.
 *   mtt_loss_label_stats: stats[0] += number of valid pixels, stats[1] += sum of valid labels (channel 0)   (stats zeroed by caller)
 *   mtt_loss_fwd        : loss[0] += task loss (mean over valid pixels; normalisation read from `stats` on the device)
 *   mtt_loss_bwd        : dpred [B, C, HW] = gout[0] * d loss / d pred */
typedef struct {
  const float* pred; const float* label; float* dpred; float* loss; const float* stats;
  int64_t B, HW; int32_t C, Cl, kind; float ignore, pos_weight;
  float* ws;           /* label_stats / fwd: mtt_loss_ws_floats(d) floats of per-workgroup partials (summed in workgroup order) */
} mtt_loss_desc;
size_t mtt_loss_ws_floats(const mtt_loss_desc* d);
int mtt_loss_label_stats(const mtt_loss_desc* d, float* stats, void* stream);
int mtt_loss_fwd(const mtt_loss_desc* d, void* stream);
int mtt_loss_bwd(const mtt_loss_desc* d, const float* gout, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * TaskPrompter-Swin forward (TaskPrompter/models/transformers/taskprompter_swin.py).
 * --------------------------------------------------------------------------------------------------------------------------- */

/* Patchify for a k = s = P patch-embed conv, P in {2, 4, 8} (timm PatchEmbed, taskprompter_swin.py:605-607):
 * img fp32 NCHW [B,3,H,W] -> cols [B*(H/P)*(W/P), ldc] (k = (c*P + dy)*P + dx, columns >= 3*P*P zero), dtype out_dtype. */
int mtt_patchify(const float* img, void* cols, int B, int H, int W, int P, int64_t ldc, int out_dtype, void* stream);

/* Bilinear resize (align_corners = False, as F.interpolate) of `planes` fp32 maps [Hin, Win] -> [Hout, Wout]: the img_ds_ratio
 * input resize (taskprompter_swin.py:666-667) on the NCHW image. */
int mtt_resize_nchw(const float* in, float* out, int planes, int Hin, int Win, int Hout, int Wout, void* stream);

/* Row gather with zero fill: for b < B, r < rows, c < C:
 *   dst[b*dst_bs + r*ld_dst + c] = idx[b*idx_bs + r] >= 0 ? src[b*src_bs + idx[...]*ld_src + c] : 0      (dtype conversion on the way)
 * One kernel for the window partition of the (cyclically shifted, zero padded) token map with the prompts joined to every window
 * (taskprompter_swin.py:340-354,175-177), its inverse (:366-384), and the 2x2 patch-merging gather (:450-456: 4 calls, one per column
 * block of dst).  C % 8 == 0; pitches / strides in elements. */
typedef struct {
  const void* src; void* dst; const int32_t* idx;
  int64_t rows; int32_t C; int64_t ld_src, ld_dst; int32_t src_dtype, dst_dtype;
  int32_t B; int64_t src_bs, dst_bs, idx_bs;
  int32_t skip_neg;              /* 1: rows with idx < 0 are left untouched instead of zero-filled (scatter-style adjoints) */
} mtt_gather_desc;
int mtt_gather_rows(const mtt_gather_desc* d, void* stream);

/* Window attention with the task prompts as the first T tokens of every window (taskprompter_swin.py:168-210), head_dim 32:
 *   qkv (dtype) [nwin, N = T + ws2, 3*nH*32] -> out (dtype) [nwin, N, nH*32],
 *   S = scale * q k^T;  S[i >= T, j >= T] += bias[h, i-T, j-T] (+ mask[w % nW, i-T, j-T] when mask != NULL);  P = softmax(S);  out = P v
 *   rawmap fp32: the UNSCALED q.k of the prompt rows against the window's pixels, written straight into image layout
 *                rawmap[(b*nH + h)*T + t][map_off + pix[w % nW][j]]  (row pitch map_ld; pix < 0 = padding pixel, dropped; b = w / nW)
 *                — the re-assembly, reverse shift and un-padding of :376-388 folded into the store.
 * bias fp32 [nH, ws2, ws2] (the relative-position table gathered by the host once per parameter version), mask fp32 [nW, ws2, ws2]
 * (0 / -100), pix int32 [nW, ws2].  N <= 160. */
typedef struct {
  const void* qkv; void* out; float* rawmap; const float* bias; const float* mask; const int32_t* pix;
  int32_t nwin, nW, nH, T, ws2, dtype; float scale; int64_t map_ld, map_off;
  int32_t mfma;                  /* ABI 11, fp32 storage only: 1 = matrix-core arithmetic — forward: every product as 3 bf16 MFMAs on hi / lo split
                                    operands (fp32-class, the x3 / x3f modes); backward: bf16 MFMAs (the bf16 backward of the x3f mode).
                                    0 = the exact fp32 VALU kernels.  bf16 storage always runs on the matrix cores. */
  const float* biasT;            /* ABI 13, optional (mtt_winattn_bwd, matrix-core kernels): bias with its last two axes transposed, fp32 [nH, ws2, ws2] —
                                    the key-owner pass then reads bias / mask of 4 consecutive queries with one 16-byte load each (the shift mask
                                    must be symmetric, as Swin's region mask is).  NULL = strided scalar loads. */
} mtt_winattn_desc;
int mtt_winattn_fwd(const mtt_winattn_desc* d, void* stream);
/* backward (d as in the forward, d->out = the forward's output): dout (dtype) [nwin, N, nH*32]; drawmap fp32 = gradient of rawmap (same
 * layout; NULL = none) -> dqkv (dtype) [nwin, N, 3*nH*32] (written), dS_out fp32 [nwin, nH, ws2, ws2] = dS of the window x window
 * part (written when not NULL; the relative-position-bias gradient is its sum over the windows). */
int mtt_winattn_bwd(const mtt_winattn_desc* d, const void* dout, const float* drawmap, void* dqkv, float* dS_out, void* stream);

/* Channel attention of the prompts over the feature channels (taskprompter_swin.py:391-409), windows over the sqrt(ce) x sqrt(ce) grid
 * of the channel-embedding dimension:
 *   q fp32 [B, T, ce];  kvT (dtype) [B, 2*ce, ldk]: rows 0..ce-1 = k^T, ce..2ce-1 = v^T, columns = feature channels c < C
 *   rawchan[b, t, win, c] = sum_{e in win} q[b,t,e] * kT[b,e,c]        (fp32 [B, T, nwin, C], unscaled)
 *   cx[b, t, e in win]    = sum_c softmax_c(scale * rawchan[b,t,win,:]) * vT[b,e,c]      (fp32 [B, T, ce]) */
typedef struct {
  const float* q; const void* kvT; float* rawchan; float* cx;
  int32_t B, T, C, ce, nh, nw, kv_dtype; int64_t ldk; float scale;
  const float* kvbias;           /* fp32 [2*ce] added to the rows of kvT (the bias of the Linear that produced them), or NULL */
} mtt_chanattn_desc;
int mtt_chanattn_fwd(const mtt_chanattn_desc* d, void* stream);
/* backward (d as in the forward with d->rawchan = the forward's logits, d->kvbias NULL): drawchan fp32 [B, T, nwin, C] (NULL = none) and
 * dcx fp32 [B, T, ce] -> dq fp32 [B, T, ce] and dkvT fp32 [B, 2*ce, ldg] (rows: d kT, then d vT), both WRITTEN; ws: mtt_chanattn_bwd_ws_floats(d)
 * floats.  Fixed summation orders, no atomics. */
size_t mtt_chanattn_bwd_ws_floats(const mtt_chanattn_desc* d);
int mtt_chanattn_bwd(const mtt_chanattn_desc* d, const float* drawchan, const float* dcx, float* dq, float* dkvT, int64_t ldg, float* ws, void* stream);

/* Small-channel 3x3 stride-2 pad-1 convolution on fp32 maps (PatchMerging.spa_attn_ds, taskprompter_swin.py:437,463):
 *   x[b][ci][y*W + x] at x + b*x_bs + ci*x_cs + x_off;  w fp32 [Co, Ci, 3, 3];  y[b][co][...] at y + b*y_bs + co*y_cs + y_off  (H, W even) */
typedef struct {
  const float* x; const float* w; const float* bias; float* y;
  int32_t B, Ci, Co, H, W; int64_t x_bs, x_cs, x_off, y_bs, y_cs, y_off;
} mtt_conv3s2_desc;
int mtt_conv3s2_nchw(const mtt_conv3s2_desc* d, void* stream);
/* backward: dy laid out as y -> dx laid out as x (written for every (b, ci, pixel); may be NULL), dw fp32 [Co, Ci, 3, 3] and db fp32 [Co]
 * (written; dw NULL skips both; db may be NULL) */
int mtt_conv3s2_nchw_bwd(const mtt_conv3s2_desc* d, const float* dy, float* dx, float* dw, float* db, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Bird's-eye-view rotated boxes [x1, y1, x2, y2, ry] of the 3-D detection branch (TaskPrompter/detection_toolbox/iou3d: iou3d_kernel.cu
 * :241-275 pairwise kernels, :277-377 NMS mask kernels, iou3d.cpp:103-203 greedy reduction).
 *   mtt_boxes_overlap_bev: out fp32 [na, nb] = overlap area (iou = 0) or IoU (iou = 1) of every pair
 *   mtt_nms_bev          : boxes [n, 5] ALREADY sorted by descending score; rotated = 1 (nms_gpu) / 0 (nms_normal_gpu: axis-aligned IoU);
 *                          keep int64 [n] <- kept indices in score order, *num_out <- their count, both on the DEVICE (no host round trip:
 *                          the reference copies the suppression masks to the host and reduces there); ws >= mtt_nms_ws_bytes(n) bytes. */
int mtt_boxes_overlap_bev(const float* boxes_a, int na, const float* boxes_b, int nb, float* out, int iou, void* stream);
size_t mtt_nms_ws_bytes(int n);
int mtt_nms_bev(const float* boxes, int n, float thresh, int rotated, long long* keep, int* num_out, void* ws, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * ABI 14 — the FCOS3D detection head and its FPN neck (the 3ddet task: TaskPrompter/detection_toolbox/det_head.py, fpn.py; the
 * mmcv 1.6.2 layers they build through ConvModule).  All four families below are new entry points; no earlier struct changed.
 *
 * GroupNorm (+ ReLU) on NHWC rows (ConvModule's 'gn' + 'activate', det_head.py:208-216,238-246; nn.GroupNorm semantics):
 *   x (x_dtype) [Z*B*HW rows, ld]: Z stacked layers of B images of HW pixels, C valid channels in G groups of C/G channels.
 *   Statistics per (z, image, group) over HW*C/G values, biased variance; mean / rstd fp32 [Z*B*G] are written by the forward.
 *   y = act((x - mean) * rstd * gamma[z*C + c] + beta[z*C + c]); act = ReLU when relu != 0.  y (y_dtype: F32 / BF16 / SPLIT with the lo
 *   plane at y_lo) has pitch ld; channels C..ld-1 are written as zeros.  G may be large (a batch of branch layers as ONE GroupNorm).
 *   bwd: dy (dy_dtype, pitch ld) -> dx (dx_dtype, pitch ld, padding written as zeros), dgamma / dbeta fp32 [Z*C] (written); reads x,
 *   mean, rstd, gamma, beta of the forward (the ReLU mask is recomputed).
 *   Both directions reduce through per-workgroup partials in ws (>= mtt_groupnorm_ws_floats(d) floats), summed in a fixed order. */
/* sizeof() of the ABI 14 descriptors: 0 gn, 1 dcn, 2 nearest, 3 bboxpost (0 otherwise) */
size_t mtt_det_desc_size(int which);

typedef struct {
  const void* x; void* y; void* y_lo; const float* gamma; const float* beta; float* mean; float* rstd;
  const void* dy; void* dx; float* dgamma; float* dbeta;
  int32_t Z, B; int64_t HW; int32_t C, G; int64_t ld;
  int32_t x_dtype, y_dtype, dy_dtype, dx_dtype;
  int32_t relu; float eps;
  float* ws;
} mtt_gn_desc;
size_t mtt_groupnorm_ws_floats(const mtt_gn_desc* d);
int mtt_groupnorm_fwd(const mtt_gn_desc* d, void* stream);
int mtt_groupnorm_bwd(const mtt_gn_desc* d, void* stream);

/* Modulated deformable 3x3 convolution (DCNv2), the columns half: ModulatedDeformConv2dPack of mmcv 1.6.2 with deform_groups = groups = 1,
 * selected by dcn_on_last_conv (det_head.py:225-226,248-249).  Sampling, restated from mmcv's modulated_deform_conv kernels:
 *   tap k = i*3 + j of output pixel (ho, wo): h = ho*stride - pad + i*dil + dh_k,  w = wo*stride - pad + j*dil + dw_k
 *   dh_k = offset[row, 2k], dw_k = offset[row, 2k+1]  (offset NULL: 0);  m_k = mask[row, k] (sigmoid of it when mask_sigmoid; NULL: 1)
 *   value = 0 when h <= -1 || w <= -1 || h >= H || w >= W; otherwise the bilinear sample of the four corners around (h, w), corners
 *   outside [0, H-1] x [0, W-1] contributing 0.  col[row, k*Cp + c] = m_k * value   (row = (b*Ho + ho)*Wo + wo, c < Cp).
 *   x (x_dtype) NHWC [B*H*W, ldx] (channels C..Cp-1 zero); col (col_dtype F32 / BF16 / SPLIT with col_lo) [B*Ho*Wo, ldc >= 9*Cp].
 * The convolution itself is mtt_gemm on col with the pack of mtt_gemm's implicit 3x3 conv (k = tap*Cp + ci).  With offset = mask = NULL
 * this is a plain strided im2col (the FPN's stride-2 extra conv, fpn.py add_extra_convs='on_output').
 * mtt_dcn_col2im_bwd: dcol (dcol_dtype, pitch ldc) -> dx (dx_dtype, pitch ldx, channels < Cp written) = the transpose of the sampling;
 *   doffset / dmask (optional, off_dtype, layouts of offset / mask; dmask is the gradient of the mask LOGIT when mask_sigmoid).  dx is a
 *   gather, no floating-point atomics: the samples are bucketed by their floor cell with a stable radix sort (integer keys, sample order
 *   within a bucket) in ws (>= mtt_dcn_col2im_ws_floats(d) floats), then each input pixel sums its four neighbouring buckets in a fixed
 *   order.  Bitwise reproducible run to run. */
typedef struct {
  const void* x; int32_t x_dtype; int64_t ldx;
  const void* offset; int64_t ld_off;
  const void* mask; int64_t ld_mask; int32_t mask_sigmoid; int32_t off_dtype;   /* offset / mask / doffset / dmask: F32 or BF16 */
  void* col; void* col_lo; int32_t col_dtype; int64_t ldc;
  int32_t B, H, W, C, Cp, Ho, Wo, stride, pad, dil;
  const void* dcol; int32_t dcol_dtype;
  void* dx; int32_t dx_dtype;
  void* doffset; void* dmask;
  void* ws;
} mtt_dcn_desc;
size_t mtt_dcn_col2im_ws_floats(const mtt_dcn_desc* d);
int mtt_dcn_im2col(const mtt_dcn_desc* d, void* stream);
int mtt_dcn_col2im_bwd(const mtt_dcn_desc* d, void* stream);

/* FPN top-down step on NHWC maps (fpn.py: laterals[i-1] += F.interpolate(laterals[i], size=prev_shape, mode='nearest')):
 *   out[b, y, x, c] = a[b, y, x, c] + src[b, iy(y), ix(x), c] for c < C (out may alias a), with torch's nearest index rule
 *   iy = min(floor(y * (float)Hi / Ho), Hi - 1) (likewise ix) — any ratio, including 1.  dtype (F32 / BF16) for all three maps.
 * mtt_nearest_add_bwd: a = the gradient of out [B, Ho, Wo] -> out = the gradient of src [B, Hi, Wi] (written, c < C): every coarse pixel
 *   gathers the fine pixels that read it, in row-major order (the gradient of a is a itself). */
typedef struct {
  const void* a; const void* src; void* out;
  int32_t B, C, Ho, Wo, Hi, Wi; int64_t ld_a, ld_src, ld_out; int32_t dtype;
} mtt_nearest_desc;
int mtt_nearest_add(const mtt_nearest_desc* d, void* stream);
int mtt_nearest_add_bwd(const mtt_nearest_desc* d, void* stream);

/* Per-level tail of FCOS3DHead.forward_single (det_head.py:440-457) and the NHWC -> NCHW store of the head outputs:
 *   input channel j (0 <= j < nch = sum dims) is column j - (start of its group) of group g: x[g] fp32 [B*H*W, ldx[g]] (ngroups <= 8)
 *   out fp32 NCHW [B, nch, H, W].  scales == NULL: out = x (a layout change).  scales fp32 [4] = (offset, depth, size, bbox2d):
 *     j < 2: s0*x;  j == 2: exp(s1*x);  3 <= j < 6: exp(s2*x) + 1e-6;  last 4 channels when bbox2d: relu(s3*x);  others: x.
 * mtt_fcos_bbox_post_bwd: dout (layout of out) -> dx[g] (layout of x[g]; columns dims[g]..ldx[g]-1 written as zeros) and, with scales,
 *   dscales fp32 [4] (written), reduced through per-workgroup partials in ws (>= mtt_fcos_bbox_post_ws_floats(d) floats), fixed order. */
typedef struct {
  const float* x[8]; int64_t ldx[8]; int32_t dims[8]; int32_t ngroups;
  float* out; const float* scales; int32_t bbox2d;
  int32_t B, H, W;
  const float* dout; float* dx[8]; float* dscales; float* ws;
} mtt_bboxpost_desc;
size_t mtt_fcos_bbox_post_ws_floats(const mtt_bboxpost_desc* d);
int mtt_fcos_bbox_post(const mtt_bboxpost_desc* d, void* stream);
int mtt_fcos_bbox_post_bwd(const mtt_bboxpost_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * ABI 15 — the FCOS3D criterion of the 3ddet task (TaskPrompter/detection_toolbox/det_model.py DetModel.loss, :253-481, with
 * pred_bbox2d: 13 regression channels = offset 2, depth 1, size 3, rotation 3, bbox2d 4).  New entry points only.
 *
 * Points: level l has H[l] x W[l] points, p = y * W + x (row-major, levels concatenated: P points per image);
 *   xs = (float)x * stride[l] + half[l],  ys = (float)y * stride[l] + half[l]   (half = fp32(stride // 2)).
 * Ground truth: labelled image k (0 <= k < n_lab) owns gts [img[k], img[k] + img[n_lab + k]) of gts (fp32 records of 16:
 *   x1 y1 x2 y2 (bbox_modal), label, cx cy depth (center_I), size_S[3], rotation_S[3], 2 unused); img[2 n_lab + k] = its batch index,
 *   img[3 n_lab + b] = the labelled index of batch image b, or -1 when it is dropped (det_label_number == 0).
 * Assignment (_get_target_single, :858-955), in fp32 in the reference's operation order (the source is built without FMA contraction):
 *   inside the centre box when min(xs - (cx - radius[l]), ys - (cy - radius[l]), (cx + radius[l]) - xs, (cy + radius[l]) - ys) > 0,
 *   in range when rr_lo[l] <= max(l, t, r, b) <= rr_hi[l]; dist = sqrt(dx*dx + dy*dy), 1e8 when either test fails; the smallest dist
 *   wins, the FIRST gt on ties; 1e8 = background (label C).  target (n_lab, 13, P) = (dx / stride, dy / stride, depth, size, rotation,
 *   l / stride, t / stride, r / stride, b / stride) of the selected gt (gt 0 for background; zeros for an image without gts);
 *   centerness (n_lab, P) = exp(-ctr_alpha * sqrt(dx*dx + dy*dy) / (1.414f * radius[l])); label int32 (n_lab, P).
 * mtt_fcos3d_targets: the assignment alone (the head maps may be NULL; ws is not used).
 * mtt_fcos3d_loss_fwd: the assignment and, in the same pass, the loss sums of every labelled point, read from the head's NCHW fp32 maps
 *   in place (cls [B, C, H, W], bbox [B, 13, H, W], dir [B, 6, H, W], ctr [B, 1, H, W] per level); per-workgroup partials in ws
 *   (>= mtt_fcos3d_ws_floats(d) floats), then one workgroup sums them in workgroup order and writes out[9] = (loss_cls, loss_offset,
 *   loss_depth, loss_size, loss_rotsin, loss_dir, loss_centerness, loss_bbox2d, loss_sum) and stats[2] = (num_pos, num_pos + n_lab):
 *   cls = sigmoid focal / (num_pos + n_lab); smooth-L1 x code_weight (rotation as sin(p)cos(t) - cos(p)sin(t)), the three 2-way
 *   softmax CEs on floor(limit_period(rot - dir_offset, 0, 2 pi) / pi) and the centerness BCE-with-logits over positives / num_pos; each
 *   times its loss weight; every positive-only term 0 when num_pos == 0.  Nothing is read back to the host.
 * mtt_fcos3d_loss_bwd: gout[9] = the upstream gradient of out (component i receives gout[i] + gout[8]) -> every element of dcls / dbbox /
 *   ddir / dctr (layouts of the maps) is written: zeros for dropped images and, in the bbox / dir / ctr maps, for non-positive points.
 *   Reads label / target / centerness / stats of the forward.  No atomics: bitwise reproducible. */
#define MTT_FCOS3D_MAX_LEVELS 8
typedef struct {
  const float* cls[8]; const float* bbox[8]; const float* dir[8]; const float* ctr[8];
  float* dcls[8]; float* dbbox[8]; float* ddir[8]; float* dctr[8];
  int32_t H[8], W[8];
  float stride[8], half[8], radius[8], rr_lo[8], rr_hi[8];
  int32_t nlev, B, n_lab, C;
  int64_t P;
  const int32_t* img; const float* gts;
  int32_t* label; float* target; float* centerness;
  float* ws; float* out; float* stats; const float* gout;
  float code_weight[13];
  float loss_weight[5];            /* cls, bbox (offset / depth / size / rotsin), dir, centerness, bbox2d */
  float gamma, alpha, beta, beta2d, ctr_alpha, dir_offset;
} mtt_fcos3d_desc;
size_t mtt_fcos3d_desc_size(void);
size_t mtt_fcos3d_ws_floats(const mtt_fcos3d_desc* d);
int mtt_fcos3d_targets(const mtt_fcos3d_desc* d, void* stream);
int mtt_fcos3d_loss_fwd(const mtt_fcos3d_desc* d, void* stream);
int mtt_fcos3d_loss_bwd(const mtt_fcos3d_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * ABI 16 — FCOS3D box decoding and per-class NMS of the 3ddet task at inference (det_model.py get_bboxes / _get_bboxes_single :483-681,
 * det_tools.py box3d_multiclass_nms :85-210).  New entry points only; all four take one descriptor and read / write only the buffers
 * named below, all caller-owned.  Maps: the head's NCHW fp32 maps as in ABI 15's descriptor, 13 regression channels; points as there.
 *
 * Candidates: level l contributes n_l = nms_pre when nms_pre > 0 and P_l > nms_pre, else P_l; cand_off[l] = sum of the earlier n_l and
 *   cand_off[nlev] = N (N <= MTT_DET_MAX_CAND, C <= MTT_DET_MAX_CLASSES).  key_off is the same for P_l (key_off[nlev] = P).
 * mtt_det_select: one workgroup per (level, image).  keys[b, key_off[l] + p] = max_c sigmoid(cls_c) * sigmoid(ctr); sel[b, cand_off[l]
 *   + i] = the level-local point index of the i-th selected point: the n_l largest keys (a radix select on the fp32 bit pattern, the
 *   histogram in LDS; among keys equal to the n_l-th largest the lowest point indices), in ascending point order; the whole level in
 *   order when n_l == P_l.
 * mtt_det_decode: one thread per (image, candidate).  denorm[l] multiplies the offset and the 2-D distances (the level's stride for the
 *   head's normalised maps, 1 for denormalised ones).  box9 [B, N, 9] = (camera centre = (u d, v d, d, 1) . inv[b]^T, size, the three
 *   angles rot - floor((rot - dir_offset) / pi) pi + pi dir_cls), cen2d [B, N, 3] = (u, v, d) with (u, v) = point - offset, box2d
 *   [B, N, 4] = point -/+ distances clamped to [0, img_size[b] = (H, W)], nmsbox [B, N, 5] = columns (0, 2, 4, 3, 8) of box9 as
 *   (x - w/2, z - l/2, x + w/2, z + l/2, yaw), dircls int32 [B, N, 3] (1 when the second logit is larger), scores [B, N, C] =
 *   sigmoid(cls) * sigmoid(ctr).  inv fp32 [B, 16]: the row-major inverse of the 4 x 4 padded camera matrix.
 * mtt_det_nms_seg: one segment per (image, class): the candidates with scores > score_thr, sorted by descending score (bitonic, in LDS;
 *   equal scores by ascending candidate index), the 64 x 64 suppression masks of mtt_nms_bev's kernels on them (rotated = 1 / 0) and its
 *   greedy pass, all on the device.  seg_n int32 [B, C] = candidates above the threshold, seg_idx int32 [B, C, N] = their candidate
 *   indices in sorted order, kept_n int32 [B, C], kept int32 [B, C, N] = the kept candidates' indices in score order; ws >=
 *   mtt_det_nms_ws_bytes(d) bytes (sorted scores and boxes, kept scores, masks).
 * mtt_det_collect: the kept lists concatenated in class order; when more than max_per_img remain, the max_per_img best by descending
 *   score (equal scores in concatenation order).  out fp32 [B, max_per_img, 18] = (box9, score, cen2d, box2d, the label's int32 bit
 *   pattern), count int32 [B]; rows at and beyond count[b] are not written.  Reads kept / kept_n and ws of mtt_det_nms_seg.
 * No allocation, synchronisation or atomics on floats; bitwise reproducible. */
#define MTT_DET_MAX_CAND 8192
#define MTT_DET_MAX_CLASSES 16
#define MTT_DET_OUT_COLS 18
typedef struct {
  const float* cls[8]; const float* bbox[8]; const float* dir[8]; const float* ctr[8];
  int32_t H[8], W[8];
  float stride[8], half[8], denorm[8];
  int32_t cand_off[9], key_off[9];
  int32_t nlev, B, C, N, nms_pre, rotated, max_per_img;
  float dir_offset, score_thr, nms_thr;
  const float* inv; const float* img_size;
  float* keys; int32_t* sel;
  float* box9; float* cen2d; float* box2d; float* nmsbox; int32_t* dircls; float* scores;
  int32_t* seg_n; int32_t* seg_idx; int32_t* kept_n; int32_t* kept;
  void* ws;
  float* out; int32_t* count;
} mtt_det_decode_desc;
size_t mtt_det_decode_desc_size(void);
size_t mtt_det_nms_ws_bytes(const mtt_det_decode_desc* d);
int mtt_det_select(const mtt_det_decode_desc* d, void* stream);
int mtt_det_decode(const mtt_det_decode_desc* d, void* stream);
int mtt_det_nms_seg(const mtt_det_decode_desc* d, void* stream);
int mtt_det_collect(const mtt_det_decode_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * ABI 17 — evaluation of the dense tasks on the device: what the reference's validation loop computes between model(images) and
 * get_score (TaskPrompter/utils/utils.py get_output :27-63; evaluation/eval_semseg.py, eval_human_parts.py, eval_sal.py, eval_depth.py,
 * eval_normals.py, eval_edge.py).  New entry points only.  Logits fp32 NCHW [B, C, HW], labels fp32 [B, Cl, HW]; fp32 arithmetic in the
 * reference's operation order (no contraction into FMAs); one thread per pixel, or per four consecutive pixels (16-byte loads) when HW is a
 * multiple of 4 and pred, label and out are 16-byte aligned: which of the two runs is a function of the descriptor alone, and fixes the
 * order in which the fp64 partial sums are taken.
 *
 * kind                 C / Cl   map (mtt_eval_map -> out)                                accumulator `acc` (8-byte slots, caller zeroes)
 *  MTT_EVAL_CONFUSION  C / 1    int64 [B, HW]: arg-max over C, first index wins ties;    int64 tp[n], fp[n], fn[n]  (n <= 256, HW < 2^32)
 *                               class_map (int64 [n_map], optional): p < n_map -> map[p]
 *  MTT_EVAL_SAL        2 / 1    fp32 [B, HW]: 255 * softmax(x)[1]                        int64 pp_hist[T + 1], tp_hist[T + 1], ap  (T <= 255)
 *  MTT_EVAL_DEPTH      1 / 1    fp32 [B, HW]: max(x, 0); out may be pred (in place)      int64 count; fp64 sum (g-v)^2, (log g - log v)^2,
 *                                                                                        |g-v|/g, (g-v)^2/g
 *  MTT_EVAL_NORMALS    3 / 3    fp32 [B, HW, 3]: (x / max(|x|, 1e-12) + 1) * 255 / 2     int64 count; fp64 sum of the angle in degrees
 *  MTT_EVAL_EDGE       1 / 1    fp32 [B, HW]: 255 / (1 + exp(-x))                        int64 count; fp64 sum of term / factor
 *
 * mtt_eval_accum adds one batch to `acc`.  source = MTT_EVAL_FROM_LOGITS: pred = the logits; MTT_EVAL_FROM_MAP: pred = the map that
 * mtt_eval_map wrote (int64 for CONFUSION).  Both sources feed the same per-pixel value into the same code: bitwise equal accumulators.
 * valid pixel: label != ignore (all three channels for NORMALS); DEPTH with mask_mode 0: min_depth < label < max_depth, 1: label != ignore.
 *   CONFUSION  p = arg-max, g = label: g == p < n -> tp[p]; otherwise fp[p] when 0 <= p < n and fn[g] when g is an integer in [0, n)
 *   SAL        s = sigmoid(map / 255) (the reference squashes the probability a second time), k = #{i : s >= thresholds[i]} (fp32 [T],
 *              ascending), t = (int64) label: pp_hist[k] += 1, tp_hist[k] += t, ap += t
 *   DEPTH      g' = g <= 0 ? 1e-9 : g, v' likewise from v = max(x, 0)
 *   NORMALS    p = normalize(2 map / 255 - 1), g = normalize(label) (a zero norm gives the zero vector): deg(2 atan2(|p - g|, |p + g|))
 *   EDGE       z = map / 255, w = pos_weight, factor = 1 / (1 - w), pw = w factor: term = (1 - y) z + (1 + (pw - 1) y) softplus(-z)
 * Integer counters: a histogram per workgroup in LDS, then 64-bit integer atomics on acc (order-independent).  fp64 sums: no atomics;
 * per-workgroup partials go to ws (>= mtt_eval_ws_floats(d) floats, 8-byte aligned; 0 for the integer-only kinds) and a second launch
 * adds them to acc in workgroup order.  Neither entry point modifies its inputs, except mtt_eval_map when out aliases pred (DEPTH). */
enum { MTT_EVAL_CONFUSION = 0, MTT_EVAL_SAL = 1, MTT_EVAL_DEPTH = 2, MTT_EVAL_NORMALS = 3, MTT_EVAL_EDGE = 4 };
enum { MTT_EVAL_FROM_LOGITS = 0, MTT_EVAL_FROM_MAP = 1 };
typedef struct {
  const void* pred; const float* label;
  void* out;                       /* mtt_eval_map */
  void* acc; double* ws;           /* mtt_eval_accum */
  const float* thresholds; const int64_t* class_map;
  int64_t B, HW;
  int32_t C, Cl, kind, source, n_classes, n_thresh, n_map, mask_mode;
  float ignore, pos_weight, min_depth, max_depth;
} mtt_eval_desc;
size_t mtt_eval_desc_size(void);
size_t mtt_eval_ws_floats(const mtt_eval_desc* d);
int mtt_eval_map(const mtt_eval_desc* d, void* stream);
int mtt_eval_accum(const mtt_eval_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Training-batch augmentation on the device (additive exports, ABI 17 unchanged): what the reference composes per sample in numpy and
 * OpenCV in get_transformations (TaskPrompter/utils/common_config.py:96-124) from data/transforms.py -- RandomScaling, RandomCrop,
 * RandomHorizontalFlip, PhotoMetricDistortion, Normalize, PadImage, AddIgnoreRegions, ToTensor -- as ONE gather per output pixel.
 * The random draws are made on the host and live in a table, int32 [B, MTT_AUG_COLS] (floats as their bit patterns), present twice: a
 * host copy the entry points validate before they launch, and the device copy the kernels read.  A ragged batch is one packed buffer per
 * key (HWC samples back to back); off / off_host hold each sample's first ELEMENT, int64 [B].
 *
 * Host check (MTT_E_BADARG, nothing launched): 1 <= H, W, SH, SW <= 32768; off >= 0 and off + H*W*C <= src_numel; RESIZED, FLIP and
 * the switches in {0, 1}; SH == H and SW == W unless RESIZED; NTEST in {0, 10}; CHOSEN in [0, 10]; every candidate offset in
 * [0, max(S - crop, 0)]; HDELTA in [-18, 17].  In the kernels every table value is clamped to those ranges again and every source index
 * to [0, src_numel - 1]: no content of the device table makes them read outside the packed buffer; writes depend on B, h, w alone.
 *
 * Output pixel (y, x) of the h x w result maps back through pad (the crop of Hc x Wc = min(S, crop) sits at (h - Hc) / 2, (w - Wc) / 2),
 * flip (x -> Wc - 1 - x), crop (candidate CHOSEN) and scale.  One thread per pixel, or per 4 consecutive pixels with 16-byte stores when
 * w % 4 == 0.  No floating-point atomics, no contraction into FMAs: bitwise reproducible.
 *
 * mtt_aug_select  src = the packed semseg maps (fp32, C = 1, labels integral in [0, 255]).  For rows with NTEST = 10 (CHOSEN = 10 on
 *   entry) candidates 0..9 are histogrammed over the nearest-resampled map (LDS integer histograms); a candidate passes when more than
 *   one label other than 255 occurs and max / sum < cat_max_ratio in fp64; CHOSEN becomes the first that passes (integer atomic min).
 * mtt_aug_image   src uint8 or fp32 HWC (C = 3), values in [0, 255].  RESIZED: bilinear, fx = (float)((dx + 0.5) * (src / dst) - 0.5)
 *   with the product in fp64, taps clamped at both borders, horizontal a0*s0 + a1*s1 then vertical.  photometric: truncation to 8 bits,
 *   brightness, contrast before (FMODE) or after saturation and hue; each `convert` is clip(v * alpha + beta, 0, 255) truncated;
 *   saturation and hue each take an RGB -> HSV -> RGB round trip (H in 0..179; integer forward conversion with the 12-bit reciprocal
 *   tables, float sector inverse, round to nearest even).  Then (v / 255 - mean) / std with IEEE divisions; pad = 0.  out fp32 [B,3,h,w].
 * mtt_aug_labels  src fp32 HWC, C = 1 (3 for MTT_AUG_NORMALS).  Nearest: sx = min(dx * src / dst, src - 1) in integers.  MTT_AUG_DEPTH:
 *   divided by SCALE when RESIZED; 0 -> -1 when depth_ignore.  MTT_AUG_NORMALS: x negated under FLIP; a zero vector -> 255 on the three
 *   channels.  Pad = fill, BEFORE those two rules (as PadImage precedes AddIgnoreRegions).  MTT_AUG_HUMAN_PARTS: flags int32 [B] records
 *   per image whether a label other than 0 / 255 occurs (integer atomic); a second launch fills the images without one with 255.
 *   out fp32 [B, C, h, w]. */
#define MTT_AUG_CANDS 11
#define MTT_AUG_COLS 40
enum { MTT_AUG_H = 0, MTT_AUG_W = 1, MTT_AUG_SH = 2, MTT_AUG_SW = 3, MTT_AUG_RESIZED = 4, MTT_AUG_FLIP = 5, MTT_AUG_NTEST = 6, MTT_AUG_CHOSEN = 7,
       MTT_AUG_CAND_Y = 8, MTT_AUG_CAND_X = 19,
       MTT_AUG_BRIGHT = 30, MTT_AUG_BETA = 31, MTT_AUG_FMODE = 32, MTT_AUG_CONTRAST = 33, MTT_AUG_CALPHA = 34, MTT_AUG_SAT = 35, MTT_AUG_SALPHA = 36,
       MTT_AUG_HUE = 37, MTT_AUG_HDELTA = 38, MTT_AUG_SCALE = 39 };
enum { MTT_AUG_PLAIN = 0, MTT_AUG_DEPTH = 1, MTT_AUG_NORMALS = 2, MTT_AUG_HUMAN_PARTS = 3 };
typedef struct {
  const void* src; const int64_t* off; const int64_t* off_host;
  int32_t* table; const int32_t* table_host;
  float* out; int32_t* flags;
  int64_t src_numel;
  double cat_max_ratio;            /* mtt_aug_select */
  int32_t B, h, w, C, src_u8, kind, photometric, depth_ignore;
  float fill, mean[3], std[3];
} mtt_aug_desc;
size_t mtt_aug_desc_size(void);
int mtt_aug_select(const mtt_aug_desc* d, void* stream);
int mtt_aug_image(const mtt_aug_desc* d, void* stream);
int mtt_aug_labels(const mtt_aug_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Cityscapes-3D batch preparation on the device (additive exports, ABI 17 unchanged): the per-sample work of the reference's dataset
 * class (TaskPrompter/data/cityscapes3d.py:137-241) on a batch of equally sized frames.  Both entry points launch on the caller's
 * stream, never synchronise and return MTT_E_* without launching anything when the descriptor is refused.
 *
 * The resampling rules are Pillow's, and their tables are built on the HOST in doubles (multi-task-transformer_amd/cs3d.py):
 *   bilinear, 8 bit   per axis bounds int32 [n_out, 2] = (first source index, tap count) and coeff int32 [n_out, ksize], the weights
 *                     fixed to 22 bits.  One pass is out = clip8((2^21 + sum k_i * p_i) >> 22) in 32-bit integers; the horizontal pass
 *                     runs first and is rounded to 8 bits before the vertical one.  An axis that keeps its size gets the identity table
 *                     (ksize 1, coefficient 2^22), which reproduces the pixel exactly.
 *   nearest           per axis index int32 [n_out], built by Pillow's recurrence xo = 0.5 * in/out; xo += in/out in doubles.
 * xtab / ytab are device tables, xtab_host / ytab_host their host copies: the entry point validates the HOST copy (xn == w, yn == h,
 * every index inside the source, bounds non-decreasing, 0 < count <= ksize) and derives the tile's LDS need from it; the kernels clamp
 * what they read from the DEVICE copy to the same ranges again, so no table content makes them read outside src or their LDS window.
 *
 * mtt_cs3d_image   src uint8 [B, H, W, 3] (16-byte aligned), bgr != 0: channel order B, G, R as cv2.imread delivers.  out fp32
 *   [B, 3, h, w] = ((u8 / 255) - mean) / std with IEEE divisions (ToTensor + Normalize), channels R, G, B.  All four tables NULL:
 *   h == H and w == W, a streaming kernel (H * W % 16 == 0 and 16-byte aligned pointers: a workgroup moves 4096 pixels through LDS,
 *   three 16-byte loads and twelve 16-byte stores per thread, a wave's stores contiguous; otherwise one pixel per thread).
 *   Otherwise both axes carry tables and a workgroup owns MTT_CS3D_TILE_H x MTT_CS3D_TILE_W output pixels: it stages the source rows
 *   of its window into LDS with 16-byte loads, runs the horizontal pass into LDS as uint8 [row][channel][64], then the vertical pass
 *   and the normalisation, 4 pixels per thread.  MTT_E_UNSUPPORTED when a tile's window exceeds MTT_CS3D_MAX_ROWS source rows or
 *   MTT_CS3D_MAX_COLS source columns (a reduction by more than about 11 along y or 80 along x).
 * mtt_cs3d_labels  src = raw labelIds uint8 [B, H, W], disp = disparity uint16 [B, H, W] or NULL.  xtab / ytab nearest tables or
 *   NULL (identity: the axis keeps its size).  semseg int64 [B, h, w]: the 256-entry restatement of encode_segmap (void ids -> 255, the
 *   19 valid ids -> 0..18, everything else kept).  flags int32 [B] is cleared, then flags[b] = 1 when an output pixel of image b is
 *   neither 255 nor below 19 (integer atomic OR).  out = depth fp32 [B, 1, h, w] (only with disp): d > 0 -> (d - 1) / 256; then 0 ->
 *   -1 (d == 1 included); then 0 where the RAW label id is 10. */
#define MTT_CS3D_TILE_H 16
#define MTT_CS3D_TILE_W 64
#define MTT_CS3D_MAX_ROWS 208
#define MTT_CS3D_MAX_COLS 5440
typedef struct {
  const uint8_t* src; const uint16_t* disp;
  const int32_t* xtab; const int32_t* ytab; const int32_t* xtab_host; const int32_t* ytab_host;
  const int32_t* xcoeff; const int32_t* ycoeff;     /* mtt_cs3d_image: device, [xn, xk] and [yn, yk] */
  float* out; int64_t* semseg; int32_t* flags;
  int32_t B, H, W, h, w, xn, yn, xk, yk, bgr;
  float mean[3], std[3];
} mtt_cs3d_desc;
size_t mtt_cs3d_desc_size(void);
int mtt_cs3d_image(const mtt_cs3d_desc* d, void* stream);
int mtt_cs3d_labels(const mtt_cs3d_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Rendering predictions on the device (additive exports, ABI 17 unchanged): what the reference's vis_pred_for_one_task
 * (TaskPrompter/utils/visualization_utils.py:122-198) and save_model_pred_for_one_task (evaluation/evaluate_utils.py:126-154) do to a
 * prediction before it is encoded into a file, in one pass over the logits.  Both entry points launch on the caller's stream, never
 * synchronise and return MTT_E_* without launching anything when the descriptor is refused.
 *
 * src fp32 NCHW [B, C, h, w], read in place.  Per pixel (y, x) of the (H, W) grid, all in fp32 registers:
 *   1. bilinear interpolation with align_corners = False under PyTorch's rules: scale = (float)in / out, source coordinate
 *      s = max(scale * (d + 0.5) - 0.5, 0), lower tap i0 = min((int)s, in - 1), upper tap min(i0 + 1, in - 1), weights 1 - l and l with
 *      l = s - i0; the horizontal pair of each row first, (1 - lx) * v0 + lx * v1, then the vertical one, no fused multiply-adds.
 *      (H, W) == (h, w) takes a path without taps and returns the source values themselves.
 *   2. the rule of get_output (TaskPrompter/utils/utils.py:27-63) selected by `mode`:
 *        MTT_RENDER_CLASS         arg-max over C (1..256), the first index wins ties
 *        MTT_RENDER_SIGMOID255    C == 1: 255 / (1 + exp(-x))
 *        MTT_RENDER_SOFTMAX1_255  C == 2: exp(x1 - m) / (exp(x0 - m) + exp(x1 - m)) * 255, m = max(x0, x1)
 *        MTT_RENDER_NORMALS       C == 3: (x / max(sqrt(x0^2 + x1^2 + x2^2), 1e-12) + 1) * 255 / 2 per component
 *        MTT_RENDER_DEPTH         C == 1: x > 0 ? x : 0
 *   3. the output selected by `out_kind`:
 *        MTT_RENDER_OUT_U8        uint8 [.., H, W]: the class index; the value truncated (SIGMOID255, SOFTMAX1_255); for DEPTH the index
 *                                 (v - min_b) / (max_b - min_b) * 255 truncated, min_b / max_b read from `minmax` (mtt_render_minmax), and 0
 *                                 everywhere when max_b == min_b (the reference divides 0 by 0 there)
 *        MTT_RENDER_OUT_LUT1      uint8 [.., H, W]: table[index], table uint8 [256] on the device (CLASS only)
 *        MTT_RENDER_OUT_LUT3      uint8 [.., H, W, 3]: table[index][0..2], table uint8 [256, 3] on the device, in the table's channel
 *                                 order (CLASS, DEPTH)
 *        MTT_RENDER_OUT_RGB3      uint8 [.., H, W, 3]: the three truncated components, reversed when swap_rb != 0 (NORMALS only)
 *        MTT_RENDER_OUT_F32       fp32 [.., H, W] (DEPTH only)
 *   4. the window: win == NULL writes the whole grid, image b at pixel offset b * H * W.  Otherwise win is int64 [B, 5] on the device,
 *      rows (y0, x0, H_out, W_out, offset): image b writes the pixels [y0, y0 + H_out) x [x0, x0 + W_out) of its grid, packed, starting
 *      at pixel `offset` of out.  win_host is the host copy, which the entry point validates: windows inside the grid, offsets
 *      non-negative, offset + H_out * W_out <= out_pixels (the capacity of out in pixels, checked without a window too).
 * Four pixels per thread along x (16-byte loads at equal size, one 4-, 12- or 16-byte store) when w, W, every window's x0, W_out and
 * offset are multiples of 4 and src / out are 16-byte aligned; otherwise one pixel per thread, any size and alignment.
 *
 * mtt_render_minmax  C == 1: per-image minimum and maximum of the interpolated, clamped map over the same pixels, as unsigned integer
 *   atomics on the bit patterns of the non-negative floats (exact, independent of order).  minmax uint32 [2, B]: row 0 the minima, row 1
 *   the maxima; the entry point initialises both before the launch. */
enum { MTT_RENDER_CLASS = 0, MTT_RENDER_SIGMOID255 = 1, MTT_RENDER_SOFTMAX1_255 = 2, MTT_RENDER_NORMALS = 3, MTT_RENDER_DEPTH = 4 };
enum { MTT_RENDER_OUT_U8 = 0, MTT_RENDER_OUT_LUT1 = 1, MTT_RENDER_OUT_LUT3 = 2, MTT_RENDER_OUT_RGB3 = 3, MTT_RENDER_OUT_F32 = 4 };
typedef struct {
  const float* src; void* out; const uint8_t* table;
  const int64_t* win; const int64_t* win_host;
  uint32_t* minmax;
  int64_t out_pixels;
  int32_t B, C, h, w, H, W;
  int32_t mode, out_kind, swap_rb;
} mtt_render_desc;
size_t mtt_render_desc_size(void);
int mtt_render_map(const mtt_render_desc* d, void* stream);
int mtt_render_minmax(const mtt_render_desc* d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MTT_HIP_H */
