/* libmmtg_hip.so -- C ABI of the MI355X (gfx950) kernels behind MMTG's
 * training + generation hot path.
 *
 * The reference (Aman-4-Real/MMTG) has no native layer: every operator on the
 * path is a stock PyTorch call inside src/model.py / src/loss.py /
 * src/generate.py.  Each entry point below therefore cites the reference
 * *operator call site(s)* it replaces (file:line into /root/reference/src).
 *
 * Conventions
 *   - plain pointers + sizes only; all pointers are DEVICE pointers unless
 *     stated; the caller owns every buffer (nothing is allocated, freed or
 *     retained across calls);
 *   - `dtype` selects the storage type of activations / weight copies:
 *     MMTG_F32 (exact fp32 MFMA, the parity-gate mode) or MMTG_BF16 (bf16
 *     storage, fp32 accumulate).  Statistics, losses, gradients of parameters
 *     and optimizer state are always fp32;
 *   - `stream` is a hipStream_t; every call is asynchronous and stream-ordered,
 *     performs no host synchronisation and is hipGraph-capturable;
 *   - return 0 on success, a negative MMTG_ERR_* otherwise; the message is
 *     available (thread-local) from mmtg_last_error().  Nothing throws/exits.
 */
#ifndef MMTG_HIP_H
#define MMTG_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define MMTG_ABI_VERSION 12

/* The library is built with -fvisibility=hidden: only the entry points below are exported. */
#define MMTG_API __attribute__((visibility("default")))

enum { MMTG_OK = 0, MMTG_ERR_BAD_ARG = -1, MMTG_ERR_HIP = -2, MMTG_ERR_UNSUPPORTED = -3 };
enum { MMTG_F32 = 0, MMTG_BF16 = 1 };

/* GEMM epilogues */
enum {
    MMTG_EPI_NONE = 0,   /* C = acc + bias                                    */
    MMTG_EPI_GELU = 1,   /* aux2 = acc + bias ; C = gelu_new(aux2)            */
    MMTG_EPI_TANH = 2,   /* C = tanh(acc + bias)                              */
    MMTG_EPI_RESID = 3,  /* C = dropout(acc + bias) + aux                     */
    MMTG_EPI_DGELU = 4,  /* C = acc * gelu_new'(aux) ; optional aux2 (f32 [ceil(M/64)][N]) <- column sums of C
                            per 64-row band; mmtg_colsum over the bands = the c_fc bias gradient, without a
                            pass over the [M,N] pre-activation gradient */
    MMTG_EPI_DTANH = 5,  /* C = acc * (1 - aux^2)                             */
    MMTG_EPI_ATOMIC = 6, /* C(f32) += alpha * acc  (atomics; split-K allowed) */
    MMTG_EPI_ROWDOT = 7, /* C = acc ; aux2(f32)[m, n/64] = sum over each 64-column group of C * aux
                            (attention backward's delta = rowsum(dO * O) per head, fused into the
                            GEMM that produces dO; N % 64 == 0, no bias) */
    MMTG_EPI_SPLIT = 8,  /* deterministic split-K for small M (decode): C is fp32 [splits][M][ldc]; K split s
                            stores its raw partial product in slab s (plain stores; out_f32, no bias);
                            mmtg_splitk_finish sums the slabs in order and applies bias / activation /
                            residual (/ LayerNorm) */
    MMTG_EPI_TANH_ADD = 9 /* C = tanh(acc + bias + aux[aux_rows[m]]) -- mmtg_gemm_gather only */
};
#define MMTG_GEMM_NO_TR 1 /* flags: gather K-strided bf16 fragments without ds_read_b64_tr_b16 */
#define MMTG_GEMM_REGSTAGE 2 /* flags: register-staged v1 pipeline instead of the LDS-DMA one (bf16) */
#define MMTG_GEMM_SKINNY 4    /* flags: force the 256x32-tile small-M configuration (bf16, transA=0,transB=1) */
#define MMTG_GEMM_NO_SKINNY 8 /* flags: never pick it automatically (it is the default for M <= 256) */
#define MMTG_GEMM_WIDE 16     /* flags: force 192x128 tiles / 6 waves (bf16, transA=0); chosen automatically when it
                                 saves a partial round of workgroups (N = 768) or for N >= 4096 */
#define MMTG_GEMM_NO_WIDE 32  /* flags: never pick 192x128 automatically */
#define MMTG_GEMM_PERSIST 64  /* flags: use the persistent pipelined 128x128 kernel (one workgroup per CU slot walks the
                                 (tile, K split) items, next item prefetched, epilogue deferred into it); opt-in:
                                 measured on par with the plain launch */
#define MMTG_GEMM_NO_PERSIST 128 /* flags: reserved (the persistent kernel is never picked automatically) */
#define MMTG_GEMM_ROW_ORDER 256  /* flags: keep the plain tile_n-fastest item order: no tile_m-fastest weight gradients, no
                                    column blocks for forward / dgrad products (A/B measurements) */
#define MMTG_GEMM_OCC4 512       /* flags: force the single-stage 128x128 kernel, four workgroups per CU (bf16); automatic for
                                    weight gradients and for forward / dgrad products of more than 2 x CUs tiles */
#define MMTG_GEMM_NO_OCC4 1024   /* flags: never pick it automatically (A/B measurements) */
#define MMTG_GEMM_NO_P8 8192     /* flags: never pick the eight-phase 256x256 / 192x256 kernel (bf16, transA = 0, transB = 1, K % 128 == 0: the
                                    default for M >= 1024, N >= 256) -- A/B measurements and bit-equality tests against the older kernels */
#define MMTG_GEMM_GELU_GRAD 32768 /* flags (round 3): MMTG_EPI_GELU stores gelu_new'(pre-activation) in aux2 instead of the pre-activation, and
                                    MMTG_EPI_DGELU multiplies by aux as it is (C = acc * aux): the backward then needs no transcendental --
                                    the only consumer of the saved pre-activation was gelu' (both products of a pair must carry the flag) */
#define MMTG_GEMM_P8 16384       /* flags: eight-phase kernel also for the dGELU product (otherwise on the single-stage kernel by measurement) */
#define MMTG_GEMM_AUX2_BF16 131072 /* flags (round 6, mmtg_gemm_x3 only): MMTG_EPI_GELU stores aux2 (the pre-activation) as bf16 rows [M, ldc] instead of
                                     fp32 -- the hybrid mode (compute_dtype "bf16x3f") runs its backward on the bf16 kernels */
#define MMTG_GEMM_P8_288 65536   /* flags (round 4): force the eight-phase kernel's 288-row tiles where it applies (the tile rule picks them by cost; tests / A-B) */
#define MMTG_GEMM_P256 4096      /* flags: persistent pipelined kernel with 256x128 tiles, 8 waves, one workgroup per CU (bf16, transA = 0) */
#define MMTG_GEMM_COL_BLOCK 2048 /* flags: force the column-blocked item order with blocks of two tile columns (test hook;
                                    automatic when the weights do not stay in an XCD's L2 over several sweeps) */

/* profiling categories (mmtg_prof_*) */
enum {
    MMTG_PROF_GEMM_BF16 = 0, MMTG_PROF_GEMM_F32, MMTG_PROF_ATTN_FWD, MMTG_PROF_ATTN_BWD,
    MMTG_PROF_LAYERNORM, MMTG_PROF_EMBED, MMTG_PROF_LOSS, MMTG_PROF_OPTIM, MMTG_PROF_ENCODER,
    MMTG_PROF_DECODE, MMTG_PROF_MISC, MMTG_PROF_NCAT
};

MMTG_API int mmtg_abi_version(void);
/* extra -D flags the library was compiled with ("" for the product build; diagnostic builds name theirs) */
MMTG_API const char* mmtg_build_flags(void);
MMTG_API const char* mmtg_last_error(void);

/* Live per-kernel timing with HIP events recorded on the launch stream.
 * enable(1) starts bracketing every launch; read() synchronises the recorded
 * events and returns, per category, launches / total ms / algorithmic flops /
 * algorithmic bytes (arrays of MMTG_PROF_NCAT), then clears the log. */
MMTG_API int mmtg_prof_enable(int on);
MMTG_API int mmtg_prof_read(int* launches, double* ms, double* flops, double* bytes);

/* ---------------------------------------------------------------- GEMM
 * C[M,N] = epi(opA[M,K] * opB[K,N]).  transA=0: A[m*lda+k]; 1: A[k*lda+m].
 * transB=0: B[k*ldb+n]; 1: B[n*ldb+k] (an nn.Linear weight [out,in]).
 * Replaces every nn.Linear / Conv1D / lm_head product on the path:
 * model.py:77 (topic_fc), :78-79 (GRU projections), :134-136 (alpha QKV),
 * :199 (out_linear), :279-281 (projector), and the c_attn / c_proj / c_fc /
 * lm_head products inside GPT2LMHeadModel (call sites model.py:282-288,
 * 320-326), plus their autograd backward products (train.py:193).           */
MMTG_API int mmtg_gemm(int dtype, int transA, int transB, int M, int N, int K,
              const void* A, long lda, const void* B, long ldb, void* C, long ldc,
              const float* bias, int epi, const void* aux, long ldaux, void* aux2,
              int out_f32, float alpha, int splits, unsigned drop_thresh, unsigned drop_seed,
              int flags, void* stream);

/* Split-precision ("bf16x3") product, round 5 -- the mode in which north_star's numeric gates (logits within 1e-3, greedy ids
 * bit-exact) hold at bf16 matrix-core speed.  Replaces the SAME fp32 products as mmtg_gemm (the Conv1D / Linear layers of GPT-2
 * behind model.py:282-288,320-326 and the tied lm_head) when both operands are K-contiguous:
 *   C[M, N] (fp32) = epi( A . B^T + bias ),   A [M, K], B [N, K] fp32 tensors handed over as (hi | lo) PLANE PAIRS of bf16
 *   (hi = bf16(x), lo = bf16(x - hi); the lo plane lies planeA / planeB ELEMENTS behind the hi plane, same leading dimension),
 *   computed as A_hi B_hi^T + A_lo B_hi^T + A_hi B_lo^T with fp32 accumulation in ONE kernel (a 3K-deep loop of the eight-phase
 *   kernel).  aux / aux2 / C are fp32 with the meanings of mmtg_gemm's epilogues NONE, GELU, TANH, RESID (+ dropout), DGELU
 *   (+ column sums), DTANH, ROWDOT.  `planes` (nullable; ld = ldp, lo plane plane_out elements behind) receives the epilogue's
 *   result as a plane pair for the next split-precision product; C may be NULL when only the planes are consumed.
 *   K % 128 == 0; N, lda, ldb, ldc, ldp % 8 == 0; every plane pair below 2 GiB.  Plane pairs come from mmtg_split_planes,
 *   mmtg_layernorm_fwd_x3, this function's `planes` output, and mmtg_adamw (weights).                                      */
MMTG_API int mmtg_gemm_x3(int M, int N, int K, const void* A, long lda, long planeA, const void* B, long ldb, long planeB,
                 float* C, long ldc, void* planes, long ldp, long plane_out, const float* bias, int epi,
                 const float* aux, long ldaux, void* aux2, unsigned drop_thresh, unsigned drop_seed, int flags, void* stream);
/* fp32 [rows, cols] (ld = lds) -> its (hi | lo) bf16 plane pair (ld = ldp, lo plane `plane` elements behind the hi plane). */
MMTG_API int mmtg_split_planes(const float* src, long lds, int rows, int cols, void* planes, long ldp, long plane, void* stream);
/* LayerNorm forward (fp32 rows in, statistics out as mmtg_layernorm_fwd) whose output goes straight to a plane pair: the
 * GPT-2 LayerNorms feed products only (ln_1 -> c_attn, ln_2 -> c_fc, ln_f -> lm_head), so the fp32 rows are never stored.
 * x_bf16 (nullable, round 6): also receives bf16(x) [rows, cols] -- the input rows as the bf16 LayerNorm backward reads them
 * (compute_dtype "bf16x3f": split-precision forward, bf16 backward). */
MMTG_API int mmtg_layernorm_fwd_x3(const float* x, void* planes, long ldp, long plane, const float* gamma, const float* beta,
                          float* mean, float* rstd, int rows, int cols, float eps, void* x_bf16, void* stream);

/* Products whose operand rows are GATHERED from a table by index -- the multi-modal conditioning front end of
 * GPT2_Decoder.forward (model.py:254-281) without materialising X[m] = E[id_m] + c[b, seg_m] (62 MB at B = 64):
 *   mode 0 (forward):  C[M, N] = epi( E[rows[m], :] . B[N, K]^T + bias [+ aux[aux_rows[m], :]] ), epi in {NONE, TANH, TANH_ADD}.
 *                      By linearity (E[id] + c) W1^T = E[id] W1^T + (c W1^T)[b, seg]: the caller computes the small product
 *                      c W1^T once ([B*S + 1, N], last row zero) and passes it as aux with aux_rows[m] = b*S + seg or B*S.
 *                      The table row of output row m enters the LDS-DMA as the lane's source offset.
 *   mode 1 (weight gradient):  slabs C[s][M, N] (fp32, MMTG_EPI_SPLIT layout) = A[k, M]^T . E[rows[k], :] over K split s
 *                      (A = d(pre-activation) [K = tokens, M], K-strided; the table rows of a K tile are looked up one tile ahead);
 *                      mmtg_slab_sum finishes it; the c-part of the gradient is the small product segment_sum(dA)^T . c.
 * bf16 only; K % 64 == 0 (mode 0); rows / aux_rows: int32 device arrays; E: [*, ldb_or_lda] row-major, below 2 GiB.        */
MMTG_API int mmtg_gemm_gather(int mode, int M, int N, int K, const void* A, long lda, const void* B, long ldb, void* C, long ldc,
                     const float* bias, int epi, const int* rows, int table_rows, const void* aux, long ldaux, const int* aux_rows,
                     int splits, void* stream);

/* Diagnostic timeline of the bf16 LDS-DMA GEMM kernels (tools/gemm_timeline.py): while `buf` is
 * non-null, wave 0 of workgroup w < max_wgs of every such launch writes 6 x u64 at buf + 48*w --
 * s_memrealtime (100 MHz) at kernel entry, after the first K tile has landed, at the end of the K
 * loop, at exit; the K tile count; the hardware id (XCC / SE / CU).  Null switches it off (default). */
MMTG_API int mmtg_gemm_trace(void* buf, int max_wgs);
/* CUs the tile-shape rule of the eight-phase kernel (one workgroup = one whole CU) may count on: 0 = all, > 0 = that many,
 * < 0 = all but that many.  A rule input only -- results never depend on it.  mmtg_amd.ddp reserves CUs for the RCCL kernels
 * that run beside the backward (replaces nothing in the reference: its nn.DataParallel, train.py:112-114, serialises). */
MMTG_API int mmtg_gemm_cu_budget(int cus);
/* Measurement hook (tools/ddp_contention.py; never on the product path): `workgroups` 256-thread workgroups that each hold
 * `lds_bytes` of LDS (163840 = a whole CU) and sleep for `usec` microseconds -- a stand-in for a collective's ring kernels holding
 * their CUs beside the backward, so that the CU reservation above can be priced on one GPU. */
MMTG_API int mmtg_debug_occupy(int workgroups, int lds_bytes, double usec, void* stream);

/* Second half of a MMTG_EPI_SPLIT product: out[m, :] = epi(sum_s part[s][m][:] + bias) in the storage type
 * (slabs summed in index order -> deterministic); epi in {NONE, GELU, TANH, RESID (+ aux)}.  With ln_out the
 * row just produced is also LayerNormed (gamma, beta, eps) into ln_out [M, N] -- in the KV-cached decode step
 * (generate.py:117-126 -> GPT2Block) this replaces the ln_1 / ln_2 / ln_f launches.  part: [splits][M][ldp].   */
MMTG_API int mmtg_splitk_finish(int dtype, const float* part, int splits, int M, int N, long ldp, const float* bias,
                       int epi, const void* aux, long ldaux, void* out, long ldo,
                       const float* ln_gamma, const float* ln_beta, void* ln_out, float eps, void* stream);

/* column sums: out[n] += sum_m X[m,n]  (bias gradients), X of `dtype`, out f32.  Round 4: summed in a FIXED order -- one workgroup
 * owns 64 columns and walks all the rows; inputs above 2048 rows go through row slices in `ws` first -- so the result is bit-identical
 * run to run (the round-1 kernel finished with fp32 atomics from ~1000 workgroups). */
MMTG_API long mmtg_colsum_ws(int M, int N);      /* workspace floats mmtg_colsum needs for M rows (0: none) */
MMTG_API int mmtg_colsum(int dtype, const void* X, long ldx, int M, int N, float* out, float* ws, long ws_floats, void* stream);
/* Round 6: many small ordered column sums in ONE launch -- out_i[c] += sum_{r < M_i} X_i[r * ldx_i + c], c < N_i, every item summed in
 * the order mmtg_colsum uses for the same rows (the same bits); fp32 rows, M_i <= 2048.  `items` is a HOST array (the items travel in
 * the kernel arguments, 64 per launch); the items of a call run concurrently, so no two may share output elements.  The backward of a GPT-2 block ends four such reductions (two LayerNorm second stages, the
 * dGELU bands, the attention kernels' bias rows: the bias / LayerNorm gradients autograd produces behind model.py:282-288) that nothing
 * reads before the optimizer: mmtg_layernorm_bwd_partial / MMTG_ATTN_DBIAS_ROWS leave them as partial rows, this call sums them.      */
typedef struct { const float* X; float* out; long ldx; int M; int N; } mmtg_colsum_item;
MMTG_API int mmtg_colsum_batch(const mmtg_colsum_item* items, int n, void* stream);

/* ---------------------------------------------------------------- LayerNorm
 * torch.nn.LayerNorm (model.py:380-382) and GPT-2's ln_1/ln_2/ln_f.          */
MMTG_API int mmtg_layernorm_fwd(int dtype, const void* x, void* y, const float* gamma, const float* beta,
                       float* mean, float* rstd, int rows, int cols, float eps, void* stream);
/* dx = LN'(dy) (+ dres if non-null); dgamma/dbeta accumulated (+=) in fp32.
 * Optional fused tail for the residual stream: dx_masked = dx * dropout_mask(drop_seed) (the
 * gradient entering the previous residual branch; null = not needed) and
 * dcolsum[c] += sum_rows dx_masked (that branch's bias gradient; without dx_masked: of dx).
 * ws: caller-owned scratch of >= mmtg_layernorm_bwd_ws(rows, cols) floats.     */
MMTG_API long mmtg_layernorm_bwd_ws(int rows, int cols);
MMTG_API int mmtg_layernorm_bwd(int dtype, const void* dy, const void* x, const float* gamma,
                       const float* mean, const float* rstd, const void* dres, void* dx,
                       float* dgamma, float* dbeta, int rows, int cols,
                       void* dx_masked, unsigned drop_thresh, unsigned drop_seed, float* dcolsum,
                       float* ws, long ws_floats, void* stream);
/* The first stage of mmtg_layernorm_bwd alone (round 6): dx (+ dx_masked) as above, and the partial rows ws[k][q][cols], k < *partial_rows
 * (host, out), q = 0: d gamma, 1: d beta, 2: column sums of dx_masked / dx when want_colsum -- to be summed by mmtg_colsum_batch
 * (X = ws + q * cols, ldx = 3 * cols, M = *partial_rows, N = cols): the same bits as the one-call form.  ws must stay untouched until then. */
MMTG_API int mmtg_layernorm_bwd_partial(int dtype, const void* dy, const void* x, const float* gamma,
                       const float* mean, const float* rstd, const void* dres, void* dx, int rows, int cols,
                       void* dx_masked, unsigned drop_thresh, unsigned drop_seed, int want_colsum,
                       float* ws, long ws_floats, int* partial_rows, void* stream);
/* x3 mode: mmtg_layernorm_bwd on fp32 rows whose dropout-masked input gradient (dx itself without dropout) goes to a (hi | lo) bf16
 * plane pair [rows, cols] (lo plane `plane` elements behind) instead of an fp32 tensor: only split-precision products read it. */
MMTG_API int mmtg_layernorm_bwd_x3(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                          const float* dres, float* dx, float* dgamma, float* dbeta, int rows, int cols,
                          void* dx_planes, long plane, unsigned drop_thresh, unsigned drop_seed, float* dcolsum,
                          float* ws, long ws_floats, void* stream);
/* ... and its first stage alone (as mmtg_layernorm_bwd_partial): the partial rows stay in ws for mmtg_colsum_batch */
MMTG_API int mmtg_layernorm_bwd_x3_partial(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                          const float* dres, float* dx, int rows, int cols, void* dx_planes, long plane,
                          unsigned drop_thresh, unsigned drop_seed, int want_colsum,
                          float* ws, long ws_floats, int* partial_rows, void* stream);

/* ---------------------------------------------------------------- causal self-attention
 * GPT2Attention._attn: softmax(QK^T/sqrt(dh) + causal + key padding) V with
 * attention dropout, heads merged (call sites model.py:282-288, 320-326).
 * qkv: [B*T, 3*D] rows = tokens, columns q|k|v with head h at h*dh (dh = 64);
 * keep: [B,T] int32 key mask (1 = attend); out: [B*T, D]; lse: [B,nH,T] f32.  */
MMTG_API int mmtg_attn_fwd(int dtype, const void* qkv, const int* keep, void* out, float* lse,
                  int B, int T, int nH, int dh, unsigned drop_thresh, unsigned drop_seed, void* stream);
/* x3 mode (round 5): causal attention of the fp32-storage split-precision mode on the bf16 matrix cores -- the tiled algorithm of
 * mmtg_attn_fwd / mmtg_attn_bwd with every product (Q K^T, P V, dO V^T, dO^T P, Q^T dS, dS K) as three passes over (hi | lo) splits;
 * P and dS are split in registers; softmax / masks / dropout in fp32 as the fp32 kernels (same dropout counter stream).
 * qkv [B*T, 3D] and dout [B*T, D] arrive as (hi | lo) bf16 plane pairs (lo planes qplane / doplane elements behind the hi planes:
 * what mmtg_gemm_x3 writes for c_attn / the c_proj dgrad); out fp32.  Forward: context rows to `out` (fp32: the backward's delta
 * reads them) AND, when out_planes is given, to a plane pair [B*T, D] (attn.c_proj's operand).  Backward: d(qkv) is written ONLY as
 * a plane pair [B*T, 3D] (lo plane dplane elements behind): the c_attn dgrad / weight gradient read nothing else.  dq32: fp32
 * scratch of dq32_floats >= ceil(T/128) * B*T * D floats (one [B*T, D] buffer per block of 128 keys: plain stores, summed in block
 * order by the finish kernel -- no atomics, bit-reproducible); delta: [B*T, nH] scratch; dbias
 * (nullable): [3D] += column sums of d(qkv), through dbias_ws (>= (B * ceil(T/128) + ceil(B*T/16)) * 3D floats); delta_ready != 0:
 * delta[m, h] = sum_d dout * out was filled by the caller (mmtg_gemm_x3's MMTG_EPI_ROWDOT epilogue does it for free).
 * Round 6: dbias == NULL with dbias_ws non-null leaves the partial bias rows UNSUMMED at the head of dbias_ws -- [B * ceil(T/128)][3D]
 * (k and v parts; the q part zero), then [ceil(B*T/16)][D] (the q part) -- for the caller's mmtg_colsum_batch (as two items with
 * disjoint output columns: [D, 3D) from the first rows, [0, D) from the second).                                                    */
MMTG_API int mmtg_attn_fwd_x3(const void* qkv_planes, long qplane, const int* keep, float* out, void* out_planes, long plane, float* lse,
                     int B, int T, int nH, int dh, unsigned drop_thresh, unsigned drop_seed, void* stream);
MMTG_API int mmtg_attn_bwd_x3(const void* qkv_planes, long qplane, const int* keep, const float* out, const void* dout_planes, long doplane,
                     const float* lse, float* delta,
                     int delta_ready, float* dq32, long dq32_floats, void* dqkv_planes, long dplane, float* dbias, float* dbias_ws,
                     long dbias_ws_floats, int B, int T, int nH, int dh, unsigned drop_thresh, unsigned drop_seed, void* stream);
/* delta: [B*T, nH] f32, delta[m,h] = sum_d dout[m,h,d] * out[m,h,d]: computed by the call, or --
 * delta_ready != 0 -- already filled by the caller (the GEMM producing dout with
 * MMTG_EPI_ROWDOT does it for free); dq32: [B*T, D] f32 scratch (zeroed by the call);
 * dqkv: [B*T, 3*D] output; dbias (optional): f32 [3*D] += column sums of dqkv as stored (the
 * c_attn bias gradient, from the workgroups that produce each head's columns); dbias_ws (optional
 * scratch, f32 [B * ceil(T / key block) + 44][3*D], key block = 256 bf16 / 128 f32): partial rows that the
 * call sums into dbias in a fixed order (the 44 spare rows: workspace of the tiled kernels' column sum of dQ) --
 * without it the workgroups use atomics on dbias (slower: contended, and not reproducible bit for bit).       */
/* diagnostic: per-wave timeline of the whole-head forward kernel (bf16, T <= 256): buf = u64 [B*nH*8][8]
 * (s_memrealtime at entry / loads issued / first chunk landed / long tile done / stored / exit, XCC id, valid) or NULL */
MMTG_API int mmtg_attn_trace(void* buf);
/* flags (round 6): MMTG_ATTN_ELEM_MASK -- the bf16 whole-head kernels (T <= 512) regenerate the attention-dropout mask of the tiled /
 * split-precision kernels (keep (q, k) iff hash(seed, ((b nH + h) T + q) T + k) >= drop_thresh, scale 1 / (1 - p) exactly) instead of
 * their own 12-bit word masks: the bf16x3f mode's backward then differentiates the mask its split-precision forward applied.        */
#define MMTG_ATTN_ELEM_MASK 1
/* MMTG_ATTN_DBIAS_ROWS (round 6) -- where mmtg_attn_bwd_dbias_rows(dtype, B, T) > 0 (the bf16 whole-head kernels) the c_attn bias
 * gradient is left as that many partial rows [rows, 3D] at the head of dbias_ws for the caller's mmtg_colsum_batch (dbias is then only
 * the request for them); other shapes ignore the flag and sum inside the call.                                                        */
#define MMTG_ATTN_DBIAS_ROWS 2
MMTG_API int mmtg_attn_bwd_dbias_rows(int dtype, int B, int T);
MMTG_API int mmtg_attn_bwd(int dtype, const void* qkv, const int* keep, const void* out, const void* dout,
                  const float* lse, float* delta, int delta_ready, float* dq32, void* dqkv, float* dbias, float* dbias_ws,
                  int B, int T, int nH, int dh, unsigned drop_thresh, unsigned drop_seed, int flags, void* stream);

/* ---------------------------------------------------------------- conditioning front end
 * WenLan lookup + experience add (model.py:254-268):
 *   x[b,t] = E[topic_ids[b,t]]                           t <  P
 *   x[b,P+p] = E[targets[b,p]] + (p/two_sents < S ? c[b,p/two_sents] : 0)
 * table [V,E], c [B,S,E], x [B,P+L,E] of `dtype`; ids int64.                  */
MMTG_API int mmtg_embed_condition(int dtype, const void* table, const long long* topic_ids,
                         const long long* targets, const void* c, void* x,
                         int B, int P, int L, int S, int E, int two_sents, int V, void* stream);
/* out[b,k,:] = sum_{p in segment k} g[b,P+p,:]   (backward of the add), out of `dtype` */
MMTG_API int mmtg_segment_sum(int dtype, const void* g, void* out, int B, int P, int L, int S, int H,
                     int two_sents, void* stream);
/* GPT-2 input embedding: h[m,:] = dropout(g[m,:] + wpe[m % T,:] + wte[type_ids[m],:])
 * (GPT2Model.forward via model.py:282-288).  In place on g allowed.           */
MMTG_API int mmtg_embed_add(int dtype, const void* g, const void* wpe, const void* wte, const long long* type_ids,
                   void* h, int M, int T, int D, unsigned drop_thresh, unsigned drop_seed, void* stream);
/* backward: dwpe[t,:] += sum_b dh[b,t,:]; dwte[type,:] += sum dh; (dh masked in place if dropout).  ws (optional, f32,
 * mmtg_embed_add_bwd_ws(M, D, ntypes) floats): per-row-block bins of the token-type rows, summed in a fixed order (round 4:
 * bit-reproducible); without it the bins end in fp32 atomics on dwte. */
MMTG_API long mmtg_embed_add_bwd_ws(int M, int D, int ntypes);
MMTG_API int mmtg_embed_add_bwd(int dtype, void* dh, const long long* type_ids, float* dwpe, float* dwte,
                       int M, int T, int D, int ntypes, unsigned drop_thresh, unsigned drop_seed, float* ws, long ws_floats,
                       void* stream);
/* elementwise dropout mask application (backward of a fused-epilogue dropout) */
MMTG_API int mmtg_dropout_apply(int dtype, const void* x, void* y, long n, int N, unsigned drop_thresh,
                       unsigned drop_seed, void* stream);

/* ---------------------------------------------------------------- LM head loss (loss.py:45-74 + GPT-2's internal CE)
 * logits: f32 [M, ldl] (columns >= V ignored).  labels per row t are
 * cat(topic_ids, targets)[b, t+1] (label_zero != 0: all labels 0, the
 * inference branch's dummy labels, model.py:314).  A label outside
 * [0, V) is clamped into the row (forward and backward alike): below 0
 * reads column 0, V or more reads column V - 1.  The logits in columns
 * below V must be finite: rows longer than 16384 are reduced with a running
 * (max, sum), and there an aligned run of eight -inf followed by a finite
 * slice turns the row's sum into NaN (training logits are an unmasked
 * product, so nothing masks them with -inf).
 * Outputs (all f32): nll[M] (0 on each sample's last row), lse[M],
 * sample_ce[B], coef[B] = d loss / d CE_b / n_tok / batch_denominator,
 * scalars[0] = MyLoss (sum_b l_b / batch_den), scalars[1] = GPT-2 LM loss.    */
MMTG_API int mmtg_loss_fwd(int logits_dtype, const void* logits, long ldl, int V, const long long* topic_ids,
                  const long long* targets, const long long* ratings, int stage, int label_zero,
                  int B, int P, int L, float batch_den, float* nll, float* lse, float* sample_ce,
                  float* coef, float* scalars, void* stream);
/* dlogits[m,v] = rc[m] * (softmax(logits[m])_v - [v == label]),
 * rc[m] = gscale * coef[b] on MyLoss rows (P <= t <= T-2) + lm_coef on GPT-2 LM-loss rows
 * (t <= T-2; pass d lm_loss / B / (T-1), 0 when the LM loss is unused as in train.py:188);
 * 0 on each sample's last row and on pad columns; dlogits of `dtype`, ld = ldd.  `logits_dtype` is the
 * storage type of the logits (fp32, or bf16 with bf16 dlogits -- then dlogits may alias logits). */
MMTG_API int mmtg_loss_bwd(int dtype, int logits_dtype, const void* logits, long ldl, int V, const long long* topic_ids,
                  const long long* targets, const float* lse, const float* coef, float gscale, float lm_coef,
                  int B, int P, int L, void* dlogits, long ldd, int Vpad, void* stream);
/* x3 mode: the same gradient of fp32 logits written as a (hi | lo) bf16 plane pair (ld = ldd, lo plane `plane` elements behind
 * the hi plane) -- the operand of the LM head's split-precision dgrad / weight gradient; the fp32 rows are never stored. */
MMTG_API int mmtg_loss_bwd_x3(const float* logits, long ldl, int V, const long long* topic_ids, const long long* targets, const float* lse,
                     const float* coef, float gscale, float lm_coef, int B, int P, int L, void* planes, long ldd, long plane,
                     int Vpad, void* stream);

/* ---------------------------------------------------------------- token-level unlikelihood on repeated lyric tokens
 * The training-time counterpart of the decoders' repetition controls: the unlikelihood term of Welleck et al., 2019 (fairseq's
 * unlikelihood_loss) next to the reference's per-sequence objective (loss.py:45-74; the term is added where train.py:191-192 form
 * the total loss).  Opt-in: MMTGTrainer(ul_weight=...).
 *
 * Notation as above: P topic columns, L lyric columns, Tt = P + L, row m = b * Tt + t.  The loss rows of a sample are
 * P <= t <= Tt - 2 (ntok = Tt - 1 - P of them); row t predicts targets[b, j], j = t + 1 - P; p_t(v) = exp(x[m, v] - lse[m]).
 *
 *   candidates  C(b, t) = the DISTINCT ids among targets[b, 0 .. j-1] that lie in [0, V), are not targets[b, j] (the label) and
 *               are not in the exclude list (a device array of at most 32 ids; the trainer's default is PAD and the ids the
 *               decoders ban, (0, 1, 2, 100, 102): they repeat by the slot format, not by the model's choice).  The topic prompt
 *               is not context; an id that occurs several times counts once.
 *   row term    ul_row[m] = sum over c in C of -log(q_c),  q_c = max(1 - p_t(c), MMTG_UL_FLOOR)
 *   weight      g_c = p_t(c) / (1 - p_t(c)) where 1 - p_t(c) >= MMTG_UL_FLOOR, else 0 (a clamped candidate carries no gradient);
 *               S[m] = sum over c of g_c
 *   sample      ul_sample[b] = (1 / ntok) * sum over the loss rows of ul_row;   ul = sum_b ul_sample[b] / batch_den
 *               (every sample takes part whatever its rating; rows t < P and each sample's last row carry none: 0)
 *   objective   MyLoss + alpha * KL (+ lm_weight * LM) + ul_weight * ul
 *   gradient    on a loss row, with u = ul_weight * gscale / (ntok * batch_den) and cf the row factor of mmtg_loss_bwd:
 *               d[m, v] = cf * (p_v - [v == label]) - (u * S[m]) * p_v + u * [v in C] * g_v
 *               (the first term is mmtg_loss_bwd's expression in its order: with u = 0 the same bits are written)
 * All sums run in a fixed order and nothing is accumulated with atomics: equal inputs give equal bits.                       */
#define MMTG_UL_FLOOR 1e-5f
#define MMTG_UL_MAX_EXCLUDE 32
#define MMTG_UL_MAX_L 1024     /* lyric columns the candidate search stages per row; a larger L is refused */
/* Forward of the term on the logits and the row lse of mmtg_loss_fwd (logits of `logits_dtype`, row stride ldl).
 * Outputs (f32): ul_row[M], ul_S[M] (both 0 outside the loss rows), ul_sample[B], ul[1].                                    */
MMTG_API int mmtg_loss_ul_fwd(int logits_dtype, const void* logits, long ldl, int V, const long long* targets, const float* lse,
                     const long long* exclude, int n_exclude, int B, int P, int L, float batch_den,
                     float* ul_row, float* ul_S, float* ul_sample, float* ul, void* stream);
/* mmtg_loss_bwd with the term's gradient folded in (ul_S from mmtg_loss_ul_fwd on the same logits, ul_coef = u above, finite
 * and >= 0): the same storage forms, zeros and in-place rule; the candidates' logits are read before the row is rewritten.   */
MMTG_API int mmtg_loss_bwd_ul(int dtype, int logits_dtype, const void* logits, long ldl, int V, const long long* topic_ids,
                     const long long* targets, const float* lse, const float* coef, float gscale, float lm_coef,
                     const float* ul_S, float ul_coef, const long long* exclude, int n_exclude,
                     int B, int P, int L, void* dlogits, long ldd, int Vpad, void* stream);
/* ... and mmtg_loss_bwd_x3 with it: the candidate columns are fixed up in the hi and the lo plane.                            */
MMTG_API int mmtg_loss_bwd_ul_x3(const float* logits, long ldl, int V, const long long* topic_ids, const long long* targets,
                        const float* lse, const float* coef, float gscale, float lm_coef, const float* ul_S, float ul_coef,
                        const long long* exclude, int n_exclude, int B, int P, int L, void* planes, long ldd, long plane,
                        int Vpad, void* stream);

/* ---------------------------------------------------------------- contrastive token loss on the last-layer states
 * The training-time counterpart of contrastive search (mmtg_decode_contrastive_sim reads the cosines between last-layer states;
 * this term shapes them): the margin loss of SimCTG (Su et al., 2022) on the output of ln_f, the operand of the LM head.
 * Opt-in: MMTGTrainer(cl_weight=..., cl_margin=...).
 *
 * Notation as above: P topic columns, L lyric columns, Tt = P + L, row m = b * Tt + t.  hf [M, D] is the output of ln_f (storage
 * type `dtype`, row stride ldh), keep the forward's int32 [B, Tt] attention mask (row stride ldkeep), rho the margin in (0, 1].
 *
 *   positions   I_b = { t in [P, Tt) : keep[b, t] != 0 },  n_b = |I_b|: the context mmtg_decode_contrastive_sim compares against --
 *               lyric columns, [#START#] / [#EOS#] included, PAD excluded, topic columns never.
 *   unit vector r_i = ||hf[b, i, :]||_2 in fp32 over the values as stored (widened exactly), rinv_i = 1 / r_i;
 *               u_i = h_i * rinv_i, the zero vector (rinv_i = 0) when r_i = 0.
 *   cosine      s_ij = (h_i . h_j) * (rinv_i * rinv_j): the dot accumulated in fp32 in one fixed k order, the two reciprocals
 *               multiplied first, so s_ij and s_ji are the same bits; s_ii is taken as exactly 1 and never computed.
 *   pair term   l_ij = max(0, rho - 1 + s_ij) for i != j in I_b;  activity a_ij = [rho - 1 + s_ij > 0] (strict).
 *   row         cl_row[m] = sum over j != i of l_ij  (0 on rows outside I_b)
 *   sample      cl_sample[b] = sum over i of cl_row / (n_b (n_b - 1))  (0 when n_b < 2)
 *   batch       cl = sum_b cl_sample[b] / batch_den   (every sample takes part whatever its rating, as in the unlikelihood term)
 *               The normalisation is PER SAMPLE, not SimCTG's batch-global pair count: a window of micro-batches, and a
 *               data-parallel shard, then equal the big batch.
 *   objective   MyLoss + alpha * KL (+ lm_weight * LM) (+ ul_weight * ul) + cl_weight * cl
 *   gradient    with c = cl_weight * gscale / batch_den (the `coef` argument):
 *               g_i = (2 / (n_b (n_b - 1))) * sum over j != i of a_ij u_j      (the 2: a_ij == a_ji, by the cosine's definition)
 *               d(hf)[m, :] += c * (g_i - (g_i . u_i) u_i) * rinv_i
 *               Rows outside I_b and rows with r_i = 0 keep their d(hf) bits.  The increment is formed at fp32 accuracy (u_j in
 *               fp32, the a x U product on the fp32 matrix cores in every storage form) and rounded once, when it is added.
 * All sums run in a fixed order and nothing is accumulated with atomics: equal inputs give equal bits.                       */
#define MMTG_CL_MAX_L 1024     /* lyric columns; a larger L is refused */
#define MMTG_CL_MAX_D 1024     /* D must be a multiple of 32 up to this (GPT-2-medium) */
/* Forward.  Outputs (f32): rinv[M] (0 outside I_b and on zero rows), cl_row[M], cl_sample[B], cl[1].  hf rows 16-byte aligned. */
MMTG_API int mmtg_cl_fwd(int dtype, const void* hf, long ldh, const int* keep, long ldkeep, float margin, int B, int P, int L, int D,
                     float batch_den, float* rinv, float* cl_row, float* cl_sample, float* cl, void* stream);
/* Backward: adds the increment into dhf IN PLACE (storage type out_dtype, row stride ldd; f32 -> f32, bf16 -> bf16 and
 * f32 -> bf16).  rinv from mmtg_cl_fwd on the same hf and keep; coef finite and >= 0 (0: no launch, the bits stay).          */
MMTG_API int mmtg_cl_bwd(int dtype, int out_dtype, const void* hf, long ldh, const int* keep, long ldkeep, const float* rinv,
                     float margin, float coef, int B, int P, int L, int D, void* dhf, long ldd, void* stream);

/* ---------------------------------------------------------------- encoder / fuser pieces
 * GRU cell (nn.GRU math, model.py:78-79): gi (row stride ld_gi), gh (row stride ld_gh >= 3H, or 0 = one
 * [3H] row for every b: at step 0, h_prev = 0, the recurrent product is just b_hh)
 * pre-activations (r|z|n), h_prev (row stride ld_hp; null = zeros) -> h (row
 * stride ld_h); saves r,z,n,ghn (each [B,H]) in `save` [4,B,H] f32.  The row
 * strides address one step of a batch-first [B,S,*] sequence in place.         */
MMTG_API int mmtg_gru_cell_fwd(int dtype, const void* gi, long ld_gi, const void* gh, long ld_gh, const void* h_prev, long ld_hp,
                      void* h, long ld_h, float* save, int B, int H, void* stream);
/* dh: total gradient wrt h_t (f32 [B,H]); outputs dgi (row stride ld_dgi), dgh [B,3H]
 * of `dtype`, dh_prev (f32 [B,H]) = dh * z (caller adds dgh * W_hh).           */
MMTG_API int mmtg_gru_cell_bwd(int dtype, const float* dh, const float* save, const void* h_prev, long ld_hp,
                      void* dgi, long ld_dgi, void* dgh, float* dh_prev, int B, int H, void* stream);
/* The same with the assembly of dh_t fused in: dh_t = rows[b, :] (gradient arriving through the LayerNorm of step t,
 * `dtype`, row stride ld_rows) + carry (f32 [B,H], nullable; may alias dh_prev) + the ordered sum of the `splits`
 * fp32 slabs part[splits][B][H] of the carry product d(gh_{t+1}) W_hh (MMTG_EPI_SPLIT; splits = 0: none).          */
MMTG_API int mmtg_gru_cell_bwd_fused(int dtype, const void* rows, long ld_rows, const float* carry, const float* part, int splits,
                            const float* save, const void* h_prev, long ld_hp, void* dgi, long ld_dgi, void* dgh,
                            float* dh_prev, int B, int H, void* stream);
/* The other recurrent cells MultiModalEncoder accepts (reference src/model.py:41-59: nn.RNN(nonlinearity="relu") / nn.LSTM).
 * Pre-activations a = gi + gh ([B, G*H] rows; G = 1 / 4, LSTM gate order i|f|g|o; ld_gh = 0: one bias row for every b).
 * LSTM: c_prev / c fp32 [B,H] (c_prev null = zeros), save [5,B,H] f32 = i, f, g, o, tanh(c);  ReLU cell: c_prev, c, save unused. */
#define MMTG_RNN_RELU 0
#define MMTG_RNN_LSTM 1
MMTG_API int mmtg_rnn_cell_fwd(int dtype, int kind, const void* gi, long ld_gi, const void* gh, long ld_gh, const float* c_prev,
                      void* h, long ld_h, float* c, float* save, int B, int H, void* stream);
/* One BPTT step: dh_t = rows[b, :] (`dtype`, row stride ld_rows) + part (f32 [B,H], nullable: d(a_{t+1}) W_hh) -> da (`dtype`,
 * [B, G*H] rows of stride ld_da; it is d(gi) and d(gh) at once).  LSTM: dc (f32 [B,H]) is read when dc_in != 0 (dc_{t+1} f_{t+1})
 * and rewritten with dc_t f_t; ReLU cell: h = the step's output rows (stride ld_h).                                              */
MMTG_API int mmtg_rnn_cell_bwd(int dtype, int kind, const void* rows, long ld_rows, const float* part, const float* save,
                      const float* c_prev, const void* h, long ld_h, float* dc, int dc_in, void* da, long ld_da,
                      int B, int H, void* stream);
/* alpha attention (model.py:138-161): qkv [B*S, 3H] -> ctx [B*S, H], probs [B,heads,S,S] f32,
 * kl += mean_i KLDiv_batchmean(log P[:,:,i,:], prior_i); prior [S,S] f32.       */
MMTG_API int mmtg_alpha_attn_fwd(int dtype, const void* qkv, const float* prior, void* ctx, float* probs,
                        float* kl, int B, int S, int H, int heads, void* stream);
MMTG_API int mmtg_alpha_attn_bwd(int dtype, const void* qkv, const float* prior, const float* probs,
                        const void* dctx, float dkl, void* dqkv, int B, int S, int H, int heads,
                        void* stream);
/* beta attention / multi-modal fuser (model.py:191-198): topic [B,H], img/txt [B*S,H] (row b*S+i)
 * att_w [S,H] f32, att_b [S] f32 -> o [B*S,H], a [B,S,3] f32.                   */
MMTG_API int mmtg_beta_fuse_fwd(int dtype, const void* topic, const void* img, const void* txt,
                       const float* att_w, const float* att_b, void* o, float* a,
                       int B, int S, int H, void* stream);
MMTG_API long mmtg_beta_fuse_bwd_ws(int B, int S, int H);
/* ws (optional, f32, mmtg_beta_fuse_bwd_ws floats): per-(b, step) contributions to d att_w / d att_b, summed over b in a fixed
 * order, d topic by its single owner (round 4: bit-reproducible); without it the round-1 fp32 atomics. */
MMTG_API int mmtg_beta_fuse_bwd(int dtype, const void* topic, const void* img, const void* txt,
                       const float* att_w, const float* a, const void* d_o,
                       float* dtopic, void* dimg, void* dtxt, float* datt_w, float* datt_b,
                       int B, int S, int H, float* ws, long ws_floats, void* stream);

/* Software prefetch (no counterpart in the reference): streams `bytes` of `src` through the cache hierarchy with
 * `workgroups` workgroups of 16-byte loads so that they sit in the 256 MB Infinity Cache when the next kernel of the
 * backward pass reads them (saved activations are cold by then).  Launched on a side stream, gated by events; `sink` is a
 * 4-byte device scratch that is never written in practice.                                                       */
MMTG_API int mmtg_prefetch(const void* src, long bytes, int workgroups, void* sink, void* stream);
/* zero n ranges of an fp32 buffer in one launch: desc (device, int64) holds (first element, count) pairs, both multiples of 4
 * (optimizer.zero_grad of train.py:192 for the gradients that are accumulated into; the rest is overwritten) */
MMTG_API int mmtg_zero_ranges(float* base, const long* desc, int n, void* stream);

/* ---------------------------------------------------------------- optimizer (train.py:194-197)
 * sumsq: *out = sum x^2 (global grad-norm), one partial per workgroup in `ws` (mmtg_sumsq_ws(n) floats) + an ordered final sum:
 * bit-reproducible (round 4; the round-1 kernel added ~2000 partials to *out with fp32 atomics).                          */
MMTG_API long mmtg_sumsq_ws(long n);
MMTG_API int mmtg_sumsq(const float* x, long n, float* out, float* ws, long ws_floats, void* stream);
/* clip (coef = min(1, max_norm / (sqrt(*normsq) + 1e-6))) + transformers.AdamW
 * (bias-corrected, eps outside the sqrt, decoupled wd) + optional bf16 copy.
 * count (optional, device scalar): g holds a SUM over rows and *count the global row count
 * (all-reduced on the device, never read by the host): the gradient is g * grad_scale / *count;
 * a *count that is not greater than 0 (0, negative, NaN) skips the step: p, m, v and both copies keep
 * every bit (the reference skips an empty batch, train.py:184-185). */
/* p_lo (nullable; with p_bf16): the x3 mode's lo plane, bf16(p - bf16(p)) -- p_bf16 / p_lo are then the weights' plane pair. */
MMTG_API int mmtg_adamw(float* p, const float* g, float* m, float* v, void* p_bf16, void* p_lo, long n,
               float lr, float beta1, float beta2, float eps, float wd, int step,
               const float* normsq, float max_norm, float grad_scale, const float* count, void* stream);
/* ---- parameter groups: frozen tensors, per-group learning rate and decay over the same flat buffers.
 * A table of nsegs (begin, end, group) triples of int64, sorted, disjoint, non-empty, inside [0, n): elements outside every
 * segment (alignment gaps, pads) and elements of frozen groups are neither read nor written by the two launch entries.
 * mmtg_param_groups_check validates a host table (1 <= ngroups <= MMTG_MAX_PARAM_GROUPS, 0 <= nsegs <= MMTG_MAX_PARAM_SEGS)
 * without any device call; the launch entries run the same checks on segs_host (the host copy of the device table segs_dev,
 * which is built once and stays in device memory) before they launch.                                                     */
#define MMTG_MAX_PARAM_GROUPS 16
#define MMTG_MAX_PARAM_SEGS 1024
typedef struct { float lr_scale; float weight_decay; int frozen; int pad; } mmtg_param_group;
MMTG_API int mmtg_param_groups_check(const long* segs, int nsegs, int ngroups, long n);
/* out[g] = sum x^2 over group g's segments (0 for a group whose bit is set in frozen_mask, or without segments),
 * out[ngroups] = the non-frozen groups' values added in group order: the clip norm of the trainable tensors.  Written, not
 * accumulated; one partial per workgroup and group in `ws` (mmtg_sumsq_groups_ws(n, ngroups) floats) + an ordered final sum:
 * no atomics, equal bits call after call.                                                                                */
MMTG_API long mmtg_sumsq_groups_ws(long n, int ngroups);
MMTG_API int mmtg_sumsq_groups(const float* x, long n, const long* segs_dev, const long* segs_host, int nsegs, int ngroups,
               unsigned frozen_mask, float* out, float* ws, long ws_floats, void* stream);
/* mmtg_adamw per group: every element of a non-frozen group g gets the bits mmtg_adamw gives it when called with
 * lr = (float)((double)lr * (double)groups[g].lr_scale) and wd = groups[g].weight_decay (same clip coefficient, count rule
 * and planes).  `groups` is a host array of ngroups records, handed to the kernel by value.                               */
MMTG_API int mmtg_adamw_groups(float* p, const float* g, float* m, float* v, void* p_bf16, void* p_lo, long n,
               const long* segs_dev, const long* segs_host, int nsegs, const mmtg_param_group* groups, int ngroups,
               float lr, float beta1, float beta2, float eps, int step,
               const float* normsq, float max_norm, float grad_scale, const float* count, void* stream);
/* ---- weight averaging: an exponential moving average of the flat parameter buffer.
 * ema[i] = fmaf(w, p[i] - ema[i], ema[i]) with w = 1 - decay in [0, 1]: the difference is rounded once and the multiply-add once,
 * on the 16-byte path and the scalar path alike (equal bits whatever the alignment), and p[i] == ema[i] gives ema[i] back bit for
 * bit -- frozen tensors, pads and gaps keep tracking p without a segment table.  (One select on top of the expression: a result
 * that compares equal to ema[i] is ema[i], so that an ema[i] of -0, which the multiply-add would return as +0, keeps its sign;
 * w = 0 therefore keeps every bit too.)  count (nullable): mmtg_adamw's device scalar; a
 * *count that is not greater than 0 (0, negative, NaN) leaves every bit of ema, as it left every bit of p.  The two ranges must
 * not overlap.                                                                                                             */
MMTG_API int mmtg_ema_update(float* ema, const float* p, long n, float w, const float* count, void* stream);
/* a[0:n] <-> b[0:n], moved as 32-bit words (NaN payloads and -0 survive); the two ranges must not overlap */
MMTG_API int mmtg_swap_f32(float* a, float* b, long n, void* stream);
MMTG_API int mmtg_cast_f32_to(int dtype, const float* src, void* dst, long n, void* stream);
/* dst[r, 0:cols] = cast(src[r, 0:cols]); dst[r, cols:ldd] = 0 */
MMTG_API int mmtg_cast_pad_rows(int dtype, const float* src, long lds_, void* dst, long ldd, int rows, int cols, void* stream);
MMTG_API int mmtg_cast_to_f32(int dtype, const void* src, float* dst, long n, void* stream);
MMTG_API int mmtg_axpy_f32(float* y, const float* x, float a, long n, void* stream);
/* Second half of a weight-gradient product computed as K-split slabs (mmtg_gemm with transA = 1 and
 * MMTG_EPI_SPLIT: slab s = fp32 [M, ldc] at C + s * M * ldc): dst[i] (+)= sum_s part[s * stride + i],
 * slabs added in order -- the deterministic replacement of the fp32-atomic epilogue for the autograd
 * weight gradients of nn.Linear / Conv1D (model.py:77-79,134-136,199,279-281 and the GPT-2 products).
 * Slab producers: the bf16 single-stage LDS-DMA kernel and (round 6) the exact-fp32 kernel.
 * n and stride in floats, multiples of 4; accumulate = 0 overwrites dst.                              */
MMTG_API int mmtg_slab_sum(const float* part, int splits, long stride, float* dst, int accumulate, long n, void* stream);
/* Grouped weight-gradient products with an in-kernel deterministic split-K reduction (csrc/wgrad.hip): ONE launch for
 * the n <= 8 products  C_p[M_p, N_p] (fp32, ld = ldc_p) (+)= A_p^T . B_p,  A_p [K, lda_p], B_p [K, ldb_p] bf16 row-major with
 * K = tokens -- the autograd weight gradients of the four Conv1D layers of a GPT-2 block (transformers 4.12.3 behind
 * model.py:282-288), which become available within one block of the backward and otherwise need 5-12 K splits EACH to fill
 * the chip.  Work items = (sum of 128x128 tiles) x splits.  K split s of a tile stores its raw partial tile in slot
 * (tile, s) of `ws` (tile-contiguous, >= tiles * splits * 16384 floats); every wave then bumps the arrival counter of
 * its 64x64 quadrant (`counters`: >= 4 * tiles unsigned, ZERO on entry, zero again on return) and the wave that arrives
 * last adds the partial quadrants in split order and writes (accumulate = 0) or adds to (accumulate = 1) C.  No workgroup
 * ever waits for another; results are bit-reproducible.  splits = 1 needs neither ws nor counters.
 * `probs` is a HOST array (read during the call).  M, N, lda, ldb multiples of 8; operands below 2 GiB.
 * config 0: 128x128 tiles, four 256-thread workgroups per CU (any shape; 16384 floats and 4 counters per tile and split);
 * config 1: 256x256 tiles on the eight-phase K-strided main loop, one 512-thread workgroup per CU (65536 floats and 8
 *           counters per tile and split; K slices are multiples of 128).
 * config 2 (round 5, the split-precision mode; 128x128 tiles): A_p and B_p are (hi | lo) bf16 plane pairs of fp32 tensors -- the
 *           lo plane planeA / planeB ELEMENTS behind the hi plane -- and every K slice is walked three times,
 *           A_hi^T B_hi + A_lo^T B_hi + A_hi^T B_lo (see mmtg_gemm_x3); planeA / planeB are ignored otherwise.
 * config 6 (= 2 | 4): the same products on combined stages -- a 64 KB stage holds the K tile of all four planes and every fragment
 *           pair feeds the three MFMA passes (two workgroups per CU; a third fewer bytes through the L2 -> LDS port).
 * config 8: 256x256 tiles, ONE 1024-thread workgroup per CU (sixteen waves, a 64x64 quadrant each) over a ring of three 32-k
 *           stages (96 KB of LDS), two stages in flight while one is read (65536 floats and 16 counters per tile and split; K
 *           slices are multiples of 64).  Same summation order per element as config 0: bit-equal to it at an equal split
 *           count.  (bf16 operands only: not combined with 2 / 4.)
 * Every other value of config is refused, 4 without 2 (alone or beside 1 / 8) included.                                      */
typedef struct mmtg_wgrad_problem {
    const void* A; long lda;
    const void* B; long ldb;
    float* C; long ldc;
    int M, N;
    long planeA, planeB;
} mmtg_wgrad_problem;
MMTG_API int mmtg_wgrad_group(int config, int n, const mmtg_wgrad_problem* probs, int K, int splits, float* ws, long ws_floats,
                     unsigned* counters, long n_counters, int accumulate, void* stream);
/* Batched transpose (bf16 mode keeps K-contiguous [out,in] copies of GPT-2's Conv1D [in,out] weights
 * so that forward products run in the NT layout): matrix i = [rows, cols] row-major at src + desc[4i]
 * elements -> [cols, rows] at dst + desc[4i+3]; desc = n x {src_off, rows, cols, dst_off} (long, device);
 * every offset / extent a multiple of 16 bytes; max_rows / max_cols bound the grid.                    */
MMTG_API int mmtg_transpose_batch(int dtype, const void* src, void* dst, const long* desc, int n, int max_rows, int max_cols, void* stream);

/* ---------------------------------------------------------------- generation (generate.py:127-141)
 * per row: repetition penalty per occurrence (ids 0 and 102 skipped), /temperature,
 * ban {1,2,100,102}, sticky PAD, arg-max (lowest index on ties) -> next[B].     */
MMTG_API int mmtg_logits_process_argmax(const float* logits, long ldl, int V, const long long* generated,
                               long ldg, const int* gen_len, float temperature, float rep_penalty,
                               long long* next, int B, void* stream);
/* Stochastic counterpart (generate.py:64-94,127-141 with top_k / top_p as given): same processed logits, then the
 * reference's top-k filter (values below the k-th largest dropped, ties kept; 0 = off) and nucleus filter (sorted
 * descending, an id stays while the probability mass before it is <= top_p; 0 = off), softmax, and ONE draw per row
 * by inverse CDF over the kept ids in index order with the caller's uniforms[b] in [0,1) (torch.multinomial's
 * generator is not reproducible outside torch; the distribution is the reference's).  filtered (nullable, [B, ldl]):
 * the filtered processed logits (-inf where dropped), as top_k_top_p_filtering returns them.                        */
MMTG_API int mmtg_logits_process_sample(const float* logits, long ldl, int V, const long long* generated, long ldg,
                               const int* gen_len, float temperature, float rep_penalty, int top_k, float top_p,
                               const float* uniforms, long long* next, float* filtered, int B, void* stream);
/* The same with four more truncation stages between the nucleus filter and the draw (transformers' MinPLogitsWarper,
 * TypicalLogitsWarper, EpsilonLogitsWarper and EtaLogitsWarper with min_tokens_to_keep = 1, in generate's warper order).  The reference
 * has none of them (generate.py:64-94).  Each stage sees the softmax p over the survivors of everything before it (a dropped id has
 * p = 0); pmax is p's largest value, H = -sum p log p with 0 log 0 = 0, and "the maximum" is the largest surviving logit:
 *   min_p (0 = off, in [0, 1]):           drop ids with p < min_p * pmax.
 *   typical_p (1 = off, in (0, 1]):       key = |-log p - H|; walk the survivors by ascending key accumulating p; keep every id whose
 *                                         key is at most the key of the first id at which the mass reaches typical_p (ids tied at that
 *                                         key stay; if the mass is never reached in floating point every survivor stays; p = 0 has key
 *                                         +inf and is never kept).  The most probable id may go.
 *   epsilon_cutoff (0 = off, in [0, 1)):  drop ids with p < epsilon_cutoff, but never the ids that hold the maximum.
 *   eta_cutoff (0 = off, in [0, 1)):      eta = min(eta_cutoff, sqrt(eta_cutoff) * exp(-H)); drop ids with p < eta, but never the ids
 *                                         that hold the maximum.
 * No stage empties a row.  The draw is mmtg_logits_process_sample's, over the kept ids.  fp32 throughout: a kept set can differ from
 * an exact evaluation only at an id within rounding of a stage's cut.  With all four off the result is mmtg_logits_process_sample's
 * (from a kernel of its own: that entry's kernel is unchanged).  A value outside its range fails before any device call.           */
MMTG_API int mmtg_logits_process_sample_warp(const float* logits, long ldl, int V, const long long* generated, long ldg,
                               const int* gen_len, float temperature, float rep_penalty, int top_k, float top_p, float min_p,
                               float typical_p, float epsilon_cutoff, float eta_cutoff, const float* uniforms, long long* next,
                               float* filtered, int B, void* stream);
/* The same with Mirostat (Basu et al. 2021, version 2, llama.cpp's `mirostat = 2`) as the last stage, behind top-k, top-p, min-p,
 * typical, epsilon and eta: a cut that adapts after every draw so that the observed surprise of the text stays near mirostat_tau bits
 * per token.  The state is mu[b], one fp32 per row, in bits; the caller starts it at 2 * mirostat_tau.  On a row that draws, with S
 * the survivors of every earlier stage and p the softmax over S:
 *   1. keep v in S when -log2 p(v) <= mu[b], and every id that holds S's largest logit (so no row is emptied);
 *   2. q = softmax over the kept ids; draw x by inverse CDF over the kept ids in index order with uniforms[b];
 *   3. s = -log2 q(x);  mu[b] <- mu[b] - mirostat_eta * (s - mirostat_tau).
 * llama.cpp keeps only the first id of its sorted list when mu lies below every surprise; this rule keeps every id tied at the
 * maximum.  The two differ only on an exact tie at the top.  Version 1 (a Zipf exponent estimate) is not built.
 * mirostat_tau in (0, 32], mirostat_eta in [0, 1] (0 freezes mu: the stage is then epsilon_cutoff = 2^-mu sampling); mu [B] is read and
 * written and required; surprise (nullable, [B]) receives the step's s.  A sticky-PAD row writes next = 0 and surprise = 0 and leaves
 * mu alone.  A value outside its range fails before any device call.  fp32 throughout: the mass and the scan's total come from
 * fixed-order reductions, so with top_p and typical_p off the mu trajectory is reproducible bit for bit.  A kernel of its own.  */
MMTG_API int mmtg_logits_process_sample_mirostat(const float* logits, long ldl, int V, const long long* generated, long ldg,
                               const int* gen_len, float temperature, float rep_penalty, int top_k, float top_p, float min_p,
                               float typical_p, float epsilon_cutoff, float eta_cutoff, const float* uniforms, long long* next,
                               float* filtered, int B, float mirostat_tau, float mirostat_eta, float* mu, float* surprise,
                               void* stream);

/* ---------------------------------------------------------------- KV-cached decode step (generate.py:117-142)
 * Batched, lock-step: every row is at position *pos_ptr (a DEVICE int, so a captured hipGraph of
 * the step replays for every position).  seq[B, ldseq] = prompt ids (0..P-1) then lyric ids.
 * decode_embed: x[b] = E[seq[b,pos]] (+ c[b,(pos-P)/two_sents]) and the inference-branch type id /
 *   key mask of the token (model.py:296-312): type_out[b], keep[b,pos].
 * decode_embed_add: h = g + wpe[pos] + wte[type].
 * decode_attn: appends the token's K/V to the caches [B,nH,Tmax,64] and attends over keys 0..pos.
 * decode_select: next lyric token = forced [#EOS#]/[#START#] by the 22-slot cadence, sticky PAD, or
 *   arg-max of the processed logits (null logits: forced tokens only); writes seq[b, pos+1].
 * decode_advance: *pos_ptr += 1.                                                              */
MMTG_API int mmtg_decode_embed(int dtype, const void* table, const long long* seq, long ldseq, const void* c, void* x,
                      const int* pos_ptr, const long long* tpw_type, const long long* tpw_mask,
                      long long* type_out, int* keep, long ldkeep, int B, int P, int S, int E, int two_sents,
                      int V, int sent, int max_sent_num, void* stream);
/* stats (optional, f32 [B][32][2]): the LayerNorm statistics (sum, sum of squares) of every row of h as stored, in partial 0
 * (partials 1..31 zeroed) -- the input of the first LN-fold product of the fused decode step (mmtg_decode_gemm).          */
MMTG_API int mmtg_decode_embed_add(int dtype, const void* g, const void* wpe, const void* wte, const long long* type_ids,
                          const int* pos_ptr, void* h, int B, int D, float* stats, void* stream);
/* Round 3: the decode step's batch-sized products with the row-wise glue fused in (bf16; A [M, lda], W [N, ldw] K-contiguous;
 * 64 x 64 tiles; replaces the products + mmtg_splitk_finish launches behind generate.py:124's per-token model call):
 *   mode 0 "LN-fold"        C = act( rstd_m (A W^T - mu_m colsum_n) + bias_n ), act in {MMTG_EPI_NONE, MMTG_EPI_GELU}; C bf16
 *                           [M, ldc] or fp32 (out_f32).  W = the gamma-folded weight copy, colsum / bias = its column sums and
 *                           folded bias (mmtg_ln_fold_weights); mu_m / rstd_m from stats_in.
 *   mode 1 "LN-fold slabs"  split-K: C = fp32 [splits][M][ldc], slab s = rstd_m (A_s W_s^T) - [s == 0] rstd_m mu_m colsum_n
 *                           (the bias is left to the consumer, mmtg_decode_attn_split).
 *   mode 2 "reduce"         split-K reduced IN the kernel by the last-arriving wave of every 32 x 32 wave tile (partials in
 *                           `ws`: >= tiles * splits * 4096 floats; `counters`: >= 4 * tiles, zero on entry and on return):
 *                           C (bf16) = sum_s partial_s + bias + resid, and stats_out[m][n / 32] = (sum, sum of squares) of the
 *                           stored row segment -- the LayerNorm statistics of the new residual stream as 32-column partials.
 *                           With type_ids != null the residual is the GPT-2 input embedding instead of a tensor:
 *                           emb_pos[*pos_ptr][n] + emb_type[type_ids[m]][n] (rows of stride ldr; resid = null) -- projector_layer2
 *                           and model.py:282-288's position / token-type embedding add in one launch.
 * stats_in / stats_out: f32 [M][32][2] (N <= 1024 in mode 2); np_in = partials to add (1 after mmtg_decode_embed_add, N / 32 after a mode-2 product).  */
MMTG_API int mmtg_decode_gemm(int mode, int M, int N, int K, const void* A, long lda, const void* W, long ldw, void* C, long ldc,
                     const float* bias, const float* colsum, const float* stats_in, int np_in, float eps, int act, int out_f32,
                     const void* resid, long ldr, float* stats_out, int splits, float* ws, long ws_floats, unsigned* counters,
                     long n_counters, const void* emb_pos, const void* emb_type, const long long* type_ids, const int* pos_ptr,
                     void* stream);
/* ---- split-precision ("bf16x3") token step, round 5.  The products of the decode step on (hi | lo) bf16 plane pairs of fp32 tensors
 * (three passes A_hi W_hi + A_lo W_hi + A_hi W_lo, fp32 accumulate; see mmtg_gemm_x3): fp32 residual stream, fp32 KV cache, fp32
 * logits -- greedy ids equal to the reference's fp32 loop (generate.py:117-142) at a multiple of the exact-fp32 kernels' speed.
 * mmtg_decode_gemm_x3: the three modes of mmtg_decode_gemm with A [M, K] / W [N, K] as plane pairs (lo plane planeA / planeW elements
 *   behind), K % 64 == 0.  mode 0: fp32 rows C (the logits) OR the activation as a plane pair Cp (ld = ldcp, lo plane planeC elements
 *   behind); mode 1: fp32 slabs C [splits][M][ldc]; mode 2: v = act(sum + bias) + residual with act in {NONE, TANH}, residual = resid
 *   (fp32, nullable) or wpe[*pos] + wte[type_ids[m]] (fp32 tables), written as fp32 rows C and / or a plane pair Cp, + the row
 *   statistics of v (stats_out nullable).
 * mmtg_ln_fold_weights_x3: W' = gamma (.) W re-split into a plane pair, colsum[n] = sum_k W'[n, k], bias_f = bias + beta W.
 * mmtg_decode_attn_split_x3: mmtg_decode_attn_split on an fp32 KV cache, the context rows written as a plane pair.
 * mmtg_decode_embed_x3: mmtg_decode_embed on the fp32 table / experience vectors, x written as a plane pair.                         */
MMTG_API int mmtg_decode_gemm_x3(int mode, int M, int N, int K, const void* A, long lda, long planeA, const void* W, long ldw, long planeW,
                        float* C, long ldc, void* Cp, long ldcp, long planeC, const float* bias, const float* colsum,
                        const float* stats_in, int np_in, float eps, int act, const float* resid, long ldr, float* stats_out,
                        int splits, float* ws, long ws_floats, unsigned* counters, long n_counters, const float* emb_pos,
                        const float* emb_type, const long long* type_ids, const int* pos_ptr, void* stream);
MMTG_API int mmtg_ln_fold_weights_x3(const void* W, long ldw, long planeW, const float* gamma, const float* beta, const float* bias,
                            void* Wf, long ldf, long planeF, float* colsum, float* bias_f, int N, int K, void* stream);
MMTG_API int mmtg_decode_attn_split_x3(const float* part, int splits, const float* bias, float* kcache, float* vcache, const int* keep,
                              long ldkeep, const int* pos_ptr, void* out_planes, long plane, int B, int nH, int dh, int Tmax, void* stream);
MMTG_API int mmtg_decode_embed_x3(const float* table, const long long* seq, long ldseq, const float* c, void* x_planes, long plane,
                         const int* pos_ptr, const long long* tpw_type, const long long* tpw_mask, long long* type_out, int* keep,
                         long ldkeep, int B, int P, int S, int E, int two_sents, int V, int sent, int max_sent_num, void* stream);

/* Wf[n, k] = gamma[k] W[n, k] (bf16), colsum[n] = sum_k Wf[n, k], bias_f[n] = bias[n] + sum_k beta[k] W[n, k]: the operands of the
 * LN-fold products, LN(x) W^T + b = rstd (x Wf^T - mu colsum) + bias_f.  W: [N, ldw] bf16 K-contiguous; bias may be null.   */
MMTG_API int mmtg_ln_fold_weights(const void* W, long ldw, const float* gamma, const float* beta, const float* bias, void* Wf,
                         float* colsum, float* bias_f, int N, int K, void* stream);
/* qkv [B, 3 * nH * 64]: the token's q | k | v.  k and v are stored into slot *pos_ptr of kcache / vcache [B, nH, Tmax, 64]; out [B, nH * 64]
 * = softmax(q . K / 8) V over the slots 0 .. *pos_ptr whose keep[b, slot] is non-zero (keep: int32, row stride ldkeep).  No slot above
 * *pos_ptr is read, nor (at *pos_ptr >= 1) slot *pos_ptr itself before it is written.
 * Cache contents (a condition on the caller, for this entry and every mmtg_decode_attn_split* form): every slot at or below
 * max(*pos_ptr - 1, 0) of both caches must hold FINITE values, whether its key is masked or not -- a masked key's value row is not
 * skipped but weighted with an exact zero, and at *pos_ptr = 0 the old contents of slot 0 are read the same way before the token's
 * own row replaces them.  A NaN or infinity there reaches the output (0 * NaN).  Caches allocated zeroed satisfy it.            */
MMTG_API int mmtg_decode_attn(int dtype, const void* qkv, void* kcache, void* vcache, const int* keep, long ldkeep,
                     const int* pos_ptr, void* out, int B, int nH, int dh, int Tmax, void* stream);
/* the same, taking the c_attn product as MMTG_EPI_SPLIT slabs (part: f32 [splits][B][3*D]) plus its bias:
 * the slabs are summed in order and rounded to the storage type as mmtg_splitk_finish would (one launch less) */
MMTG_API int mmtg_decode_attn_split(int dtype, const float* part, int splits, const float* bias, void* kcache, void* vcache,
                           const int* keep, long ldkeep, const int* pos_ptr, void* out, int B, int nH, int dh, int Tmax,
                           void* stream);
/* pos_next (optional, must not alias pos_ptr): receives *pos_ptr + 1 -- the decoder keeps the position in a PAIR of slots
 * and alternates them step by step (every kernel of a step reads one slot, this last kernel writes the other), which removes
 * the one-thread mmtg_decode_advance launch from the captured step.                                                        */
MMTG_API int mmtg_decode_select(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                       int P, int sent, float temperature, float rep_penalty, int B, int* pos_next, void* stream);
/* decode_select with the stochastic selection above; the draw of position pos uses uniforms[pos * ldu + b]
 * (a [positions, ldu] device array filled before the graph is replayed).                                    */
MMTG_API int mmtg_decode_sample(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                       int P, int sent, float temperature, float rep_penalty, int top_k, float top_p,
                       const float* uniforms, long ldu, int B, int* pos_next, void* stream);
MMTG_API int mmtg_decode_advance(int* pos_ptr, void* stream);

/* ---- beam search on the decode step (BeamDecoder, mmtg_amd/decode.py).  Rows b0 .. b0 + nb - 1 are the nb (1..16) beams of prompt
 * b0 / nb.  rows: the ancestry table, int32 [B, ldrows >= Tmax]: rows[b, j] = the batch row whose cache slot j holds position j's
 * K / V for beam b (only ever pointing backwards: a slot is written once, by the row that sits there at that step).
 * mmtg_decode_attn_split_rows / mmtg_decode_attn_split_x3_rows: mmtg_decode_attn_split / mmtg_decode_attn_split_x3 with the keys
 *   j < pos read from cache row rows[b, j] (the token's own K / V still go to row b, slot pos).
 * mmtg_decode_beam_candidates: per row, the processed logits x of mmtg_decode_select (cut at V) and the row's nb best
 *   (log_softmax(x)[v] in fp32, v) by x descending, then v ascending, into cand_val / cand_id [B, nb]; a row whose last token is
 *   PAD offers (0, PAD) then -inf; nothing is written at forced positions.
 * mmtg_decode_beam_merge: per prompt, candidate (p, k) scores scores[b0 + p] + cand_val[b0 + p, k]; the nb best by (score
 *   descending, p ascending, k ascending) become beams 0 .. nb - 1: their rows of seq / keep / rows are reordered in place,
 *   seq[b, pos + 1] = the token, scores[b] = the score, rows[b, pos + 1] = b; forced positions (or cand_val = null) keep every
 *   beam and append the forced token.  pos_next as in mmtg_decode_select.  nb outside 1..16 fails before any device call.  */
MMTG_API int mmtg_decode_attn_split_rows(int dtype, const float* part, int splits, const float* bias, void* kcache, void* vcache,
                                const int* keep, long ldkeep, const int* rows, long ldrows, const int* pos_ptr, void* out,
                                int B, int nH, int dh, int Tmax, void* stream);
MMTG_API int mmtg_decode_attn_split_x3_rows(const float* part, int splits, const float* bias, float* kcache, float* vcache, const int* keep,
                                   long ldkeep, const int* rows, long ldrows, const int* pos_ptr, void* out_planes, long plane, int B,
                                   int nH, int dh, int Tmax, void* stream);
MMTG_API int mmtg_decode_beam_candidates(const float* logits, long ldl, int V, const long long* seq, long ldseq, const int* pos_ptr,
                                int P, int sent, float temperature, float rep_penalty, int nb, float* cand_val, int* cand_id,
                                int B, void* stream);
MMTG_API int mmtg_decode_beam_merge(const float* cand_val, const int* cand_id, float* scores, long long* seq, long ldseq, int* keep,
                           long ldkeep, int* rows, long ldrows, const int* pos_ptr, int P, int sent, int nb, int n_prompts,
                           int* pos_next, void* stream);

/* ---- prefixed generation (GreedyDecoder / BeamDecoder with prefix=..., mmtg_amd/decode.py): the caller gives each row the first
 * lyric ids -- the reference's sample_sequence conditioned on a longer `targets` (src/generate.py:97-145, the commented-out --prefix of
 * src/predict.py) -- and writes them into seq before the steps.  fixed_end: int32 [B], the absolute position up to which row b's seq
 * is host-written.  At a step with pos + 1 < fixed_end[b] the row's column pos + 1 is left alone; pos_next is written as ever.
 * The check rides in the step's existing last launch (no extra graph node).  Each entry is its plain namesake plus fixed_end
 * (null fails before any device call):
 * mmtg_decode_select_fixed / mmtg_decode_sample_fixed: as mmtg_decode_select / mmtg_decode_sample (generate.py:127-142);
 * mmtg_decode_beam_candidates_fixed: a fixed row offers no candidates;
 * mmtg_decode_beam_merge_fixed: a prompt whose rows are fixed (one prefix per prompt: its beams share fixed_end, the merge reads
 *   fixed_end[b0] of its first beam) keeps every beam, its scores and its tokens, and sets rows[b, pos + 1] = b.  The kernels of
 *   the plain entries compile to the same code as before these were added.                                                   */
MMTG_API int mmtg_decode_select_fixed(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                             int P, int sent, float temperature, float rep_penalty, int B, int* pos_next, const int* fixed_end,
                             void* stream);
MMTG_API int mmtg_decode_sample_fixed(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                             int P, int sent, float temperature, float rep_penalty, int top_k, float top_p,
                             const float* uniforms, long ldu, int B, int* pos_next, const int* fixed_end, void* stream);
MMTG_API int mmtg_decode_beam_candidates_fixed(const float* logits, long ldl, int V, const long long* seq, long ldseq, const int* pos_ptr,
                                      int P, int sent, float temperature, float rep_penalty, int nb, float* cand_val, int* cand_id,
                                      int B, const int* fixed_end, void* stream);
MMTG_API int mmtg_decode_beam_merge_fixed(const float* cand_val, const int* cand_id, float* scores, long long* seq, long ldseq, int* keep,
                                 long ldkeep, int* rows, long ldrows, const int* pos_ptr, int P, int sent, int nb, int n_prompts,
                                 int* pos_next, const int* fixed_end, void* stream);

/* ---- diverse beam search (BeamDecoder with num_beam_groups=G, diversity_penalty=lambda, mmtg_amd/decode.py): the nb beams of a
 * prompt are G groups of s = nb / G rows, rows b0 + g*s .. b0 + g*s + s - 1 being group g; each group runs its own beam search
 * (the caller starts every group at [0, -inf, ...]) and is penalised for an id an earlier group chose at the same step.  At a
 * step with candidates (not forced, not a held prefix column, cand_val not null) the groups are served in order g = 0 .. G - 1:
 *   group g sees the s * nb candidates (p, k) whose parent p is one of its own rows; with v = cand_id[p, k],
 *     base = scores[p] + cand_val[p, k]  (NaN becomes -inf),   sel = base - lambda * n(v)  (fp32: the product, then the difference),
 *   n(v) = the number of slots groups 0 .. g - 1 filled at this step with id v whose stored score is above -inf, counted only for
 *   a content id v (not 0, 1, 2, 100, 102: PAD ends a line, it is structure and never penalised);
 *   the group keeps its s best by (sel descending, p ascending, k ascending -- k the unpenalised rank of the candidates kernel),
 *   which become its rows in that order: seq / keep / rows reordered in place as in mmtg_decode_beam_merge, seq[b, pos + 1] = v,
 *   rows[b, pos + 1] = b and scores[b] = base -- the penalty steers the choice and is not remembered, so scores stay the sums of
 *   the processed log-probabilities and compare across groups.
 * The candidates' top nb per parent is enough: earlier groups placed at most nb - s distinct ids, the penalty only lowers those,
 * so a parent's s best ids after the penalty lie among its s + (nb - s) = nb best before it -- the selection equals a penalised
 * search over the whole vocabulary.  Forced positions, null candidates and (the *_fixed form) held prompts do what
 * mmtg_decode_beam_merge / mmtg_decode_beam_merge_fixed do.  groups = 1 selects exactly what those select, whatever the penalty.
 * One kernel (beam_merge_groups_kernel: one workgroup per prompt, one candidate per thread, G rounds with one barrier pair each,
 * no atomics, equal inputs give equal bits); every other kernel compiles to the same code as before these were added.
 * Each entry is its namesake plus groups and diversity_penalty; groups < 1, nb % groups != 0, a negative or non-finite penalty
 * (and nb outside 1..16, a null fixed_end) fail before any device call.                                                        */
MMTG_API int mmtg_decode_beam_merge_groups(const float* cand_val, const int* cand_id, float* scores, long long* seq, long ldseq, int* keep,
                                  long ldkeep, int* rows, long ldrows, const int* pos_ptr, int P, int sent, int nb, int n_prompts,
                                  int* pos_next, int groups, float diversity_penalty, void* stream);
MMTG_API int mmtg_decode_beam_merge_groups_fixed(const float* cand_val, const int* cand_id, float* scores, long long* seq, long ldseq,
                                        int* keep, long ldkeep, int* rows, long ldrows, const int* pos_ptr, int P, int sent, int nb,
                                        int n_prompts, int* pos_next, const int* fixed_end, int groups, float diversity_penalty,
                                        void* stream);

/* ---- n-gram blocking (GreedyDecoder / BeamDecoder with no_repeat_ngram_size=n, mmtg_amd/decode.py): a row never writes a content
 * n-gram it already holds.  Row b about to fill a free lyric column j (not forced, not sticky PAD, not a held prefix column) has the
 * history g[0..j-1], its own lyric columns (prefix columns included, the topic prompt not).  Content ids: all but 0, 1, 2, 100, 102
 * (PAD, [#START#], [#EOS#], [UNK], [SEP]), so those break n-grams.  Key: g[j-n+1 .. j-1] (empty for n = 1).  If j >= n - 1 and the
 * key is all content, every v = g[i+n-1] (0 <= i <= j-n) with g[i .. i+n-1] all content and g[i .. i+n-2] equal to the key is
 * banned: its processed logit becomes -inf after the penalty, temperature and fixed bans, before the arg-max / the top-k, top-p
 * filters and the draw / the beam's log_softmax and top-nb.  Everything else is as in the plain entries.  The ban set is built
 * per row in the step's existing last launch.  Each entry is its plain namesake plus fixed_end (null: no prefix; else as the
 * *_fixed entries) and ngram, 1 <= ngram <= sent - 2 (a longer n-gram cannot be all content); outside that range, or without
 * logits, the entry fails before any device call.  The beam merge is unchanged: bans act in the candidates.  The kernels of the
 * plain and *_fixed entries compile to the same code as before these were added.                                              */
MMTG_API int mmtg_decode_select_ngram(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                             int P, int sent, float temperature, float rep_penalty, int B, int* pos_next, const int* fixed_end,
                             int ngram, void* stream);
MMTG_API int mmtg_decode_sample_ngram(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                             int P, int sent, float temperature, float rep_penalty, int top_k, float top_p,
                             const float* uniforms, long ldu, int B, int* pos_next, const int* fixed_end, int ngram, void* stream);
MMTG_API int mmtg_decode_beam_candidates_ngram(const float* logits, long ldl, int V, const long long* seq, long ldseq, const int* pos_ptr,
                                      int P, int sent, float temperature, float rep_penalty, int nb, float* cand_val, int* cand_id,
                                      int B, const int* fixed_end, int ngram, void* stream);

/* ---- line-length bounds and line-end token sets (GreedyDecoder / BeamDecoder with line_lengths= / line_end_ids=,
 * mmtg_amd/decode.py): the form of the lyric.  The reference ends a line where the model happens to pick PAD and pads the slot from
 * there (generate.py:137-138, its sticky PAD; the slots are those of generate.py:117-123); these entries decide PAD by rule.
 * Lyric index j is line l = j / sent, content column c = j % sent - 1 (0 .. sent - 3).  Row b carries per line lo[b, l] <= hi[b, l]
 * <= sent - 2 (bytes, [B, n_lines]; a line l >= n_lines is unconstrained) and optionally an end set: set_of[b, l] (int16, -1: none)
 * names a row of `sets`, n_sets bit rows of ceil(V / 32) words (bit v & 31 of word v >> 5: content id v is a member).  (0, sent - 2,
 * no set) is unconstrained and gives the *_ngram entry's output bit for bit.  At a column the row's model chooses (not a held prefix
 * column, not forced, the row not in sticky PAD):
 *   c >= hi: the row writes PAD without consulting the logits (beams: PAD at log-probability 0, -inf fillers, as sticky PAD);
 *   else PAD's processed logit is -inf when c < lo, or when the line has an end set and seq[j - 1] is not a member ([#START#] at
 *   c = 0 is none: such a line is never empty); and at c == hi - 1 of a line with an end set every id outside the set is -inf.
 * The bans act where the n-gram bans act (after the penalty, temperature and fixed bans; before the arg-max / the top-k, top-p
 * filters and the draw / the beam's log_softmax and top-nb) and compose with them.  A row whose every logit is -inf writes PAD
 * (arg-max and draw) / offers id 0 at -inf for every rank (beams), as the plain kernels do.  Each entry is its *_ngram namesake
 * (fixed_end may be null; ngram 0 .. sent - 2, 0: no n-gram bans) plus the tables; sets, set_of and n_sets are null / 0 together.
 * Without logits, or with tables missing, the entry fails before any device call.  The beam merge is unchanged: a full line is
 * offered by the candidates the way sticky PAD is.  The kernels of the plain, *_fixed and *_ngram entries compile to the same code
 * as before these were added.                                                                                                  */
MMTG_API int mmtg_decode_select_lines(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                             int P, int sent, float temperature, float rep_penalty, int B, int* pos_next, const int* fixed_end,
                             int ngram, const unsigned char* lo, const unsigned char* hi, int n_lines, const unsigned* sets,
                             int n_sets, const short* set_of, void* stream);
MMTG_API int mmtg_decode_sample_lines(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                             int P, int sent, float temperature, float rep_penalty, int top_k, float top_p,
                             const float* uniforms, long ldu, int B, int* pos_next, const int* fixed_end, int ngram,
                             const unsigned char* lo, const unsigned char* hi, int n_lines, const unsigned* sets, int n_sets,
                             const short* set_of, void* stream);
MMTG_API int mmtg_decode_beam_candidates_lines(const float* logits, long ldl, int V, const long long* seq, long ldseq, const int* pos_ptr,
                                      int P, int sent, float temperature, float rep_penalty, int nb, float* cand_val, int* cand_id,
                                      int B, const int* fixed_end, int ngram, const unsigned char* lo, const unsigned char* hi,
                                      int n_lines, const unsigned* sets, int n_sets, const short* set_of, void* stream);

/* ---- line templates (GreedyDecoder / BeamDecoder with templates=, mmtg_amd/decode.py): given characters and id classes inside a
 * line -- an acrostic, a fill-in, a tone or rhyme pattern.  The reference leaves every content column to the model
 * (generate.py:117-142); these entries extend the line rule above by one symbol per row, line and content column:
 * tmpl int32 [B, n_lines, sent - 2], tmpl[b, l, c] >= 0 a given id, -1 free, <= -2 the class -2 - value, a row of the SAME `sets` bit
 * table the end sets use (a value that names no row of it is read as free).  A template of k symbols fixes the line's opening; the
 * host folds its length into the bounds -- closed: (lo, hi) = (k, k); open: lo = max(lo, k), hi >= k -- so a column with a symbol
 * has c < lo <= hi, PAD is banned there by the line rule and the tables need no further field.  At a column the row's model chooses
 * (not a held prefix column, not forced, the row not in sticky PAD, the line not full):
 *   given v: the row writes v without consulting the logits, the way a full line writes PAD (beams: v at log-probability 0 and -inf
 *     fillers, so the merge keeps every live beam and its score); v is subject to no ban or mask, and counts as history for the
 *     penalty, for later n-gram keys and as the end set's "previous token" like any written token;
 *   class S: every id outside S is -inf where the end-set mask acts, composing with the n-gram bans and, at c == hi - 1 of a line
 *     with an end set, with that set (an id survives only if every rule admits it);
 *   free: the line rule alone.
 * Sticky PAD wins over a template: once an all-banned column (n-gram bans can empty a class) has made the row write PAD, the
 * line has ended and its later given columns are PAD too; the all -inf behaviour is that of the *_lines entries.  Both masks are
 * read from global memory in the one pass the line rule makes over the count words: the dynamic LDS request is the *_lines
 * entry's.  Each entry is its *_lines namesake plus the table; without logits or with a null table it fails before any device call.
 * The beam merge is unchanged.  The kernels of every earlier entry compile to the same code as before these were added.       */
MMTG_API int mmtg_decode_select_tmpl(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                            int P, int sent, float temperature, float rep_penalty, int B, int* pos_next, const int* fixed_end,
                            int ngram, const unsigned char* lo, const unsigned char* hi, int n_lines, const unsigned* sets,
                            int n_sets, const short* set_of, const int* tmpl, void* stream);
MMTG_API int mmtg_decode_sample_tmpl(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                            int P, int sent, float temperature, float rep_penalty, int top_k, float top_p,
                            const float* uniforms, long ldu, int B, int* pos_next, const int* fixed_end, int ngram,
                            const unsigned char* lo, const unsigned char* hi, int n_lines, const unsigned* sets, int n_sets,
                            const short* set_of, const int* tmpl, void* stream);
MMTG_API int mmtg_decode_beam_candidates_tmpl(const float* logits, long ldl, int V, const long long* seq, long ldseq, const int* pos_ptr,
                                     int P, int sent, float temperature, float rep_penalty, int nb, float* cand_val, int* cand_id,
                                     int B, const int* fixed_end, int ngram, const unsigned char* lo, const unsigned char* hi,
                                     int n_lines, const unsigned* sets, int n_sets, const short* set_of, const int* tmpl,
                                     void* stream);

/* ---- rhyme schemes (GreedyDecoder / BeamDecoder with rhyme_scheme=, mmtg_amd/decode.py): lines that end on one rhyme, the rhyme
 * being the model's choice.  The reference has no such constraint (generate.py:117-142).  The caller partitions the ids that have a
 * rhyme into classes, rows of the SAME `sets` bit table the end sets and template classes use: class_of int16 [V], class_of[v] the row
 * of v's class or -1.  A scheme ("AABB") groups the lines; the first line of a group with more than one line is its leader, the
 * others its followers: lead int8 [B, n_lines], lead[b, l] = the leader's line (< l) of follower l, else -1 (so n_lines <= 128).
 *   leader: an ordinary line whose static end set (set_of) is the union of the classes; nothing here is new for it;
 *   follower l with leader r: t = the last non-PAD id among lyric columns r * sent + 1 .. r * sent + sent - 2 of the row's own
 *     history (a beam's reordered history; given prefix columns count), k = class_of[t].  If t and k exist, the line behaves as a
 *     line whose end set is row k of `sets`: PAD is -inf unless the previous token is a member, and at c == hi - 1 every id outside
 *     the row is -inf.  With distinct != 0 the end ids of the earlier lines of the group (leader included) are taken out of that set
 *     for both effects.  If the leader's line is empty or t has no class, line l has no rhyme constraint in that row.  A follower's
 *     own set_of entry is -1 (the host rejects a static end set on a follower).
 * The rule acts where the end set acts and composes with n-gram bans, bounds and templates (an id survives only if every rule admits
 * it); all -inf behaves as in the *_lines entries.  tmpl may be null (no templates): one form serves both.  Finding t reads at most
 * sent - 2 ids of the row before the occurrence count; the mask is read from global memory in the *_tmpl entries' one pass over the
 * count words, so the dynamic LDS request is theirs; distinct adds one sentinel write per earlier line of the group.  Each entry is
 * its *_tmpl namesake plus (class_of, lead, distinct) before the stream; a null class_of or lead, n_sets == 0, n_lines > 128 or a
 * distinct other than 0 / 1 fails before any device call.  The beam merge is unchanged.  The kernels of every earlier entry compile
 * to the same code as before these were added.                                                                                      */
MMTG_API int mmtg_decode_select_rhyme(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                            int P, int sent, float temperature, float rep_penalty, int B, int* pos_next, const int* fixed_end,
                            int ngram, const unsigned char* lo, const unsigned char* hi, int n_lines, const unsigned* sets,
                            int n_sets, const short* set_of, const int* tmpl, const short* class_of, const signed char* lead,
                            int distinct, void* stream);
MMTG_API int mmtg_decode_sample_rhyme(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                            int P, int sent, float temperature, float rep_penalty, int top_k, float top_p,
                            const float* uniforms, long ldu, int B, int* pos_next, const int* fixed_end, int ngram,
                            const unsigned char* lo, const unsigned char* hi, int n_lines, const unsigned* sets, int n_sets,
                            const short* set_of, const int* tmpl, const short* class_of, const signed char* lead, int distinct,
                            void* stream);
MMTG_API int mmtg_decode_beam_candidates_rhyme(const float* logits, long ldl, int V, const long long* seq, long ldseq, const int* pos_ptr,
                                     int P, int sent, float temperature, float rep_penalty, int nb, float* cand_val, int* cand_id,
                                     int B, const int* fixed_end, int ngram, const unsigned char* lo, const unsigned char* hi,
                                     int n_lines, const unsigned* sets, int n_sets, const short* set_of, const int* tmpl,
                                     const short* class_of, const signed char* lead, int distinct, void* stream);

/* ---- token log-probabilities (GreedyDecoder with return_logprobs=, mmtg_amd/decode.py): what the model itself says of the id a
 * step has placed.  The reference has no such output (generate.py:117-142 keeps the ids only).  Launched after a step's selection
 * entry on the same stream; one workgroup of 256 threads per row b.  With pos = *pos_ptr, j = pos + 1 - P and
 * v = seq[b * ldseq + pos + 1] (the id the column holds AFTER the selection), over the RAW logits x = logits[b * ldl + 0 .. V - 1]:
 *   out[b * ldo + j] = x[v] - max - log(sum_u exp(x[u] - max)),   max = max_u x[u],   fp32 throughout.
 * No penalty, no temperature, no bans: V is the cut the selection uses, nothing else of the selection's rule reaches the number, so
 * the entry scores a pick, a draw, a template's given id, a full line's PAD, a sticky PAD and a held prefix id alike.
 *   j < 0, j >= ncols, pos + 1 >= ldseq or v outside 0 .. V - 1: nothing is written;
 *   -inf entries add 0 to the sum; x[v] == -inf gives -inf; a row whose maximum is -inf gives -inf (never NaN).
 * The row is read once (16-byte aligned rows as float4, up to 16 per thread in flight; otherwise and for the tail one logit at a
 * time), reduced by wave shuffles and four words of static LDS in a fixed order: equal inputs give equal bits.  It reads *pos_ptr,
 * which the selection entries leave alone (they publish into pos_next), and changes nothing but that one column of `out`.  A null
 * pointer, V < 1, ldl < V, ldseq <= P, ncols < 1 or ldo < ncols fails before any device call.  The kernels of every earlier entry
 * compile to the same code as before this was added (profiles/r14_logprob_decode_disassembly_diff.txt).                            */
MMTG_API int mmtg_decode_logprob(const float* logits, long ldl, int V, const long long* seq, long ldseq, const int* pos_ptr, int P,
                        float* out, long ldo, int ncols, int B, void* stream);

/* ---- keyword-constrained beam search (BeamDecoder with keywords=, mmtg_amd/decode.py): lyrics that contain given words, each at a
 * place of the model's choice -- the banked beam allocation of Post & Vilar (2018) / Hu et al. (2019) in the step's last two launches.
 * Keywords.  A prompt carries K keywords, 0 <= K <= 8, shared by its beams: phrases int32 [prompts, 8, 4] and phrase_len int8
 *   [prompts, 8] (prompt = row / nb).  A keyword is a phrase of 1 .. 4 content ids (not 0, 1, 2, 100, 102; below the vocabulary
 *   cut): one character is one token, so four ids are a four-character word.  The phrases of a prompt are distinct and none is a
 *   contiguous sub-phrase of another (the host refuses both).  nb * (nb + K) <= 256: one merge workgroup has a candidate per thread.
 *   The tables live on the device, so an entry cannot read them: phrase_cap is the caller's bound on the longest phrase, checked
 *   here (1 .. 4), and the kernel ignores a keyword whose stored length is outside 1 .. phrase_cap (no slot, nothing in a bank).
 * History and met.  A row's history h is its own lyric columns 1 .. j - 1 (prefix columns included, the prompt not; a beam's is
 *   its reordered history).  A keyword is met in h if its phrase occurs in h as a contiguous window.  Phrases hold content ids
 *   only, so no window spans [#EOS#] / [#START#] / PAD: a keyword always lies inside one line, with no special case.
 * Bank.  met(s): the keywords met in s.  prog(s): the largest m, 1 <= m < len_i, over the keywords i not in met(s), with the last m
 *   ids of s equal to phrase_i[0..m); 0 if none.  bank(s) = sum over i in met(s) of len_i + prog(s).  The bank is stateless: it is
 *   recomputed from the history at every step, so an abandoned partial phrase unwinds by itself and nothing is reordered with the
 *   beams.
 * Candidates (mmtg_decode_beam_candidates_kw; cand_val / cand_id / cand_bank are [B, W], W = nb + K).  A row that chooses at a free
 *   column offers W slots.  Slots 0 .. nb - 1 are mmtg_decode_beam_candidates_rhyme's on the same inputs, in value, id and order.
 *   Slot nb + i belongs to keyword i: if it is not met in h, with m_i the largest m < len_i such that the last m ids of h equal
 *   phrase_i[0..m) (0 if none), the slot offers t = phrase_i[m_i] at the value (x[t] - max) - log(sum) of the processed logits, as
 *   the top slots.  The slot is dead (value -inf, id 0) if the keyword is met, if x[t] is -inf (any ban of any rule wins: keywords
 *   compose with n-gram bans, bounds, end sets, templates and rhymes and never override them; an id at or above V is banned), if
 *   t is among the row's top nb ids, or if an earlier keyword slot of this row offers t.  cand_bank[b, k] = bank(h + [id]) of the
 *   slot, 0 for a dead one.  A row that offers one candidate (sticky PAD, a full line's PAD, a template's given id) offers it in
 *   slot 0 with bank(h + [id]) -- a given id may complete a keyword, PAD resets prog -- and W - 1 dead slots.  The rule is the
 *   *_rhyme entry's (fixed_end .. distinct as there), except that n_lines = 0 with every table null means no line rule at all,
 *   and with n_lines > 0 n_sets may be 0 (lead all -1: no followers; class_of is then never read but still needed).
 * Merge (mmtg_decode_beam_merge_kw / _kw_fixed; one workgroup per prompt, candidate o = p * W + k).  base = scores[p] +
 *   cand_val[p, k], NaN becomes -inf; live means base > -inf.  A live candidate's r is the number of live candidates of the SAME
 *   bank that precede it by (base descending, o ascending).  The live candidates are ordered by (r ascending, bank descending):
 *   the best of every bank, highest bank first, then the second best of every bank, and so on; the dead ones follow in o order.
 *   The first nb are kept in that order with the stored score base: the allocation steers the choice, the score stays the sum of
 *   the processed log-probabilities.  Held prefix columns, forced cadence columns and null candidates do what
 *   mmtg_decode_beam_merge / mmtg_decode_beam_merge_fixed do.  With every bank equal (K = 0) the order is the plain merge's, bit for
 *   bit.  No atomics, a fixed order: equal inputs give equal bits.
 * The search is best effort: a keyword that no allowed column can hold stays unmet; nothing here fails on the device.
 * Null pointers, K outside 0..8, nb * (nb + K) > 256 and (K > 0) phrase_cap outside 1..4 fail before any device call.  Two new
 * kernels (beam_candidates_kw_kernel, beam_merge_kw_kernel<NoRule | FixedEnd>); every other kernel compiles to the same code as
 * before these were added.                                                                                                   */
MMTG_API int mmtg_decode_beam_candidates_kw(const float* logits, long ldl, int V, const long long* seq, long ldseq, const int* pos_ptr,
                                   int P, int sent, float temperature, float rep_penalty, int nb, float* cand_val, int* cand_id,
                                   int B, const int* fixed_end, int ngram, const unsigned char* lo, const unsigned char* hi,
                                   int n_lines, const unsigned* sets, int n_sets, const short* set_of, const int* tmpl,
                                   const short* class_of, const signed char* lead, int distinct, const int* phrases,
                                   const signed char* phrase_len, int K, int phrase_cap, int* cand_bank, void* stream);
MMTG_API int mmtg_decode_beam_merge_kw(const float* cand_val, const int* cand_id, const int* cand_bank, float* scores, long long* seq,
                              long ldseq, int* keep, long ldkeep, int* rows, long ldrows, const int* pos_ptr, int P, int sent,
                              int nb, int n_prompts, int* pos_next, int K, void* stream);
MMTG_API int mmtg_decode_beam_merge_kw_fixed(const float* cand_val, const int* cand_id, const int* cand_bank, float* scores, long long* seq,
                                    long ldseq, int* keep, long ldkeep, int* rows, long ldrows, const int* pos_ptr, int P, int sent,
                                    int nb, int n_prompts, int* pos_next, const int* fixed_end, int K, void* stream);

/* ---- refrain schemes (GreedyDecoder / BeamDecoder with refrain_scheme=, mmtg_amd/decode.py): lines that repeat a line, whatever
 * the model wrote there.  The reference has no such constraint (generate.py:117-142); a template repeats only text the caller knows,
 * a rhyme makes lines agree on a class, and n-gram blocking forbids a repeated line outright.  A scheme ("AB.A") groups the lines: the
 * first line of a letter is its source, an ordinary line under every rule above; every later line of the letter is a copy.
 * src int8 [B, n_lines], src[b, l] = the source's line (< l) of copy line l, else -1 (so n_lines <= 128; a line l >= n_lines is no
 * copy; a value outside 0 .. l - 1 is read as -1).  With beams a prompt's rows share its row of the table.
 *   copy column: row b about to fill lyric index j, not on a held prefix column (pos + 1 >= fixed_end[b]) and not on a forced
 *     [#START#] / [#EOS#] column, with l = j / sent and r = src[b, l] >= 0, writes seq[j - (l - r) * sent] of its OWN history: the id it
 *     holds at the same column of line r (a beam's reordered history; a source inside a given prefix counts; r < l, so the source line
 *     is complete).  The copy is literal and comes first: it is decided before the sticky-PAD test, before the test for logits, before
 *     the line rule, the template symbol and every ban; no logits are consulted, and no ban or mask applies to it.  A source that ended
 *     at column c is reproduced with its PADs, so no line-end logic is involved.  Beams: the id at log-probability 0 in slot 0 and id-0
 *     fillers at -inf, as a template's given id is offered (the merge keeps every live beam and its score); on a step without logits
 *     nothing is offered, as ever.  The copied ids are ordinary history afterwards: for the penalty, for later n-gram keys, as a later
 *     end set's "previous token".  A copy can never trip the n-gram rule, but the text after it cannot repeat it.
 *   every other column: the *_rhyme entry's rule on the same tables, bit for bit.
 * The rhyme form's own tables may be the "no rule" forms, n_lines still being the width of src: lo and hi null together (no line
 * rule at all: then sets, set_of, tmpl, class_of and lead are null and n_sets and distinct 0), and class_of and lead null together
 * (no rhyme scheme: distinct 0).  One form so serves a refrain with or without bounds, end sets, templates and rhymes.
 * Each entry is its *_rhyme namesake plus src before the stream.  A null src, n_lines outside 1 .. 128, tables that do not come
 * together as above, or an n-gram size outside 0 .. sent - 2 fail before any device call.  mmtg_decode_select_refrain alone takes
 * null logits (the decoders skip the head on a step whose every row copies or is held): a copy column is written, and every other
 * row does what the plain entries do without logits (the forced cadence; else nothing).  The copy is one table read and one id
 * read, the same addresses in every thread of the row's workgroup; thread 0 stores.  The beam merge is unchanged.  Keywords and a
 * refrain are not combined: mmtg_decode_beam_candidates_kw has no src.  The kernels of every earlier entry compile to the same code as
 * before these were added (profiles/r17_refrain_decode_disassembly_diff.txt).                                                      */
MMTG_API int mmtg_decode_select_refrain(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                              int P, int sent, float temperature, float rep_penalty, int B, int* pos_next, const int* fixed_end,
                              int ngram, const unsigned char* lo, const unsigned char* hi, int n_lines, const unsigned* sets,
                              int n_sets, const short* set_of, const int* tmpl, const short* class_of, const signed char* lead,
                              int distinct, const signed char* src, void* stream);
MMTG_API int mmtg_decode_sample_refrain(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                              int P, int sent, float temperature, float rep_penalty, int top_k, float top_p,
                              const float* uniforms, long ldu, int B, int* pos_next, const int* fixed_end, int ngram,
                              const unsigned char* lo, const unsigned char* hi, int n_lines, const unsigned* sets, int n_sets,
                              const short* set_of, const int* tmpl, const short* class_of, const signed char* lead, int distinct,
                              const signed char* src, void* stream);
/* mmtg_decode_sample_refrain with the four truncation stages of mmtg_logits_process_sample_warp (min_p, typical_p, epsilon_cutoff,
 * eta_cutoff after top_p; the rule is stated there) between the nucleus filter and the draw: the selection entry of a sampled
 * generation with any of the four on, whatever its constraints.  One entry over the most general rule serves them all through that
 * rule's "no rule" forms: fixed_end null (no prefix), ngram 0, lo / hi null (no line rule), tmpl null, class_of / lead null (no rhyme
 * scheme), and a src table of -1 (no copy line; src itself and n_lines in 1 .. 128 are still required).  The stages act on the
 * processed logits after every ban, so a banned id has p = 0 in all of them.  Logits and uniforms are required: a step without the
 * head ends in the entry it always ended in.  A kernel of its own; the kernels of every earlier entry compile to the same code.   */
MMTG_API int mmtg_decode_sample_warp(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                              int P, int sent, float temperature, float rep_penalty, int top_k, float top_p, float min_p,
                              float typical_p, float epsilon_cutoff, float eta_cutoff, const float* uniforms, long ldu, int B,
                              int* pos_next, const int* fixed_end, int ngram, const unsigned char* lo, const unsigned char* hi,
                              int n_lines, const unsigned* sets, int n_sets, const short* set_of, const int* tmpl,
                              const short* class_of, const signed char* lead, int distinct, const signed char* src, void* stream);
/* mmtg_decode_sample_warp with the Mirostat stage of mmtg_logits_process_sample_mirostat (the rule is stated there) behind its four:
 * the selection entry of every head step of a generation with mirostat_tau on, whatever its other sampling values and constraints.
 * mu [B] (required) is row b's state; only a column that the row draws updates it.  The forced [#START#] / [#EOS#] cadence, a held
 * prefix column, a refrain's copy column, a template's given id, a full line's PAD and sticky PAD leave mu[b] exactly as it was;
 * columns narrowed by bans draw and update.  A kernel of its own over the refrain rule.                                         */
MMTG_API int mmtg_decode_sample_mirostat(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                              int P, int sent, float temperature, float rep_penalty, int top_k, float top_p, float min_p,
                              float typical_p, float epsilon_cutoff, float eta_cutoff, const float* uniforms, long ldu, int B,
                              int* pos_next, const int* fixed_end, int ngram, const unsigned char* lo, const unsigned char* hi,
                              int n_lines, const unsigned* sets, int n_sets, const short* set_of, const int* tmpl,
                              const short* class_of, const signed char* lead, int distinct, const signed char* src,
                              float mirostat_tau, float mirostat_eta, float* mu, void* stream);
MMTG_API int mmtg_decode_beam_candidates_refrain(const float* logits, long ldl, int V, const long long* seq, long ldseq,
                                       const int* pos_ptr, int P, int sent, float temperature, float rep_penalty, int nb,
                                       float* cand_val, int* cand_id, int B, const int* fixed_end, int ngram, const unsigned char* lo,
                                       const unsigned char* hi, int n_lines, const unsigned* sets, int n_sets, const short* set_of,
                                       const int* tmpl, const short* class_of, const signed char* lead, int distinct,
                                       const signed char* src, void* stream);

/* ---- contrastive search (ContrastiveDecoder, mmtg_amd/decode.py; Su et al. 2022, `penalty_alpha` / `top_k` of transformers'
 * generate): among the model's k most probable next tokens, keep the one whose last-layer hidden state is least like the
 * context's.  The reference has no such method (generate.py:117-142 is greedy / top-k / top-p); it is the deterministic answer to
 * the repetition its repetition_penalty 1.5 fights on ids, made on representations.
 * Layout.  A prompt owns k rows b0 .. b0 + k - 1 (k = top_k, 1..16, b0 = prompt * k: the beam decoder's layout, with its ancestry
 *   table `rows`).  scores[b] is the processed log-probability at which the token in row b's NEWEST column was offered; a row at
 *   -inf (or NaN) is dead.  Invariant: after every merge the k rows of a prompt agree in every column but the newest, which holds
 *   the k candidates.  Token step `pos` embeds column pos of every row, runs the layers (and the head, where the beam decoder runs
 *   it) and ends in three launches on one chain:
 * 1. Candidates: the mmtg_decode_beam_candidates* entry the generation's rules name, with nb = k, unchanged, on a step with the
 *   head: cand_val / cand_id [B, k].  Prefix, n-gram, line, template, rhyme and refrain rules act there and nowhere else.
 * 2. Similarity, mmtg_decode_contrastive_sim: one workgroup of 256 threads per row b; nothing happens while pos < P.  x_b = x[b * ldx
 *   + 0 .. D - 1] is the residual stream the last block left (what the head's LayerNorm-folded product reads; dtype MMTG_BF16 or
 *   MMTG_F32).  h = gamma * (x_b - mean) / sqrt(var + eps) + beta with the population variance, u_b = h / ||h||_2 (the zero vector if
 *   the norm is 0), fp32 throughout.  u_b is stored as fp32 into the hidden cache hc [B, hc_len, D] at [b, pos - P, :] (when pos - P >= hc_len or
 *   pos is past a table's width, nothing is stored or read and sim[b] = 0), and
 *     sim[b] = max over t in [P, pos) with keep[b, t] != 0 of dot(u_b, hc[rows[b, t], t - P, :]),   0 for an empty context.
 *   The context is the row's own LYRIC columns through the ancestry table, [#START#] / [#EOS#] columns included and PAD columns
 *   (keep 0) excluded.  The prompt's topic words are NOT context: the batched prefill leaves no last-layer states for them, and the
 *   penalty is about the lyric repeating itself.  A dead row (scores given and scores[b] not above -inf) stores u_b and gets
 *   sim[b] = 0 without reading its context; scores may be null (every row is read).  A table entry outside 0 .. B - 1 is skipped.
 *   A dot product is summed in one fixed order and a max does not depend on the order: equal inputs give equal bits.
 * 3. Merge, mmtg_decode_contrastive_merge: one workgroup per prompt; it publishes *pos_next = pos + 1 as the beam merge does.
 *   pos < P (a decoder without prefill): the plain merge's identity, rows[b, pos + 1] = b, nothing else.  Otherwise:
 *   choose   r* = argmax over the live rows r of (1 - alpha) * expf(scores[b0 + r]) - alpha * sim[b0 + r], the lowest r on a tie
 *            (row 0 if no row is live); alpha = penalty_alpha in [0, 1].
 *   column pos of seq, keep and rows of every row of the prompt becomes row b0 + r*'s (so rows[.., pos] = b0 + r*: the previous
 *            merge pointed rows[b, pos] at b).  By the invariant no earlier column needs copying.
 *   score    total[prompt] += scores[b0 + r*].
 *   column pos + 1, the first case that applies: a prefix column (fixed_end given and pos + 1 < fixed_end[b0]) is left alone; a
 *            forced [#EOS#] / [#START#] cadence column gets its token in every row; with candidates, row r gets
 *            cand_id[b0 + r*, r]; without (a step that skipped the head) it is left alone.  scores[b0 + r] = cand_val[b0 + r*, r]
 *            in the candidates case and [0, -inf, ...] in the others: what was not the model's choice is offered by row 0 alone,
 *            which is also how the candidates offer a sticky PAD, a full line's PAD, a given id and a copy.
 *   ancestry rows[b, pos + 1] = b.
 * alpha = 0 is greedy decoding for any k (cand_val descends in r, ties go to the lowest r), and so is k = 1 for any alpha.  The
 * host starts a prompt at scores [0, -inf, ...] and total 0; after the last step the lyric is row b0 and its score
 * total[prompt] + scores[b0]: the last column keeps its most probable candidate, since no later step judges it.
 * Null pointers (cand_val / cand_id, scores of the similarity entry and fixed_end may be null), k outside 1..16, alpha outside
 * [0, 1], D not a multiple of 4 in 4..1024, hc_len < 1, a table narrower than P + 1 and pos_next == pos_ptr fail before any device
 * call.  Two new kernels in a source file of their own; every other kernel compiles to the same code as before.                  */
MMTG_API int mmtg_decode_contrastive_sim(int dtype, const void* x, long ldx, const float* gamma, const float* beta, float eps,
                                float* hc, int hc_len, float* sim, const float* scores, const int* keep, long ldkeep,
                                const int* rows, long ldrows, const int* pos_ptr, int P, int B, int D, void* stream);
MMTG_API int mmtg_decode_contrastive_merge(const float* cand_val, const int* cand_id, float* scores, const float* sim, float* total,
                                  float alpha, long long* seq, long ldseq, int* keep, long ldkeep, int* rows, long ldrows,
                                  const int* pos_ptr, int P, int sent, int k, int n_prompts, int* pos_next,
                                  const int* fixed_end, void* stream);

/* ---- stochastic beam search (StochasticBeamDecoder, mmtg_amd/decode.py; Kool, van Hoof and Welling 2019, "Stochastic Beams and
 * Where to Find Them"): nb DIFFERENT lyrics per prompt, an exact sample of size nb without replacement from the distribution the
 * sampler draws from -- the processed logits: penalty, temperature, bans and every line rule.  The reference has no such method
 * (generate.py:117-142 draws its samples independently, so they can coincide).  Log-probabilities are perturbed with Gumbel noise,
 * every child conditioned on its parent's perturbed value, and a beam search of width nb runs over the perturbed values.
 * State.  A prompt owns nb rows b0 .. b0 + nb - 1 (nb in 1..16, b0 = prompt * nb: the beam decoder's layout, its ancestry table
 *   `rows` and its `scores`).  scores[b] is the sum of the processed log-probabilities of row b's tokens, a beam score's scale.
 *   gum[b] (fp32) is the row's perturbed value; a row with gum[b] or scores[b] not above -inf (NaN included) is dead.  The host
 *   starts a prompt at scores = [0, -inf, ...] and gum = [0, -inf, ...].
 * Noise.  Counter-based and stateless, from hash_u32 of csrc/common.h (the murmur3 finaliser the dropout uses):
 *     h = hash_u32(hash_u32(row_seed[b], (uint32) pos), (uint32) v)      row_seed uint32 [B], written by the host
 *     u = ((h >> 9) + 0.5f) * 2^-23                                      exact in fp32, strictly inside (0, 1)
 *     n_v = -logf(-logf(u))
 *   pos is read from pos_ptr, so a replayed graph draws fresh noise at every step.
 * Candidates, mmtg_decode_gumbel_candidates: one workgroup of 256 threads per row, at a step where mmtg_decode_beam_candidates*
 *   would offer candidates (nothing is written on a forced cadence column, a held prefix column or while pos + 1 - P < 1).  With x
 *   the processed logits exactly as those kernels compute them (the refrain form's rule, whose "no rule" forms serve every
 *   generation: fixed_end null, ngram 0, lo / hi / tmpl / class_of / lead null, a src table of -1):
 *     lp_v = log_softmax(x)[v] in fp32 = (x_v - max x) - logf(sum exp(x - max x)), the beam candidates' own expressions and order
 *     t_v  = lp_v + n_v   over the ids with x_v > -inf;     Zt = max_v t_v
 *   The row offers its nb largest t_v, by t descending and then id ascending: cand_id, cand_val = lp_v, and cand_g [B, nb]:
 *     G  = scores[b] + t_v
 *     w  = (gum[b] - G) + log1mexp(t_v - Zt)
 *     cand_g = gum[b] - fmaxf(0, w) - log1pf(expf(-fabsf(w)))
 *     log1mexp(a) = a > -ln 2 ? logf(-expm1f(a)) : log1pf(-expf(a))          log1mexp(0) = -inf
 *   the numerically stable form of -log(exp(-T) - exp(-Z) + exp(-G)) (T = gum[b], Z = scores[b] + Zt) of the paper's appendix,
 *   with logf / expf / log1pf / expm1f, not the fast intrinsics.  The transform is monotone in t_v, so the order by t is the order
 *   by cand_g.  The child at Zt gets cand_g == gum[b] bit for bit, and every cand_g <= gum[b].  cand_val of an id has the bits
 *   mmtg_decode_beam_candidates_refrain gives that id: the winners' lp is computed again from the logits; the noise is never
 *   subtracted back out.  Slots past the allowed ids hold -inf in both tables and id 0.
 *   Single-choice columns -- a refrain's copy, sticky PAD, a full line's PAD, a template's given id, in that order: slot 0 offers
 *   that id with cand_val = 0 and cand_g = gum[b] (a continuation of probability 1); the other slots hold -inf and id 0.
 *   Rows that offer nothing: a dead row (tested before everything but the forced / held columns), and a row with every id banned,
 *   offer -inf in both tables and id 0.  No table ever holds a NaN.
 *   LDS: the count words and one V-float image (x, then t): what the beam candidates request.  Fixed-order reductions, no atomics
 *   beyond the count table's: equal inputs give equal bits.
 * Merge, mmtg_decode_gumbel_merge: one workgroup per prompt over its nb * nb candidates; it publishes *pos_next = pos + 1.
 *   The nb largest cand_g are kept, ordered by cand_g descending, then parent ascending, then rank ascending (a strict total
 *   order; a NaN counts as -inf).  The kept candidates become rows 0 .. nb - 1 in that order: seq / keep / rows are reordered in
 *   place as mmtg_decode_beam_merge reorders them, seq[b, pos + 1] = the id, rows[b, pos + 1] = b,
 *   scores[b] = scores[parent] + cand_val (a NaN sum counts as -inf) and gum[b] = cand_g.
 *   A forced cadence column, a held prefix column (fixed_end given, nullable: one prefix per prompt, pos + 1 < fixed_end[b0]) and
 *   null candidates (a step that skipped the head) do what mmtg_decode_beam_merge_fixed does, and gum is left as it was: a
 *   continuation of probability 1 inherits its parent's value.
 * Invariants: after every merge gum[b0] == 0.0 exactly; gum is non-increasing over a prompt's rows; the live rows of a prompt are
 *   pairwise different sequences; nb = 1 is ancestral sampling by the Gumbel-max trick.
 * Fail before any device call: nb outside 1..16, null scores / gum / row_seed / cand_g (cand_val / cand_id / cand_g of the merge
 *   may be null together; fixed_end may be null), the refrain form's table checks, pos_next == pos_ptr.
 * Two new kernels (the candidates behind every other function of decode.hip, the merge in a source file of its own); every other
 * kernel compiles to the same code as before.                                                                                    */
MMTG_API int mmtg_decode_gumbel_candidates(const float* logits, long ldl, int V, const long long* seq, long ldseq,
                                  const int* pos_ptr, int P, int sent, float temperature, float rep_penalty, int nb,
                                  float* cand_val, int* cand_id, int B, const int* fixed_end, int ngram, const unsigned char* lo,
                                  const unsigned char* hi, int n_lines, const unsigned* sets, int n_sets, const short* set_of,
                                  const int* tmpl, const short* class_of, const signed char* lead, int distinct,
                                  const signed char* src, const float* scores, const float* gum, const unsigned* row_seed,
                                  float* cand_g, void* stream);
MMTG_API int mmtg_decode_gumbel_merge(const float* cand_val, const int* cand_id, const float* cand_g, float* scores, float* gum,
                             long long* seq, long ldseq, int* keep, long ldkeep, int* rows, long ldrows, const int* pos_ptr,
                             int P, int sent, int nb, int n_prompts, int* pos_next, const int* fixed_end, void* stream);

/* ---- classifier-free guidance (GuidedDecoder, mmtg_amd/decode.py; generate_samples / sample_sequence with guidance_scale=): how
 * strongly the text follows its inputs.  The reference has no such control (generate.py:117-142 runs one prompt); the rule is
 * transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor.  The decoder runs 2 N rows: rows 0 .. N - 1 are the prompts, rows
 * N .. 2 N - 1 their negatives; a step with the head puts mmtg_decode_guidance between the head and the selection entry, which then
 * reads `out` over N rows, and every step ends in mmtg_decode_mirror, which keeps the negatives on the prompts' text.
 * mmtg_decode_guidance: one workgroup of 256 threads per pair b < N.  With c = cond[b * ldl + 0 .. V - 1], u = uncond[b * ldl + 0 ..
 *   V - 1] (RAW logits) and L(x) = max x + log(sum_v exp(x[v] - max x)), fp32 throughout and in this order of operations:
 *     lc = c[v] - L(c)      lu = u[v] - L(u)      out[b * ldo + v] = lu + scale * (lc - lu)           for v < V,
 *   so c == u gives out = lu bit for bit at any scale, scale 1 follows c and scale 0 follows u.  An id where c or u is -inf gets
 *   -inf, never NaN; a row whose V entries are all -inf (either row) gives all -inf.  Columns V .. ldo - 1 of `out` and the input
 *   columns >= V are not touched.  Each row is read once from HBM for the (max, sum) pair (16-byte aligned rows as float4, others
 *   one logit at a time: ldl may be odd) and once more for the combine, which finds it in the L2 the first pass left it in; wave
 *   shuffles and static LDS words reduce in a fixed order, without atomics: equal inputs give equal bits.
 *   Fails before any device call: a null pointer, N < 1, V < 1, ldl < V, ldo < V, scale not finite or < 0, `out` overlapping
 *   `cond` or `uncond`.
 * mmtg_decode_mirror: with pos = *pos_ptr (the slot the selection leaves alone), seq[(N + b) * ldseq + pos + 1] =
 *   seq[b * ldseq + pos + 1] for b < N when pos + 1 < ldseq (and pos + 1 >= 0); nothing otherwise.  Nothing else is written.
 *   Fails before any device call: a null pointer, N < 1, ldseq < 1.                                                              */
MMTG_API int mmtg_decode_guidance(const float* cond, const float* uncond, long ldl, int V, float scale, float* out, long ldo, int N,
                         void* stream);
MMTG_API int mmtg_decode_mirror(long long* seq, long ldseq, const int* pos_ptr, int N, void* stream);

/* ---- per-modality guidance (ModalityGuidedDecoder, mmtg_amd/decode.py; generate_samples / sample_sequence with image_guidance_scale=
 * / text_guidance_scale=; csrc/decode_guidance_multi.hip): a prompt beside up to three negatives -- without its experience, without
 * its images, without its texts -- each with a scale of its own.  The decoder runs K N rows, K - 1 the number of running negatives:
 * block 0 (rows 0 .. N - 1) holds the prompts, block k (rows k N .. k N + N - 1) the k-th running negative of the same prompts.
 * Additive to ABI 12.
 * mmtg_decode_guidance_multi: one workgroup per prompt b < N; branch k of prompt b is row k N + b of `logits`.  With x_k = logits[(k N
 *   + b) * ldl + 0 .. V - 1] (RAW logits; c = x_0), L(x) = max x + log(sum_v exp(x[v] - max x)), w_k = scales[k - 1] - 1 (an fp32
 *   subtraction), fp32 throughout and in this order of operations:
 *     lc = c[v] - L(c)     l_k = x_k[v] - L(x_k)     g = lc;  g = g + w_k * (lc - l_k)  for k = 1 .. K - 1 in turn     out[b * ldo + v] = g
 *   for v < V.  So every scale at 1 gives lc; x_k == c makes branch k vanish bit for bit at any scale (both rows go through the same
 *   reduction); K = 2 is mmtg_decode_guidance's lu + s (lc - lu) up to rounding.  An id that is -inf in any of the K rows gets -inf,
 *   never NaN; a row whose V entries are all -inf (any of the K) gives all -inf.  The weight the rule puts on lc, 1 + sum_k w_k, may
 *   be negative (three scales at 0 give -2): allowed, the result is still a finite score per id, not a log-probability.
 *   `scales` is a HOST array of K - 1 floats, read at call time and handed to the kernel by value: a captured launch holds the
 *   numbers, not a pointer.  Columns V .. ldo - 1 of `out`, rows >= N of `out` and the input columns >= V are not touched.
 *   Two forms.  Register-resident (V <= 14336): 512 threads; all loads of a prompt's K rows are issued before the first is used (up
 *   to seven float4 per thread and row when `logits`, `out` and both strides are 16-byte aligned, else up to 28 single logits:
 *   ldl may be odd), the rows stay in registers over the max, the sum and the combine, and each is read once.  Re-read (any V): 256
 *   threads, one streaming pass per row for a running (max, sum), a second pass for the combine.  Either way wave shuffles and static
 *   LDS words reduce in a fixed order, without atomics: equal inputs give equal bits (per form).
 *   Fails before any device call: a null pointer (logits, scales, out), N < 1, V < 1, K outside 2 .. 4, ldl < V, ldo < V, a scale not
 *   finite or < 0, `out` overlapping the K N input rows.
 * mmtg_decode_guidance_multi_form: the same with the form named -- 0: what mmtg_decode_guidance_multi chooses (register-resident up to
 *   V = 14336, re-read beyond), 1: register-resident (fails where V > 14336), 2: re-read.  For tools/bench_mguidance.py and the tests.
 * mmtg_decode_mirror_multi: with pos = *pos_ptr, seq[(k N + b) * ldseq + pos + 1] = seq[b * ldseq + pos + 1] for k = 1 .. K - 1 and
 *   b < N when 0 <= pos + 1 < ldseq; nothing otherwise.  Nothing else is written.
 *   Fails before any device call: a null pointer, N < 1, K outside 2 .. 4, ldseq < 1.                                               */
MMTG_API int mmtg_decode_guidance_multi(const float* logits, long ldl, int V, int K, const float* scales, float* out, long ldo, int N,
                               void* stream);
MMTG_API int mmtg_decode_guidance_multi_form(const float* logits, long ldl, int V, int K, const float* scales, float* out, long ldo,
                                    int N, int form, void* stream);
MMTG_API int mmtg_decode_mirror_multi(long long* seq, long ldseq, const int* pos_ptr, int N, int K, void* stream);

/* ---- the training side of guidance (MMTGTrainer(experience_drop=...), evaluate_guided; csrc/guidance_train.hip).  Classifier-free
 * guidance assumes a model that was also trained with the condition removed (Ho & Salimans, 2022); the two entries give the fused
 * step that input and measure the guided distribution on held-out lyrics.  Additive to ABI 12.
 * mmtg_experience_drop: one launch for both channels.  img, txt: fp32 [B, n] (n = S * E), never written; img_out, txt_out: [B, n] of
 *   `dtype` (MMTG_F32 or MMTG_BF16); code: int32 [B].  Per sample b, with h = hash_u32(seed, b) (the counter hash of csrc/common.h:
 *   h = b * 0x9E3779B1 + seed; h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16) compared as 64-bit values:
 *     h < c_both -> code 3;  else h < c_img -> code 1;  else h < c_txt -> code 2;  else code 0.
 *   Bit 0 of the code: the images are dropped; bit 1: the texts are dropped.  A dropped channel's row is +0.0 in every element; a kept
 *   row holds the bits mmtg_cast_f32_to would write (f32 -> f32 is a copy).  No rescaling: a condition switch, not a dropout of
 *   activations.  One hash per sample decides both channels, so the three events are disjoint; equal inputs give equal bits.  The
 *   thresholds are cumulative, c_both <= c_img <= c_txt <= 2^32; the host computes each probability's share in float64 as
 *   min(int(p * 2^32), 2^32) and accumulates: p = 1 drops every row, p = 0 none.  Rows with n % 4 == 0 on 16-byte aligned bases
 *   move as 16-byte loads, all others one element at a time.
 *   Fails before any device call: a null pointer, B < 1, n < 1, thresholds negative, not monotone or above 2^32, an unknown dtype,
 *   an output overlapping an input.
 * mmtg_guided_loss: the cross-entropy of the lyric under softmax(lu + s_k (lc - lu)) for K scales in one sweep.  cond, uncond: the
 *   logits [M, ldl] of `logits_dtype` (fp32, or bf16 widened to fp32 first: exact), M = B (P + L), columns >= V ignored; lse_c, lse_u:
 *   each matrix's fp32 row log-sum-exp [M] as mmtg_loss_fwd produced it; scales: a HOST array of K floats, 1 <= K <=
 *   MMTG_GUIDED_MAX_SCALES, each finite and >= 0, read before the launch and passed by value.  Rows and labels are those of
 *   mmtg_loss_fwd's sample_ce: the loss rows P <= t <= T - 2 of each sample (T = P + L, ntok = T - 1 - P), the label
 *   cat(topic_ids, targets)[b, t + 1] clamped into [0, V) -- always an element of targets, so topic_ids is never read and may be
 *   null; PAD rows are included, as the reference's loss includes them.  In fp32 and in mmtg_decode_guidance's order:
 *     lc = c[v] - lse_c[m]      lu = u[v] - lse_u[m]      g_k[v] = lu + s_k * (lc - lu)
 *     nll_k[m] = L(g_k) - g_k[label],   L(x) = max x + log(sum_v exp(x[v] - max x))
 *   (the exponentials are v_exp_f32 in both storage forms, the one log per row and scale is logf).  Outputs, all fp32:
 *   nll [K, M] (0 outside the loss rows), sample_ce [K, B] = (1 / ntok) * the sum of the sample's loss rows, ce [K] = sum_b
 *   sample_ce[k, b] / batch_den.  One workgroup of 256 threads per row; every logit is fetched once (16-byte aligned rows in slices
 *   of eight, the tail and unaligned fp32 rows one logit at a time: an fp32 ldl may be odd) and feeds the K running (max, sum)
 *   pairs; nothing is staged, so V and L have no limit.  Wave shuffles and static LDS words reduce in a fixed order, one wave sums
 *   a sample's rows and one thread a scale's samples in sample order: no atomics, equal inputs give equal bits.  Where c == u bit
 *   for bit and lse_c == lse_u, g_k = lu for every k and all K results of the row are the same bits.
 *   Fails before any device call: a null pointer (topic_ids excepted), K outside 1 .. 8, a scale that is not finite or is negative,
 *   V < 1, ldl < V, bf16 rows that are not 16-byte aligned (ldl % 8, the bases), B < 1, P < 0, L < 2, batch_den not finite or <= 0.
 * mmtg_guided_loss_multi: the cross-entropy of the lyric under the distribution mmtg_decode_guidance_multi selects from
 *   (evaluate_modality_guided), for G scale tuples in one sweep over K logits matrices.  logits: a HOST array of K device pointers,
 *   2 <= K <= MMTG_GUIDED_MAX_BRANCHES, pointer 0 the conditional matrix and pointers 1 .. K - 1 the running negatives, each [M, ldl] of
 *   `logits_dtype` with the one stride ldl; lse: a HOST array of K device pointers to the fp32 row log-sum-exps [M] as mmtg_loss_fwd
 *   produced them; both arrays are read at call time and their entries handed to the kernel by value.  scales: a HOST array of
 *   G (K - 1) floats, tuple-major (scales[g (K - 1) + k - 1] is tuple g's scale for branch k), 1 <= G <= MMTG_GUIDED_MAX_SCALES, each
 *   finite and >= 0, passed by value.  targets, B, P, L, batch_den, the loss rows, the clamped labels and the PAD rows are
 *   mmtg_guided_loss's; there is no topic_ids.  In fp32 and in mmtg_decode_guidance_multi's order of operations, so that the
 *   training-side and the decode-side numbers describe one distribution:
 *     l_k[v] = x_k[v] - lse_k[m]   (lc = l_0)      w_k = scales[g][k - 1] - 1   (an fp32 subtraction, on the host)
 *     g = lc;   g = g + w_k * (lc - l_k)   for k = 1 .. K - 1 in turn   (one fused multiply-add per branch, in every instantiation)
 *     nll_g[m] = L(g) - g[label],   L(x) = max x + log(sum_v exp(x[v] - max x))
 *   Outputs, all fp32: nll [G, M] (0 outside the loss rows), sample_ce [G, B], ce [G] = sum_b sample_ce[g, b] / batch_den in sample
 *   order.  One workgroup of 256 threads per row, with mmtg_guided_loss's trip structure: every logit of each of the K rows is
 *   fetched once and feeds all G running (max, sum) pairs; 16-byte loads (slices of eight logits, the K rows' loads of a slice issued
 *   before the first is used) only where ALL K row pointers are 16-byte aligned, otherwise and for the tail V % 8 one logit at a
 *   time (an fp32 ldl may be odd); nothing is staged, so V and L have no limit.  Wave shuffles and static LDS words reduce in a fixed
 *   order: no atomics, equal inputs give equal bits, equal tuples give equal bits.  One expression serves every K, so a branch whose
 *   w_k is 0 (scale 1) adds +-0 and the row's nll is the bits of the launch without that matrix, at K - 1; x_k equal to x_0 bit for
 *   bit with equal lse makes branch k vanish bit for bit at any scale; all scales at 1 give L(lc) - lc[label] for every tuple.  The
 *   weight on lc, 1 + sum_k w_k, may be negative (three scales at 0 give -2): allowed.
 *   Fails before any device call: a null pointer (any of the K entries of either array included), K outside 2 .. 4, G outside 1 .. 8,
 *   a scale that is not finite or is negative, V < 1, ldl < V, bf16 rows that are not 16-byte aligned (ldl % 8, any base), an fp32
 *   base that is not 4-byte aligned, B < 1, P < 0, L < 2, batch_den not finite or <= 0, nll overlapping any of the K matrices.       */
#define MMTG_GUIDED_MAX_SCALES 8
#define MMTG_GUIDED_MAX_BRANCHES 4
MMTG_API int mmtg_experience_drop(int dtype, const float* img, const float* txt, void* img_out, void* txt_out, int* code, int B, long n,
                         unsigned seed, long long c_both, long long c_img, long long c_txt, void* stream);
MMTG_API int mmtg_guided_loss(int logits_dtype, const void* cond, const void* uncond, long ldl, int V, const float* lse_c,
                     const float* lse_u, const long long* topic_ids, const long long* targets, const float* scales, int K,
                     int B, int P, int L, float batch_den, float* nll, float* sample_ce, float* ce, void* stream);
MMTG_API int mmtg_guided_loss_multi(int logits_dtype, const void* const* logits, const float* const* lse, int K, long ldl, int V,
                           const long long* targets, const float* scales, int G, int B, int P, int L, float batch_den,
                           float* nll, float* sample_ce, float* ce, void* stream);

/* ---------------------------------------------------------------- distillation of a teacher's (guided) distribution
 * The training-time end of the guidance arc (csrc/distill.hip; MMTGTrainer(distill_weight=..., distill_teacher=...,
 * distill_scale=...)): the model is pulled towards q = softmax(lu + s (lc - lu)) of a teacher's conditional and negative logits,
 * after which plain decoding at full batch gives what guided decoding gave at half of it (guidance distillation, Meng et al.,
 * 2023).  With no negative the same term is ordinary knowledge distillation (Hinton et al., 2015).  Additive to ABI 12.
 *
 * Notation as in the unlikelihood section: P topic columns, L lyric columns, Tt = P + L, row m = b * Tt + t.  The loss rows of a
 * sample are P <= t <= Tt - 2 (ntok = Tt - 1 - P of them; PAD rows included, as in mmtg_guided_loss); every sample takes part
 * whatever its rating.
 *   student     x: the step's own logits, lse[m] from mmtg_loss_fwd;  logp_v = x_v - lse[m],  p_v = exp(logp_v)
 *   teacher     c: its logits for the batch, u: its logits for the negative (u may be null); lse_c, lse_u: each matrix's fp32 row
 *               log-sum-exp; s: a host float, finite and >= 0, passed by value.  In fp32, in mmtg_decode_guidance's order:
 *                 lc = c_v - lse_c[m]      lu = u_v - lse_u[m]      g_v = lu + s * (lc - lu)      (u null: g_v = lc, s is ignored)
 *                 Lg[m] = max g + log(sum_v exp(g_v - max g))       q_v = exp(g_v - Lg[m])
 *   row term    kd_row[m] = sum_v q_v (g_v - Lg[m] - logp_v) = KL(q || p) >= 0
 *   sample      kd_sample[b] = (1 / ntok) * sum over the loss rows of kd_row;   kd = sum_b kd_sample[b] / batch_den
 *               (rows t < P and each sample's last row carry none: kd_row = kd_lg = 0)
 *   objective   MyLoss + alpha * KL (+ lm_weight * LM) (+ cl_weight * cl) + distill_weight * kd
 *   gradient    on a loss row, with w = distill_weight * gscale / (ntok * batch_den) and cf the row factor of mmtg_loss_bwd:
 *               d[m, v] = cf * (p_v - [v == label]) + w * (p_v - q_v)
 *               (the first term is mmtg_loss_bwd's expression in its order; a row without the term -- w = 0, or t < P -- is written
 *               by that expression alone: the same bits.  Rows outside the loss rows and pad columns hold what mmtg_loss_bwd writes.)
 * There is no temperature.  All sums run in a fixed order and nothing is accumulated with atomics: equal inputs give equal bits.
 *
 * mmtg_distill_fwd: one sweep, one workgroup of 256 threads per row; every element of the two or three matrices is fetched once
 *   (rows whose bases are all 16-byte aligned in slices of eight, the tail and unaligned fp32 rows one element at a time: an fp32
 *   ldl or ldt may be odd).  Student (`logits_dtype`, stride ldl) and teacher (`teacher_dtype`, stride ldt; cond and uncond share
 *   both) are each fp32 or bf16, independently; bf16 widens to fp32 exactly.  Nothing is staged, so V has no limit.  A lane carries
 *   (max g, S = sum e^(g - max), A = sum e^(g - max) (g - logp)), rescales S and A together when the max moves; lanes combine by
 *   the wave's butterfly, waves in wave order.  Lg = max + log S, kd_row = A / S - Lg.  The exponentials are v_exp_f32, the log logf.
 *   Outputs (fp32): kd_row [M], kd_lg [M] (Lg, which the backward reads), kd_sample [B], kd [1].
 * mmtg_loss_bwd_kd: mmtg_loss_bwd with the term folded in (kd_lg from mmtg_distill_fwd on the same inputs, kd_coef = w above): the
 *   same storage forms (dtype of dlogits x logits_dtype), zeros, Vpad and in-place rule -- bf16 dlogits may alias the student's
 *   logits, no output may overlap a teacher matrix.  p_v is expf as in mmtg_loss_bwd, q_v is v_exp_f32.
 * mmtg_loss_bwd_kd_x3: the (hi | lo) plane-pair form, beside mmtg_loss_bwd_x3.
 * All three fail before any device call on: a null pointer (uncond and lse_u excepted, which are null together or not at all;
 *   topic_ids where no row reads it), a scale that is not finite or is negative, V < 1, a leading dimension below V, bf16 rows that
 *   are not 16-byte aligned, B < 1, P < 0, L < 2, batch_den not finite or <= 0, kd_coef not finite or negative, an output that
 *   overlaps a teacher input.                                                                                                    */
MMTG_API int mmtg_distill_fwd(int logits_dtype, const void* logits, long ldl, int teacher_dtype, const void* cond, const void* uncond,
                     long ldt, int V, const float* lse, const float* lse_c, const float* lse_u, float scale, int B, int P, int L,
                     float batch_den, float* kd_row, float* kd_lg, float* kd_sample, float* kd, void* stream);
MMTG_API int mmtg_loss_bwd_kd(int dtype, int logits_dtype, const void* logits, long ldl, int V, const long long* topic_ids,
                     const long long* targets, const float* lse, const float* coef, float gscale, float lm_coef,
                     int teacher_dtype, const void* cond, const void* uncond, long ldt, const float* lse_c, const float* lse_u,
                     float scale, const float* kd_lg, float kd_coef, int B, int P, int L, void* dlogits, long ldd, int Vpad,
                     void* stream);
MMTG_API int mmtg_loss_bwd_kd_x3(const float* logits, long ldl, int V, const long long* topic_ids, const long long* targets,
                        const float* lse, const float* coef, float gscale, float lm_coef, int teacher_dtype, const void* cond,
                        const void* uncond, long ldt, const float* lse_c, const float* lse_u, float scale, const float* kd_lg,
                        float kd_coef, int B, int P, int L, void* planes, long ldd, long plane, int Vpad, void* stream);

/* ---- Round 6: the MLP of a GPT-2 block of the decode token step as ONE launch (bf16, n_embd = 768, M <= 256 rows) -- the
 * c_fc -> gelu_new -> mlp.c_proj -> + residual half of the transformers GPT-2 block the reference runs per token through
 * model.py:320-326 / generate.py:124; replaces the mode-0 + mode-2 mmtg_decode_gemm pair of the fused step.
 *   C = X + gelu( rstd (X W1f^T - mu colsum1) + bias1f ) W2t^T + bias2,   stats_out[m][p] = (sum, sum of squares) of C[m, 48 p .. 48 p + 48)
 * X [M, ldx] bf16: the un-normalised residual rows (also the residual added back); stats_in [M][32][2] their statistics partials
 * (np_in of them); W1f [3072, ldw1] / colsum1 / bias1f: the gamma-folded c_fc copy of mmtg_ln_fold_weights; W2t [768, ldw2]: the
 * [out,in] copy of mlp.c_proj; G [M, ldg] bf16: scratch for the hidden activations (written and read inside the launch); C [M, ldc] bf16
 * (may not alias X); stats_out: 16 partials per row.  ws: mmtg_decode_mlp_ws_floats(M) floats of fp32 partial products; sync:
 * mmtg_decode_mlp_sync_words() 64-bit words, ZERO before the first launch (the launch re-arms them; word [65] is the error report:
 * 2 = a wait ran into its 4 ms bound, 4 = a hand-off group was found on two XCDs in the plain mode -- results are then undefined,
 * the host must check and clear it).  The launch is 256 workgroups that must be co-resident, one per CU (mmtg_decode_mlp_census).
 * plain_handoff: 0 = the hidden activations cross workgroups through write-through stores + agent-scope loads (valid under any
 * workgroup placement); 1 = through the XCD's L2 (valid when workgroups b and b + 8 k share an XCD: checked per launch, error bit 4).
 * trace (nullable): 12 x 256 real-time-counter stamps (diagnostic).
 * mmtg_decode_mlp_census: out64[8 v + x] += workgroups b with b % 8 == v found on physical XCD x, for a launch of the same shape
 * (256 workgroups, one per CU): the placement the plain hand-off relies on holds when every row v has one entry of 32.          */
MMTG_API long mmtg_decode_mlp_ws_floats(int M);
MMTG_API int mmtg_decode_mlp_sync_words(void);
MMTG_API int mmtg_decode_mlp_census(unsigned* out64, void* stream);
MMTG_API int mmtg_decode_mlp(int M, int D, const void* X, long ldx, const float* stats_in, int np_in, float eps,
                    const void* W1f, long ldw1, const float* colsum1, const float* bias1f,
                    const void* W2t, long ldw2, const float* bias2, void* G, long ldg, void* C, long ldc,
                    float* stats_out, float* ws, long ws_floats, unsigned long long* sync, int plain_handoff,
                    unsigned long long* trace, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * The data-parallel exchange ("a second small ABI").  One process per GPU holds ONE RCCL communicator;
 * gradient buckets -- contiguous slices of the flat fp32 gradient, in the order the backward finishes them -- are SUM all-reduced
 * in place over xGMI.  Replaces torch.nn.DataParallel's per-step reduce_add_coalesced of every gradient to GPU 0 and its
 * parameter broadcast (reference src/train.py:112-114; generate.py:191, predict.py:195 wrap the model the same way).
 * Conventions that differ from the kernels above: the library owns the communicator, one side stream and two events (created by
 * mmtg_comm_init, released by mmtg_comm_destroy); RCCL is bound at first use (dlopen: the host process's copy when it has one,
 * else MMTG_RCCL_LIB, else librccl.so.1) -- without it these calls return MMTG_ERR_UNSUPPORTED, nothing falls back to the host.
 * Collectives must be issued in the same order on every rank, from one thread.
 *   mmtg_comm_unique_id   rank 0 draws the 128-byte id (ncclGetUniqueId); the host ships it to the other ranks (any side channel)
 *   mmtg_comm_init        collective: every rank calls it with the same id, on the device it has made current
 *   mmtg_comm_info        rank / world / device of the live communicator (world 0: none) and the bound RCCL's version code
 *   mmtg_allreduce_bucket in-place SUM of `count` elements (MMTG_F32 | MMTG_BF16) enqueued on `stream`
 *   mmtg_allreduce_bucket_async  the same on the library's side stream, ordered after everything already on `after_stream`
 *                         (the compute stream): the exchange runs beside the rest of the backward
 *   mmtg_comm_join        `stream` waits for every bucket enqueued with _async so far (no host wait)
 *   mmtg_comm_destroy     drains the side stream and releases the communicator (no-op without one)                            */
#define MMTG_COMM_ID_BYTES 128
MMTG_API int mmtg_comm_unique_id(void* id /* host, MMTG_COMM_ID_BYTES */);
MMTG_API int mmtg_comm_init(int rank, int world, const void* id /* host, MMTG_COMM_ID_BYTES */);
MMTG_API int mmtg_comm_info(int* rank, int* world, int* device, int* rccl_version);
MMTG_API int mmtg_allreduce_bucket(void* ptr, long count, int dtype, void* stream);
MMTG_API int mmtg_allreduce_bucket_async(void* ptr, long count, int dtype, void* after_stream);
MMTG_API int mmtg_comm_join(void* stream);
MMTG_API int mmtg_comm_destroy(void);

#ifdef __cplusplus
}
#endif
#endif /* MMTG_HIP_H */
