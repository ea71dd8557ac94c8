// The training side of classifier-free guidance (MMTGTrainer(experience_drop=...), evaluate_guided): the per-sample condition switch
// that shows the model the input GuidedDecoder's default negative feeds it, and the cross-entropy of the held-out lyric under the
// guided distribution for up to eight scales in one sweep.  include/mmtg_hip.h states both rules.  A source file of its own: every
// other kernel compiles to the same code as before.
//
// guided_row_kernel is a streaming row kernel: per logit pair two loads, K fused multiply-adds and K exponentials (v_exp_f32 in
// both storage forms -- eight libm expf per pair would make the fp32 form VALU-bound three times over), one HBM pass.  Both row
// log-sum-exps are inputs, so g_k is known at the first touch of a pair and the (max, sum) of every scale runs online; nothing is
// staged, so there is no size limit on V or L.
#include <math.h>

#include "common.h"

namespace {

// ---------------------------------------------------------------- experience dropout
// code of sample b: one hash decides both channels (the three events are disjoint); compared as 64-bit values, so 2^32 takes every row
__device__ __forceinline__ int drop_code(uint32_t seed, int b, unsigned long long c_both, unsigned long long c_img,
                                         unsigned long long c_txt) {
    const unsigned long long h = hash_u32(seed, (uint32_t)b);
    return h < c_both ? 3 : h < c_img ? 1 : h < c_txt ? 2 : 0;
}

template <typename T> struct Out4;
template <> struct Out4<float> { typedef f32x4 type; };
template <> struct Out4<bf16> { typedef bf16x4 type; };

// grid (B, blocks per row, 2): blockIdx.z is the channel (0 images, 1 texts).  Rows of n % 4 == 0 elements on aligned bases move as
// 16-byte loads (16- or 8-byte stores); every other row one element at a time.
template <typename T>
__global__ __launch_bounds__(256) void experience_drop_kernel(const float* __restrict__ img, const float* __restrict__ txt,
        T* __restrict__ img_out, T* __restrict__ txt_out, int* __restrict__ code, long n, uint32_t seed,
        unsigned long long c_both, unsigned long long c_img, unsigned long long c_txt) {
    const int b = blockIdx.x, ch = blockIdx.z;
    const int cd = drop_code(seed, b, c_both, c_img, c_txt);
    if (ch == 0 && blockIdx.y == 0 && threadIdx.x == 0) code[b] = cd;
    const bool drop = (cd >> ch) & 1;
    const float* src = (ch ? txt : img) + (long)b * n;
    T* dst = (ch ? txt_out : img_out) + (long)b * n;
    const long start = (long)blockIdx.y * 256 + threadIdx.x, step = (long)gridDim.y * 256;
    typedef typename Out4<T>::type O4;
    if ((n & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 && (reinterpret_cast<uintptr_t>(dst) & (sizeof(O4) - 1)) == 0) {
        const long n4 = n >> 2;
        const f32x4* s4 = reinterpret_cast<const f32x4*>(src);
        O4* d4 = reinterpret_cast<O4*>(dst);
        for (long i = start; i < n4; i += step) {
            O4 o;
            if (drop) {
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = (T)0.f;
            } else {
                const f32x4 v = s4[i];
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = (T)v[e];
            }
            d4[i] = o;
        }
        return;
    }
    for (long i = start; i < n; i += step) dst[i] = drop ? (T)0.f : (T)src[i];
}

// ---------------------------------------------------------------- guided cross-entropy
constexpr int GK = MMTG_GUIDED_MAX_SCALES;
struct Scales { float s[GK]; };

__device__ __forceinline__ float exp_fast(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }

__device__ __forceinline__ void load8(const float* p, float (&x)[8]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
    x[0] = a[0]; x[1] = a[1]; x[2] = a[2]; x[3] = a[3]; x[4] = b[0]; x[5] = b[1]; x[6] = b[2]; x[7] = b[3];
}
__device__ __forceinline__ void load8(const bf16* p, float (&x)[8]) {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = (float)a[e];
}

// the rule, in mmtg_decode_guidance's order
__device__ __forceinline__ float guide(float lc, float lu, float s) { return lu + s * (lc - lu); }

// (max, sum of exp relative to it) of two parts as one; a part that holds nothing has max -inf and sum 0
__device__ __forceinline__ void ms_merge(float& m, float& s, float om, float os) {
    const float nm = fmaxf(m, om);
    s = nm == -INFINITY ? 0.f : s * exp_fast(m - nm) + os * exp_fast(om - nm);
    m = nm;
}

// eight pairs into the K running (max, sum)s of a thread
template <int K>
__device__ __forceinline__ void fold8(const float (&c)[8], const float (&u)[8], float Lc, float Lu, const Scales& sc, float (&mx)[GK],
                                      float (&sm)[GK]) {
    float lc[8], lu[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { lc[e] = c[e] - Lc; lu[e] = u[e] - Lu; }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float g[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) g[e] = guide(lc[e], lu[e], sc.s[k]);
        const float m8 = fmaxf(fmaxf(fmaxf(g[0], g[1]), fmaxf(g[2], g[3])), fmaxf(fmaxf(g[4], g[5]), fmaxf(g[6], g[7])));
        if (m8 > mx[k]) { sm[k] *= exp_fast(mx[k] - m8); mx[k] = m8; }
#pragma unroll
        for (int e = 0; e < 8; ++e) sm[k] += exp_fast(g[e] - mx[k]);
    }
}

// one workgroup per row m: nll[k * M + m] for k < K.  Loss rows only (P <= t <= Tt - 2); the others write their K zeros.
template <typename LT, int K>
__global__ __launch_bounds__(256) void guided_row_kernel(const LT* __restrict__ cond, const LT* __restrict__ uncond, long ldl, int V,
        const float* __restrict__ lse_c, const float* __restrict__ lse_u, const long long* __restrict__ targets, Scales sc,
        int P, int L, long M, float* __restrict__ nll) {
    __shared__ float shm[GK][4];
    __shared__ float shs[GK][4];
    const int Tt = P + L;
    const long m = blockIdx.x;
    const int b = (int)(m / Tt), t = (int)(m % Tt), tid = threadIdx.x;
    if (t < P || t + 1 >= Tt) {
        if (tid < K) nll[(long)tid * M + m] = 0.f;
        return;
    }
    const LT* c = cond + m * ldl;
    const LT* u = uncond + m * ldl;
    const float Lc = lse_c[m], Lu = lse_u[m];
    float mx[GK], sm[GK];
#pragma unroll
    for (int k = 0; k < GK; ++k) { mx[k] = -INFINITY; sm[k] = 0.f; }
    int done = 0;
    if (((reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(u)) & 15) == 0) {
        const int V8 = V & ~7;
        int v = tid * 8;
        for (; v + 2048 < V8; v += 4096) {          // two slices in flight: four independent 16- or 32-byte requests
            float c0[8], u0[8], c1[8], u1[8];
            load8(c + v, c0); load8(u + v, u0); load8(c + v + 2048, c1); load8(u + v + 2048, u1);
            fold8<K>(c0, u0, Lc, Lu, sc, mx, sm);
            fold8<K>(c1, u1, Lc, Lu, sc, mx, sm);
        }
        if (v < V8) {
            float c0[8], u0[8];
            load8(c + v, c0); load8(u + v, u0);
            fold8<K>(c0, u0, Lc, Lu, sc, mx, sm);
        }
        done = V8;
    }
    for (int v = done + tid; v < V; v += 256) {
        const float lc = (float)c[v] - Lc, lu = (float)u[v] - Lu;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float g = guide(lc, lu, sc.s[k]);
            if (g > mx[k]) { sm[k] *= exp_fast(mx[k] - g); mx[k] = g; }
            sm[k] += exp_fast(g - mx[k]);
        }
    }
    // fixed order: the wave's butterfly, then the four waves' pairs in wave order
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float om = __shfl_xor(mx[k], off, 64);
            const float os = __shfl_xor(sm[k], off, 64);
            ms_merge(mx[k], sm[k], om, os);
        }
        if ((tid & 63) == 0) { shm[k][tid >> 6] = mx[k]; shs[k][tid >> 6] = sm[k]; }
    }
    __syncthreads();
    if (tid < K) {
        float mm = shm[tid][0], sv = shs[tid][0];
        for (int w = 1; w < 4; ++w) ms_merge(mm, sv, shm[tid][w], shs[tid][w]);
        long long lab = targets[(long)b * L + (t + 1 - P)];
        if (lab < 0) lab = 0;
        if (lab >= V) lab = V - 1;
        const float gl = guide((float)c[lab] - Lc, (float)u[lab] - Lu, sc.s[tid]);
        nll[(long)tid * M + m] = (mm + logf(sv)) - gl;
    }
}

// single workgroup: sample_ce [K, B] (one wave per (k, b), the loss rows spread over its lanes), then ce [K] in sample order
__global__ __launch_bounds__(1024) void guided_sample_kernel(const float* __restrict__ nll, int K, int B, int P, int L, long M,
        float batch_den, float* __restrict__ sample_ce, float* __restrict__ ce) {
    const int Tt = P + L;
    const int ntok = Tt - 1 - P;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int i = wave; i < K * B; i += 16) {
        const int k = i / B, b = i % B;
        float s = 0.f;
        for (int t = P + lane; t < Tt - 1; t += 64) s += nll[(long)k * M + (long)b * Tt + t];
        s = wave_sum(s);
        if (lane == 0) sample_ce[i] = s / ntok;
    }
    __syncthreads();            // (the workgroup's own global writes are visible behind the barrier)
    if ((int)threadIdx.x < K) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += sample_ce[(long)threadIdx.x * B + b];       // fixed order
        ce[threadIdx.x] = s / batch_den;
    }
}

// whether the byte ranges [a, a + na) and [b, b + nb) share a byte
bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + na, b0 = (uintptr_t)b, b1 = b0 + nb;
    return a0 < b1 && b0 < a1;
}

}  // namespace

extern "C" int mmtg_experience_drop(int dtype, const float* img, const float* txt, void* img_out, void* txt_out, int* code, int B, long n,
                                    unsigned seed, long long c_both, long long c_img, long long c_txt, void* stream) {
    const char* what = "experience_drop";
    MMTG_REQUIRE(dtype == MMTG_F32 || dtype == MMTG_BF16, "%s: bad dtype %d", what, dtype);
    MMTG_REQUIRE(img, "%s: img is a null pointer", what);
    MMTG_REQUIRE(txt, "%s: txt is a null pointer", what);
    MMTG_REQUIRE(img_out, "%s: img_out is a null pointer", what);
    MMTG_REQUIRE(txt_out, "%s: txt_out is a null pointer", what);
    MMTG_REQUIRE(code, "%s: code is a null pointer", what);
    MMTG_REQUIRE(B >= 1, "%s: B = %d must be positive", what, B);
    MMTG_REQUIRE(n >= 1, "%s: n = %ld must be positive", what, n);
    MMTG_REQUIRE(0 <= c_both && c_both <= c_img && c_img <= c_txt && c_txt <= 4294967296LL,
                 "%s: thresholds %lld, %lld, %lld must be monotone within 0 .. 2^32", what, c_both, c_img, c_txt);
    const size_t nin = (size_t)B * n * 4, nout = (size_t)B * n * (dtype == MMTG_F32 ? 4 : 2);
    MMTG_REQUIRE(!overlaps(img_out, nout, img, nin) && !overlaps(img_out, nout, txt, nin), "%s: img_out overlaps an input", what);
    MMTG_REQUIRE(!overlaps(txt_out, nout, img, nin) && !overlaps(txt_out, nout, txt, nin), "%s: txt_out overlaps an input", what);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_MISC, s, 0, 2.0 * (4.0 + (dtype == MMTG_F32 ? 4 : 2)) * B * n);
    const dim3 grid((unsigned)B, (unsigned)(n >= 2048 * 64 ? 64 : cdiv(n, 2048)), 2);
#define ED(T) hipLaunchKernelGGL(experience_drop_kernel<T>, grid, dim3(256), 0, s, img, txt, (T*)img_out, (T*)txt_out, code, n, seed, \
                                 (unsigned long long)c_both, (unsigned long long)c_img, (unsigned long long)c_txt)
    if (dtype == MMTG_F32) ED(float);
    else ED(bf16);
#undef ED
    MMTG_LAUNCH_CHECK("experience_drop");
    return MMTG_OK;
}

template <typename LT>
static void launch_guided_rows(int K, long M, hipStream_t s, const LT* cond, const LT* uncond, long ldl, int V, const float* lse_c,
                               const float* lse_u, const long long* targets, const Scales& sc, int P, int L, float* nll) {
#define GR(KK) hipLaunchKernelGGL((guided_row_kernel<LT, KK>), dim3((unsigned)M), dim3(256), 0, s, cond, uncond, ldl, V, lse_c, lse_u, \
                                  targets, sc, P, L, M, nll)
    switch (K) {
        case 1: GR(1); break;
        case 2: GR(2); break;
        case 3: GR(3); break;
        case 4: GR(4); break;
        case 5: GR(5); break;
        case 6: GR(6); break;
        case 7: GR(7); break;
        default: GR(8); break;
    }
#undef GR
}

extern "C" int mmtg_guided_loss(int logits_dtype, const void* cond, const void* uncond, long ldl, int V, const float* lse_c,
                                const float* lse_u, const long long* topic_ids, const long long* targets, const float* scales, int K,
                                int B, int P, int L, float batch_den, float* nll, float* sample_ce, float* ce, void* stream) {
    const char* what = "guided_loss";
    (void)topic_ids;            // (the labels of the loss rows all lie in targets)
    MMTG_REQUIRE(logits_dtype == MMTG_F32 || logits_dtype == MMTG_BF16, "%s: bad logits dtype %d", what, logits_dtype);
    MMTG_REQUIRE(cond, "%s: cond is a null pointer", what);
    MMTG_REQUIRE(uncond, "%s: uncond is a null pointer", what);
    MMTG_REQUIRE(lse_c, "%s: lse_c is a null pointer", what);
    MMTG_REQUIRE(lse_u, "%s: lse_u is a null pointer", what);
    MMTG_REQUIRE(targets, "%s: targets is a null pointer", what);
    MMTG_REQUIRE(scales, "%s: scales is a null pointer", what);
    MMTG_REQUIRE(nll, "%s: nll is a null pointer", what);
    MMTG_REQUIRE(sample_ce, "%s: sample_ce is a null pointer", what);
    MMTG_REQUIRE(ce, "%s: ce is a null pointer", what);
    MMTG_REQUIRE(K >= 1 && K <= MMTG_GUIDED_MAX_SCALES, "%s: K = %d scales (1 .. %d)", what, K, MMTG_GUIDED_MAX_SCALES);
    Scales sc;
    for (int k = 0; k < GK; ++k) {
        sc.s[k] = k < K ? scales[k] : 0.f;
        MMTG_REQUIRE(sc.s[k] >= 0.f && sc.s[k] <= 3.0e38f, "%s: scale %d = %g must be finite and >= 0", what, k, (double)sc.s[k]);
    }
    MMTG_REQUIRE(V >= 1, "%s: V = %d must be positive", what, V);
    MMTG_REQUIRE(ldl >= V, "%s: ldl %ld is below V %d", what, ldl, V);
    MMTG_REQUIRE(logits_dtype == MMTG_F32 || (ldl % 8 == 0 && MMTG_ALIGNED16(cond) && MMTG_ALIGNED16(uncond)),
                 "%s: bf16 rows must be 16-byte aligned (ldl %ld a multiple of 8, aligned bases)", what, ldl);
    MMTG_REQUIRE(logits_dtype == MMTG_BF16 || ((((uintptr_t)cond) | ((uintptr_t)uncond)) & 3) == 0, "%s: fp32 rows must be 4-byte aligned", what);
    MMTG_REQUIRE(B >= 1, "%s: B = %d must be positive", what, B);
    MMTG_REQUIRE(P >= 0, "%s: P = %d must not be negative", what, P);
    MMTG_REQUIRE(L >= 2, "%s: L = %d lyric columns; a loss row needs 2", what, L);
    MMTG_REQUIRE(batch_den > 0.f && batch_den <= 3.0e38f, "%s: batch_den = %g must be finite and > 0", what, (double)batch_den);
    const long M = (long)B * (P + L);
    MMTG_REQUIRE(M <= 0x7fffffffL, "%s: %ld rows", what, M);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_LOSS, s, (4.0 + 3.0 * K) * B * (L - 1) * V, (logits_dtype == MMTG_F32 ? 8.0 : 4.0) * B * (L - 1) * V);
    if (logits_dtype == MMTG_F32)
        launch_guided_rows<float>(K, M, s, (const float*)cond, (const float*)uncond, ldl, V, lse_c, lse_u, targets, sc, P, L, nll);
    else
        launch_guided_rows<bf16>(K, M, s, (const bf16*)cond, (const bf16*)uncond, ldl, V, lse_c, lse_u, targets, sc, P, L, nll);
    hipLaunchKernelGGL(guided_sample_kernel, dim3(1), dim3(1024), 0, s, (const float*)nll, K, B, P, L, M, batch_den, sample_ce, ce);
    MMTG_LAUNCH_CHECK("guided_loss");
    return MMTG_OK;
}
