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

// ---------------------------------------------------------------- guided cross-entropy, K logits matrices and G scale tuples
constexpr int MB = MMTG_GUIDED_MAX_BRANCHES;
template <typename LT> struct Mats { const LT* x[MB]; const float* lse[MB]; };
struct Weights { float w[GK][MB - 1]; };           // w[g][k - 1] = scale of tuple g for branch k, minus 1 (the host's fp32 subtraction)

// the rule, in mmtg_decode_guidance_multi's order: d[k - 1] = lc - l_k.  One expression for every K: a branch with w = 0 (or d = 0)
// adds +-0 and leaves the bits of the K - 1 form.  The step is an EXPLICIT fused multiply-add, and the functions below switch the
// compiler's own contraction off: left to it, the K = 2 instantiation fused the step (v_fmac_f32) where K = 3 multiplied and added
// in packed halves (v_pk_mul_f32, v_pk_add_f32), and the two forms round differently.
template <int K>
__device__ __forceinline__ float guide_multi(float lc, const float (&d)[MB - 1], const float (&w)[MB - 1]) {
    float g = lc;
#pragma unroll
    for (int k = 1; k < K; ++k) g = __builtin_fmaf(w[k - 1], d[k - 1], g);
    return g;
}

// eight logits of each of the K rows into the G running (max, sum)s of a thread: fold8's steps per tuple
template <int K, int G>
__device__ __forceinline__ void fold8_multi(const float (&x)[MB][8], const float (&Ls)[MB], const Weights& wt, float (&mx)[GK],
                                            float (&sm)[GK]) {
#pragma clang fp contract(off)
    float lc[8], d[8][MB - 1];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        lc[e] = x[0][e] - Ls[0];
#pragma unroll
        for (int k = 1; k < K; ++k) d[e][k - 1] = lc[e] - (x[k][e] - Ls[k]);
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = guide_multi<K>(lc[e], d[e], wt.w[g]);
        const float m8 = fmaxf(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])), fmaxf(fmaxf(v[4], v[5]), fmaxf(v[6], v[7])));
        if (m8 > mx[g]) { sm[g] *= exp_fast(mx[g] - m8); mx[g] = m8; }
#pragma unroll
        for (int e = 0; e < 8; ++e) sm[g] += exp_fast(v[e] - mx[g]);
    }
}

// one workgroup per row m: nll[g * M + m] for g < G, from the K rows x[k] + m * ldl.  guided_row_kernel's trip structure: slices of
// 2048 logits (eight per thread), two in flight, then the odd trailing slice, then the tail V % 8 -- or, where one of the K rows is
// not 16-byte aligned, every logit on its own.  The 2 K (or K) loads of a trip are issued before the first is used.
template <typename LT, int K, int G>
__global__ __launch_bounds__(256) void guided_multi_row_kernel(Mats<LT> mt, long ldl, int V, const long long* __restrict__ targets,
        Weights wt, int P, int L, long M, float* __restrict__ nll) {
#pragma clang fp contract(off)
    __shared__ float shm[GK][4];
    __shared__ float shs[GK][4];
    const int Tt = P + L;
    const long m = blockIdx.x;
    const int b = (int)(m / Tt), t = (int)(m % Tt), tid = threadIdx.x;
    if (t < P || t + 1 >= Tt) {
        if (tid < G) nll[(long)tid * M + m] = 0.f;
        return;
    }
    const LT* r[MB];
    float Ls[MB];
    uintptr_t bits = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        r[k] = mt.x[k] + m * ldl;
        Ls[k] = mt.lse[k][m];
        bits |= reinterpret_cast<uintptr_t>(r[k]);
    }
    float mx[GK], sm[GK];
#pragma unroll
    for (int g = 0; g < GK; ++g) { mx[g] = -INFINITY; sm[g] = 0.f; }
    int done = 0;
    if ((bits & 15) == 0) {
        const int V8 = V & ~7;
        int v = tid * 8;
        for (; v + 2048 < V8; v += 4096) {
            float x0[MB][8], x1[MB][8];
#pragma unroll
            for (int k = 0; k < K; ++k) load8(r[k] + v, x0[k]);
#pragma unroll
            for (int k = 0; k < K; ++k) load8(r[k] + v + 2048, x1[k]);
            fold8_multi<K, G>(x0, Ls, wt, mx, sm);
            fold8_multi<K, G>(x1, Ls, wt, mx, sm);
        }
        if (v < V8) {
            float x0[MB][8];
#pragma unroll
            for (int k = 0; k < K; ++k) load8(r[k] + v, x0[k]);
            fold8_multi<K, G>(x0, Ls, wt, mx, sm);
        }
        done = V8;
    }
    for (int v = done + tid; v < V; v += 256) {
        float x[MB], d[MB - 1];
#pragma unroll
        for (int k = 0; k < K; ++k) x[k] = (float)r[k][v];
        const float lc = x[0] - Ls[0];
#pragma unroll
        for (int k = 1; k < K; ++k) d[k - 1] = lc - (x[k] - Ls[k]);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float gv = guide_multi<K>(lc, d, wt.w[g]);
            if (gv > mx[g]) { sm[g] *= exp_fast(mx[g] - gv); mx[g] = gv; }
            sm[g] += exp_fast(gv - mx[g]);
        }
    }
    // fixed order: the wave's butterfly, then the four waves' pairs in wave order
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float om = __shfl_xor(mx[g], off, 64);
            const float os = __shfl_xor(sm[g], off, 64);
            ms_merge(mx[g], sm[g], om, os);
        }
        if ((tid & 63) == 0) { shm[g][tid >> 6] = mx[g]; shs[g][tid >> 6] = sm[g]; }
    }
    __syncthreads();
    if (tid < G) {
        float mm = shm[tid][0], sv = shs[tid][0];
        for (int w = 1; w < 4; ++w) ms_merge(mm, sv, shm[tid][w], shs[tid][w]);
        long long lab = targets[(long)b * L + (t + 1 - P)];
        if (lab < 0) lab = 0;
        if (lab >= V) lab = V - 1;
        float d[MB - 1], w[MB - 1];
        const float lc = (float)r[0][lab] - Ls[0];
#pragma unroll
        for (int k = 1; k < K; ++k) {
            d[k - 1] = lc - ((float)r[k][lab] - Ls[k]);
            w[k - 1] = wt.w[tid][k - 1];
        }
        nll[(long)tid * M + m] = (mm + logf(sv)) - guide_multi<K>(lc, d, w);
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

template <typename LT, int K>
static void launch_guided_multi_rows(int G, long M, hipStream_t s, const Mats<LT>& mt, long ldl, int V, const long long* targets,
                                     const Weights& wt, int P, int L, float* nll) {
#define GM(GG) hipLaunchKernelGGL((guided_multi_row_kernel<LT, K, GG>), dim3((unsigned)M), dim3(256), 0, s, mt, ldl, V, targets, wt, P, L, M, nll)
    switch (G) {
        case 1: GM(1); break;
        case 2: GM(2); break;
        case 3: GM(3); break;
        case 4: GM(4); break;
        case 5: GM(5); break;
        case 6: GM(6); break;
        case 7: GM(7); break;
        default: GM(8); break;
    }
#undef GM
}

template <typename LT>
static void launch_guided_multi(int K, int G, long M, hipStream_t s, const void* const* logits, const float* const* lse, long ldl, int V,
                                const long long* targets, const Weights& wt, int P, int L, float* nll) {
    Mats<LT> mt;
    for (int k = 0; k < MB; ++k) {          // (the slots behind K repeat matrix 0: never read)
        mt.x[k] = (const LT*)logits[k < K ? k : 0];
        mt.lse[k] = lse[k < K ? k : 0];
    }
    if (K == 2) launch_guided_multi_rows<LT, 2>(G, M, s, mt, ldl, V, targets, wt, P, L, nll);
    else if (K == 3) launch_guided_multi_rows<LT, 3>(G, M, s, mt, ldl, V, targets, wt, P, L, nll);
    else launch_guided_multi_rows<LT, 4>(G, M, s, mt, ldl, V, targets, wt, P, L, nll);
}

extern "C" int mmtg_guided_loss_multi(int logits_dtype, const void* const* logits, const float* const* lse, int K, long ldl, int V,
                                      const long long* targets, const float* scales, int G, int B, int P, int L, float batch_den,
                                      float* nll, float* sample_ce, float* ce, void* stream) {
    const char* what = "guided_loss_multi";
    MMTG_REQUIRE(logits_dtype == MMTG_F32 || logits_dtype == MMTG_BF16, "%s: bad logits dtype %d", what, logits_dtype);
    MMTG_REQUIRE(logits, "%s: logits is a null pointer", what);
    MMTG_REQUIRE(lse, "%s: lse is a null pointer", what);
    MMTG_REQUIRE(targets, "%s: targets is a null pointer", what);
    MMTG_REQUIRE(scales, "%s: scales is a null pointer", what);
    MMTG_REQUIRE(nll, "%s: nll is a null pointer", what);
    MMTG_REQUIRE(sample_ce, "%s: sample_ce is a null pointer", what);
    MMTG_REQUIRE(ce, "%s: ce is a null pointer", what);
    MMTG_REQUIRE(K >= 2 && K <= MMTG_GUIDED_MAX_BRANCHES, "%s: K = %d logits matrices (2 .. %d)", what, K, MMTG_GUIDED_MAX_BRANCHES);
    MMTG_REQUIRE(G >= 1 && G <= MMTG_GUIDED_MAX_SCALES, "%s: G = %d scale tuples (1 .. %d)", what, G, MMTG_GUIDED_MAX_SCALES);
    for (int k = 0; k < K; ++k) {
        MMTG_REQUIRE(logits[k], "%s: logits[%d] is a null pointer", what, k);
        MMTG_REQUIRE(lse[k], "%s: lse[%d] is a null pointer", what, k);
    }
    Weights wt;
    for (int g = 0; g < GK; ++g)
        for (int k = 1; k < MB; ++k) {
            float sv = 1.f;
            if (g < G && k < K) {
                sv = scales[g * (K - 1) + (k - 1)];
                MMTG_REQUIRE(sv >= 0.f && sv <= 3.0e38f, "%s: scale %d of tuple %d = %g must be finite and >= 0", what, k - 1, g, (double)sv);
            }
            wt.w[g][k - 1] = sv - 1.f;
        }
    MMTG_REQUIRE(V >= 1, "%s: V = %d must be positive", what, V);
    MMTG_REQUIRE(ldl >= V, "%s: ldl %ld is below V %d", what, ldl, V);
    for (int k = 0; k < K; ++k) {
        MMTG_REQUIRE(logits_dtype == MMTG_F32 || (ldl % 8 == 0 && MMTG_ALIGNED16(logits[k])),
                     "%s: bf16 rows must be 16-byte aligned (ldl %ld a multiple of 8, aligned bases; matrix %d)", what, ldl, k);
        MMTG_REQUIRE(logits_dtype == MMTG_BF16 || (((uintptr_t)logits[k]) & 3) == 0, "%s: fp32 rows must be 4-byte aligned (matrix %d)", what, k);
    }
    MMTG_REQUIRE(B >= 1, "%s: B = %d must be positive", what, B);
    MMTG_REQUIRE(P >= 0, "%s: P = %d must not be negative", what, P);
    MMTG_REQUIRE(L >= 2, "%s: L = %d lyric columns; a loss row needs 2", what, L);
    MMTG_REQUIRE(batch_den > 0.f && batch_den <= 3.0e38f, "%s: batch_den = %g must be finite and > 0", what, (double)batch_den);
    const long M = (long)B * (P + L);
    MMTG_REQUIRE(M <= 0x7fffffffL, "%s: %ld rows", what, M);
    const size_t es = logits_dtype == MMTG_F32 ? 4 : 2;
    for (int k = 0; k < K; ++k)
        MMTG_REQUIRE(!overlaps(nll, (size_t)G * M * 4, logits[k], ((size_t)(M - 1) * ldl + V) * es), "%s: nll overlaps logits matrix %d", what, k);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_LOSS, s, (3.0 * (K - 1) + 1.0 + (2.0 * (K - 1) + 3.0) * G) * B * (L - 1) * V, (double)es * K * B * (L - 1) * V);
    if (logits_dtype == MMTG_F32) launch_guided_multi<float>(K, G, M, s, logits, (const float* const*)lse, ldl, V, targets, wt, P, L, nll);
    else launch_guided_multi<bf16>(K, G, M, s, logits, (const float* const*)lse, ldl, V, targets, wt, P, L, nll);
    hipLaunchKernelGGL(guided_sample_kernel, dim3(1), dim3(1024), 0, s, (const float*)nll, G, B, P, L, M, batch_den, sample_ce, ce);
    MMTG_LAUNCH_CHECK("guided_loss_multi");
    return MMTG_OK;
}
