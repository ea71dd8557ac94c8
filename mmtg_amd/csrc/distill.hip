// Distillation of a teacher's (guided) distribution into the step's own logits (MMTGTrainer(distill_weight=...)): the row term
// KL(q || p) of the student's softmax p against q = softmax(lu + s (lc - lu)) of a teacher's conditional and negative logits (or
// softmax(lc) with no negative), and mmtg_loss_bwd with the term's gradient w (p - q) folded in.  include/mmtg_hip.h states the
// rule.  A source file of its own: every other kernel compiles to the same code as before.
//
// distill_row_kernel is a streaming row kernel like guided_row_kernel: the three row log-sum-exps are inputs, so g and log p are
// known at the first touch of an element and the triple (max g, S = sum e^(g - max), A = sum e^(g - max) (g - log p)) runs online;
// S and A are rescaled together when the max moves.  Nothing is staged, so V has no limit.  The exponentials are v_exp_f32.
#include <math.h>

#include "common.h"

namespace {

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

// the teacher's guided log-probability before its normaliser, in mmtg_decode_guidance's order; with no negative it is lc
template <bool HASU>
__device__ __forceinline__ float guide(float c, float u, float Lc, float Lu, float s) {
    const float lc = c - Lc;
    if constexpr (!HASU) return lc;
    else {
        const float lu = u - Lu;
        return lu + s * (lc - lu);
    }
}

// one element into a thread's running triple
__device__ __forceinline__ void fold1(float g, float logp, float& mx, float& S, float& A) {
    if (g > mx) {
        const float r = exp_fast(mx - g);
        S *= r; A *= r; mx = g;
    }
    const float e = exp_fast(g - mx);
    S += e;
    A += e * (g - logp);
}

// two triples as one; a part that holds nothing has max -inf, S = A = 0
__device__ __forceinline__ void msa_merge(float& m, float& S, float& A, float om, float oS, float oA) {
    const float nm = fmaxf(m, om);
    if (nm == -INFINITY) { S = 0.f; A = 0.f; }
    else {
        const float r = exp_fast(m - nm), q = exp_fast(om - nm);
        S = S * r + oS * q;
        A = A * r + oA * q;
    }
    m = nm;
}

// one workgroup per row m: kd_row[m] = KL(q || p) and kd_lg[m] = Lg on the loss rows (P <= t <= Tt - 2), 0 on the others
template <typename LT, typename TT, bool HASU>
__global__ __launch_bounds__(256) void distill_row_kernel(const LT* __restrict__ logits, long ldl, const TT* __restrict__ cond,
        const TT* __restrict__ uncond, long ldt, int V, const float* __restrict__ lse, const float* __restrict__ lse_c,
        const float* __restrict__ lse_u, float s, int P, int L, float* __restrict__ kd_row, float* __restrict__ kd_lg) {
    __shared__ float shm[4], shs[4], sha[4];
    const int Tt = P + L;
    const long m = blockIdx.x;
    const int t = (int)(m % Tt), tid = threadIdx.x;
    if (t < P || t + 1 >= Tt) {
        if (tid == 0) { kd_row[m] = 0.f; kd_lg[m] = 0.f; }
        return;
    }
    const LT* x = logits + m * ldl;
    const TT* c = cond + m * ldt;
    const TT* u = HASU ? uncond + m * ldt : c;
    const float l = lse[m], Lc = lse_c[m], Lu = HASU ? lse_u[m] : 0.f;
    float mx = -INFINITY, S = 0.f, A = 0.f;
    int done = 0;
    if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(u)) & 15) == 0) {
        const int V8 = V & ~7;
        for (int v = tid * 8; v < V8; v += 2048) {
            float x8[8], c8[8], u8[8];
            load8(x + v, x8); load8(c + v, c8);
            if constexpr (HASU) load8(u + v, u8);
            float g[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) g[e] = guide<HASU>(c8[e], HASU ? u8[e] : 0.f, Lc, Lu, s);
            const float m8 = fmaxf(fmaxf(fmaxf(g[0], g[1]), fmaxf(g[2], g[3])), fmaxf(fmaxf(g[4], g[5]), fmaxf(g[6], g[7])));
            if (m8 > mx) {
                const float r = exp_fast(mx - m8);
                S *= r; A *= r; mx = m8;
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float ex = exp_fast(g[e] - mx);
                S += ex;
                A += ex * (g[e] - (x8[e] - l));
            }
        }
        done = V8;
    }
    for (int v = done + tid; v < V; v += 256)
        fold1(guide<HASU>((float)c[v], HASU ? (float)u[v] : 0.f, Lc, Lu, s), (float)x[v] - l, mx, S, A);
    // fixed order: the wave's butterfly, then the four waves' triples in wave order
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float om = __shfl_xor(mx, off, 64), oS = __shfl_xor(S, off, 64), oA = __shfl_xor(A, off, 64);
        msa_merge(mx, S, A, om, oS, oA);
    }
    if ((tid & 63) == 0) { shm[tid >> 6] = mx; shs[tid >> 6] = S; sha[tid >> 6] = A; }
    __syncthreads();
    if (tid == 0) {
        float mm = shm[0], sv = shs[0], av = sha[0];
        for (int w = 1; w < 4; ++w) msa_merge(mm, sv, av, shm[w], shs[w], sha[w]);
        const float Lg = mm + logf(sv);
        kd_lg[m] = Lg;
        kd_row[m] = av / sv - Lg;
    }
}

// single workgroup: kd_sample [B] (one wave per sample, the loss rows spread over its lanes), then kd in sample order
__global__ __launch_bounds__(1024) void distill_sample_kernel(const float* __restrict__ kd_row, int B, int P, int L, float batch_den,
        float* __restrict__ kd_sample, float* __restrict__ kd) {
    const int Tt = P + L;
    const int ntok = Tt - 1 - P;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int b = wave; b < B; b += 16) {
        float s = 0.f;
        for (int t = P + lane; t < Tt - 1; t += 64) s += kd_row[(long)b * Tt + t];
        s = wave_sum(s);
        if (lane == 0) kd_sample[b] = s / ntok;
    }
    __syncthreads();            // (the workgroup's own global writes are visible behind the barrier)
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += kd_sample[b];       // fixed order
        kd[0] = s / batch_den;
    }
}

// loss_bwd_kernel (csrc/loss.hip) with w (p_v - q_v) added on the loss rows.  A row without the term (w == 0, or t < P) runs
// loss_bwd_kernel's expression alone and writes its bits.  dlogits may alias logits when both are stored in one type: a thread
// rewrites only what it read.  plane > 0: the (hi | lo) bf16 plane pair of the x3 mode.
template <typename T, typename LT, typename TT, bool HASU>
__global__ __launch_bounds__(256) void loss_bwd_kd_kernel(const LT* logits, long ldl, int V, const long long* __restrict__ topic_ids,
        const long long* __restrict__ targets, const float* __restrict__ lse, const float* __restrict__ coef, float gscale,
        float lm_coef, const TT* __restrict__ cond, const TT* __restrict__ uncond, long ldt, const float* __restrict__ lse_c,
        const float* __restrict__ lse_u, float s, const float* __restrict__ kd_lg, float w, int P, int L, T* dlogits, long ldd,
        int Vpad, long plane) {
    const int Tt = P + L;
    const long m = blockIdx.x;
    const int b = (int)(m / Tt), t = (int)(m % Tt);
    T* drow = dlogits + m * ldd;
    const bool active = t + 1 < Tt && (t >= P || lm_coef != 0.f);
    const bool dvec = (Vpad & 7) == 0 && (reinterpret_cast<uintptr_t>(drow) & 15) == 0 &&
                      (plane == 0 || (reinterpret_cast<uintptr_t>(drow + plane) & 15) == 0);
    if (!active) {
        if (dvec) {
            typedef typename Vec16<T>::type V16;
            V16 z;
#pragma unroll
            for (int e = 0; e < Vec16<T>::N; ++e) z[e] = (T)0.f;
            for (int v = threadIdx.x * Vec16<T>::N; v < Vpad; v += 256 * Vec16<T>::N) {
                *reinterpret_cast<V16*>(drow + v) = z;
                if (plane) *reinterpret_cast<V16*>(drow + plane + v) = z;
            }
        } else {
            for (int v = threadIdx.x; v < Vpad; v += 256) {
                drow[v] = (T)0.f;
                if (plane) drow[plane + v] = (T)0.f;
            }
        }
        return;
    }
    const LT* row = logits + m * ldl;
    const bool kd = t >= P && w != 0.f;         // (uniform over the workgroup)
    const TT* c = cond + m * ldt;
    const TT* u = HASU ? uncond + m * ldt : c;
    const float l = lse[m], cf = (t >= P ? coef[b] * gscale : 0.f) + lm_coef;
    const float Lc = kd ? lse_c[m] : 0.f, Lu = kd && HASU ? lse_u[m] : 0.f, Lg = kd ? kd_lg[m] : 0.f;
    long long lab = t + 1 < P ? topic_ids[(long)b * P + t + 1] : targets[(long)b * L + (t + 1 - P)];
    if (lab < 0) lab = 0;
    if (lab >= V) lab = V - 1;
    // the 16-byte path reads the row up to Vpad: every matrix it touches must hold that many columns on an aligned row
    bool vec = dvec && ldl >= Vpad && (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    if (kd) vec = vec && ldt >= Vpad && ((reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(u)) & 15) == 0;
    if (vec) {
        for (int v = threadIdx.x * 8; v < Vpad; v += 2048) {
            float d[8], x[8], c8[8], u8[8];
            load8(row + v, x);
            if (kd) {
                load8(c + v, c8);
                if constexpr (HASU) load8(u + v, u8);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int vv = v + e;
                const float pv = expf(x[e] - l);
                float dv = cf * (pv - (vv == (int)lab ? 1.f : 0.f));
                if (kd) dv += w * (pv - exp_fast(guide<HASU>(c8[e], HASU ? u8[e] : 0.f, Lc, Lu, s) - Lg));
                d[e] = vv < V ? dv : 0.f;
            }
            if constexpr (sizeof(T) == 2) {
                bf16x8 o = {(bf16)d[0], (bf16)d[1], (bf16)d[2], (bf16)d[3], (bf16)d[4], (bf16)d[5], (bf16)d[6], (bf16)d[7]};
                *reinterpret_cast<bf16x8*>(drow + v) = o;
                if (plane) {
                    bf16x8 lo;
#pragma unroll
                    for (int e = 0; e < 8; ++e) lo[e] = (bf16)(d[e] - (float)o[e]);
                    *reinterpret_cast<bf16x8*>(drow + plane + v) = lo;
                }
            } else {
                *reinterpret_cast<f32x4*>(drow + v) = f32x4{d[0], d[1], d[2], d[3]};
                *reinterpret_cast<f32x4*>(drow + v + 4) = f32x4{d[4], d[5], d[6], d[7]};
            }
        }
        return;
    }
    for (int v = threadIdx.x; v < Vpad; v += 256) {
        float d = 0.f;
        if (v < V) {
            const float pv = expf((float)row[v] - l);
            d = cf * (pv - (v == (int)lab ? 1.f : 0.f));
            if (kd) d += w * (pv - exp_fast(guide<HASU>((float)c[v], HASU ? (float)u[v] : 0.f, Lc, Lu, s) - Lg));
        }
        const T hi = (T)d;
        drow[v] = hi;
        if constexpr (sizeof(T) == 2) {
            if (plane) drow[plane + v] = (bf16)(d - (float)hi);
        }
    }
}

// whether the byte ranges [a, a + na) and [b, b + nb) share a byte
bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + na, b0 = (uintptr_t)b, b1 = b0 + nb;
    return a0 < b1 && b0 < a1;
}

bool finite_nonneg(float v) { return v >= 0.f && v <= 3.0e38f; }       // (NaN fails both comparisons)

size_t esize(int dtype) { return dtype == MMTG_F32 ? 4 : 2; }

// what the three entries refuse alike about the teacher; 0 when all is well
int check_teacher(const char* what, int teacher_dtype, const void* cond, const void* uncond, long ldt, int V, const float* lse_c,
                  const float* lse_u, float scale) {
    MMTG_REQUIRE(teacher_dtype == MMTG_F32 || teacher_dtype == MMTG_BF16, "%s: bad teacher dtype %d", what, teacher_dtype);
    MMTG_REQUIRE(cond, "%s: cond is a null pointer", what);
    MMTG_REQUIRE(lse_c, "%s: lse_c is a null pointer", what);
    MMTG_REQUIRE((uncond == nullptr) == (lse_u == nullptr), "%s: uncond and lse_u are null together or not at all", what);
    MMTG_REQUIRE(finite_nonneg(scale), "%s: scale = %g must be finite and >= 0", what, (double)scale);
    MMTG_REQUIRE(ldt >= V, "%s: ldt %ld is below V %d", what, ldt, V);
    MMTG_REQUIRE(teacher_dtype == MMTG_F32 || (ldt % 8 == 0 && MMTG_ALIGNED16(cond) && MMTG_ALIGNED16(uncond)),
                 "%s: bf16 teacher rows must be 16-byte aligned (ldt %ld a multiple of 8, aligned bases)", what, ldt);
    MMTG_REQUIRE(teacher_dtype == MMTG_BF16 || ((((uintptr_t)cond) | ((uintptr_t)uncond)) & 3) == 0,
                 "%s: fp32 teacher rows must be 4-byte aligned", what);
    return MMTG_OK;
}

// does the output [out, out + n) touch a teacher input
bool hits_teacher(const void* out, size_t n, int teacher_dtype, const void* cond, const void* uncond, long ldt, int V, const float* lse_c,
                  const float* lse_u, long M) {
    const size_t nt = ((size_t)(M - 1) * ldt + V) * esize(teacher_dtype), nl = (size_t)M * 4;
    return overlaps(out, n, cond, nt) || (uncond && overlaps(out, n, uncond, nt)) || overlaps(out, n, lse_c, nl) ||
           (lse_u && overlaps(out, n, lse_u, nl));
}

struct BwdArgs {
    const void* logits; long ldl; int V; const long long* topic_ids; const long long* targets; const float* lse; const float* coef;
    float gscale, lm_coef; const void* cond; const void* uncond; long ldt; const float* lse_c; const float* lse_u; float scale;
    const float* kd_lg; float kd_coef; int P, L; void* dlogits; long ldd; int Vpad; long plane;
};

template <typename T, typename LT, typename TT, bool HASU>
void launch_bwd(const BwdArgs& a, long M, hipStream_t s) {
    hipLaunchKernelGGL((loss_bwd_kd_kernel<T, LT, TT, HASU>), dim3((unsigned)M), dim3(256), 0, s, (const LT*)a.logits, a.ldl, a.V,
                       a.topic_ids, a.targets, a.lse, a.coef, a.gscale, a.lm_coef, (const TT*)a.cond, (const TT*)a.uncond, a.ldt, a.lse_c,
                       a.lse_u, a.scale, a.kd_lg, a.kd_coef, a.P, a.L, (T*)a.dlogits, a.ldd, a.Vpad, a.plane);
}
template <typename T, typename LT>
void launch_bwd_t(int teacher_dtype, const BwdArgs& a, long M, hipStream_t s) {
    if (teacher_dtype == MMTG_F32) {
        if (a.uncond) launch_bwd<T, LT, float, true>(a, M, s);
        else launch_bwd<T, LT, float, false>(a, M, s);
    } else {
        if (a.uncond) launch_bwd<T, LT, bf16, true>(a, M, s);
        else launch_bwd<T, LT, bf16, false>(a, M, s);
    }
}

template <typename LT, typename TT>
void launch_fwd(const void* logits, long ldl, const void* cond, const void* uncond, long ldt, int V, const float* lse, const float* lse_c,
                const float* lse_u, float scale, int P, int L, long M, float* kd_row, float* kd_lg, hipStream_t s) {
    if (uncond)
        hipLaunchKernelGGL((distill_row_kernel<LT, TT, true>), dim3((unsigned)M), dim3(256), 0, s, (const LT*)logits, ldl, (const TT*)cond,
                           (const TT*)uncond, ldt, V, lse, lse_c, lse_u, scale, P, L, kd_row, kd_lg);
    else
        hipLaunchKernelGGL((distill_row_kernel<LT, TT, false>), dim3((unsigned)M), dim3(256), 0, s, (const LT*)logits, ldl, (const TT*)cond,
                           (const TT*)uncond, ldt, V, lse, lse_c, lse_u, scale, P, L, kd_row, kd_lg);
}

}  // namespace

extern "C" int mmtg_distill_fwd(int logits_dtype, const void* logits, long ldl, int teacher_dtype, const void* cond, const void* uncond,
                                long ldt, int V, const float* lse, const float* lse_c, const float* lse_u, float scale, int B, int P,
                                int L, float batch_den, float* kd_row, float* kd_lg, float* kd_sample, float* kd, void* stream) {
    const char* what = "distill_fwd";
    MMTG_REQUIRE(logits_dtype == MMTG_F32 || logits_dtype == MMTG_BF16, "%s: bad logits dtype %d", what, logits_dtype);
    MMTG_REQUIRE(logits, "%s: logits is a null pointer", what);
    MMTG_REQUIRE(lse, "%s: lse is a null pointer", what);
    MMTG_REQUIRE(kd_row, "%s: kd_row is a null pointer", what);
    MMTG_REQUIRE(kd_lg, "%s: kd_lg is a null pointer", what);
    MMTG_REQUIRE(kd_sample, "%s: kd_sample is a null pointer", what);
    MMTG_REQUIRE(kd, "%s: kd is a null pointer", what);
    MMTG_REQUIRE(V >= 1, "%s: V = %d must be positive", what, V);
    MMTG_REQUIRE(ldl >= V, "%s: ldl %ld is below V %d", what, ldl, V);
    if (int rc = check_teacher(what, teacher_dtype, cond, uncond, ldt, V, lse_c, lse_u, scale)) return rc;
    MMTG_REQUIRE(logits_dtype == MMTG_F32 || (ldl % 8 == 0 && MMTG_ALIGNED16(logits)),
                 "%s: bf16 rows must be 16-byte aligned (ldl %ld a multiple of 8, an aligned base)", what, ldl);
    MMTG_REQUIRE(logits_dtype == MMTG_BF16 || (((uintptr_t)logits) & 3) == 0, "%s: fp32 rows must be 4-byte aligned", what);
    MMTG_REQUIRE(B >= 1, "%s: B = %d must be positive", what, B);
    MMTG_REQUIRE(P >= 0, "%s: P = %d must not be negative", what, P);
    MMTG_REQUIRE(L >= 2, "%s: L = %d lyric columns; a loss row needs 2", what, L);
    MMTG_REQUIRE(batch_den > 0.f && batch_den <= 3.0e38f, "%s: batch_den = %g must be finite and > 0", what, (double)batch_den);
    const long M = (long)B * (P + L);
    MMTG_REQUIRE(M <= 0x7fffffffL, "%s: %ld rows", what, M);
    MMTG_REQUIRE(!hits_teacher(kd_row, (size_t)M * 4, teacher_dtype, cond, uncond, ldt, V, lse_c, lse_u, M) &&
                 !hits_teacher(kd_lg, (size_t)M * 4, teacher_dtype, cond, uncond, ldt, V, lse_c, lse_u, M) &&
                 !hits_teacher(kd_sample, (size_t)B * 4, teacher_dtype, cond, uncond, ldt, V, lse_c, lse_u, M) &&
                 !hits_teacher(kd, 4, teacher_dtype, cond, uncond, ldt, V, lse_c, lse_u, M), "%s: an output overlaps a teacher input", what);
    hipStream_t s = (hipStream_t)stream;
    const double rows = (double)B * (L - 1);
    ProfScope prof(MMTG_PROF_LOSS, s, 12.0 * rows * V, (esize(logits_dtype) + (uncond ? 2.0 : 1.0) * esize(teacher_dtype)) * rows * V);
#define DF(LT, TT) launch_fwd<LT, TT>(logits, ldl, cond, uncond, ldt, V, lse, lse_c, lse_u, scale, P, L, M, kd_row, kd_lg, s)
    if (logits_dtype == MMTG_F32) { if (teacher_dtype == MMTG_F32) DF(float, float); else DF(float, bf16); }
    else { if (teacher_dtype == MMTG_F32) DF(bf16, float); else DF(bf16, bf16); }
#undef DF
    hipLaunchKernelGGL(distill_sample_kernel, dim3(1), dim3(1024), 0, s, (const float*)kd_row, B, P, L, batch_den, kd_sample, kd);
    MMTG_LAUNCH_CHECK("distill_fwd");
    return MMTG_OK;
}

// the checks mmtg_loss_bwd_kd and mmtg_loss_bwd_kd_x3 share, then the launch (plane == 0: rows of `dtype`; else the plane pair)
static int loss_bwd_kd_any(const char* what, int dtype, int logits_dtype, int teacher_dtype, const BwdArgs& a, int B, void* stream) {
    MMTG_REQUIRE(a.logits, "%s: logits is a null pointer", what);
    MMTG_REQUIRE(a.targets, "%s: targets is a null pointer", what);
    MMTG_REQUIRE(a.lse, "%s: lse is a null pointer", what);
    MMTG_REQUIRE(a.coef, "%s: coef is a null pointer", what);
    MMTG_REQUIRE(a.kd_lg, "%s: kd_lg is a null pointer", what);
    MMTG_REQUIRE(a.dlogits, "%s: dlogits is a null pointer", what);
    MMTG_REQUIRE(dtype == MMTG_F32 || dtype == MMTG_BF16, "%s: bad dtype %d", what, dtype);
    MMTG_REQUIRE(logits_dtype == MMTG_F32 || (logits_dtype == MMTG_BF16 && dtype == MMTG_BF16), "%s: bf16 logits go with bf16 dlogits", what);
    MMTG_REQUIRE(a.V >= 1, "%s: V = %d must be positive", what, a.V);
    MMTG_REQUIRE(a.ldl >= a.V, "%s: ldl %ld is below V %d", what, a.ldl, a.V);
    MMTG_REQUIRE(a.Vpad >= a.V && a.ldd >= a.Vpad, "%s: Vpad %d is below V %d or ldd %ld below Vpad", what, a.Vpad, a.V, a.ldd);
    if (int rc = check_teacher(what, teacher_dtype, a.cond, a.uncond, a.ldt, a.V, a.lse_c, a.lse_u, a.scale)) return rc;
    MMTG_REQUIRE(logits_dtype == MMTG_F32 || (a.ldl % 8 == 0 && MMTG_ALIGNED16(a.logits)),
                 "%s: bf16 rows must be 16-byte aligned (ldl %ld a multiple of 8, an aligned base)", what, a.ldl);
    MMTG_REQUIRE(logits_dtype == MMTG_BF16 || (((uintptr_t)a.logits) & 3) == 0, "%s: fp32 rows must be 4-byte aligned", what);
    MMTG_REQUIRE((((uintptr_t)a.dlogits) & (esize(dtype) - 1)) == 0, "%s: dlogits is misaligned", what);
    MMTG_REQUIRE(B >= 1, "%s: B = %d must be positive", what, B);
    MMTG_REQUIRE(a.P >= 0, "%s: P = %d must not be negative", what, a.P);
    MMTG_REQUIRE(a.L >= 2, "%s: L = %d lyric columns; a loss row needs 2", what, a.L);
    MMTG_REQUIRE(a.P == 0 || a.lm_coef == 0.f || a.topic_ids, "%s: topic_ids required (the LM-loss rows t < P read them)", what);
    MMTG_REQUIRE(finite_nonneg(a.kd_coef), "%s: kd_coef = %g must be finite and >= 0", what, (double)a.kd_coef);
    MMTG_REQUIRE(a.logits != a.dlogits || (logits_dtype == dtype && a.ldl == a.ldd && a.plane == 0),
                 "%s: in-place needs one storage type and one row stride", what);
    const long M = (long)B * (a.P + a.L);
    MMTG_REQUIRE(M <= 0x7fffffffL, "%s: %ld rows", what, M);
    if (a.plane) {
        MMTG_REQUIRE(a.Vpad % 8 == 0 && a.ldd % 8 == 0 && MMTG_ALIGNED16(a.dlogits), "%s: Vpad, ldd multiples of 8 and aligned planes", what);
        MMTG_REQUIRE(a.plane % 8 == 0 && a.plane >= (M - 1) * a.ldd + a.Vpad, "%s: the lo plane must lie behind the hi plane", what);
    }
    const size_t nout = ((size_t)a.plane + (size_t)(M - 1) * a.ldd + a.Vpad) * esize(dtype);
    MMTG_REQUIRE(!hits_teacher(a.dlogits, nout, teacher_dtype, a.cond, a.uncond, a.ldt, a.V, a.lse_c, a.lse_u, M) &&
                 !overlaps(a.dlogits, nout, a.kd_lg, (size_t)M * 4), "%s: dlogits overlaps a teacher input", what);
    hipStream_t s = (hipStream_t)stream;
    const double tb = (a.kd_coef != 0.f ? (a.uncond ? 2.0 : 1.0) * esize(teacher_dtype) : 0.0) * B * (a.L - 1) * a.V;
    ProfScope prof(MMTG_PROF_LOSS, s, 8.0 * M * a.V, (esize(logits_dtype) + (a.plane ? 4.0 : (double)esize(dtype))) * M * a.V + tb);
    if (dtype == MMTG_F32) launch_bwd_t<float, float>(teacher_dtype, a, M, s);
    else if (logits_dtype == MMTG_F32) launch_bwd_t<bf16, float>(teacher_dtype, a, M, s);
    else launch_bwd_t<bf16, bf16>(teacher_dtype, a, M, s);
    MMTG_LAUNCH_CHECK(what);
    return MMTG_OK;
}

extern "C" int mmtg_loss_bwd_kd(int dtype, int logits_dtype, const void* logits, long ldl, int V, const long long* topic_ids,
                                const long long* targets, const float* lse, const float* coef, float gscale, float lm_coef,
                                int teacher_dtype, const void* cond, const void* uncond, long ldt, const float* lse_c, const float* lse_u,
                                float scale, const float* kd_lg, float kd_coef, int B, int P, int L, void* dlogits, long ldd, int Vpad,
                                void* stream) {
    const BwdArgs a = {logits, ldl, V, topic_ids, targets, lse, coef, gscale, lm_coef, cond, uncond, ldt, lse_c, lse_u, scale,
                       kd_lg, kd_coef, P, L, dlogits, ldd, Vpad, 0};
    return loss_bwd_kd_any("loss_bwd_kd", dtype, logits_dtype, teacher_dtype, a, B, stream);
}

/* x3 mode: the same gradient of fp32 logits into a (hi | lo) bf16 plane pair (ld = ldd, lo plane `plane` elements behind). */
extern "C" int mmtg_loss_bwd_kd_x3(const float* logits, long ldl, int V, const long long* topic_ids, const long long* targets,
                                   const float* lse, const float* coef, float gscale, float lm_coef, int teacher_dtype, const void* cond,
                                   const void* uncond, long ldt, const float* lse_c, const float* lse_u, float scale, const float* kd_lg,
                                   float kd_coef, int B, int P, int L, void* planes, long ldd, long plane, int Vpad, void* stream) {
    const char* what = "loss_bwd_kd_x3";
    MMTG_REQUIRE(plane > 0, "%s: plane = %ld must be positive", what, plane);
    MMTG_REQUIRE(ldl % 4 == 0 && ldl >= Vpad && MMTG_ALIGNED16(logits), "%s: ldl %ld must be a multiple of 4 and >= Vpad, logits aligned", what, ldl);
    const BwdArgs a = {logits, ldl, V, topic_ids, targets, lse, coef, gscale, lm_coef, cond, uncond, ldt, lse_c, lse_u, scale,
                       kd_lg, kd_coef, P, L, planes, ldd, Vpad, plane};
    return loss_bwd_kd_any(what, MMTG_BF16, MMTG_F32, teacher_dtype, a, B, stream);
}
