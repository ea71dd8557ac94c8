// Per-modality guidance for the decode token step (ModalityGuidedDecoder, mmtg_amd/decode.py): the per-step combine of a prompt's
// distribution with those of up to three negatives, each with a scale of its own, and the column mirror that keeps all K blocks of
// the batch on one text.  include/mmtg_hip.h states the rule.  A source file of its own: every other kernel compiles to the same
// code as before.
//
// Two forms of the combine.  With K rows per workgroup only max_batch / K workgroups run (64 at K = 4, 85 at K = 3, over 256 CUs):
// the launch is bound by the latency of one workgroup, not by bandwidth, so what counts is how many dependent trips to memory a
// workgroup makes.
//   register-resident (V <= 14336): 512 threads hold the K rows -- seven float4 (or twenty-eight single logits) per thread and row,
//     116 VGPRs of data at K = 4 -- from one round of loads, all issued before the first is used.  The max and the sum are two
//     workgroup reductions over registers (the sum against the row's final max: one exponential per logit, no rescaling), the combine
//     reads registers.  One trip to memory.
//   re-read (any V): decode_guidance_kernel's scheme on K rows -- 256 threads, one streaming pass per row for a running (max, sum),
//     a second pass for the combine, which trusts the L2 to hold what the first pass read.  Two trips.
// tools/bench_mguidance.py times the two; DESIGN.md section 7 has the numbers and which one mmtg_decode_guidance_multi launches.
#include <math.h>

#include "common.h"

namespace {

constexpr int RT = 512;                     // threads of the register-resident form: 8 waves, up to 256 VGPRs each
constexpr int RV4 = 7;                      // float4 per thread and row on its aligned path: 7 * 4 * 512 = 14336 logits
constexpr int RS = 28;                      // logits per thread and row on its one-logit path: 28 * 512 = 14336 logits
constexpr int RESIDENT_MAX_V = RT * RS;     // what either path holds
constexpr float LOG2E = 1.4426950408889634f;

struct Scales { float s[3]; };              // by value: a captured launch holds the numbers

// g = lc;  g = g + (s_k - 1) * (lc - l_k) in branch order, on log-probabilities; an id any row excludes stays excluded (-inf - -inf
// would be NaN; a row without a distribution has L = -inf and every logit -inf, so it is covered)
template <int K>
__device__ __forceinline__ float guide_multi(const float (&x)[K], const float (&L)[K], const Scales& sc) {
    bool dead = false;
#pragma unroll
    for (int k = 0; k < K; ++k) dead |= x[k] == -INFINITY;
    const float lc = x[0] - L[0];
    float g = lc;
#pragma unroll
    for (int k = 1; k < K; ++k) g = g + (sc.s[k - 1] - 1.f) * (lc - (x[k] - L[k]));
    return dead ? -INFINITY : g;
}

// ---------------------------------------------------------------- register-resident
// VEC: every row start of the launch (inputs and out) is 16-byte aligned -- decided by the host from the pointers and strides.
template <int K, bool VEC>
__global__ __launch_bounds__(RT) void guidance_multi_resident_kernel(const float* __restrict__ logits, long ldl, int V, int N, Scales sc,
        float* __restrict__ out, long ldo) {
    constexpr int NR = VEC ? RV4 * 4 + 1 : RS;          // floats per thread and row (aligned path: + one of the V % 4 tail logits)
    constexpr int NW = RT / 64;
    __shared__ float red[2][K][NW];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nvec = V >> 2, tail = nvec << 2;
    float x[K][NR];
    // every load of the K rows, before anything reads one (a slot past the row holds -inf: it adds nothing to the max or the sum)
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float* row = logits + ((long)k * N + b) * ldl;
        if constexpr (VEC) {
            const f32x4* row4 = reinterpret_cast<const f32x4*>(row);
#pragma unroll
            for (int i = 0; i < RV4; ++i) {
                const int idx = tid + i * RT;
                const f32x4 v = idx < nvec ? row4[idx] : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
                for (int e = 0; e < 4; ++e) x[k][4 * i + e] = v[e];
            }
            x[k][NR - 1] = tail + tid < V ? row[tail + tid] : -INFINITY;
        } else {
#pragma unroll
            for (int i = 0; i < RS; ++i) {
                const int idx = tid + i * RT;
                x[k][i] = idx < V ? row[idx] : -INFINITY;
            }
        }
    }
    // the K maxima: registers, the wave, the 8 waves (a max does not round, so its order does not matter)
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float m = x[k][0];
#pragma unroll
        for (int j = 1; j < NR; ++j) m = fmaxf(m, x[k][j]);
        m = wave_max(m);
        if (lane == 0) red[0][k][wave] = m;
    }
    __syncthreads();
    float M[K], L[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        M[k] = red[0][k][0];
#pragma unroll
        for (int w = 1; w < NW; ++w) M[k] = fmaxf(M[k], red[0][k][w]);
    }
    // the K sums against the final maxima: one exponential per logit (exp2(-inf) = 0: excluded ids and empty slots add nothing); the
    // thread's slots in order, the xor butterfly, the waves in order -- a fixed order, so equal inputs give equal bits
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float s = 0.f;
        if (M[k] != -INFINITY) {
#pragma unroll
            for (int j = 0; j < NR; ++j) s += __builtin_amdgcn_exp2f((x[k][j] - M[k]) * LOG2E);
        }
        s = wave_sum(s);
        if (lane == 0) red[1][k][wave] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float s = red[1][k][0];
#pragma unroll
        for (int w = 1; w < NW; ++w) s += red[1][k][w];
        L[k] = M[k] == -INFINITY ? -INFINITY : M[k] + logf(s);      // a row without a distribution: every id of it is -inf below
    }
    float* o = out + (long)b * ldo;
    float xs[K];
    if constexpr (VEC) {
        f32x4* o4 = reinterpret_cast<f32x4*>(o);
#pragma unroll
        for (int i = 0; i < RV4; ++i) {
            const int idx = tid + i * RT;
            f32x4 g;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
#pragma unroll
                for (int k = 0; k < K; ++k) xs[k] = x[k][4 * i + e];
                g[e] = guide_multi<K>(xs, L, sc);
            }
            if (idx < nvec) o4[idx] = g;
        }
#pragma unroll
        for (int k = 0; k < K; ++k) xs[k] = x[k][NR - 1];
        if (tail + tid < V) o[tail + tid] = guide_multi<K>(xs, L, sc);
    } else {
#pragma unroll
        for (int i = 0; i < RS; ++i) {
            const int idx = tid + i * RT;
#pragma unroll
            for (int k = 0; k < K; ++k) xs[k] = x[k][i];
            if (idx < V) o[idx] = guide_multi<K>(xs, L, sc);
        }
    }
}

// ---------------------------------------------------------------- re-read (decode_guidance_kernel's scheme, restated for K rows)
// (max, sum of exp(x - max)) of two parts as one; a part whose max is -inf holds nothing, and two such parts stay (-inf, 0)
__device__ __forceinline__ void lse_merge(float& m, float& s, float om, float os) {
    const float nm = fmaxf(m, om);
    s = nm == -INFINITY ? 0.f : s * expf(m - nm) + os * expf(om - nm);
    m = nm;
}

// One thread's share of a row's (max, sum): a 16-byte aligned row as float4, the UN loads of a sweep requested before the first is
// used; the tail and an unaligned row one logit at a time.  Fixed order.
template <int UN>
__device__ __forceinline__ void row_lse_part(const float* __restrict__ row, int V, int tid, float& m, float& s) {
    m = -INFINITY;
    s = 0.f;
    int done = 0;
    if (MMTG_ALIGNED16(row)) {
        const int nvec = V >> 2;
        const f32x4* row4 = reinterpret_cast<const f32x4*>(row);
        for (int base = 0; base < nvec; base += 256 * UN) {
            f32x4 r[UN];
#pragma unroll
            for (int i = 0; i < UN; ++i) {
                const int idx = base + i * 256 + tid;
                r[i] = idx < nvec ? row4[idx] : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            }
            float pm = -INFINITY;
#pragma unroll
            for (int i = 0; i < UN; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) pm = fmaxf(pm, r[i][e]);
            if (pm != -INFINITY) {
                float ps = 0.f;
#pragma unroll
                for (int i = 0; i < UN; ++i)
#pragma unroll
                    for (int e = 0; e < 4; ++e) ps += expf(r[i][e] - pm);
                lse_merge(m, s, pm, ps);
            }
        }
        done = nvec << 2;
    }
    for (int v = done + tid; v < V; v += 256) {
        const float xv = row[v];
        if (xv != -INFINITY) lse_merge(m, s, xv, 1.f);
    }
}

template <int K>
__global__ __launch_bounds__(256) void guidance_multi_reread_kernel(const float* __restrict__ logits, long ldl, int V, int N, Scales sc,
        float* __restrict__ out, long ldo) {
    __shared__ float sm[K][4];
    __shared__ float ss[K][4];
    __shared__ float sL[K];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* rows[K];
    float m[K], s[K];
    bool vec = true;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        rows[k] = logits + ((long)k * N + b) * ldl;
        vec = vec && MMTG_ALIGNED16(rows[k]);
        row_lse_part<8>(rows[k], V, tid, m[k], s[k]);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float om = __shfl_xor(m[k], off, 64);
            const float os = __shfl_xor(s[k], off, 64);
            lse_merge(m[k], s[k], om, os);
        }
        if ((tid & 63) == 0) { sm[k][tid >> 6] = m[k]; ss[k][tid >> 6] = s[k]; }
    }
    __syncthreads();
    if (tid < K) {
        float mm = sm[tid][0], sv = ss[tid][0];
        for (int w = 1; w < 4; ++w) lse_merge(mm, sv, sm[tid][w], ss[tid][w]);
        sL[tid] = mm == -INFINITY ? -INFINITY : mm + logf(sv);
    }
    __syncthreads();
    float L[K], xs[K];
#pragma unroll
    for (int k = 0; k < K; ++k) L[k] = sL[k];
    float* o = out + (long)b * ldo;
    int done = 0;
    if (vec && MMTG_ALIGNED16(o)) {
        const int nvec = V >> 2;
        f32x4* o4 = reinterpret_cast<f32x4*>(o);
        for (int idx = tid; idx < nvec; idx += 256) {
            f32x4 v[K], g;
#pragma unroll
            for (int k = 0; k < K; ++k) v[k] = reinterpret_cast<const f32x4*>(rows[k])[idx];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
#pragma unroll
                for (int k = 0; k < K; ++k) xs[k] = v[k][e];
                g[e] = guide_multi<K>(xs, L, sc);
            }
            o4[idx] = g;
        }
        done = nvec << 2;
    }
    for (int v = done + tid; v < V; v += 256) {
#pragma unroll
        for (int k = 0; k < K; ++k) xs[k] = rows[k][v];
        o[v] = guide_multi<K>(xs, L, sc);
    }
}

template <int K>
__global__ __launch_bounds__(256) void decode_mirror_multi_kernel(long long* __restrict__ seq, long ldseq, const int* __restrict__ pos_ptr,
        int N) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    const long col = (long)*pos_ptr + 1;
    if (b >= N || col < 0 || col >= ldseq) return;
    const long long v = seq[(long)b * ldseq + col];
#pragma unroll
    for (int k = 1; k < K; ++k) seq[((long)k * N + b) * ldseq + col] = v;
}

// whether the float ranges [a, a + na) and [b, b + nb) share an element
bool overlaps(const float* a, long na, const float* b, long nb) {
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (uintptr_t)na * sizeof(float);
    const uintptr_t b0 = (uintptr_t)b, b1 = b0 + (uintptr_t)nb * sizeof(float);
    return a0 < b1 && b0 < a1;
}

template <int K>
void launch_combine(bool resident, bool vec, hipStream_t s, const float* logits, long ldl, int V, int N, const Scales& sc, float* out,
                    long ldo) {
    if (!resident)
        hipLaunchKernelGGL(guidance_multi_reread_kernel<K>, dim3(N), dim3(256), 0, s, logits, ldl, V, N, sc, out, ldo);
    else if (vec)
        hipLaunchKernelGGL((guidance_multi_resident_kernel<K, true>), dim3(N), dim3(RT), 0, s, logits, ldl, V, N, sc, out, ldo);
    else
        hipLaunchKernelGGL((guidance_multi_resident_kernel<K, false>), dim3(N), dim3(RT), 0, s, logits, ldl, V, N, sc, out, ldo);
}

int guidance_multi(const char* what, const float* logits, long ldl, int V, int K, const float* scales, float* out, long ldo, int N,
                   int form, void* stream) {
    MMTG_REQUIRE(logits, "%s: logits is a null pointer", what);
    MMTG_REQUIRE(scales, "%s: scales is a null pointer", what);
    MMTG_REQUIRE(out, "%s: out is a null pointer", what);
    MMTG_REQUIRE(N > 0, "%s: N %d must be positive", what, N);
    MMTG_REQUIRE(V > 0, "%s: V %d must be positive", what, V);
    MMTG_REQUIRE(K >= 2 && K <= 4, "%s: K %d must be 2, 3 or 4 (a prompt beside one to three negatives)", what, K);
    MMTG_REQUIRE(ldl >= V, "%s: ldl %ld is below V %d", what, ldl, V);
    MMTG_REQUIRE(ldo >= V, "%s: ldo %ld is below V %d", what, ldo, V);
    Scales sc = {{1.f, 1.f, 1.f}};
    for (int k = 0; k < K - 1; ++k) {
        MMTG_REQUIRE(isfinite(scales[k]) && scales[k] >= 0.f, "%s: scale %d, %g, must be finite and >= 0", what, k, (double)scales[k]);
        sc.s[k] = scales[k];
    }
    MMTG_REQUIRE(form >= 0 && form <= 2, "%s: form %d must be 0 (chosen here), 1 (register-resident) or 2 (re-read)", what, form);
    MMTG_REQUIRE(form != 1 || V <= RESIDENT_MAX_V, "%s: form 1 (register-resident) holds V up to %d, got %d", what, RESIDENT_MAX_V, V);
    const long nin = ((long)K * N - 1) * ldl + V, nout = (long)(N - 1) * ldo + V;
    MMTG_REQUIRE(!overlaps(out, nout, logits, nin), "%s: out overlaps logits", what);
    const bool resident = form == 1 || (form == 0 && V <= RESIDENT_MAX_V);
    const bool vec = MMTG_ALIGNED16(logits) && MMTG_ALIGNED16(out) && ldl % 4 == 0 && ldo % 4 == 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_DECODE, s, (4.0 * K + 2.0) * N * V, 4.0 * (K + 1) * N * V);
    if (K == 2) launch_combine<2>(resident, vec, s, logits, ldl, V, N, sc, out, ldo);
    else if (K == 3) launch_combine<3>(resident, vec, s, logits, ldl, V, N, sc, out, ldo);
    else launch_combine<4>(resident, vec, s, logits, ldl, V, N, sc, out, ldo);
    MMTG_LAUNCH_CHECK(what);
    return MMTG_OK;
}

}  // namespace

extern "C" int mmtg_decode_guidance_multi(const float* logits, long ldl, int V, int K, const float* scales, float* out, long ldo, int N,
                                          void* stream) {
    return guidance_multi("decode_guidance_multi", logits, ldl, V, K, scales, out, ldo, N, 0, stream);
}

extern "C" int mmtg_decode_guidance_multi_form(const float* logits, long ldl, int V, int K, const float* scales, float* out, long ldo,
                                               int N, int form, void* stream) {
    return guidance_multi("decode_guidance_multi_form", logits, ldl, V, K, scales, out, ldo, N, form, stream);
}

extern "C" int mmtg_decode_mirror_multi(long long* seq, long ldseq, const int* pos_ptr, int N, int K, void* stream) {
    const char* what = "decode_mirror_multi";
    MMTG_REQUIRE(seq, "%s: seq is a null pointer", what);
    MMTG_REQUIRE(pos_ptr, "%s: pos_ptr is a null pointer", what);
    MMTG_REQUIRE(N > 0, "%s: N %d must be positive", what, N);
    MMTG_REQUIRE(K >= 2 && K <= 4, "%s: K %d must be 2, 3 or 4", what, K);
    MMTG_REQUIRE(ldseq > 0, "%s: ldseq %ld must be positive", what, ldseq);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_DECODE, s, 0.0, 8.0 * K * N);
    const dim3 grid(cdiv(N, 256)), block(256);
    if (K == 2) hipLaunchKernelGGL(decode_mirror_multi_kernel<2>, grid, block, 0, s, seq, ldseq, pos_ptr, N);
    else if (K == 3) hipLaunchKernelGGL(decode_mirror_multi_kernel<3>, grid, block, 0, s, seq, ldseq, pos_ptr, N);
    else hipLaunchKernelGGL(decode_mirror_multi_kernel<4>, grid, block, 0, s, seq, ldseq, pos_ptr, N);
    MMTG_LAUNCH_CHECK(what);
    return MMTG_OK;
}
