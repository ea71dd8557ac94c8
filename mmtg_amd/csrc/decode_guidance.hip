// Classifier-free guidance for the decode token step (GuidedDecoder, mmtg_amd/decode.py): the per-step combine of a prompt's and its
// negative's distributions, and the column mirror that keeps the two halves of the batch on one text.  include/mmtg_hip.h states the
// rule.  Two kernels in a source file of their own: every other kernel compiles to the same code as before.
//
// Second pass: the combine needs both rows again after their (max, sum) pairs are known.  A pair is 2 x 13317 x 4 B = 104 KB, which
// would fit the 160 KB of LDS but pins one workgroup to a CU and costs a store and a load per logit on top of the HBM read.  The
// rows are re-read instead: a workgroup reads its own 104 KB back right after the first pass, and at 128 pairs the launch's whole
// working set is 13.6 MB, 1.7 MB per 4 MB L2 if the workgroups spread evenly over the 8 XCDs, so the second pass should be served
// by the L2.  That is inferred from the sizes, not measured: no HBM read counter was taken and no LDS-staged variant was timed, and
// the estimate leaves out whatever else of the step's graph is in the L2 at the time.
#include <math.h>

#include "common.h"

namespace {

// (max, sum of exp(x - max)) of two parts as one; a part whose max is -inf holds nothing, and two such parts stay (-inf, 0)
__device__ __forceinline__ void lse_merge(float& m, float& s, float om, float os) {
    const float nm = fmaxf(m, om);
    s = nm == -INFINITY ? 0.f : s * expf(m - nm) + os * expf(om - nm);
    m = nm;
}

// One thread's share of a row's (max, sum): 16-byte aligned rows as float4, all UN loads of a pass requested before the first is
// used; the tail and unaligned rows one logit at a time.  -inf entries add 0 to the sum.  Fixed order: bit-reproducible.
template <int UN>
__device__ __forceinline__ void row_lse_part(const float* __restrict__ row, int V, int tid, float& m, float& s) {
    m = -INFINITY;
    s = 0.f;
    int done = 0;
    if ((reinterpret_cast<uintptr_t>(row) & 15) == 0) {
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
                    for (int e = 0; e < 4; ++e) ps += expf(r[i][e] - pm);      // exp(-inf) = 0: -inf entries and the fillers add nothing
                lse_merge(m, s, pm, ps);
            }
        }
        done = nvec << 2;
    }
    for (int u = done + tid; u < V; u += 256) {
        const float x = row[u];
        if (x != -INFINITY) lse_merge(m, s, x, 1.f);
    }
}

// lu + scale * (lc - lu) on log-probabilities; an id either row excludes stays excluded (-inf - -inf would be NaN)
__device__ __forceinline__ float guide(float c, float u, float Lc, float Lu, float scale) {
    if (c == -INFINITY || u == -INFINITY) return -INFINITY;
    const float lc = c - Lc, lu = u - Lu;
    return lu + scale * (lc - lu);
}

__global__ __launch_bounds__(256) void decode_guidance_kernel(const float* __restrict__ cond, const float* __restrict__ uncond, long ldl,
        int V, float scale, float* __restrict__ out, long ldo) {
    __shared__ float sm[2][4];
    __shared__ float ss[2][4];
    __shared__ float sL[2];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* c = cond + (long)b * ldl;
    const float* u = uncond + (long)b * ldl;
    float* o = out + (long)b * ldo;
    float m[2], s[2];
    row_lse_part<8>(c, V, tid, m[0], s[0]);
    row_lse_part<8>(u, V, tid, m[1], s[1]);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float om = __shfl_xor(m[r], off, 64);
            const float os = __shfl_xor(s[r], off, 64);
            lse_merge(m[r], s[r], om, os);
        }
        if ((tid & 63) == 0) { sm[r][tid >> 6] = m[r]; ss[r][tid >> 6] = s[r]; }
    }
    __syncthreads();
    if (tid < 2) {
        float mm = sm[tid][0], sv = ss[tid][0];
        for (int w = 1; w < 4; ++w) lse_merge(mm, sv, sm[tid][w], ss[tid][w]);
        sL[tid] = mm == -INFINITY ? -INFINITY : mm + logf(sv);      // a row without a distribution: every id of it is -inf below
    }
    __syncthreads();
    const float Lc = sL[0], Lu = sL[1];
    int done = 0;
    if (((reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(o)) & 15) == 0) {
        const int nvec = V >> 2;
        const f32x4* c4 = reinterpret_cast<const f32x4*>(c);
        const f32x4* u4 = reinterpret_cast<const f32x4*>(u);
        f32x4* o4 = reinterpret_cast<f32x4*>(o);
        for (int idx = tid; idx < nvec; idx += 256) {
            const f32x4 cv = c4[idx], uv = u4[idx];
            f32x4 g;
#pragma unroll
            for (int e = 0; e < 4; ++e) g[e] = guide(cv[e], uv[e], Lc, Lu, scale);
            o4[idx] = g;
        }
        done = nvec << 2;
    }
    for (int v = done + tid; v < V; v += 256) o[v] = guide(c[v], u[v], Lc, Lu, scale);
}

__global__ __launch_bounds__(256) void decode_mirror_kernel(long long* __restrict__ seq, long ldseq, const int* __restrict__ pos_ptr,
        int N) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    const long col = (long)*pos_ptr + 1;
    if (b >= N || col < 0 || col >= ldseq) return;
    seq[(long)(N + b) * ldseq + col] = seq[(long)b * ldseq + col];
}

// whether the float ranges [a, a + na) and [b, b + nb) share an element
bool overlaps(const float* a, long na, const float* b, long nb) {
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (uintptr_t)na * sizeof(float);
    const uintptr_t b0 = (uintptr_t)b, b1 = b0 + (uintptr_t)nb * sizeof(float);
    return a0 < b1 && b0 < a1;
}

}  // namespace

extern "C" int mmtg_decode_guidance(const float* cond, const float* uncond, long ldl, int V, float scale, float* out, long ldo, int N,
                                    void* stream) {
    const char* what = "decode_guidance";
    MMTG_REQUIRE(cond, "%s: cond is a null pointer", what);
    MMTG_REQUIRE(uncond, "%s: uncond is a null pointer", what);
    MMTG_REQUIRE(out, "%s: out is a null pointer", what);
    MMTG_REQUIRE(N > 0, "%s: N %d must be positive", what, N);
    MMTG_REQUIRE(V > 0, "%s: V %d must be positive", what, V);
    MMTG_REQUIRE(ldl >= V, "%s: ldl %ld is below V %d", what, ldl, V);
    MMTG_REQUIRE(ldo >= V, "%s: ldo %ld is below V %d", what, ldo, V);
    MMTG_REQUIRE(isfinite(scale) && scale >= 0.f, "%s: scale %g must be finite and >= 0", what, (double)scale);
    const long nin = (long)(N - 1) * ldl + V, nout = (long)(N - 1) * ldo + V;
    MMTG_REQUIRE(!overlaps(out, nout, cond, nin), "%s: out overlaps cond", what);
    MMTG_REQUIRE(!overlaps(out, nout, uncond, nin), "%s: out overlaps uncond", what);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_DECODE, s, 8.0 * N * V, 12.0 * N * V);
    hipLaunchKernelGGL(decode_guidance_kernel, dim3(N), dim3(256), 0, s, cond, uncond, ldl, V, scale, out, ldo);
    MMTG_LAUNCH_CHECK("decode_guidance");
    return MMTG_OK;
}

extern "C" int mmtg_decode_mirror(long long* seq, long ldseq, const int* pos_ptr, int N, void* stream) {
    const char* what = "decode_mirror";
    MMTG_REQUIRE(seq, "%s: seq is a null pointer", what);
    MMTG_REQUIRE(pos_ptr, "%s: pos_ptr is a null pointer", what);
    MMTG_REQUIRE(N > 0, "%s: N %d must be positive", what, N);
    MMTG_REQUIRE(ldseq > 0, "%s: ldseq %ld must be positive", what, ldseq);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_DECODE, s, 0.0, 16.0 * N);
    hipLaunchKernelGGL(decode_mirror_kernel, dim3(cdiv(N, 256)), dim3(256), 0, s, seq, ldseq, pos_ptr, N);
    MMTG_LAUNCH_CHECK("decode_mirror");
    return MMTG_OK;
}
