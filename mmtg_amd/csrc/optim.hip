// Step tail of the training loop (train.py:194-197): global grad-norm,
// clip + transformers.AdamW update fused with the bf16 weight-copy refresh,
// and the dtype casts the engine needs.  Pure HBM streaming kernels:
// 16-byte vectors, grid-stride, <= 2048 blocks.
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ x, long n, float* __restrict__ out) {
    __shared__ float sh[4];
    float a = 0.f;
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
        a += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    if (blockIdx.x == 0)
        for (long i = (n4 << 2) + threadIdx.x; i < n; i += 256) a += x[i] * x[i];
    a = wave_sum(a);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
    __syncthreads();
    // round 4: one partial per workgroup (plain store) + an ordered final sum instead of ~2000 fp32 atomics on one word -- the
    // norm, and through the clip coefficient every parameter, is reproducible bit for bit
    if (threadIdx.x == 0) out[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// out[0] = sum of the n partials in a fixed order (thread t: partials t, t + 256, ...; then lanes, then waves)
__global__ __launch_bounds__(256) void sumsq_final_kernel(const float* __restrict__ part, int n, float* __restrict__ out) {
    __shared__ float sh[4];
    float a = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) a += part[i];
    a = wave_sum(a);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = sh[0] + sh[1] + sh[2] + sh[3];
}

// One parameter's update, shared by the 16-byte path and the scalar fallback of adamw_kernel so that both round alike: left to
// the compiler's contraction the two loops fused b1 m + (1 - b1) g differently (the vector loop around (1 - b1) g, the scalar
// loop around b1 m), and the last bit of m depended on the alignment of the pointers.  The fused forms are the vector loop's.
__device__ __forceinline__ void adamw_update(float g, float& m, float& v, float& p, float coef, float b1, float b2, float eps,
                                             float lrwd, float step_size) {
#pragma clang fp contract(off)
    const float gi = g * coef;
    const float mi = fmaf(1.f - b1, gi, b1 * m);
    const float vi = fmaf(b2, v, gi * ((1.f - b2) * gi));
    float pi = fmaf(-step_size, mi / (sqrtf(vi) + eps), p);
    if (lrwd > 0.f) pi = fmaf(-lrwd, pi, pi);
    m = mi; v = vi; p = pi;
}

__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
        float* __restrict__ m, float* __restrict__ v, bf16* __restrict__ pc, bf16* __restrict__ pl, long n, float lr, float b1, float b2,
        float eps, float wd, float step_size, const float* __restrict__ normsq, float max_norm, float gscale,
        const float* __restrict__ count) {
    // data-parallel steps hand over SUMS of per-row gradients and the global row count as a device scalar
    // (the all-reduced count never visits the host); an empty global batch leaves every buffer untouched,
    // as the reference skips the step (train.py:184-185)
    if (count) {
        const float c = *count;
        if (!(c > 0.f)) return;
        gscale *= 1.0f / c;
    }
    float coef = gscale;
    if (normsq) {
        // torch.nn.utils.clip_grad_norm_: coef = max_norm / (norm + 1e-6), clamped to 1
        const float nrm = sqrtf(*normsq) * gscale;
        coef *= fminf(1.0f, max_norm / (nrm + 1e-6f));
    }
    const float lrwd = wd > 0.f ? lr * wd : 0.f;      // decoupled decay p -= lr wd p (wd > 0 only)
    // 16-byte vectors (four parameters per lane and pass); the flat buffers are 16-byte aligned and n is a multiple of 4
    // for every layout the engine builds (a scalar tail covers anything else)
    const bool vec_ok = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                          reinterpret_cast<uintptr_t>(v)) & 15) == 0 && ((reinterpret_cast<uintptr_t>(pc) | reinterpret_cast<uintptr_t>(pl)) & 7) == 0;
    const long n4 = vec_ok ? n >> 2 : 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f32x4 g4 = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 m4 = reinterpret_cast<f32x4*>(m)[i], v4 = reinterpret_cast<f32x4*>(v)[i], p4 = reinterpret_cast<f32x4*>(p)[i];
        bf16x4 c4, l4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float mi = m4[e], vi = v4[e], pi = p4[e];
            adamw_update(g4[e], mi, vi, pi, coef, b1, b2, eps, lrwd, step_size);
            m4[e] = mi; v4[e] = vi; p4[e] = pi;
            c4[e] = (bf16)pi;
            l4[e] = (bf16)(pi - (float)c4[e]);
        }
        reinterpret_cast<f32x4*>(m)[i] = m4;
        reinterpret_cast<f32x4*>(v)[i] = v4;
        reinterpret_cast<f32x4*>(p)[i] = p4;
        if (pc) reinterpret_cast<bf16x4*>(pc)[i] = c4;
        if (pl) reinterpret_cast<bf16x4*>(pl)[i] = l4;
    }
    for (long i = (n4 << 2) + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        float mi = m[i], vi = v[i], pi = p[i];
        adamw_update(g[i], mi, vi, pi, coef, b1, b2, eps, lrwd, step_size);
        m[i] = mi; v[i] = vi; p[i] = pi;
        if (pc) pc[i] = (bf16)pi;
        if (pl) pl[i] = (bf16)(pi - (float)(bf16)pi);
    }
}

// ---------------------------------------------------------------- parameter groups
// The two kernels above over a table of (begin, end, group) segments of the flat buffer: same geometry (one 16-byte vector per
// lane and pass, 1024 elements per workgroup and pass, grid-stride over <= 2048 workgroups), but a lane first finds the segment of
// its vector.  The table (<= 1024 segments) is staged in LDS: ends, begins, group bytes.  A vector that lies inside one segment
// takes the 16-byte path; one that a boundary cuts, or that reaches into a gap, goes element by element; a vector without any
// element of a trainable segment issues no load and no store -- pads, gaps and frozen tensors keep every bit and cost no traffic.
struct SegTable {
    const long* end;             // LDS: end[s], ascending (the segments are sorted and disjoint)
    const long* begin;           // LDS
    const unsigned char* group;  // LDS
    int n;
};

__device__ __forceinline__ SegTable stage_segments(unsigned char* lds, const long* __restrict__ segs, int nsegs) {
    long* se = reinterpret_cast<long*>(lds);
    long* sb = se + nsegs;
    unsigned char* sg = reinterpret_cast<unsigned char*>(sb + nsegs);
    for (int s = threadIdx.x; s < nsegs; s += 256) {
        sb[s] = segs[3 * s];
        se[s] = segs[3 * s + 1];
        sg[s] = (unsigned char)segs[3 * s + 2];
    }
    return SegTable{se, sb, sg, nsegs};
}
// bytes of LDS stage_segments fills, rounded up so that what follows it is 16-byte aligned
inline size_t seg_lds_bytes(int nsegs) { return ((size_t)nsegs * 17 + 15) & ~(size_t)15; }

// first segment that ends behind element e (nsegs if there is none): the only one that can hold e
__device__ __forceinline__ int seg_find(const SegTable& t, long e) {
    int lo = 0, hi = t.n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (t.end[mid] > e) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// out[g * gridDim.x + blockIdx.x] = this workgroup's sum of x^2 over group g's elements, for every group (0 for frozen ones).
// A lane adds into one register while its vectors stay in one group and into its own LDS slot acc[g * 256 + lane] when the group
// changes; the slots are then summed per group in a fixed order (slot t, t + 64, ... per lane; lanes; nothing else).
__global__ __launch_bounds__(256) void sumsq_groups_kernel(const float* __restrict__ x, long n, const long* __restrict__ segs,
        int nsegs, int ngroups, unsigned frozen, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const SegTable t = stage_segments(lds, segs, nsegs);
    float* acc = reinterpret_cast<float*>(lds + (((size_t)nsegs * 17 + 15) & ~(size_t)15));
    for (int k = threadIdx.x; k < ngroups * 256; k += 256) acc[k] = 0.f;
    __syncthreads();
    float a = 0.f;
    int ag = -1;                // the group `a` belongs to
    const long nv = (n + 3) >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long)gridDim.x * 256) {
        const long e0 = i << 2;
        int s = seg_find(t, e0);
        if (s >= nsegs || t.begin[s] >= e0 + 4) continue;               // nothing of this vector is in a segment
        if (t.begin[s] <= e0 && t.end[s] >= e0 + 4) {
            const int g = t.group[s];
            if ((frozen >> g) & 1u) continue;
            if (g != ag) {
                if (ag >= 0) acc[ag * 256 + threadIdx.x] += a;
                a = 0.f; ag = g;
            }
            const f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
            a += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
            continue;
        }
        for (long e = e0; e < e0 + 4; ++e) {
            while (s < nsegs && t.end[s] <= e) ++s;
            if (s >= nsegs) break;
            if (t.begin[s] > e) continue;
            const int g = t.group[s];
            if ((frozen >> g) & 1u) continue;
            if (g != ag) {
                if (ag >= 0) acc[ag * 256 + threadIdx.x] += a;
                a = 0.f; ag = g;
            }
            a += x[e] * x[e];
        }
    }
    if (ag >= 0) acc[ag * 256 + threadIdx.x] += a;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int g = threadIdx.x >> 6; g < ngroups; g += 4) {
        const float* r = acc + g * 256;
        float w = ((r[lane] + r[lane + 64]) + r[lane + 128]) + r[lane + 192];
        w = wave_sum(w);
        if (lane == 0) out[(long)g * gridDim.x + blockIdx.x] = w;
    }
}

// out[g] = ordered sum of group g's np partials (sumsq_final_kernel's order), out[ngroups] = the non-frozen groups' sums added in
// group order.  One workgroup.
__global__ __launch_bounds__(256) void sumsq_groups_final_kernel(const float* __restrict__ part, int np, int ngroups, unsigned frozen,
                                                                 float* __restrict__ out) {
    __shared__ float sh[4];
    float total = 0.f;
    for (int g = 0; g < ngroups; ++g) {
        float a = 0.f;
        if (!((frozen >> g) & 1u))
            for (int i = threadIdx.x; i < np; i += 256) a += part[(long)g * np + i];
        a = wave_sum(a);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
        __syncthreads();
        if (threadIdx.x == 0) {
            const float r = sh[0] + sh[1] + sh[2] + sh[3];
            out[g] = r;
            if (!((frozen >> g) & 1u)) total += r;
        }
    }
    if (threadIdx.x == 0) out[ngroups] = total;
}

// what adamw_groups_kernel needs of every group, by value in the kernel arguments (16 groups: 196 bytes)
struct AdamGroups {
    float lr[MMTG_MAX_PARAM_GROUPS];            // (float)((double)lr * (double)lr_scale): the lr mmtg_adamw would be called with
    float wd[MMTG_MAX_PARAM_GROUPS];
    float step_size[MMTG_MAX_PARAM_GROUPS];     // that lr's bias-corrected step size, from double as in mmtg_adamw
    unsigned frozen;
};

// adamw_kernel per segment: the same clip coefficient, the same adamw_update, the same plane expressions; lrwd and step_size
// are the segment's group's.  The element path is adamw_kernel's scalar fallback, also taken by every vector when a pointer is
// misaligned.
__global__ __launch_bounds__(256) void adamw_groups_kernel(float* __restrict__ p, const float* __restrict__ g,
        float* __restrict__ m, float* __restrict__ v, bf16* __restrict__ pc, bf16* __restrict__ pl, long n,
        const long* __restrict__ segs, int nsegs, const AdamGroups grp, float b1, float b2, float eps,
        const float* __restrict__ normsq, float max_norm, float gscale, const float* __restrict__ count) {
    if (count) {
        const float c = *count;
        if (!(c > 0.f)) return;
        gscale *= 1.0f / c;
    }
    float coef = gscale;
    if (normsq) {
        // torch.nn.utils.clip_grad_norm_: coef = max_norm / (norm + 1e-6), clamped to 1
        const float nrm = sqrtf(*normsq) * gscale;
        coef *= fminf(1.0f, max_norm / (nrm + 1e-6f));
    }
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const SegTable t = stage_segments(lds, segs, nsegs);
    float* g_lrwd = reinterpret_cast<float*>(lds + (((size_t)nsegs * 17 + 15) & ~(size_t)15));
    float* g_step = g_lrwd + MMTG_MAX_PARAM_GROUPS;
    if (threadIdx.x < MMTG_MAX_PARAM_GROUPS) {
        const int k = threadIdx.x;
        const float lr = grp.lr[k], wd = grp.wd[k];
        g_lrwd[k] = wd > 0.f ? lr * wd : 0.f;      // decoupled decay p -= lr wd p (wd > 0 only)
        g_step[k] = grp.step_size[k];
    }
    __syncthreads();
    const bool vec_ok = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                          reinterpret_cast<uintptr_t>(v)) & 15) == 0 && ((reinterpret_cast<uintptr_t>(pc) | reinterpret_cast<uintptr_t>(pl)) & 7) == 0;
    const unsigned frozen = grp.frozen;
    const long nv = (n + 3) >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long)gridDim.x * 256) {
        const long e0 = i << 2;
        int s = seg_find(t, e0);
        if (s >= nsegs || t.begin[s] >= e0 + 4) continue;               // nothing of this vector is in a segment
        if (vec_ok && t.begin[s] <= e0 && t.end[s] >= e0 + 4) {
            const int k = t.group[s];
            if ((frozen >> k) & 1u) continue;
            const float lrwd = g_lrwd[k], step_size = g_step[k];
            const f32x4 g4 = reinterpret_cast<const f32x4*>(g)[i];
            f32x4 m4 = reinterpret_cast<f32x4*>(m)[i], v4 = reinterpret_cast<f32x4*>(v)[i], p4 = reinterpret_cast<f32x4*>(p)[i];
            bf16x4 c4, l4;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float mi = m4[e], vi = v4[e], pi = p4[e];
                adamw_update(g4[e], mi, vi, pi, coef, b1, b2, eps, lrwd, step_size);
                m4[e] = mi; v4[e] = vi; p4[e] = pi;
                c4[e] = (bf16)pi;
                l4[e] = (bf16)(pi - (float)c4[e]);
            }
            reinterpret_cast<f32x4*>(m)[i] = m4;
            reinterpret_cast<f32x4*>(v)[i] = v4;
            reinterpret_cast<f32x4*>(p)[i] = p4;
            if (pc) reinterpret_cast<bf16x4*>(pc)[i] = c4;
            if (pl) reinterpret_cast<bf16x4*>(pl)[i] = l4;
            continue;
        }
        for (long e = e0; e < e0 + 4; ++e) {
            while (s < nsegs && t.end[s] <= e) ++s;
            if (s >= nsegs) break;
            if (t.begin[s] > e) continue;
            const int k = t.group[s];
            if ((frozen >> k) & 1u) continue;
            float mi = m[e], vi = v[e], pi = p[e];
            adamw_update(g[e], mi, vi, pi, coef, b1, b2, eps, g_lrwd[k], g_step[k]);
            m[e] = mi; v[e] = vi; p[e] = pi;
            if (pc) pc[e] = (bf16)pi;
            if (pl) pl[e] = (bf16)(pi - (float)(bf16)pi);
        }
    }
}

// ---------------------------------------------------------------- weight averaging
// One element of the exponential moving average, shared by the 16-byte path and the scalar path so that both round alike (see
// adamw_update): the difference is rounded once, the multiply-add once.  p == e gives e back (w * 0 + e), so frozen tensors, pads
// and gaps of the flat buffer follow the master without a segment table -- bit for bit but for one case, which the select below
// takes care of: e = -0 comes out of the multiply-add as +0 (p - e = +0, and +0 + -0 = +0; likewise w = 0 with p > e), and GPT-2
// checkpoints do hold a -0 here and there.  A result that compares equal to e IS e, so the select changes nothing but that sign.
__device__ __forceinline__ float ema_step(float e, float p, float w) {
#pragma clang fp contract(off)
    const float d = p - e;
    const float r = fmaf(w, d, e);
    return r == e ? e : r;
}

__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ p, long n, float w,
                                                         const float* __restrict__ count) {
    // the device scalar mmtg_adamw takes: an empty global batch skipped the step and skips the average
    if (count && !(*count > 0.f)) return;
    const bool vec_ok = ((reinterpret_cast<uintptr_t>(ema) | reinterpret_cast<uintptr_t>(p)) & 15) == 0;
    const long n4 = vec_ok ? n >> 2 : 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f32x4 p4 = reinterpret_cast<const f32x4*>(p)[i];
        f32x4 e4 = reinterpret_cast<f32x4*>(ema)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) e4[e] = ema_step(e4[e], p4[e], w);
        reinterpret_cast<f32x4*>(ema)[i] = e4;
    }
    for (long i = (n4 << 2) + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) ema[i] = ema_step(ema[i], p[i], w);
}

// a <-> b as 32-bit words: NaN payloads and -0 survive (no floating-point instruction touches the data)
__global__ __launch_bounds__(256) void swap_kernel(unsigned* __restrict__ a, unsigned* __restrict__ b, long n) {
    const bool vec_ok = ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
    const long n4 = vec_ok ? n >> 2 : 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const u32x4 a4 = reinterpret_cast<u32x4*>(a)[i], b4 = reinterpret_cast<u32x4*>(b)[i];
        reinterpret_cast<u32x4*>(a)[i] = b4;
        reinterpret_cast<u32x4*>(b)[i] = a4;
    }
    for (long i = (n4 << 2) + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const unsigned x = a[i], y = b[i];
        a[i] = y;
        b[i] = x;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void cast_from_f32_kernel(const float* __restrict__ src, T* __restrict__ dst, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) dst[i] = (T)src[i];
}
template <typename T>
__global__ __launch_bounds__(256) void cast_to_f32_kernel(const T* __restrict__ src, float* __restrict__ dst, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) dst[i] = (float)src[i];
}
template <typename T>
__global__ __launch_bounds__(256) void cast_pad_rows_kernel(const float* __restrict__ src, long lds_, T* __restrict__ dst,
                                                            long ldd, int cols) {
    const long r = blockIdx.x;
    for (int c = threadIdx.x; c < ldd; c += 256) dst[r * ldd + c] = c < cols ? (T)src[r * lds_ + c] : (T)0.f;
}
__global__ __launch_bounds__(256) void axpy_kernel(float* __restrict__ y, const float* __restrict__ x, float a, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) y[i] += a * x[i];
}

// Second half of a weight-gradient product stored as K-split slabs (mmtg_gemm, transA, MMTG_EPI_SPLIT):
// dst[i] (+)= sum_s part[s * stride + i], slabs added in order (deterministic).  One float4 per lane;
// the slabs were written just before and are still in the Infinity Cache.
__global__ __launch_bounds__(256) void slab_sum_kernel(const float* __restrict__ part, int splits, long stride,
                                                       float* __restrict__ dst, int accumulate, long n4) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f4* src = reinterpret_cast<const f4*>(part) + i;
        f4 acc = accumulate ? reinterpret_cast<const f4*>(dst)[i] : f4{0.f, 0.f, 0.f, 0.f};
        int s = 0;
        for (; s + 4 <= splits; s += 4) {
            const f4 a = src[(s + 0) * (stride / 4)], b = src[(s + 1) * (stride / 4)];
            const f4 c = src[(s + 2) * (stride / 4)], d = src[(s + 3) * (stride / 4)];
            acc += a; acc += b; acc += c; acc += d;
        }
        for (; s < splits; ++s) acc += src[s * (stride / 4)];
        reinterpret_cast<f4*>(dst)[i] = acc;
    }
}

// Batched matrix transpose (weight-copy maintenance): matrix i is [rows, cols] row-major at
// src + desc[4i], written as [cols, rows] at dst + desc[4i+3].  One 64x64 tile per workgroup through
// a padded LDS image; 16-byte global vectors on both sides (rows, cols multiples of 16/sizeof(T)).
template <typename T>
__global__ __launch_bounds__(256) void transpose_batch_kernel(const T* __restrict__ src, T* __restrict__ dst,
                                                              const long* __restrict__ desc) {
    typedef typename Vec16<T>::type V;
    constexpr int EPC = Vec16<T>::N, CPR = 64 / EPC, RPP = 256 / CPR;   // chunks per tile row, rows per pass
    constexpr int LDT = 64 + EPC;                                         // padded LDS row (16-byte multiple)
    __shared__ __attribute__((aligned(16))) T tile[64 * LDT];
    const long* d = desc + 4 * blockIdx.y;
    const long so = d[0], dof = d[3];
    const int rows = (int)d[1], cols = (int)d[2];
    const int tc = (cols + 63) >> 6, tr = (rows + 63) >> 6;
    if ((int)blockIdx.x >= tr * tc) return;
    const int r0 = ((int)blockIdx.x / tc) * 64, c0 = ((int)blockIdx.x % tc) * 64;
    const int tid = threadIdx.x, ch = tid % CPR, rr = tid / CPR;
#pragma unroll
    for (int ps = 0; ps < 64 / RPP; ++ps) {
        const int r = rr + ps * RPP;
        V v;
#pragma unroll
        for (int e = 0; e < EPC; ++e) v[e] = (T)0.0f;
        if (r0 + r < rows && c0 + ch * EPC < cols) v = *reinterpret_cast<const V*>(src + so + (long)(r0 + r) * cols + c0 + ch * EPC);
        *reinterpret_cast<V*>(tile + r * LDT + ch * EPC) = v;
    }
    __syncthreads();
#pragma unroll
    for (int ps = 0; ps < 64 / RPP; ++ps) {
        const int j = rr + ps * RPP;          // source column = destination row
        V v;
#pragma unroll
        for (int e = 0; e < EPC; ++e) v[e] = tile[(ch * EPC + e) * LDT + j];
        if (c0 + j < cols && r0 + ch * EPC < rows) *reinterpret_cast<V*>(dst + dof + (long)(c0 + j) * rows + r0 + ch * EPC) = v;
    }
}

// Pull a buffer through the memory hierarchy (into the 256 MB Infinity Cache) ahead of the kernel that will read it:
// 16-byte loads, the xor of everything goes to a sink only if it equals a value it cannot take.
__global__ __launch_bounds__(256) void prefetch_kernel(const u32x4* __restrict__ src, long n16, unsigned* __restrict__ sink) {
    u32x4 acc = {0u, 0u, 0u, 0u};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long)gridDim.x * 256) {
        const u32x4 v = src[i];
        acc[0] ^= v[0]; acc[1] ^= v[1]; acc[2] ^= v[2]; acc[3] ^= v[3];
    }
    if ((acc[0] ^ acc[1] ^ acc[2] ^ acc[3]) == 0x9E3779B9u && sink) *sink = 1u;      // (keeps the loads alive)
}

// Zero a list of ranges of one fp32 buffer in ONE launch: desc[2 r] = first element (a multiple of 4), desc[2 r + 1] = count (a
// multiple of 4).  The fused trainer zeroes only the gradients that are ACCUMULATED into (LayerNorm / bias columns, embeddings,
// LM head, encoder): the block matrices, 340 of the 497 MB, are overwritten by their slab sums.
__global__ __launch_bounds__(256) void zero_ranges_kernel(float* __restrict__ base, const long* __restrict__ desc, int n) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < n; ++r) {
        f32x4* p = reinterpret_cast<f32x4*>(base + desc[2 * r]);
        const long cnt = desc[2 * r + 1] >> 2;
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < cnt; i += (long)gridDim.x * 256) p[i] = z;
    }
}

inline unsigned grid_for(long n) { return (unsigned)min((long)2048, (n + 255) / 256); }

}  // namespace

extern "C" int mmtg_prefetch(const void* src, long bytes, int workgroups, void* sink, void* stream) {
    MMTG_REQUIRE(src && bytes >= 16 && MMTG_ALIGNED16(src) && workgroups > 0, "prefetch: bad args");
    hipLaunchKernelGGL(prefetch_kernel, dim3((unsigned)workgroups), dim3(256), 0, (hipStream_t)stream, (const u32x4*)src, bytes / 16, (unsigned*)sink);
    MMTG_LAUNCH_CHECK("prefetch");
    return MMTG_OK;
}

extern "C" int mmtg_zero_ranges(float* base, const long* desc, int n, void* stream) {
    MMTG_REQUIRE(base && desc && n > 0 && MMTG_ALIGNED16(base), "zero_ranges: bad args");
    hipLaunchKernelGGL(zero_ranges_kernel, dim3(1024), dim3(256), 0, (hipStream_t)stream, base, desc, n);
    MMTG_LAUNCH_CHECK("zero_ranges");
    return MMTG_OK;
}

extern "C" long mmtg_sumsq_ws(long n) { return (long)grid_for(n / 4 + 1); }

extern "C" int mmtg_sumsq(const float* x, long n, float* out, float* ws, long ws_floats, void* stream) {
    MMTG_REQUIRE(x && out && n > 0 && MMTG_ALIGNED16(x), "sumsq: bad args");
    const int g = grid_for(n / 4 + 1);
    MMTG_REQUIRE(ws && ws_floats >= g, "sumsq: workspace of %d floats required (mmtg_sumsq_ws)", g);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_OPTIM, s, 2.0 * n, 4.0 * n);
    hipLaunchKernelGGL(sumsq_kernel, dim3(g), dim3(256), 0, s, x, n, ws);
    hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, s, (const float*)ws, g, out);
    MMTG_LAUNCH_CHECK("sumsq");
    return MMTG_OK;
}

extern "C" int mmtg_adamw(float* p, const float* g, float* m, float* v, void* p_bf16, void* p_lo, long n,
                          float lr, float beta1, float beta2, float eps, float wd, int step,
                          const float* normsq, float max_norm, float grad_scale, const float* count, void* stream) {
    MMTG_REQUIRE(p && g && m && v && n > 0 && step >= 1, "adamw: bad args");
    MMTG_REQUIRE(!p_lo || p_bf16, "adamw: the lo plane comes with the hi plane (p_bf16)");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_OPTIM, s, 12.0 * n, (28.0 + (p_bf16 ? 2 : 0) + (p_lo ? 2 : 0)) * n);
    // transformers.AdamW(correct_bias=True): step_size = lr * sqrt(1-b2^t) / (1-b1^t)
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    const float step_size = (float)((double)lr * sqrt(bc2) / bc1);
    hipLaunchKernelGGL(adamw_kernel, dim3(grid_for(n / 4 + 1)), dim3(256), 0, s, p, g, m, v, (bf16*)p_bf16, (bf16*)p_lo, n, lr, beta1, beta2,
                       eps, wd, step_size, normsq, max_norm, grad_scale, count);
    MMTG_LAUNCH_CHECK("adamw");
    return MMTG_OK;
}

// the table rules of the header; `trainable` (optional): elements of the groups whose bit is clear in `frozen`
static int param_groups_check(const char* who, const long* segs, int nsegs, int ngroups, long n, unsigned frozen = 0,
                              double* trainable = nullptr) {
    MMTG_REQUIRE(ngroups >= 1 && ngroups <= MMTG_MAX_PARAM_GROUPS, "%s: ngroups = %d (1 .. %d)", who, ngroups, MMTG_MAX_PARAM_GROUPS);
    MMTG_REQUIRE(nsegs >= 0 && nsegs <= MMTG_MAX_PARAM_SEGS, "%s: nsegs = %d (0 .. %d)", who, nsegs, MMTG_MAX_PARAM_SEGS);
    MMTG_REQUIRE(n > 0, "%s: n = %ld", who, n);
    MMTG_REQUIRE(segs || nsegs == 0, "%s: null segment table", who);
    double live = 0;
    for (int s = 0; s < nsegs; ++s) {
        const long b = segs[3 * s], e = segs[3 * s + 1], g = segs[3 * s + 2];
        MMTG_REQUIRE(e > b, "%s: segment %d [%ld, %ld) is empty", who, s, b, e);
        MMTG_REQUIRE(b >= 0 && e <= n, "%s: segment %d [%ld, %ld) is outside [0, %ld)", who, s, b, e, n);
        MMTG_REQUIRE(g >= 0 && g < ngroups, "%s: segment %d has group %ld (0 .. %d)", who, s, g, ngroups - 1);
        if (s > 0) {
            MMTG_REQUIRE(b >= segs[3 * s - 3], "%s: segment %d begins at %ld, before segment %d (%ld): not sorted", who, s, b, s - 1, segs[3 * s - 3]);
            MMTG_REQUIRE(b >= segs[3 * s - 2], "%s: segment %d [%ld, %ld) overlaps segment %d, which ends at %ld", who, s, b, e, s - 1, segs[3 * s - 2]);
        }
        if (!((frozen >> g) & 1u)) live += (double)(e - b);
    }
    if (trainable) *trainable = live;
    return MMTG_OK;
}

extern "C" int mmtg_param_groups_check(const long* segs, int nsegs, int ngroups, long n) {
    return param_groups_check("param_groups_check", segs, nsegs, ngroups, n);
}

extern "C" long mmtg_sumsq_groups_ws(long n, int ngroups) { return (long)grid_for(n / 4 + 1) * (ngroups > 0 ? ngroups : 0); }

extern "C" int mmtg_sumsq_groups(const float* x, long n, const long* segs_dev, const long* segs_host, int nsegs, int ngroups,
                                 unsigned frozen_mask, float* out, float* ws, long ws_floats, void* stream) {
    double live = 0;
    if (int rc = param_groups_check("sumsq_groups", segs_host, nsegs, ngroups, n, frozen_mask, &live)) return rc;
    MMTG_REQUIRE(x && out && MMTG_ALIGNED16(x) && (segs_dev || nsegs == 0), "sumsq_groups: bad args");
    const int g = grid_for(n / 4 + 1);
    MMTG_REQUIRE(ws && ws_floats >= (long)g * ngroups, "sumsq_groups: workspace of %ld floats required (mmtg_sumsq_groups_ws)", (long)g * ngroups);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_OPTIM, s, 2.0 * live, 4.0 * live);
    hipLaunchKernelGGL(sumsq_groups_kernel, dim3(g), dim3(256), seg_lds_bytes(nsegs) + (size_t)ngroups * 1024, s, x, n, segs_dev, nsegs,
                       ngroups, frozen_mask, ws);
    hipLaunchKernelGGL(sumsq_groups_final_kernel, dim3(1), dim3(256), 0, s, (const float*)ws, g, ngroups, frozen_mask, out);
    MMTG_LAUNCH_CHECK("sumsq_groups");
    return MMTG_OK;
}

extern "C" int mmtg_adamw_groups(float* p, const float* g, float* m, float* v, void* p_bf16, void* p_lo, long n,
                                 const long* segs_dev, const long* segs_host, int nsegs, const mmtg_param_group* groups, int ngroups,
                                 float lr, float beta1, float beta2, float eps, int step,
                                 const float* normsq, float max_norm, float grad_scale, const float* count, void* stream) {
    MMTG_REQUIRE(groups, "adamw_groups: null groups");
    MMTG_REQUIRE(ngroups >= 1 && ngroups <= MMTG_MAX_PARAM_GROUPS, "adamw_groups: ngroups = %d (1 .. %d)", ngroups, MMTG_MAX_PARAM_GROUPS);
    AdamGroups grp;
    memset(&grp, 0, sizeof(grp));
    // transformers.AdamW(correct_bias=True): step_size = lr * sqrt(1-b2^t) / (1-b1^t), per group from the group's fp32 lr
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    for (int k = 0; k < ngroups; ++k) {
        const float sc = groups[k].lr_scale, wd = groups[k].weight_decay;
        MMTG_REQUIRE(sc >= 0.f && sc <= 3.0e38f, "adamw_groups: group %d has lr_scale %g (finite, >= 0)", k, (double)sc);
        MMTG_REQUIRE(wd >= 0.f && wd <= 3.0e38f, "adamw_groups: group %d has weight_decay %g (finite, >= 0)", k, (double)wd);
        grp.lr[k] = (float)((double)lr * (double)sc);
        grp.wd[k] = wd;
        grp.step_size[k] = (float)((double)grp.lr[k] * sqrt(bc2) / bc1);
        if (groups[k].frozen) grp.frozen |= 1u << k;
    }
    double live = 0;
    if (int rc = param_groups_check("adamw_groups", segs_host, nsegs, ngroups, n, grp.frozen, &live)) return rc;
    MMTG_REQUIRE(p && g && m && v && step >= 1 && (segs_dev || nsegs == 0), "adamw_groups: bad args");
    MMTG_REQUIRE(!p_lo || p_bf16, "adamw_groups: the lo plane comes with the hi plane (p_bf16)");
    if (live == 0) return MMTG_OK;              // nothing trainable: nothing to launch
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_OPTIM, s, 12.0 * live, (28.0 + (p_bf16 ? 2 : 0) + (p_lo ? 2 : 0)) * live);
    hipLaunchKernelGGL(adamw_groups_kernel, dim3(grid_for(n / 4 + 1)), dim3(256), seg_lds_bytes(nsegs) + 2 * MMTG_MAX_PARAM_GROUPS * sizeof(float), s,
                       p, g, m, v, (bf16*)p_bf16, (bf16*)p_lo, n, segs_dev, nsegs, grp, beta1, beta2, eps, normsq, max_norm, grad_scale, count);
    MMTG_LAUNCH_CHECK("adamw_groups");
    return MMTG_OK;
}

// [x, x + n floats) and [y, y + n floats) share a byte
static bool ranges_overlap(const void* x, const void* y, long n) {
    const uintptr_t a = (uintptr_t)x, b = (uintptr_t)y, bytes = (uintptr_t)n * sizeof(float);
    return a < b + bytes && b < a + bytes;
}

extern "C" int mmtg_ema_update(float* ema, const float* p, long n, float w, const float* count, void* stream) {
    MMTG_REQUIRE(ema && p, "ema_update: null pointer (ema %p, p %p)", (void*)ema, (const void*)p);
    MMTG_REQUIRE(n > 0, "ema_update: n = %ld", n);
    MMTG_REQUIRE(w >= 0.f && w <= 1.f, "ema_update: w = %g (0 .. 1)", (double)w);         // (NaN fails both comparisons)
    MMTG_REQUIRE(!ranges_overlap(ema, p, n), "ema_update: ema and p overlap (%ld floats at %p and %p)", n, (void*)ema, (const void*)p);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_OPTIM, s, 3.0 * n, 12.0 * n);
    hipLaunchKernelGGL(ema_update_kernel, dim3(grid_for(n / 4 + 1)), dim3(256), 0, s, ema, p, n, w, count);
    MMTG_LAUNCH_CHECK("ema_update");
    return MMTG_OK;
}

extern "C" int mmtg_swap_f32(float* a, float* b, long n, void* stream) {
    MMTG_REQUIRE(a && b, "swap_f32: null pointer (a %p, b %p)", (void*)a, (void*)b);
    MMTG_REQUIRE(n > 0, "swap_f32: n = %ld", n);
    MMTG_REQUIRE(!ranges_overlap(a, b, n), "swap_f32: the buffers overlap (%ld floats at %p and %p)", n, (void*)a, (void*)b);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_OPTIM, s, 0, 16.0 * n);
    hipLaunchKernelGGL(swap_kernel, dim3(grid_for(n / 4 + 1)), dim3(256), 0, s, (unsigned*)a, (unsigned*)b, n);
    MMTG_LAUNCH_CHECK("swap_f32");
    return MMTG_OK;
}

extern "C" int mmtg_cast_f32_to(int dtype, const float* src, void* dst, long n, void* stream) {
    MMTG_REQUIRE(src && dst && n > 0, "cast_f32_to: bad args");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_MISC, s, 0, 6.0 * n);
    if (dtype == MMTG_BF16) hipLaunchKernelGGL(cast_from_f32_kernel<bf16>, dim3(grid_for(n)), dim3(256), 0, s, src, (bf16*)dst, n);
    else if (dtype == MMTG_F32) hipLaunchKernelGGL(cast_from_f32_kernel<float>, dim3(grid_for(n)), dim3(256), 0, s, src, (float*)dst, n);
    else MMTG_FAIL(MMTG_ERR_BAD_ARG, "cast_f32_to: bad dtype");
    MMTG_LAUNCH_CHECK("cast_f32_to");
    return MMTG_OK;
}

extern "C" int mmtg_cast_to_f32(int dtype, const void* src, float* dst, long n, void* stream) {
    MMTG_REQUIRE(src && dst && n > 0, "cast_to_f32: bad args");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_MISC, s, 0, 6.0 * n);
    if (dtype == MMTG_BF16) hipLaunchKernelGGL(cast_to_f32_kernel<bf16>, dim3(grid_for(n)), dim3(256), 0, s, (const bf16*)src, dst, n);
    else if (dtype == MMTG_F32) hipLaunchKernelGGL(cast_to_f32_kernel<float>, dim3(grid_for(n)), dim3(256), 0, s, (const float*)src, dst, n);
    else MMTG_FAIL(MMTG_ERR_BAD_ARG, "cast_to_f32: bad dtype");
    MMTG_LAUNCH_CHECK("cast_to_f32");
    return MMTG_OK;
}

extern "C" int mmtg_cast_pad_rows(int dtype, const float* src, long lds_, void* dst, long ldd, int rows, int cols, void* stream) {
    MMTG_REQUIRE(src && dst && rows > 0 && cols > 0 && ldd >= cols && lds_ >= cols, "cast_pad_rows: bad args");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_MISC, s, 0, 6.0 * rows * cols);
    if (dtype == MMTG_BF16) hipLaunchKernelGGL(cast_pad_rows_kernel<bf16>, dim3(rows), dim3(256), 0, s, src, lds_, (bf16*)dst, ldd, cols);
    else if (dtype == MMTG_F32) hipLaunchKernelGGL(cast_pad_rows_kernel<float>, dim3(rows), dim3(256), 0, s, src, lds_, (float*)dst, ldd, cols);
    else MMTG_FAIL(MMTG_ERR_BAD_ARG, "cast_pad_rows: bad dtype");
    MMTG_LAUNCH_CHECK("cast_pad_rows");
    return MMTG_OK;
}

extern "C" int mmtg_axpy_f32(float* y, const float* x, float a, long n, void* stream) {
    MMTG_REQUIRE(x && y && n > 0, "axpy: bad args");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_MISC, s, 2.0 * n, 12.0 * n);
    hipLaunchKernelGGL(axpy_kernel, dim3(grid_for(n)), dim3(256), 0, s, y, x, a, n);
    MMTG_LAUNCH_CHECK("axpy");
    return MMTG_OK;
}

extern "C" int mmtg_slab_sum(const float* part, int splits, long stride, float* dst, int accumulate, long n, void* stream) {
    MMTG_REQUIRE(part && dst && splits > 0 && n > 0, "slab_sum: bad args");
    MMTG_REQUIRE(n % 4 == 0 && stride % 4 == 0 && stride >= n && MMTG_ALIGNED16(part) && MMTG_ALIGNED16(dst),
                 "slab_sum: n and stride must be multiples of 4 floats, stride >= n, buffers 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_MISC, s, (double)splits * n, 4.0 * n * (splits + 1 + (accumulate ? 1 : 0)));
    const long n4 = n / 4;
    long blocks = (n4 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(slab_sum_kernel, dim3((unsigned)blocks), dim3(256), 0, s, part, splits, stride, dst, accumulate, n4);
    MMTG_LAUNCH_CHECK("slab_sum");
    return MMTG_OK;
}

extern "C" int mmtg_transpose_batch(int dtype, const void* src, void* dst, const long* desc, int n, int max_rows, int max_cols, void* stream) {
    MMTG_REQUIRE(src && dst && desc && n > 0 && max_rows > 0 && max_cols > 0, "transpose_batch: bad args");
    MMTG_REQUIRE(MMTG_ALIGNED16(src) && MMTG_ALIGNED16(dst), "transpose_batch: 16-byte aligned buffers required");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_MISC, s, 0, 0);
    dim3 grid(cdiv(max_rows, 64) * cdiv(max_cols, 64), n);
    if (dtype == MMTG_BF16) hipLaunchKernelGGL(transpose_batch_kernel<bf16>, grid, dim3(256), 0, s, (const bf16*)src, (bf16*)dst, desc);
    else if (dtype == MMTG_F32) hipLaunchKernelGGL(transpose_batch_kernel<float>, grid, dim3(256), 0, s, (const float*)src, (float*)dst, desc);
    else MMTG_FAIL(MMTG_ERR_BAD_ARG, "transpose_batch: bad dtype");
    MMTG_LAUNCH_CHECK("transpose_batch");
    return MMTG_OK;
}
