// Contrastive token loss on the last-layer states (SimCTG, Su et al. 2022; MMTGTrainer(cl_weight=...)).  include/mmtg_hip.h states
// the rule.  Three kernels:
//   cl_rinv_kernel    a wave per row: rinv = 1 / ||hf row||_2 on the rows of I_b, 0 elsewhere (and cl_row = 0 on the topic rows).
//   cl_tile_kernel    flash-attention-like without a softmax.  A workgroup of four waves owns 16 query positions i of one sample
//                     (their rows parked in LDS) and sweeps the sample's positions in steps of 64, 16 per wave:
//                       S^T tile [16 j x 16 i] by MFMA over D (bf16 16x16x32 or fp32 16x16x4), operands read as stored: both are
//                         K-contiguous rows, no transpose anywhere;
//                       the hinge in registers;  forward: the row sums, done;
//                       backward: the 0/1 activity tile through LDS to all four waves -- S^T's accumulator layout IS the A operand
//                         layout of a[i][j] (mma.h), and a is symmetric -- then G[16 i x D] += a[16 i x 16 j] U[16 j x D] with the
//                         fp32 MFMA in every storage form (u_j = h_j * rinv_j formed in fp32 at the load, products with 0 / 1 exact),
//                         the D columns dealt to the waves in 16-wide tiles (tile w, w + 4, ...: at most 16 tiles = 64 fp32 per lane);
//                       the epilogue projects G on the tangent of u_i and adds the increment to d(hf), rounded once.
//                     The workgroup that owns row i sees every term of g_i: no transposed pass, no atomics.
//   cl_sample_kernel  one workgroup: a wave per sample adds its rows in a fixed order, thread 0 adds the samples in order.
#include "mma.h"

constexpr int CL_TI = 16;          // query positions per workgroup
constexpr int CL_TJ = 64;          // positions per sweep step (16 per wave)

template <typename T>
__global__ __launch_bounds__(256) void cl_rinv_kernel(const T* __restrict__ hf, long ldh, const int* __restrict__ keep, long ldkeep,
        int P, int Tt, int D, long M, float* __restrict__ rinv, float* __restrict__ cl_row) {
    constexpr int N = Vec16<T>::N;
    typedef typename Vec16<T>::type V;
    const int lane = threadIdx.x & 63;
    const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const long b = m / Tt;
    const int t = (int)(m - b * Tt);
    float r = 0.f;
    if (t >= P && keep[b * ldkeep + t] != 0) {
        const T* row = hf + m * ldh;
        float q = 0.f;
        for (int c = lane; c < D / N; c += 64) {
            const V v = *reinterpret_cast<const V*>(row + (long)c * N);
#pragma unroll
            for (int e = 0; e < N; ++e) q = fmaf(to_f(v[e]), to_f(v[e]), q);
        }
        q = wave_sum(q);
        r = q > 0.f ? 1.0f / sqrtf(q) : 0.f;
    }
    if (lane == 0) {
        rinv[m] = r;
        if (t < P) cl_row[m] = 0.f;
    }
}

// dynamic LDS: rinv of the sample's lyric columns (0 on PAD and past L) | activity tile | partial sums | the 16 query rows
__host__ __device__ inline int cl_lp(int L) { return (L + CL_TJ - 1) / CL_TJ * CL_TJ; }
__host__ __device__ inline size_t cl_row_bytes(int D, size_t es) { return (size_t)D * es + 16; }      // (+16: rows 4 banks apart)
static size_t cl_lds_bytes(int L, int D, size_t es) { return (size_t)cl_lp(L) * 4 + CL_TJ * CL_TI * 4 + 4 * CL_TI * 4 + 16 + CL_TI * cl_row_bytes(D, es); }

template <typename T, int NT, bool BWD, typename TO>
__global__ __launch_bounds__(256) void cl_tile_kernel(const T* __restrict__ hf, long ldh, const int* __restrict__ keep, long ldkeep,
        const float* __restrict__ rinv_g, float margin, float coef, int P, int L, int D,
        float* __restrict__ cl_row, TO* dhf, long ldd) {
    constexpr int N = Vec16<T>::N;
    typedef typename Vec16<T>::type V;
    extern __shared__ __attribute__((aligned(16))) char cl_smem[];
    const int Lp = cl_lp(L);
    float* const s_rinv = reinterpret_cast<float*>(cl_smem);
    float* const s_act = s_rinv + Lp;
    float* const s_red = s_act + CL_TJ * CL_TI;
    int* const s_cnt = reinterpret_cast<int*>(s_red + 4 * CL_TI);
    char* const s_hi = reinterpret_cast<char*>(s_cnt + 4);
    const size_t HS = cl_row_bytes(D, sizeof(T));

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, i15 = lane & 15;
    const int b = blockIdx.y, i0 = blockIdx.x * CL_TI, Tt = P + L;
    const long row0 = (long)b * Tt + P;                    // the sample's first lyric row

    if (tid == 0) *s_cnt = 0;
    __syncthreads();
    int kept = 0;
    for (int t = tid; t < Lp; t += 256) {
        float r = 0.f;
        if (t < L && keep[(long)b * ldkeep + P + t] != 0) {
            r = rinv_g[row0 + t];
            ++kept;
        }
        s_rinv[t] = r;
    }
    if (BWD && kept) atomicAdd(s_cnt, kept);               // (an integer count: order-free)
    const int cpr = D / N;
    for (int c = tid; c < CL_TI * cpr; c += 256) {
        const int r = c / cpr, k = c - r * cpr;
        const int row = min(i0 + r, L - 1);                // (past the sample: a copy of its last row, masked by rinv = 0)
        *reinterpret_cast<V*>(s_hi + r * HS + (size_t)k * 16) = *reinterpret_cast<const V*>(hf + (row0 + row) * ldh + (long)k * N);
    }
    __syncthreads();
    const int nb = *s_cnt;
    if (BWD && nb < 2) return;

    const float mm1 = margin - 1.0f;
    const float ri = s_rinv[i0 + i15];                     // (i0 + 15 < Lp)
    const int ntile = D / 16;
    float rowsum = 0.f;
    f32x4 G[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) G[n] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int j0 = 0; j0 < L; j0 += CL_TJ) {
        const int jw = j0 + 16 * w;
        f32x4 act = {0.f, 0.f, 0.f, 0.f};
        if (jw < L) {
            // S^T[j = jw + 4g + r][i = i0 + i15] = h_j . h_i: one fixed k order, fp32 accumulation
            f32x4 c = {0.f, 0.f, 0.f, 0.f};
            const T* arow = hf + (row0 + min(jw + i15, L - 1)) * ldh + g * N;
            const char* brow = s_hi + i15 * HS + g * 16;
            const int nkb = D / (4 * N);
            for (int kb = 0; kb < nkb; ++kb) {
                const V av = *reinterpret_cast<const V*>(arow + (long)kb * 4 * N);
                const V bv = *reinterpret_cast<const V*>(brow + kb * 64);
                mma16(av, bv, c);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = jw + 4 * g + r;
                const float rj = s_rinv[j];
                const float x = mm1 + c[r] * (ri * rj);    // (the reciprocals first: s_ij and s_ji are the same bits)
                const bool on = ri > 0.f && rj > 0.f && j != i0 + i15 && x > 0.f;
                if (BWD) act[r] = on ? 1.0f : 0.f;
                else rowsum += on ? x : 0.f;
            }
        }
        if (BWD) {
#pragma unroll
            for (int r = 0; r < 4; ++r) s_act[(16 * w + 4 * g + r) * CL_TI + i15] = act[r];
            __syncthreads();
            for (int jj = 0; jj < 4; ++jj) {
                const int jb = j0 + 16 * jj;
                if (jb >= L) break;
                f32x4 a4, rj4;
                const T* urow[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int j = jb + 4 * g + s;
                    a4[s] = s_act[(16 * jj + 4 * g + s) * CL_TI + i15];
                    rj4[s] = s_rinv[j];
                    urow[s] = hf + (row0 + min(j, L - 1)) * ldh + i15;
                }
                const bool any = a4[0] != 0.f || a4[1] != 0.f || a4[2] != 0.f || a4[3] != 0.f;
                if (__ballot(any) == 0) continue;          // (a tile without an active pair adds +0 everywhere)
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    const int tile = w + 4 * n;
                    if (tile < ntile) {
                        f32x4 u4;
#pragma unroll
                        for (int s = 0; s < 4; ++s) u4[s] = rj4[s] > 0.f ? to_f(urow[s][tile * 16]) * rj4[s] : 0.f;
                        mma16(a4, u4, G[n]);
                    }
                }
            }
            __syncthreads();                               // (s_act is rewritten by the next step)
        }
    }

    if (!BWD) {
        // a lane holds the sum over its j (4g + r of every 16) for i = i15: the lane groups, then the waves, in a fixed order
        rowsum += __shfl_xor(rowsum, 16, 64);
        rowsum += __shfl_xor(rowsum, 32, 64);
        if (lane < 16) s_red[w * CL_TI + lane] = rowsum;
        __syncthreads();
        if (tid < CL_TI && i0 + tid < L)
            cl_row[row0 + i0 + tid] = ((s_red[tid] + s_red[CL_TI + tid]) + s_red[2 * CL_TI + tid]) + s_red[3 * CL_TI + tid];
        return;
    }

    // ---- backward epilogue: lane holds G[i = i0 + 4g + r][d = 16 tile + i15]
    const float scale = 2.0f / ((float)nb * (float)(nb - 1));
    float rr[4], dot[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        rr[r] = s_rinv[i0 + 4 * g + r];
        dot[r] = 0.f;
    }
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int tile = w + 4 * n;
        if (tile < ntile) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float u = to_f(*reinterpret_cast<const T*>(s_hi + (4 * g + r) * HS + (size_t)(tile * 16 + i15) * sizeof(T))) * rr[r];
                dot[r] = fmaf(G[n][r] * scale, u, dot[r]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) dot[r] += __shfl_xor(dot[r], o, 64);
        if (i15 == 0) s_red[w * CL_TI + 4 * g + r] = dot[r];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int il = 4 * g + r;
        dot[r] = ((s_red[il] + s_red[CL_TI + il]) + s_red[2 * CL_TI + il]) + s_red[3 * CL_TI + il];
    }
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int tile = w + 4 * n;
        if (tile < ntile) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (!(rr[r] > 0.f)) continue;              // outside I_b, past the sample, or a zero row: the bits stay
                const float u = to_f(*reinterpret_cast<const T*>(s_hi + (4 * g + r) * HS + (size_t)(tile * 16 + i15) * sizeof(T))) * rr[r];
                const float inc = (coef * rr[r]) * (G[n][r] * scale - dot[r] * u);
                if (inc != 0.f) {
                    TO* p = dhf + (row0 + i0 + 4 * g + r) * ldd + tile * 16 + i15;
                    *p = from_f<TO>(to_f(*p) + inc);       // the one rounding
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void cl_sample_kernel(const float* __restrict__ cl_row, const int* __restrict__ keep, long ldkeep,
        int B, int P, int L, float batch_den, float* __restrict__ cl_sample, float* __restrict__ cl) {
    const int Tt = P + L, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int b = wave; b < B; b += 4) {
        float s = 0.f;
        int n = 0;
        for (int t = P + lane; t < Tt; t += 64) {
            s += cl_row[(long)b * Tt + t];
            n += keep[(long)b * ldkeep + t] != 0;
        }
        s = wave_sum(s);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
        if (lane == 0) cl_sample[b] = n >= 2 ? s / ((float)n * (float)(n - 1)) : 0.f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float tot = 0.f;
        for (int b = 0; b < B; ++b) tot += cl_sample[b];   // fixed order
        cl[0] = tot / batch_den;
    }
}

// ---------------------------------------------------------------- host side
static int cl_check(const char* who, int dtype, const void* hf, long ldh, const int* keep, long ldkeep, float margin,
                    int B, int P, int L, int D) {
    MMTG_REQUIRE(dtype == MMTG_F32 || dtype == MMTG_BF16, "%s: bad dtype %d", who, dtype);
    MMTG_REQUIRE(hf, "%s: null pointer hf", who);
    MMTG_REQUIRE(keep, "%s: null pointer keep", who);
    MMTG_REQUIRE(B > 0 && P >= 0, "%s: bad sizes (B=%d P=%d)", who, B, P);
    MMTG_REQUIRE(L >= 1 && L <= MMTG_CL_MAX_L, "%s: L = %d lyric columns (1 .. %d)", who, L, MMTG_CL_MAX_L);
    MMTG_REQUIRE(D >= 32 && D % 32 == 0 && D <= MMTG_CL_MAX_D, "%s: D = %d (a multiple of 32, at most %d)", who, D, MMTG_CL_MAX_D);
    MMTG_REQUIRE(margin > 0.f && margin <= 1.f, "%s: margin = %g (in (0, 1])", who, (double)margin);
    MMTG_REQUIRE(ldh >= D, "%s: ldh = %ld is narrower than the row (D=%d)", who, ldh, D);
    MMTG_REQUIRE(ldkeep >= (long)P + L, "%s: ldkeep = %ld is narrower than the row (P+L=%d)", who, ldkeep, P + L);
    MMTG_REQUIRE(MMTG_ALIGNED16(hf) && ldh % (dtype == MMTG_F32 ? 4 : 8) == 0, "%s: hf rows must be 16-byte aligned (ldh=%ld)", who, ldh);
    MMTG_REQUIRE((((uintptr_t)keep) & 3) == 0, "%s: keep must be 4-byte aligned", who);
    return MMTG_OK;
}

template <typename K>
static int cl_raise_lds(K kernel, size_t bytes, bool* done, const char* who) {
    if (!*done) {
        // (once, to the most any call can ask for: 16 rows of 1024 fp32, 1024 columns)
        if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
            MMTG_FAIL(MMTG_ERR_HIP, "%s: cannot raise dynamic LDS to %zu bytes", who, bytes);
        *done = true;
    }
    return MMTG_OK;
}

template <typename T, int NT, bool BWD, typename TO>
static int cl_launch_tile(const char* who, hipStream_t s, const void* hf, long ldh, const int* keep, long ldkeep, const float* rinv,
                          float margin, float coef, int B, int P, int L, int D, float* cl_row, void* dhf, long ldd) {
    static bool done = false;
    int rc = cl_raise_lds(cl_tile_kernel<T, NT, BWD, TO>, cl_lds_bytes(MMTG_CL_MAX_L, MMTG_CL_MAX_D, 4), &done, who);
    if (rc) return rc;
    hipLaunchKernelGGL((cl_tile_kernel<T, NT, BWD, TO>), dim3((unsigned)cdiv(L, CL_TI), (unsigned)B), dim3(256),
                       cl_lds_bytes(L, D, sizeof(T)), s, (const T*)hf, ldh, keep, ldkeep, rinv, margin, coef, P, L, D, cl_row, (TO*)dhf, ldd);
    return MMTG_OK;
}

extern "C" int mmtg_cl_fwd(int dtype, const void* hf, long ldh, const int* keep, long ldkeep, float margin, int B, int P, int L, int D,
                           float batch_den, float* rinv, float* cl_row, float* cl_sample, float* cl, void* stream) {
    int rc = cl_check("cl_fwd", dtype, hf, ldh, keep, ldkeep, margin, B, P, L, D);
    if (rc) return rc;
    MMTG_REQUIRE(rinv, "cl_fwd: null pointer rinv");
    MMTG_REQUIRE(cl_row, "cl_fwd: null pointer cl_row");
    MMTG_REQUIRE(cl_sample, "cl_fwd: null pointer cl_sample");
    MMTG_REQUIRE(cl, "cl_fwd: null pointer cl");
    MMTG_REQUIRE(batch_den > 0.f && batch_den <= 3.0e38f, "cl_fwd: batch_den = %g", (double)batch_den);
    hipStream_t s = (hipStream_t)stream;
    const long M = (long)B * (P + L);
    const double es = dtype == MMTG_F32 ? 4.0 : 2.0;
    // (bytes: the floor -- every lyric row once; the tiles re-read their sample from the caches)
    ProfScope prof(MMTG_PROF_LOSS, s, 2.0 * B * L * L * D + 2.0 * B * L * D, es * B * L * D + 12.0 * M);
    if (dtype == MMTG_F32) {
        hipLaunchKernelGGL(cl_rinv_kernel<float>, dim3((unsigned)cdiv(M, 4)), dim3(256), 0, s, (const float*)hf, ldh, keep, ldkeep, P, P + L, D, M, rinv, cl_row);
        rc = cl_launch_tile<float, 1, false, float>("cl_fwd", s, hf, ldh, keep, ldkeep, rinv, margin, 0.f, B, P, L, D, cl_row, nullptr, 0);
    } else {
        hipLaunchKernelGGL(cl_rinv_kernel<bf16>, dim3((unsigned)cdiv(M, 4)), dim3(256), 0, s, (const bf16*)hf, ldh, keep, ldkeep, P, P + L, D, M, rinv, cl_row);
        rc = cl_launch_tile<bf16, 1, false, float>("cl_fwd", s, hf, ldh, keep, ldkeep, rinv, margin, 0.f, B, P, L, D, cl_row, nullptr, 0);
    }
    if (rc) return rc;
    hipLaunchKernelGGL(cl_sample_kernel, dim3(1), dim3(256), 0, s, cl_row, keep, ldkeep, B, P, L, batch_den, cl_sample, cl);
    MMTG_LAUNCH_CHECK("cl_fwd");
    return MMTG_OK;
}

template <typename T, typename TO>
static int cl_bwd_nt(hipStream_t s, const void* hf, long ldh, const int* keep, long ldkeep, const float* rinv, float margin, float coef,
                     int B, int P, int L, int D, void* dhf, long ldd) {
    // the accumulator tiles a wave holds: ceil((D / 16) / 4), compiled for 4, 12 (D = 768) and 16 (D = 1024)
    if (D <= 256) return cl_launch_tile<T, 4, true, TO>("cl_bwd", s, hf, ldh, keep, ldkeep, rinv, margin, coef, B, P, L, D, nullptr, dhf, ldd);
    if (D <= 768) return cl_launch_tile<T, 12, true, TO>("cl_bwd", s, hf, ldh, keep, ldkeep, rinv, margin, coef, B, P, L, D, nullptr, dhf, ldd);
    return cl_launch_tile<T, 16, true, TO>("cl_bwd", s, hf, ldh, keep, ldkeep, rinv, margin, coef, B, P, L, D, nullptr, dhf, ldd);
}

extern "C" int mmtg_cl_bwd(int dtype, int out_dtype, const void* hf, long ldh, const int* keep, long ldkeep, const float* rinv,
                           float margin, float coef, int B, int P, int L, int D, void* dhf, long ldd, void* stream) {
    int rc = cl_check("cl_bwd", dtype, hf, ldh, keep, ldkeep, margin, B, P, L, D);
    if (rc) return rc;
    MMTG_REQUIRE(out_dtype == MMTG_F32 || out_dtype == MMTG_BF16, "cl_bwd: bad out_dtype %d", out_dtype);
    MMTG_REQUIRE(!(dtype == MMTG_BF16 && out_dtype == MMTG_F32), "cl_bwd: out_dtype f32 goes with f32 hf (f32 -> f32, bf16 -> bf16, f32 -> bf16)");
    MMTG_REQUIRE(rinv, "cl_bwd: null pointer rinv");
    MMTG_REQUIRE(dhf, "cl_bwd: null pointer dhf");
    MMTG_REQUIRE(coef >= 0.f && coef <= 3.0e38f, "cl_bwd: coef = %g (finite, >= 0)", (double)coef);
    MMTG_REQUIRE(ldd >= D, "cl_bwd: ldd = %ld is narrower than the row (D=%d)", ldd, D);
    MMTG_REQUIRE(MMTG_ALIGNED16(dhf) && ldd % (out_dtype == MMTG_F32 ? 4 : 8) == 0, "cl_bwd: dhf rows must be 16-byte aligned (ldd=%ld)", ldd);
    if (coef == 0.f) return MMTG_OK;                       // nothing to add: no launch, the bits stay
    hipStream_t s = (hipStream_t)stream;
    const double es = dtype == MMTG_F32 ? 4.0 : 2.0, eo = out_dtype == MMTG_F32 ? 4.0 : 2.0;
    ProfScope prof(MMTG_PROF_LOSS, s, 4.0 * B * L * L * D + 8.0 * B * L * D, (2.0 * es + 2.0 * eo) * B * L * D);
    if (dtype == MMTG_BF16) rc = cl_bwd_nt<bf16, bf16>(s, hf, ldh, keep, ldkeep, rinv, margin, coef, B, P, L, D, dhf, ldd);
    else if (out_dtype == MMTG_F32) rc = cl_bwd_nt<float, float>(s, hf, ldh, keep, ldkeep, rinv, margin, coef, B, P, L, D, dhf, ldd);
    else rc = cl_bwd_nt<float, bf16>(s, hf, ldh, keep, ldkeep, rinv, margin, coef, B, P, L, D, dhf, ldd);
    if (rc) return rc;
    MMTG_LAUNCH_CHECK("cl_bwd");
    return MMTG_OK;
}
