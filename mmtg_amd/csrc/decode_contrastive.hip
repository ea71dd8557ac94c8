// Contrastive search (ContrastiveDecoder, mmtg_amd/decode.py): the two launches that follow the beam candidates of a token step.
// include/mmtg_hip.h states the rule; the candidates are mmtg_decode_beam_candidates*'s, unchanged (decode.hip).
//   similarity (one workgroup per row): u = unit(ln_f(x)) of the row's final residual stream into the hidden cache, and the largest
//     cosine between u and the cached u of the row's own lyric context, read through the ancestry table.
//   merge (one workgroup per prompt): the one row whose token stays, column pos of every row of the prompt, the next candidates.
#include "common.h"

constexpr int CS_MAXD = 1024;      // n_embd the similarity kernel holds: 4 floats per lane and pass, 4 passes of a 64-lane wave
constexpr int CS_MAXK = 16;        // rows per prompt (the beam decoder's layout)

// sum over the 256 threads of a workgroup in a fixed order (wave butterflies, then the four waves in order)
__device__ __forceinline__ float cs_block_sum(float v, float* red, int tid) {
    v = wave_sum(v);
    __syncthreads();                                       // (red may still be read from the previous reduction)
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

template <typename T>
__global__ __launch_bounds__(256) void contrastive_sim_kernel(const T* __restrict__ x, long ldx, const float* __restrict__ gamma,
        const float* __restrict__ beta, float eps, float* __restrict__ hc, int hc_len, float* __restrict__ sim,
        const float* __restrict__ scores, const int* __restrict__ keep, long ldkeep, const int* __restrict__ rows, long ldrows,
        const int* __restrict__ pos_ptr, int P, int B, int D) {
    __shared__ __attribute__((aligned(16))) float su[CS_MAXD];
    __shared__ float red[4], smax[4];
    __shared__ int sany[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, pos = *pos_ptr;
    const int c = pos - P;                                 // the lyric column this step embedded
    if (c < 0) return;                                     // inside the prompt: nothing (the merge reads no sim there)
    if (c >= hc_len || pos >= ldkeep || pos >= ldrows) {   // past the cache or the tables: no state, no context, no penalty
        if (tid == 0) sim[b] = 0.f;
        return;
    }
    // ---- u = unit(ln_f(x_b)): fp32, population variance, two passes over registers
    const T* xr = x + (long)b * ldx;
    float v[4];
    float s = 0.f;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int i = tid + 256 * p;
        v[p] = i < D ? to_f(xr[i]) : 0.f;
        s += v[p];
    }
    const float mean = cs_block_sum(s, red, tid) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const float d = tid + 256 * p < D ? v[p] - mean : 0.f;
        q += d * d;
    }
    const float rstd = 1.0f / sqrtf(cs_block_sum(q, red, tid) / (float)D + eps);
    float n2 = 0.f;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int i = tid + 256 * p;
        v[p] = i < D ? (v[p] - mean) * rstd * gamma[i] + beta[i] : 0.f;
        n2 += v[p] * v[p];
    }
    const float nrm = sqrtf(cs_block_sum(n2, red, tid));
    float* const own = hc + ((long)b * hc_len + c) * D;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int i = tid + 256 * p;
        if (i < D) {
            const float u = nrm > 0.f ? v[p] / nrm : 0.f;
            su[i] = u;
            own[i] = u;
        }
    }
    if (scores && !(scores[b] > -INFINITY)) {              // a dead row is never chosen: its cache slot is defined, its context unread
        if (tid == 0) sim[b] = 0.f;
        return;
    }
    __syncthreads();
    // ---- max over the row's lyric context: wave w takes columns w, w + 4, ...; a lane holds floats [4 lane + 256 p, + 4) of u
    f32x4 ur[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int i = 4 * lane + 256 * p;
        ur[p] = i < D ? *reinterpret_cast<const f32x4*>(su + i) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float m = -INFINITY;
    int any = 0;
    // two columns per pass, so that a wave has up to eight 16-byte loads per lane in flight; a column's own sum has one fixed order
    for (int t0 = wave; t0 < c; t0 += 8) {
        bool ok[2];
        const float* hr[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int t = min(t0 + 4 * e, c - 1);          // (the second column of the last pass may not exist: clamped, not counted)
            const int r = rows[(long)b * ldrows + P + t];
            ok[e] = t0 + 4 * e < c && keep[(long)b * ldkeep + P + t] != 0 && (unsigned)r < (unsigned)B;
            hr[e] = hc + ((long)(ok[e] ? r : b) * hc_len + t) * D;            // (a skipped column reads the row's own slot: in bounds)
        }
        f32x4 h[2][4];
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int i = 4 * lane + 256 * p;
                h[e][p] = i < D ? *reinterpret_cast<const f32x4*>(hr[e] + i) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            float dot = 0.f;
#pragma unroll
            for (int p = 0; p < 4; ++p) dot += ur[p].x * h[e][p].x + ur[p].y * h[e][p].y + ur[p].z * h[e][p].z + ur[p].w * h[e][p].w;
            dot = wave_sum(dot);
            if (ok[e]) { m = fmaxf(m, dot); any = 1; }
        }
    }
    if (lane == 0) { smax[wave] = m; sany[wave] = any; }
    __syncthreads();
    if (tid == 0) {
        float best = -INFINITY;
        int have = 0;
        for (int w = 0; w < 4; ++w)
            if (sany[w]) { best = fmaxf(best, smax[w]); have = 1; }
        sim[b] = have ? best : 0.f;                        // an empty context penalises nothing
    }
}

__device__ __forceinline__ bool cs_forced(int j, int sent) { return j > 1 && ((j + 1) % sent == 0 || (j + 1) % sent == 1); }

__global__ __launch_bounds__(64) void contrastive_merge_kernel(const float* __restrict__ cand_val, const int* __restrict__ cand_id,
        float* __restrict__ scores, const float* __restrict__ sim, float* __restrict__ total, float alpha,
        long long* __restrict__ seq, long ldseq, int* __restrict__ keep, long ldkeep, int* __restrict__ rows, long ldrows,
        const int* __restrict__ pos_ptr, int P, int sent, int k, int* __restrict__ pos_next, const int* __restrict__ fixed_end) {
    __shared__ int s_r;
    const int g = blockIdx.x, tid = threadIdx.x, pos = *pos_ptr, b0 = g * k;
    if (pos_next && g == 0 && tid == 0) *pos_next = pos + 1;
    const int j = pos + 1 - P;
    const bool next_ok = pos + 1 < ldrows && pos + 1 < ldseq;
    if (pos < P) {                                         // inside the prompt: the plain merge's identity
        if (tid < k && next_ok) rows[(long)(b0 + tid) * ldrows + pos + 1] = b0 + tid;
        return;
    }
    if (pos >= ldseq || pos >= ldkeep || pos >= ldrows) return;
    if (tid == 0) {
        // r* = argmax over the live rows of (1 - alpha) p - alpha sim, the lowest r on a tie (row 0 if none is live)
        int rs = 0;
        float best = 0.f;
        bool found = false;
        for (int r = 0; r < k; ++r) {
            const float s = scores[b0 + r];
            if (!(s > -INFINITY)) continue;
            const float cs = (1.0f - alpha) * expf(s) - alpha * sim[b0 + r];
            if (!found || cs > best) { best = cs; rs = r; found = true; }
        }
        s_r = rs;
        total[g] += scores[b0 + rs];
    }
    __syncthreads();
    const long bs = b0 + s_r;
    // column pos of every row becomes the chosen row's (rows[bs, pos] is bs: the previous merge pointed it there)
    const long long tok = seq[bs * ldseq + pos];
    const int kp = keep[bs * ldkeep + pos], rw = rows[bs * ldrows + pos];
    const bool held = fixed_end && pos + 1 < fixed_end[b0];
    const bool forced = !held && cs_forced(j, sent);       // (the first case that applies: a held column is left alone)
    const bool offer = !held && !forced && cand_val;
    float nv = tid == 0 ? 0.f : -INFINITY;
    long long nt = forced ? ((j + 1) % sent == 0 ? 2 : 1) : 0;
    if (offer && tid < k) {
        nv = cand_val[bs * k + tid];
        nt = cand_id[bs * k + tid];
    }
    __syncthreads();                                       // (every read of row bs and of the old scores is done)
    if (tid < k) {
        const long b = b0 + tid;
        seq[b * ldseq + pos] = tok;
        keep[b * ldkeep + pos] = kp;
        rows[b * ldrows + pos] = rw;
        scores[b] = nv;
        if (next_ok) {
            if (forced || offer) seq[b * ldseq + pos + 1] = nt;           // (a held column and a step without candidates: left alone)
            rows[b * ldrows + pos + 1] = (int)b;
        }
    }
}

extern "C" int mmtg_decode_contrastive_sim(int dtype, const void* x, long ldx, const float* gamma, const float* beta, float eps,
                                           float* hc, int hc_len, float* sim, const float* scores, const int* keep, long ldkeep,
                                           const int* rows, long ldrows, const int* pos_ptr, int P, int B, int D, void* stream) {
    const char* what = "decode_contrastive_sim";
    MMTG_REQUIRE(dtype == MMTG_F32 || dtype == MMTG_BF16, "%s: bad dtype %d", what, dtype);
    MMTG_REQUIRE(x && gamma && beta && hc && sim && keep && rows && pos_ptr, "%s: null pointer", what);
    MMTG_REQUIRE(D >= 4 && D % 4 == 0 && D <= CS_MAXD, "%s: n_embd %d must be a multiple of 4 in 4..%d", what, D, CS_MAXD);
    MMTG_REQUIRE(B > 0 && P >= 0 && hc_len >= 1 && ldx >= D && ldkeep > P && ldrows > P && eps >= 0.f,
                 "%s: bad sizes (B %d, P %d, hc_len %d, ldx %ld, ldkeep %ld, ldrows %ld)", what, B, P, hc_len, ldx, ldkeep, ldrows);
    MMTG_REQUIRE(MMTG_ALIGNED16(hc), "%s: the hidden cache must be 16-byte aligned", what);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_DECODE, s, 2.0 * B * D * (double)hc_len, 4.0 * B * D * (double)hc_len);
    if (dtype == MMTG_BF16)
        hipLaunchKernelGGL(contrastive_sim_kernel<bf16>, dim3(B), dim3(256), 0, s, (const bf16*)x, ldx, gamma, beta, eps, hc, hc_len, sim,
                           scores, keep, ldkeep, rows, ldrows, pos_ptr, P, B, D);
    else
        hipLaunchKernelGGL(contrastive_sim_kernel<float>, dim3(B), dim3(256), 0, s, (const float*)x, ldx, gamma, beta, eps, hc, hc_len, sim,
                           scores, keep, ldkeep, rows, ldrows, pos_ptr, P, B, D);
    MMTG_LAUNCH_CHECK(what);
    return MMTG_OK;
}

extern "C" int mmtg_decode_contrastive_merge(const float* cand_val, const int* cand_id, float* scores, const float* sim, float* total,
                                             float alpha, long long* seq, long ldseq, int* keep, long ldkeep, int* rows, long ldrows,
                                             const int* pos_ptr, int P, int sent, int k, int n_prompts, int* pos_next,
                                             const int* fixed_end, void* stream) {
    const char* what = "decode_contrastive_merge";
    MMTG_REQUIRE(k >= 1 && k <= CS_MAXK, "%s: top_k %d outside 1..%d", what, k, CS_MAXK);
    MMTG_REQUIRE(alpha >= 0.f && alpha <= 1.f, "%s: penalty_alpha %g outside [0, 1]", what, (double)alpha);
    MMTG_REQUIRE(scores && sim && total && seq && keep && rows && pos_ptr && (!cand_val || cand_id), "%s: null pointer", what);
    MMTG_REQUIRE(n_prompts > 0 && sent > 1 && P >= 0 && ldseq > P && ldkeep > P && ldrows > P,
                 "%s: bad sizes (prompts %d, sent %d, P %d, ldseq %ld, ldkeep %ld, ldrows %ld)", what, n_prompts, sent, P, ldseq, ldkeep, ldrows);
    MMTG_REQUIRE(pos_next != pos_ptr, "%s: pos_next must not alias pos_ptr", what);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_DECODE, s, 4.0 * n_prompts * k, 64.0 * n_prompts * k);
    hipLaunchKernelGGL(contrastive_merge_kernel, dim3(n_prompts), dim3(64), 0, s, cand_val, cand_id, scores, sim, total, alpha, seq, ldseq,
                       keep, ldkeep, rows, ldrows, pos_ptr, P, sent, k, pos_next, fixed_end);
    MMTG_LAUNCH_CHECK(what);
    return MMTG_OK;
}
