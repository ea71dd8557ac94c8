// Stochastic beam search (StochasticBeamDecoder, mmtg_amd/decode.py): the merge that follows mmtg_decode_gumbel_candidates (decode.hip)
// at the end of a token step.  include/mmtg_hip.h states the rule.
//   merge (one workgroup per prompt): beam_merge_kernel's selection and tiled reorder (decode.hip), ranked by the candidates'
//     perturbed values cand_g instead of their scores.  A kept candidate's row gets scores[parent] + cand_val and gum = cand_g.
#include "common.h"

constexpr int SB_MAX = 16;         // rows per prompt (the beam decoder's layout)
constexpr int SB_TW = 64;          // columns of seq / keep / rows staged per pass of the reorder

__device__ __forceinline__ bool sb_forced(int j, int sent) { return j > 1 && ((j + 1) % sent == 0 || (j + 1) % sent == 1); }

__global__ __launch_bounds__(256) void gumbel_merge_kernel(const float* __restrict__ cand_val, const int* __restrict__ cand_id,
        const float* __restrict__ cand_g, float* __restrict__ scores, float* __restrict__ gum, long long* __restrict__ seq, long ldseq,
        int* __restrict__ keep, long ldkeep, int* __restrict__ rows, long ldrows, const int* __restrict__ pos_ptr, int P, int sent,
        int nb, int* __restrict__ pos_next, const int* __restrict__ fixed_end) {
    __shared__ float sg[SB_MAX * SB_MAX];
    __shared__ float s_sc[SB_MAX], s_g[SB_MAX];
    __shared__ int s_par[SB_MAX], s_tok[SB_MAX];
    __shared__ long long st_seq[SB_MAX][SB_TW];
    __shared__ int st_keep[SB_MAX][SB_TW], st_rows[SB_MAX][SB_TW];
    const int g = blockIdx.x, tid = threadIdx.x, pos = *pos_ptr, b0 = g * nb;
    if (pos_next && g == 0 && tid == 0) *pos_next = pos + 1;
    const int j = pos + 1 - P;
    const bool next_ok = pos + 1 < ldrows;
    if (fixed_end && pos + 1 < fixed_end[b0]) {            // the prompt's prefix column (one prefix per prompt): every row keeps its
        if (tid < nb && next_ok) rows[(long)(b0 + tid) * ldrows + pos + 1] = b0 + tid;       // score, its value and its given token
        return;
    }
    if (j < 1 || sb_forced(j, sent) || !cand_val) {        // identity: the forced token (if any); a continuation of probability 1
        if (tid < nb) {                                    // inherits its parent's perturbed value, so gum stays what it was
            const long b = b0 + tid;
            if (j >= 1 && sb_forced(j, sent) && pos + 1 < ldseq) seq[b * ldseq + pos + 1] = (j + 1) % sent == 0 ? 2 : 1;
            if (next_ok) rows[b * ldrows + pos + 1] = (int)b;
        }
        return;
    }
    if (pos >= ldseq || pos >= ldkeep || pos >= ldrows) return;        // past a table: nothing to reorder or append
    const int nc = nb * nb;
    float my = -INFINITY;
    int mp = 0, mk = 0;
    if (tid < nc) {
        mp = tid / nb;
        mk = tid - mp * nb;
        my = cand_g[(long)(b0 + mp) * nb + mk];
        if (my != my) my = -INFINITY;                      // (a strict total order: every place below is taken once)
        sg[tid] = my;
    }
    __syncthreads();
    if (tid < nc) {
        // candidate o = (parent o / nb, rank o % nb): (parent, rank) ascending is o ascending
        int place = 0;
        for (int o = 0; o < nc; ++o) {
            const float so = sg[o];
            place += (so > my) || (so == my && o < tid);
        }
        if (place < nb) {
            float sc = scores[b0 + mp] + cand_val[(long)(b0 + mp) * nb + mk];
            if (sc != sc) sc = -INFINITY;
            s_par[place] = mp;
            s_tok[place] = cand_id[(long)(b0 + mp) * nb + mk];
            s_sc[place] = sc;
            s_g[place] = my;
        }
    }
    __syncthreads();                                       // (every read of the old scores is done)
    bool ident = true;
    for (int r = 0; r < nb; ++r) ident = ident && s_par[r] == r;
    if (!ident) {
        for (int c0 = 0; c0 <= pos; c0 += SB_TW) {
            const int w = min(SB_TW, pos + 1 - c0);
            for (int e = tid; e < nb * SB_TW; e += 256) {
                const int r = e / SB_TW, c = e - r * SB_TW;
                if (c < w) {
                    const long b = b0 + r;
                    st_seq[r][c] = seq[b * ldseq + c0 + c];
                    st_keep[r][c] = keep[b * ldkeep + c0 + c];
                    st_rows[r][c] = rows[b * ldrows + c0 + c];
                }
            }
            __syncthreads();
            for (int e = tid; e < nb * SB_TW; e += 256) {
                const int r = e / SB_TW, c = e - r * SB_TW;
                if (c < w) {
                    const long b = b0 + r;
                    const int p = s_par[r];
                    seq[b * ldseq + c0 + c] = st_seq[p][c];
                    keep[b * ldkeep + c0 + c] = st_keep[p][c];
                    rows[b * ldrows + c0 + c] = st_rows[p][c];
                }
            }
            __syncthreads();
        }
    }
    if (tid < nb) {
        const long b = b0 + tid;
        scores[b] = s_sc[tid];
        gum[b] = s_g[tid];
        if (pos + 1 < ldseq) seq[b * ldseq + pos + 1] = s_tok[tid];
        if (next_ok) rows[b * ldrows + pos + 1] = (int)b;
    }
}

extern "C" int mmtg_decode_gumbel_merge(const float* cand_val, const int* cand_id, const float* cand_g, float* scores, float* gum,
                                        long long* seq, long ldseq, int* keep, long ldkeep, int* rows, long ldrows, const int* pos_ptr,
                                        int P, int sent, int nb, int n_prompts, int* pos_next, const int* fixed_end, void* stream) {
    const char* what = "decode_gumbel_merge";
    MMTG_REQUIRE(nb >= 1 && nb <= SB_MAX, "%s: nb = %d rows per prompt (1..%d)", what, nb, SB_MAX);
    MMTG_REQUIRE(gum, "%s: gum [B] is null", what);
    MMTG_REQUIRE(!cand_val || cand_g, "%s: cand_g [B, nb] is null", what);
    MMTG_REQUIRE(!cand_val || cand_id, "%s: cand_id [B, nb] is null", what);
    MMTG_REQUIRE(scores && seq && keep && rows && pos_ptr, "%s: null pointer", what);
    MMTG_REQUIRE(n_prompts > 0 && sent > 1 && P >= 0 && ldseq > P && ldkeep > P && ldrows > P,
                 "%s: bad sizes (prompts %d, sent %d, P %d, ldseq %ld, ldkeep %ld, ldrows %ld)", what, n_prompts, sent, P, ldseq, ldkeep, ldrows);
    MMTG_REQUIRE(pos_next != pos_ptr, "%s: pos_next must not alias pos_ptr", what);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_DECODE, s, (double)n_prompts * nb * nb, 32.0 * n_prompts * nb * (double)ldrows);
    hipLaunchKernelGGL(gumbel_merge_kernel, dim3(n_prompts), dim3(256), 0, s, cand_val, cand_id, cand_g, scores, gum, seq, ldseq, keep,
                       ldkeep, rows, ldrows, pos_ptr, P, sent, nb, pos_next, fixed_end);
    MMTG_LAUNCH_CHECK(what);
    return MMTG_OK;
}
