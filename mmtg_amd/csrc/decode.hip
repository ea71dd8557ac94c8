// Generation-side kernels (reference src/generate.py:127-141): the fused logits
// processor + greedy arg-max.  One workgroup per batch row.  The reference divides a logit by
// the repetition penalty once PER OCCURRENCE of its id among the generated tokens; the workgroup
// first counts the occurrences into a 16-bit-per-vocabulary-slot LDS table (LDS atomics), then
// every lane applies that many sequential fp32 divisions to its own slots -- bit-for-bit the
// reference's arithmetic, in O(V + n) instead of the O(V n) scan of the first version (which made
// this kernel 9 % of a decode step: 122 us at 220 generated tokens).
#include "gemm_common.h"

namespace {

constexpr int MAXGEN = 2048;      // < 65536: the counts are 16-bit

// cnt: (V + 1) / 2 words of dynamic LDS.  Counts the ids gen[0..n) (all threads of the block call).
__device__ __forceinline__ void count_ids(unsigned* cnt, int V, const long long* gen, int n, int tid) {
    for (int i = tid; i < (V + 1) / 2; i += 256) cnt[i] = 0u;
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        const int v = (int)gen[i];
        if (v >= 0 && v < V) atomicAdd(cnt + (v >> 1), 1u << (16 * (v & 1)));
    }
    __syncthreads();
}

// the per-occurrence penalty of a logit whose id occurred c times.  NG (the n-gram forms of the selection kernels, ban_ngrams):
// the sentinel count 0xFFFF marks a banned id, whose processed logit is -inf (it stays -inf through the temperature and the bans)
template <bool NG>
__device__ __forceinline__ float penalize(float x, int c, float rep_penalty) {
    if (NG && c == 0xFFFF) return -INFINITY;
    for (int i = 0; i < c; ++i) x = x / rep_penalty;
    return x;
}

// one logit through the reference's processor (generate.py:127-136), folded into the running arg-max (lowest index wins ties)
// LN (the line forms, ban_line): PAD reads its slot too, which ban_line has set to 0 (no penalty, as ever) or to the sentinel
// (sample_row and beam_candidates_kernel restate the processing in their own loops, and the kernels below the block arg-max and
// the count / ban sequence: as shared functions they compile to other code, profiles/r11_select_rule_disassembly_diff.txt)
template <bool NG = false, bool LN = false>
__device__ __forceinline__ void scan_one(float x, int v, const unsigned* cnt, float temperature, float rep_penalty, float& best, int& besti) {
    if ((LN || v != 0) && v != 102) {
        const int c = (cnt[v >> 1] >> (16 * (v & 1))) & 0xFFFF;
        x = penalize<NG>(x, c, rep_penalty);
    }
    x = x / temperature;
    if (v == 1 || v == 2 || v == 100 || v == 102) x = -INFINITY;
    if (x > best || (x == best && v < besti)) { best = x; besti = v; }
}
// this thread's share of the processed-logit arg-max.  16-byte aligned rows are read as float4 with all of a pass's loads
// (up to 16 per thread = 16 K logits per block) requested before the first is used: one memory round trip per row instead of a
// dependent 4-byte load per 256 logits (round 3: 21.5 -> see profiles/ us for 256 rows of V = 13317).
template <bool NG = false, bool LN = false>
__device__ __forceinline__ void scan_row(const float* row, int V, const unsigned* cnt, float temperature, float rep_penalty,
                                         int tid, float& best, int& besti) {
    best = -INFINITY;
    besti = 0x7fffffff;
    int done = 0;
    if ((reinterpret_cast<uintptr_t>(row) & 15) == 0) {
        constexpr int UN = 16;
        const int nvec = V >> 2;
        const f32x4* row4 = reinterpret_cast<const f32x4*>(row);
        for (int base = 0; base < nvec; base += 256 * UN) {
            f32x4 r[UN];
#pragma unroll
            for (int i = 0; i < UN; ++i) {
                const int idx = base + i * 256 + tid;
                r[i] = idx < nvec ? row4[idx] : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int i = 0; i < UN; ++i) {
                const int idx = base + i * 256 + tid;
                if (idx < nvec) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) scan_one<NG, LN>(r[i][e], 4 * idx + e, cnt, temperature, rep_penalty, best, besti);
                }
            }
        }
        done = nvec << 2;
    }
    for (int v = done + tid; v < V; v += 256) scan_one<NG, LN>(row[v], v, cnt, temperature, rep_penalty, best, besti);
}

__global__ __launch_bounds__(256) void logits_argmax_kernel(const float* __restrict__ logits, long ldl, int V,
        const long long* __restrict__ generated, long ldg, const int* __restrict__ gen_len,
        float temperature, float rep_penalty, long long* __restrict__ next) {
    extern __shared__ unsigned cnt[];
    __shared__ float sval[4];
    __shared__ int sidx[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(gen_len[b], MAXGEN);
    const long long* gen = generated + (long)b * ldg;
    if (n > 0 && gen[n - 1] == 0) {  // sticky PAD (generate.py:137-138)
        if (tid == 0) next[b] = 0;
        return;
    }
    count_ids(cnt, V, gen, n, tid);
    float best;
    int besti;
    scan_row(logits + (long)b * ldl, V, cnt, temperature, rep_penalty, tid, best, besti);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(besti, o, 64);
        if (ov > best || (ov == best && oi < besti)) { best = ov; besti = oi; }
    }
    if ((tid & 63) == 0) { sval[tid >> 6] = best; sidx[tid >> 6] = besti; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w)
            if (sval[w] > best || (sval[w] == best && sidx[w] < besti)) { best = sval[w]; besti = sidx[w]; }
        next[b] = besti == 0x7fffffff ? 0 : besti;
    }
}

// ------------------------------------------------------------------ stochastic selection (generate.py:64-94,127-141)
// One workgroup per row: processed logits (penalty, temperature, bans, as above) -> top-k filter
// (`logits < kth largest` dropped, ties at the k-th value kept) -> nucleus filter over the survivors (sorted
// descending, an element stays while the probability mass of the elements before it is <= top_p) -> softmax ->
// one draw by inverse CDF over the kept ids in index order with the caller's uniform u in [0,1).
// No sort: both thresholds come from a 4-pass radix select over the order-preserving integer image of the
// floats -- by COUNT for top-k, by accumulated probability MASS for top-p.  px: V floats of LDS.
__device__ __forceinline__ unsigned fkey(float x) {
    const unsigned b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// (TM changes nothing in the body: it gives the template form an instantiation of its own, which its one caller inlines by force.
// As a second user of <true, true> it takes the line form's copy out of line, and left out of line itself it is a second LDS-using
// function of the module: either way the earlier sampling kernels compile to other code, profiles/r12_template_decode_disassembly_diff.txt)
template <bool NG = false, bool LN = false, bool TM = false>
__device__ int sample_row(const float* row, int V, const unsigned* cnt, float* px, float temperature, float rep_penalty,
                          int top_k, float top_p, float u, int tid, float* filtered) {
    __shared__ unsigned hcnt[256];
    __shared__ float hmass[256];
    __shared__ float sred[4];
    __shared__ unsigned s_prefix, s_rem;
    __shared__ float s_acc;
    __shared__ int s_pick;
    for (int v = tid; v < V; v += 256) {
        float x = row[v];
        if ((LN || v != 0) && v != 102) {
            const int c = (cnt[v >> 1] >> (16 * (v & 1))) & 0xFFFF;
            x = penalize<NG>(x, c, rep_penalty);
        }
        x = x / temperature;
        if (v == 1 || v == 2 || v == 100 || v == 102) x = -INFINITY;
        px[v] = x;
    }
    __syncthreads();
    // ---- top-k: key of the k-th largest value
    unsigned keyk = 0u;
    if (top_k > 0 && top_k < V) {
        if (tid == 0) { s_prefix = 0u; s_rem = (unsigned)top_k; }
        unsigned mask = 0u;
        for (int shift = 24; shift >= 0; shift -= 8) {
            hcnt[tid] = 0u;
            __syncthreads();
            const unsigned prefix = s_prefix;
            for (int v = tid; v < V; v += 256) {
                const unsigned k = fkey(px[v]);
                if ((k & mask) == prefix) atomicAdd(hcnt + ((k >> shift) & 255u), 1u);
            }
            __syncthreads();
            if (tid == 0) {
                unsigned rem = s_rem;
                int bin = 255;
                for (; bin > 0; --bin) {
                    if (hcnt[bin] >= rem) break;
                    rem -= hcnt[bin];
                }
                s_rem = rem;
                s_prefix = prefix | ((unsigned)bin << shift);
            }
            mask |= 255u << shift;
            __syncthreads();
        }
        keyk = s_prefix;
    }
    // ---- max and total mass of the survivors
    float mx = -INFINITY;
    for (int v = tid; v < V; v += 256)
        if (fkey(px[v]) >= keyk) mx = fmaxf(mx, px[v]);
    mx = wave_max(mx);
    if ((tid & 63) == 0) sred[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(sred[0], sred[1]), fmaxf(sred[2], sred[3]));
    __syncthreads();
    float tot = 0.f;
    for (int v = tid; v < V; v += 256)
        if (fkey(px[v]) >= keyk) tot += expf(px[v] - mx);
    tot = wave_sum(tot);
    if ((tid & 63) == 0) sred[tid >> 6] = tot;
    __syncthreads();
    tot = sred[0] + sred[1] + sred[2] + sred[3];
    __syncthreads();
    // ---- top-p: key of the first element (descending) whose inclusive mass exceeds top_p
    unsigned keyp = 0u;
    if (top_p > 0.f) {
        const float P = top_p * tot;
        if (tid == 0) { s_prefix = 0u; s_acc = 0.f; s_pick = 1; }
        unsigned mask = 0u;
        for (int shift = 24; shift >= 0; shift -= 8) {
            hmass[tid] = 0.f;
            __syncthreads();
            const unsigned prefix = s_prefix;
            if (s_pick)
                for (int v = tid; v < V; v += 256) {
                    const unsigned k = fkey(px[v]);
                    if (k >= keyk && (k & mask) == prefix) atomicAdd(hmass + ((k >> shift) & 255u), expf(px[v] - mx));
                }
            __syncthreads();
            if (tid == 0 && s_pick) {
                float acc = s_acc;
                int bin = 255;
                for (; bin >= 0; --bin) {
                    if (acc + hmass[bin] > P) break;
                    acc += hmass[bin];
                }
                if (bin < 0) s_pick = 0;                 // the whole mass stays within top_p: keep every survivor
                else { s_acc = acc; s_prefix = prefix | ((unsigned)bin << shift); }
            }
            mask |= 255u << shift;
            __syncthreads();
        }
        keyp = s_pick ? s_prefix : 0u;
        __syncthreads();
    }
    const unsigned keyt = keyk > keyp ? keyk : keyp;
    if (filtered)
        for (int v = tid; v < V; v += 256) filtered[v] = fkey(px[v]) >= keyt ? px[v] : -INFINITY;
    // ---- inverse CDF over the kept ids in index order
    const int chunk = (V + 255) / 256, v0 = tid * chunk, v1 = min(V, v0 + chunk);
    float mine = 0.f;
    for (int v = v0; v < v1; ++v)
        if (fkey(px[v]) >= keyt && px[v] > -INFINITY) mine += expf(px[v] - mx);
    // inclusive scan of the 256 chunk sums (in hmass)
    hmass[tid] = mine;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const float add = tid >= o ? hmass[tid - o] : 0.f;
        __syncthreads();
        hmass[tid] += add;
        __syncthreads();
    }
    const float Z = hmass[255], target = u * Z;
    if (tid == 0) s_pick = 0x7fffffff;
    __syncthreads();
    const float before = tid ? hmass[tid - 1] : 0.f;
    if (mine > 0.f && target < hmass[tid] && target >= before) {
        float acc = before;
        int pick = -1;
        for (int v = v0; v < v1; ++v)
            if (fkey(px[v]) >= keyt && px[v] > -INFINITY) {
                acc += expf(px[v] - mx);
                pick = v;
                if (target < acc) break;
            }
        if (pick >= 0) atomicMin(&s_pick, pick);
    }
    __syncthreads();
    if (s_pick == 0x7fffffff) {          // rounding at the upper end: the last kept id
        int last = -1;
        for (int v = v0; v < v1; ++v)
            if (fkey(px[v]) >= keyt && px[v] > -INFINITY) last = v;
        __syncthreads();
        if (tid == 0) s_pick = -1;
        __syncthreads();
        if (last >= 0) atomicMax(&s_pick, last);
        __syncthreads();
    }
    return s_pick < 0 ? 0 : s_pick;
}

__global__ __launch_bounds__(256) void logits_sample_kernel(const float* __restrict__ logits, long ldl, int V,
        const long long* __restrict__ generated, long ldg, const int* __restrict__ gen_len,
        float temperature, float rep_penalty, int top_k, float top_p, const float* __restrict__ uniforms,
        long long* __restrict__ next, float* __restrict__ filtered) {
    extern __shared__ unsigned cnt[];
    float* px = reinterpret_cast<float*>(cnt + (V + 1) / 2);
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(gen_len[b], MAXGEN);
    const long long* gen = generated + (long)b * ldg;
    if (n > 0 && gen[n - 1] == 0) {  // sticky PAD (generate.py:137-138)
        if (tid == 0) next[b] = 0;
        return;
    }
    count_ids(cnt, V, gen, n, tid);
    const int pick = sample_row(logits + (long)b * ldl, V, cnt, px, temperature, rep_penalty, top_k, top_p, uniforms[b], tid,
                                filtered ? filtered + (long)b * ldl : nullptr);
    if (tid == 0) next[b] = pick;
}

// ------------------------------------------------------------------ truncation beyond top-k / top-p (the *_warp entries)
// sample_row with four more stages between the nucleus filter and the draw, in transformers' warper order: min-p, locally typical,
// epsilon, eta (include/mmtg_hip.h states the rule).  A function of its own: sample_row and its instantiations are untouched, and this
// one is inlined by force into its two kernels, so the module gets no out-of-line function that uses LDS (sample_row's comment).
// No per-id memory beyond px: with e(v) = exp(px[v] - mx) and the stage's survivor mass tot, p = e / tot and log p = px[v] - mx -
// log(tot) are recomputed where needed.  Every stage is block reductions over its survivors (mass, sum of e * (px - mx) for the
// entropy, the survivors' maximum) that give one scalar cut; the typical cut is a 4-pass radix select by accumulated mass over the
// integer image of key = |-log p - H|, ascending, so ids tied at the cut key stay.  The cuts combine into `kept`, which the
// stages after them, `filtered` and the CDF pass evaluate.
// MS adds Mirostat v2 as the last stage (the *_mirostat entries): one more survivor mass gives the cut e >= 2^-mu * m, which joins
// `kept` beside the epsilon and eta cuts and keeps the survivors' maximum as they do; the pick's surprise comes from the scan's total.
template <bool MS = false>
struct WarpCuts {
    unsigned keyt;      // top-k / top-p: integer image of the smallest kept logit
    float mx;           // the row's largest processed logit
    float emin;         // min-p: e >= emin
    bool typ;           // the typical cut is set
    float lt, H;        // typical: log of the stage's mass, its entropy
    unsigned tkey;      // typical: integer image of the largest kept key
    float msurv;        // the largest logit among the typical stage's survivors (the epsilon and eta stages always keep it)
    float eps_e, eta_e; // epsilon / eta: e >= cut (p >= cutoff, times the stage's mass)
    float mu_e;         // Mirostat (MS only): e >= 2^-mu times the stage's mass
    __device__ __forceinline__ float tkeyf(float x) const { return fabsf((lt - (x - mx)) - H); }
    __device__ __forceinline__ bool kept(float x) const {
        if (!(fkey(x) >= keyt && x > -INFINITY)) return false;
        const float e = expf(x - mx);
        if (e < emin) return false;
        if (typ && fkey(tkeyf(x)) > tkey) return false;
        if constexpr (MS) return x >= msurv || (e >= eps_e && e >= eta_e && e >= mu_e);
        else return x >= msurv || (e >= eps_e && e >= eta_e);
    }
};

template <bool NG = false, bool LN = false, bool MS = false>
__device__ __forceinline__ int sample_row_warp(const float* row, int V, const unsigned* cnt, float* px, float temperature,
                                               float rep_penalty, int top_k, float top_p, float min_p, float typical_p,
                                               float epsilon_cutoff, float eta_cutoff, float u, int tid, float* filtered,
                                               [[maybe_unused]] float mu = 0.f, [[maybe_unused]] float* surprise = nullptr) {
    __shared__ unsigned hcnt[256];
    __shared__ float hmass[256];
    __shared__ float sred[4];
    __shared__ unsigned s_prefix, s_rem;
    __shared__ float s_acc;
    __shared__ int s_pick;
    for (int v = tid; v < V; v += 256) {
        float x = row[v];
        if ((LN || v != 0) && v != 102) {
            const int c = (cnt[v >> 1] >> (16 * (v & 1))) & 0xFFFF;
            x = penalize<NG>(x, c, rep_penalty);
        }
        x = x / temperature;
        if (v == 1 || v == 2 || v == 100 || v == 102) x = -INFINITY;
        px[v] = x;
    }
    __syncthreads();
    // block reductions (every thread of the block calls; the result is uniform)
    auto block_sum = [&](float a) {
        a = wave_sum(a);
        if ((tid & 63) == 0) sred[tid >> 6] = a;
        __syncthreads();
        a = sred[0] + sred[1] + sred[2] + sred[3];
        __syncthreads();
        return a;
    };
    auto block_max = [&](float a) {
        a = wave_max(a);
        if ((tid & 63) == 0) sred[tid >> 6] = a;
        __syncthreads();
        a = fmaxf(fmaxf(sred[0], sred[1]), fmaxf(sred[2], sred[3]));
        __syncthreads();
        return a;
    };
    // ---- top-k and top-p, as sample_row computes them
    unsigned keyk = 0u;
    if (top_k > 0 && top_k < V) {
        if (tid == 0) { s_prefix = 0u; s_rem = (unsigned)top_k; }
        unsigned mask = 0u;
        for (int shift = 24; shift >= 0; shift -= 8) {
            hcnt[tid] = 0u;
            __syncthreads();
            const unsigned prefix = s_prefix;
            for (int v = tid; v < V; v += 256) {
                const unsigned k = fkey(px[v]);
                if ((k & mask) == prefix) atomicAdd(hcnt + ((k >> shift) & 255u), 1u);
            }
            __syncthreads();
            if (tid == 0) {
                unsigned rem = s_rem;
                int bin = 255;
                for (; bin > 0; --bin) {
                    if (hcnt[bin] >= rem) break;
                    rem -= hcnt[bin];
                }
                s_rem = rem;
                s_prefix = prefix | ((unsigned)bin << shift);
            }
            mask |= 255u << shift;
            __syncthreads();
        }
        keyk = s_prefix;
    }
    float mx = -INFINITY;
    for (int v = tid; v < V; v += 256)
        if (fkey(px[v]) >= keyk) mx = fmaxf(mx, px[v]);
    mx = block_max(mx);
    float tot = 0.f;
    for (int v = tid; v < V; v += 256)
        if (fkey(px[v]) >= keyk) tot += expf(px[v] - mx);
    tot = block_sum(tot);
    unsigned keyp = 0u;
    if (top_p > 0.f) {
        const float P = top_p * tot;
        if (tid == 0) { s_prefix = 0u; s_acc = 0.f; s_pick = 1; }
        unsigned mask = 0u;
        for (int shift = 24; shift >= 0; shift -= 8) {
            hmass[tid] = 0.f;
            __syncthreads();
            const unsigned prefix = s_prefix;
            if (s_pick)
                for (int v = tid; v < V; v += 256) {
                    const unsigned k = fkey(px[v]);
                    if (k >= keyk && (k & mask) == prefix) atomicAdd(hmass + ((k >> shift) & 255u), expf(px[v] - mx));
                }
            __syncthreads();
            if (tid == 0 && s_pick) {
                float acc = s_acc;
                int bin = 255;
                for (; bin >= 0; --bin) {
                    if (acc + hmass[bin] > P) break;
                    acc += hmass[bin];
                }
                if (bin < 0) s_pick = 0;
                else { s_acc = acc; s_prefix = prefix | ((unsigned)bin << shift); }
            }
            mask |= 255u << shift;
            __syncthreads();
        }
        keyp = s_pick ? s_prefix : 0u;
        __syncthreads();
    }
    WarpCuts<MS> w = {keyk > keyp ? keyk : keyp, mx, 0.f, false, 0.f, 0.f, 0u, mx, 0.f, 0.f, 0.f};
    // ---- min-p: p < min_p * pmax, and pmax = 1 / tot, so e < min_p (the maximum has e = 1 >= min_p)
    w.emin = min_p;
    // ---- locally typical: the ids nearest the entropy, by ascending key, until their mass reaches typical_p
    if (typical_p < 1.f) {
        float m = 0.f, s = 0.f;
        for (int v = tid; v < V; v += 256)
            if (w.kept(px[v])) { const float e = expf(px[v] - mx); m += e; if (e > 0.f) s += e * (px[v] - mx); }
        m = block_sum(m);
        s = block_sum(s);
        const float lt = logf(m), H = lt - s / m, P = typical_p * m;
        if (tid == 0) { s_prefix = 0u; s_acc = 0.f; s_pick = 1; }
        unsigned mask = 0u;
        for (int shift = 24; shift >= 0; shift -= 8) {
            hmass[tid] = 0.f;
            __syncthreads();
            const unsigned prefix = s_prefix;
            if (s_pick)
                for (int v = tid; v < V; v += 256) {
                    const float x = px[v];
                    if (!w.kept(x)) continue;
                    const unsigned k = fkey(fabsf((lt - (x - mx)) - H));
                    if ((k & mask) == prefix) atomicAdd(hmass + ((k >> shift) & 255u), expf(x - mx));
                }
            __syncthreads();
            if (tid == 0 && s_pick) {
                float acc = s_acc;
                int bin = 0;
                for (; bin < 256; ++bin) {
                    if (acc + hmass[bin] >= P) break;
                    acc += hmass[bin];
                }
                if (bin == 256 && shift == 24) s_pick = 0;     // the mass is never reached in fp32: keep every survivor
                else {
                    if (bin == 256) bin = 255;                 // reached at the end of the bin above (the sums round apart): all of it
                    s_acc = acc;
                    s_prefix = prefix | ((unsigned)bin << shift);
                }
            }
            mask |= 255u << shift;
            __syncthreads();
        }
        if (s_pick) { w.lt = lt; w.H = H; w.tkey = s_prefix; w.typ = true; }
        __syncthreads();
        if (w.typ && (MS || epsilon_cutoff > 0.f || eta_cutoff > 0.f)) {     // the head may be gone: the later stages keep the survivors' maximum
            float ms = -INFINITY;
            for (int v = tid; v < V; v += 256)
                if (w.kept(px[v])) ms = fmaxf(ms, px[v]);
            w.msurv = block_max(ms);
        }
    }
    // ---- epsilon: p < epsilon_cutoff over the survivors
    if (epsilon_cutoff > 0.f) {
        float m = 0.f;
        for (int v = tid; v < V; v += 256)
            if (w.kept(px[v])) m += expf(px[v] - mx);
        m = block_sum(m);
        w.eps_e = epsilon_cutoff * m;
    }
    // ---- eta: p < min(eta_cutoff, sqrt(eta_cutoff) * exp(-H)) over the survivors
    if (eta_cutoff > 0.f) {
        float m = 0.f, s = 0.f;
        for (int v = tid; v < V; v += 256)
            if (w.kept(px[v])) { const float e = expf(px[v] - mx); m += e; if (e > 0.f) s += e * (px[v] - mx); }
        m = block_sum(m);
        s = block_sum(s);
        const float H = logf(m) - s / m;
        w.eta_e = fminf(eta_cutoff, sqrtf(eta_cutoff) * expf(-H)) * m;
    }
    // ---- Mirostat v2: -log2 p > mu over the survivors, that is e < 2^-mu * m (mu is the row's, read before any barrier above)
    if constexpr (MS) {
        float m = 0.f;
        for (int v = tid; v < V; v += 256)
            if (w.kept(px[v])) m += expf(px[v] - mx);
        m = block_sum(m);
        w.mu_e = exp2f(-mu) * m;
    }
    if (filtered)
        for (int v = tid; v < V; v += 256) filtered[v] = w.kept(px[v]) ? px[v] : -INFINITY;
    // ---- inverse CDF over the kept ids in index order (sample_row's)
    const int chunk = (V + 255) / 256, v0 = tid * chunk, v1 = min(V, v0 + chunk);
    float mine = 0.f;
    for (int v = v0; v < v1; ++v)
        if (w.kept(px[v])) mine += expf(px[v] - mx);
    hmass[tid] = mine;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const float add = tid >= o ? hmass[tid - o] : 0.f;
        __syncthreads();
        hmass[tid] += add;
        __syncthreads();
    }
    const float Z = hmass[255], target = u * Z;
    if (tid == 0) s_pick = 0x7fffffff;
    __syncthreads();
    const float before = tid ? hmass[tid - 1] : 0.f;
    if (mine > 0.f && target < hmass[tid] && target >= before) {
        float acc = before;
        int pick = -1;
        for (int v = v0; v < v1; ++v)
            if (w.kept(px[v])) {
                acc += expf(px[v] - mx);
                pick = v;
                if (target < acc) break;
            }
        if (pick >= 0) atomicMin(&s_pick, pick);
    }
    __syncthreads();
    if (s_pick == 0x7fffffff) {          // rounding at the upper end: the last kept id
        int last = -1;
        for (int v = v0; v < v1; ++v)
            if (w.kept(px[v])) last = v;
        __syncthreads();
        if (tid == 0) s_pick = -1;
        __syncthreads();
        if (last >= 0) atomicMax(&s_pick, last);
        __syncthreads();
    }
    if constexpr (MS)          // the pick's surprise in bits under the kept set's softmax: Z is the kept set's mass already
        *surprise = (logf(Z) - (px[s_pick < 0 ? 0 : s_pick] - mx)) * 1.44269504088896341f;
    return s_pick < 0 ? 0 : s_pick;
}

__global__ __launch_bounds__(256) void logits_sample_warp_kernel(const float* __restrict__ logits, long ldl, int V,
        const long long* __restrict__ generated, long ldg, const int* __restrict__ gen_len,
        float temperature, float rep_penalty, int top_k, float top_p, float min_p, float typical_p, float epsilon_cutoff,
        float eta_cutoff, const float* __restrict__ uniforms, long long* __restrict__ next, float* __restrict__ filtered) {
    extern __shared__ unsigned cnt[];
    float* px = reinterpret_cast<float*>(cnt + (V + 1) / 2);
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(gen_len[b], MAXGEN);
    const long long* gen = generated + (long)b * ldg;
    if (n > 0 && gen[n - 1] == 0) {  // sticky PAD (generate.py:137-138)
        if (tid == 0) next[b] = 0;
        return;
    }
    count_ids(cnt, V, gen, n, tid);
    const int pick = sample_row_warp(logits + (long)b * ldl, V, cnt, px, temperature, rep_penalty, top_k, top_p, min_p, typical_p,
                                     epsilon_cutoff, eta_cutoff, uniforms[b], tid, filtered ? filtered + (long)b * ldl : nullptr);
    if (tid == 0) next[b] = pick;
}

// logits_sample_warp_kernel with the Mirostat stage: mu[b] is the row's state, read by every thread before the first barrier and
// stored by thread 0 after the draw; a sticky-PAD row leaves it alone.
__global__ __launch_bounds__(256) void logits_sample_mirostat_kernel(const float* __restrict__ logits, long ldl, int V,
        const long long* __restrict__ generated, long ldg, const int* __restrict__ gen_len,
        float temperature, float rep_penalty, int top_k, float top_p, float min_p, float typical_p, float epsilon_cutoff,
        float eta_cutoff, float tau, float eta, const float* __restrict__ uniforms, long long* __restrict__ next,
        float* __restrict__ filtered, float* mu, float* __restrict__ surprise) {
    extern __shared__ unsigned cnt[];
    float* px = reinterpret_cast<float*>(cnt + (V + 1) / 2);
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(gen_len[b], MAXGEN);
    const long long* gen = generated + (long)b * ldg;
    if (n > 0 && gen[n - 1] == 0) {  // sticky PAD: no draw, no update
        if (tid == 0) { next[b] = 0; if (surprise) surprise[b] = 0.f; }
        return;
    }
    const float mub = mu[b];
    count_ids(cnt, V, gen, n, tid);
    float s;
    const int pick = sample_row_warp<false, false, true>(logits + (long)b * ldl, V, cnt, px, temperature, rep_penalty, top_k, top_p,
                                                         min_p, typical_p, epsilon_cutoff, eta_cutoff, uniforms[b], tid,
                                                         filtered ? filtered + (long)b * ldl : nullptr, mub, &s);
    if (tid == 0) {
        next[b] = pick;
        mu[b] = mub - eta * (s - tau);
        if (surprise) surprise[b] = s;
    }
}

// (what both *_warp entries ask of the four cuts; a NaN fails every test)
static int warp_args_check(const char* what, float min_p, float typical_p, float epsilon_cutoff, float eta_cutoff) {
    MMTG_REQUIRE(min_p >= 0.f && min_p <= 1.f, "%s: min_p must be in [0, 1]", what);
    MMTG_REQUIRE(typical_p > 0.f && typical_p <= 1.f, "%s: typical_p must be in (0, 1]", what);
    MMTG_REQUIRE(epsilon_cutoff >= 0.f && epsilon_cutoff < 1.f, "%s: epsilon_cutoff must be in [0, 1)", what);
    MMTG_REQUIRE(eta_cutoff >= 0.f && eta_cutoff < 1.f, "%s: eta_cutoff must be in [0, 1)", what);
    return MMTG_OK;
}

// (what both *_mirostat entries ask; 0 is "off" on the Python surface and has no meaning here)
static int mirostat_args_check(const char* what, float tau, float eta, const float* mu) {
    MMTG_REQUIRE(tau > 0.f && tau <= 32.f, "%s: mirostat_tau must be in (0, 32]", what);
    MMTG_REQUIRE(eta >= 0.f && eta <= 1.f, "%s: mirostat_eta must be in [0, 1]", what);
    MMTG_REQUIRE(mu, "%s: mirostat needs the mu buffer", what);
    return MMTG_OK;
}

}  // namespace

extern "C" int mmtg_logits_process_sample_mirostat(const float* logits, long ldl, int V, const long long* generated, long ldg,
                                                   const int* gen_len, float temperature, float rep_penalty, int top_k, float top_p,
                                                   float min_p, float typical_p, float epsilon_cutoff, float eta_cutoff,
                                                   const float* uniforms, long long* next, float* filtered, int B,
                                                   float mirostat_tau, float mirostat_eta, float* mu, float* surprise, void* stream) {
    if (int e = mirostat_args_check("logits_process_sample_mirostat", mirostat_tau, mirostat_eta, mu)) return e;
    MMTG_REQUIRE(logits && generated && gen_len && uniforms && next && B > 0 && V > 0 && ldl >= V, "logits_process_sample_mirostat: bad args");
    MMTG_REQUIRE(temperature > 0.f && rep_penalty > 0.f && top_k >= 0 && top_p >= 0.f, "logits_process_sample_mirostat: bad sampling parameters");
    if (int e = warp_args_check("logits_process_sample_mirostat", min_p, typical_p, epsilon_cutoff, eta_cutoff)) return e;
    MMTG_REQUIRE(V <= 24000, "logits_process_sample_mirostat: vocabulary of %d exceeds the LDS row image (24000)", V);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_DECODE, s, 44.0 * B * V, 4.0 * B * V);
    const size_t shm = (size_t)((V + 1) / 2) * 4 + (size_t)V * 4;
    static bool attr_done = false;
    if (!attr_done) {
        if (hipFuncSetAttribute((const void*)logits_sample_mirostat_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096) != hipSuccess)
            MMTG_FAIL(MMTG_ERR_HIP, "logits_process_sample_mirostat: cannot raise dynamic LDS");
        attr_done = true;
    }
    hipLaunchKernelGGL(logits_sample_mirostat_kernel, dim3(B), dim3(256), shm, s, logits, ldl, V, generated, ldg, gen_len, temperature,
                       rep_penalty, top_k, top_p, min_p, typical_p, epsilon_cutoff, eta_cutoff, mirostat_tau, mirostat_eta, uniforms, next,
                       filtered, mu, surprise);
    MMTG_LAUNCH_CHECK("logits_process_sample_mirostat");
    return MMTG_OK;
}

extern "C" int mmtg_logits_process_sample_warp(const float* logits, long ldl, int V, const long long* generated, long ldg,
                                               const int* gen_len, float temperature, float rep_penalty, int top_k, float top_p,
                                               float min_p, float typical_p, float epsilon_cutoff, float eta_cutoff,
                                               const float* uniforms, long long* next, float* filtered, int B, void* stream) {
    MMTG_REQUIRE(logits && generated && gen_len && uniforms && next && B > 0 && V > 0 && ldl >= V, "logits_process_sample_warp: bad args");
    MMTG_REQUIRE(temperature > 0.f && rep_penalty > 0.f && top_k >= 0 && top_p >= 0.f, "logits_process_sample_warp: bad sampling parameters");
    if (int e = warp_args_check("logits_process_sample_warp", min_p, typical_p, epsilon_cutoff, eta_cutoff)) return e;
    MMTG_REQUIRE(V <= 24000, "logits_process_sample_warp: vocabulary of %d exceeds the LDS row image (24000)", V);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_DECODE, s, 40.0 * B * V, 4.0 * B * V);
    const size_t shm = (size_t)((V + 1) / 2) * 4 + (size_t)V * 4;
    static bool attr_done = false;
    if (!attr_done) {
        if (hipFuncSetAttribute((const void*)logits_sample_warp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096) != hipSuccess)
            MMTG_FAIL(MMTG_ERR_HIP, "logits_process_sample_warp: cannot raise dynamic LDS");
        attr_done = true;
    }
    hipLaunchKernelGGL(logits_sample_warp_kernel, dim3(B), dim3(256), shm, s, logits, ldl, V, generated, ldg, gen_len, temperature,
                       rep_penalty, top_k, top_p, min_p, typical_p, epsilon_cutoff, eta_cutoff, uniforms, next, filtered);
    MMTG_LAUNCH_CHECK("logits_process_sample_warp");
    return MMTG_OK;
}

extern "C" int mmtg_logits_process_argmax(const float* logits, long ldl, int V, const long long* generated,
                                          long ldg, const int* gen_len, float temperature, float rep_penalty,
                                          long long* next, int B, void* stream) {
    MMTG_REQUIRE(logits && generated && gen_len && next && B > 0 && V > 0 && ldl >= V, "logits_process_argmax: bad args");
    MMTG_REQUIRE(temperature > 0.f && rep_penalty > 0.f, "logits_process_argmax: temperature / penalty must be > 0");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_DECODE, s, 4.0 * B * V, 4.0 * B * V);
    MMTG_REQUIRE(V <= 30000, "logits_process_argmax: vocabulary of %d exceeds the 60 KB LDS occurrence table", V);
    hipLaunchKernelGGL(logits_argmax_kernel, dim3(B), dim3(256), (size_t)((V + 1) / 2) * 4, s, logits, ldl, V, generated, ldg, gen_len,
                       temperature, rep_penalty, next);
    MMTG_LAUNCH_CHECK("logits_process_argmax");
    return MMTG_OK;
}

extern "C" int mmtg_logits_process_sample(const float* logits, long ldl, int V, const long long* generated, long ldg,
                                          const int* gen_len, float temperature, float rep_penalty, int top_k, float top_p,
                                          const float* uniforms, long long* next, float* filtered, int B, void* stream) {
    MMTG_REQUIRE(logits && generated && gen_len && uniforms && next && B > 0 && V > 0 && ldl >= V, "logits_process_sample: bad args");
    MMTG_REQUIRE(temperature > 0.f && rep_penalty > 0.f && top_k >= 0 && top_p >= 0.f, "logits_process_sample: bad sampling parameters");
    MMTG_REQUIRE(V <= 24000, "logits_process_sample: vocabulary of %d exceeds the LDS row image (24000)", V);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_DECODE, s, 12.0 * B * V, 4.0 * B * V);
    const size_t shm = (size_t)((V + 1) / 2) * 4 + (size_t)V * 4;
    static bool attr_done = false;
    if (!attr_done) {
        if (hipFuncSetAttribute((const void*)logits_sample_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096) != hipSuccess)
            MMTG_FAIL(MMTG_ERR_HIP, "logits_process_sample: cannot raise dynamic LDS");
        attr_done = true;
    }
    hipLaunchKernelGGL(logits_sample_kernel, dim3(B), dim3(256), shm, s, logits, ldl, V, generated, ldg, gen_len, temperature,
                       rep_penalty, top_k, top_p, uniforms, next, filtered);
    MMTG_LAUNCH_CHECK("logits_process_sample");
    return MMTG_OK;
}

// =====================================================================================
// KV-cached single-token decode step (batched, lock-step positions).
//
// The whole step is device-driven: the current position lives in device memory (`pos_ptr`),
// so one captured hipGraph of the step can be replayed for every position without any
// host-side argument changes.  Sequence buffer seq[B, ldseq] holds prompt ids (positions
// 0..P-1) followed by lyric ids (lyric index j = pos - P, j = 0 is the initial [#START#]).
// Type ids / key mask follow the inference branch of GPT2_Decoder.forward (model.py:290-312).
namespace {

template <typename T>
__global__ __launch_bounds__(256) void decode_embed_kernel(const T* __restrict__ table, const long long* __restrict__ seq,
        long ldseq, const T* __restrict__ c, T* __restrict__ x, const int* __restrict__ pos_ptr,
        const long long* __restrict__ tpw_type, const long long* __restrict__ tpw_mask,
        long long* __restrict__ type_out, int* __restrict__ keep, long ldkeep,
        int P, int S, int E, int two_sents, int V, int sent, int max_sent_num, bf16* __restrict__ xp = nullptr, long planeX = 0) {
    typedef typename Vec16<T>::type V16t;
    constexpr int N = Vec16<T>::N;
    const int b = blockIdx.x, pos = *pos_ptr;
    long long tok = seq[(long)b * ldseq + pos];
    if (threadIdx.x == 0) {
        long long ty;
        int kp;
        if (pos < P) {
            ty = tpw_type[(long)b * P + pos];
            kp = tpw_mask[(long)b * P + pos] != 0;
        } else {
            const int i = pos - P;
            const bool pad = tok == 0;
            const bool edge = ((i + 1) % sent == 0) || ((i + 1) % sent == 1);
            const int sidx = i / sent;
            const int slot = sidx < max_sent_num - 1 ? sidx + 1 : 1;     // [1..max_sent_num-1, 1]
            ty = (edge || pad) ? 0 : slot;
            kp = !pad;
        }
        type_out[b] = ty;
        keep[(long)b * ldkeep + pos] = kp;
    }
    if (tok < 0) tok = 0;
    if (tok >= V) tok = V - 1;
    const int seg = pos < P ? -1 : (pos - P) / two_sents;
    const T* src = table + tok * E;
    const T* cs = (seg >= 0 && seg < S) ? c + ((long)b * S + seg) * E : nullptr;
    T* dst = x + (long)b * E;
    for (int e = threadIdx.x * N; e < E; e += 256 * N) {
        V16t v = *reinterpret_cast<const V16t*>(src + e);
        if (cs) {
            V16t w = *reinterpret_cast<const V16t*>(cs + e);
#pragma unroll
            for (int k = 0; k < N; ++k) v[k] = (T)((float)v[k] + (float)w[k]);
        }
        if constexpr (N == 4) {
            if (xp) {        // x3: the conditioned embedding as a (hi | lo) plane pair (the projector product is its only reader)
                bf16x4 hi, lo;
#pragma unroll
                for (int k = 0; k < 4; ++k) { hi[k] = (bf16)(float)v[k]; lo[k] = (bf16)((float)v[k] - (float)hi[k]); }
                *reinterpret_cast<bf16x4*>(xp + (long)b * E + e) = hi;
                *reinterpret_cast<bf16x4*>(xp + planeX + (long)b * E + e) = lo;
                continue;
            }
        }
        *reinterpret_cast<V16t*>(dst + e) = v;
    }
}

// =====================================================================================
// Round 3: the decode step's batch-sized products with the row-wise glue fused in (5 graph nodes per GPT-2 block instead of 7).
//
// Until now every split-K product of the step was followed by a "finish" launch (sum the slabs, bias, residual, and the LayerNorm
// of the NEXT product's input).  A graph node costs ~4 us whatever it does, so the finish kernels were 24 x 5.2 us
// of a 758 us step.  They are gone:
//   * mode 2 ("reduce"): a split-K product whose K slices are reduced IN the kernel -- every split stores its raw fp32 partial
//     wave tile into slot (tile, split) of a workspace with agent-scope stores, bumps the wave tile's arrival counter, and the
//     wave that arrives last adds the partials in split order (its own from registers), adds bias and residual, rounds and stores
//     the bf16 row segment AND the (sum, sum of squares) of what it stored for each of its rows -- the LayerNorm statistics of
//     the new residual stream, as 32-column partials (the mechanism of mmtg_wgrad_group, csrc/wgrad.hip);
//   * modes 0 / 1 ("LN-fold"): the product that consumes a LayerNorm takes the UN-normalised rows and applies the LayerNorm
//     algebraically: LN(x) W = rstd (x W' - mu c) + b' with W' = gamma (.) W (a bf16 copy, mmtg_ln_fold_weights), c_n = sum_k
//     W'_kn, b' = b + beta W; mu / rstd come from the statistics partials.  Decode has no backward: nothing else needs LN(x).
// Tile = 64 x 64 per 256-thread workgroup (2 x 2 waves of 32 x 32), K-contiguous operands, 4-deep LDS-DMA ring, counted vmcnt
// (the main loop of gemm_dma_kernel<false, false, 64, 64, 2, 2, 4>, gemm.hip).
// (DG_NP = 32 statistics partials per row: gemm_common.h)

// Partial tiles cross XCDs: their stores and loads carry the agent-scope bit (sc1: write through / always miss; cache-policy
// operand 16 of the raw buffer builtins) instead of an L2-wide write-back + invalidate per wave (csrc/wgrad.hip).  Compiler-visible
// loads: every other split's pieces are requested back to back and waited for once.
__device__ __forceinline__ void dg_st4_agent(__amdgpu_buffer_rsrc_t r, int byte_off, const f32x4& v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, byte_off, 0, 16);
}
__device__ __forceinline__ f32x4 dg_ld4_agent(__amdgpu_buffer_rsrc_t r, int byte_off) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 16));
}

struct DgArgs {
    const bf16* A; const bf16* W; void* C;
    long lda, ldw, ldc, ldr;
    int M, N, K, kper, splits, ntiles, tiles_n;
    int bytesA, bytesW;
    const float* bias; const float* colsum; const float* stats_in; int np_in; float eps; float inv_k;
    int act, out_f32;
    const bf16* resid; float* stats_out; int np_out;
    float* ws; unsigned* cnt; int ws_bytes;
    // mode 2, residual = wpe[*pos_ptr] + wte[type_ids[m]] instead of a tensor (the GPT-2 input embedding added in the projector's epilogue)
    const bf16* emb_pos; const bf16* emb_type; const long long* type_ids; const int* pos_ptr;
    // x3 (round 5, mmtg_decode_gemm_x3): A and W are (hi | lo) bf16 plane pairs of fp32 tensors, walked as three passes; C / resid /
    // the embedding tables are fp32; Cp (nullable) receives the result as a plane pair for the next product
    int planeA, planeW;        // bytes from the hi plane to the lo plane
    bf16* Cp; long ldcp, planeC;       // planeC: elements
};

// One 64 x 64 output tile (x one K slice) = work item `bid` of a stand-alone launch (one item per workgroup).
// (The persistent one-launch token step and the chained launches of round 4 -- bit-equal, measured slower -- live in
//  tools/experiments/decode_persistent_and_chained.patch.)
// X3 (round 5): the split-precision form -- operands as (hi | lo) plane pairs, the K slice walked three times (A hi x W hi, A lo x W hi,
// A hi x W lo: only the scalar offsets of a tile change), fp32 residual stream / embeddings, results as fp32 and / or plane pairs.
// X3C: the x3 form with ONE K loop over combined stages -- a stage holds the K tile of all four planes (A hi | A lo | W hi | W lo,
// 32 KB) and every fragment pair feeds three MFMAs -- instead of three passes that re-stage A hi and W hi: two thirds of the bytes
// through the CU's L2 -> LDS port, a third of the barriers; NBUF = 2 (64 KB: still two workgroups per CU).
template <int MODE, int NBUF, int MAXS = 8, bool X3 = false, bool X3C = false>
__device__ __forceinline__ void dg_tile(const DgArgs& p, const int bid, char* smem) {
    static_assert(!X3C || X3, "combined stages belong to the x3 form");
    constexpr int TB = 64, NW = 4, BK = 64, NB = 2;
    constexpr int TA = TB * 128, STAGE = (X3C ? 4 : 2) * TA;
    float* const smu = reinterpret_cast<float*>(smem + NBUF * STAGE);
    float* const srs = smu + TB;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, l15 = lane & 15;
    const int wm = wave >> 1, wn = wave & 1;
    // plain item order: consecutive workgroups = consecutive column tiles of one row tile, dealt round-robin to the 8 XCDs.
    // (An XCD-contiguous order with the row tiles of a weight panel side by side on one XCD -- the training kernels' order --
    //  measured 789 vs 728 us per token step here: the step is latency-bound, and spreading a product's first requests over all
    //  eight L2s matters more than fetching a 96 KB panel once.)
    const int split = bid / p.ntiles, t = bid - split * p.ntiles;
    const int m0 = (t / p.tiles_n) * TB, n0 = (t % p.tiles_n) * TB;
    const int kbeg = split * p.kper;
    const int klen = max(0, min(p.K, kbeg + p.kper) - kbeg);
    const int nk1 = (klen + BK - 1) / BK;                  // (x3: the host keeps K slices whole 64-deep tiles)
    const int nk = (X3 && !X3C) ? 3 * nk1 : nk1, nk_full = X3 ? nk : klen / BK;
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(p.A), 0, p.bytesA, 0x00020000);
    const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(p.W), 0, p.bytesW, 0x00020000);
    int sa = (int)(((long)m0 * p.lda + kbeg) * 2), sb = (int)(((long)n0 * p.ldw + kbeg) * 2);
    int va[NB], vb[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        va[i] = dma_voff<false, TB>(p.lda, m0, p.M, BK, wave + NW * i, lane);
        vb[i] = dma_voff<false, TB>(p.ldw, n0, p.N, BK, wave + NW * i, lane);
    }

    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#define DG_ISSUE(tt)                                                                                                   \
    do {                                                                                                               \
        char* st_ = smem + ((tt) % NBUF) * STAGE;                                                                      \
        const bool full_ = (tt) < nk_full, live_ = (tt) < nk;                                                          \
        const int krem_ = klen - (tt) * BK;                                                                            \
        /* x3: pass = tt / nk1 (1 reads A's lo plane, 2 reads W's), K tile tt % nk1 of the slice */                     \
        const int pass_ = (X3 && !X3C) ? ((tt) >= nk1 ? 1 : 0) + ((tt) >= 2 * nk1 ? 1 : 0) : 0;                        \
        const int sa_ = X3 ? sa + ((tt) - pass_ * nk1) * (BK * 2) + (pass_ == 1 ? p.planeA : 0) : sa;                  \
        const int sb_ = X3 ? sb + ((tt) - pass_ * nk1) * (BK * 2) + (pass_ == 2 ? p.planeW : 0) : sb;                  \
        if constexpr (X3C) {        /* all four planes of K tile tt: A hi | A lo | W hi | W lo */                      \
            _Pragma("unroll") for (int i = 0; i < NB; ++i) {                                                           \
                const int oa_ = live_ ? va[i] : OOB, ob_ = live_ ? vb[i] : OOB;                                        \
                __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, LDS_PTR(void, st_ + (wave + NW * i) * 1024), 16, oa_, live_ ? sa_ : 0, 0, 0); \
                __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, LDS_PTR(void, st_ + TA + (wave + NW * i) * 1024), 16, oa_, live_ ? sa_ + p.planeA : 0, 0, 0); \
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, LDS_PTR(void, st_ + 2 * TA + (wave + NW * i) * 1024), 16, ob_, live_ ? sb_ : 0, 0, 0); \
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, LDS_PTR(void, st_ + 3 * TA + (wave + NW * i) * 1024), 16, ob_, live_ ? sb_ + p.planeW : 0, 0, 0); \
            }                                                                                                          \
        } else                                                                                                         \
        _Pragma("unroll") for (int i = 0; i < NB; ++i) {                                                               \
            const int oa_ = !live_ ? OOB : full_ ? va[i] : dma_voff<false, TB>(p.lda, m0, p.M, krem_, wave + NW * i, lane); \
            const int ob_ = !live_ ? OOB : full_ ? vb[i] : dma_voff<false, TB>(p.ldw, n0, p.N, krem_, wave + NW * i, lane); \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, LDS_PTR(void, st_ + (wave + NW * i) * 1024), 16, oa_, live_ ? sa_ : 0, 0, 0); \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, LDS_PTR(void, st_ + TA + (wave + NW * i) * 1024), 16, ob_, live_ ? sb_ : 0, 0, 0); \
        }                                                                                                              \
        if constexpr (!X3) {                                                                                           \
            sa += BK * 2;                                                                                              \
            sb += BK * 2;                                                                                              \
        }                                                                                                              \
    } while (0)
#pragma unroll
    for (int t0 = 0; t0 < NBUF - 1; ++t0) DG_ISSUE(t0);
    const int mw0 = m0 + wm * 32, nw0 = n0 + wn * 32;
    // LN-fold: mu / rstd of the tile's 64 rows from the statistics partials, and this lane's column sums / folded biases, while
    // the first K tiles are in flight (published to the other waves by the K loop's barriers; consumed in the epilogue)
    f32x4 c4[2], b4[2];
    if constexpr (MODE != 2) {
        if (tid < TB) {
            const int m = min(m0 + tid, p.M - 1);
            const f32x4* src = reinterpret_cast<const f32x4*>(p.stats_in + (long)m * DG_NP * 2);
            f32x4 sp[DG_NP / 2];
#pragma unroll
            for (int i = 0; i < DG_NP / 2; ++i) sp[i] = i * 2 < p.np_in ? src[i] : f32x4{0.f, 0.f, 0.f, 0.f};
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int i = 0; i < DG_NP / 2; ++i) { s1 += sp[i][0] + sp[i][2]; s2 += sp[i][1] + sp[i][3]; }
            const float mu = s1 * p.inv_k;
            const float var = fmaxf(s2 * p.inv_k - mu * mu, 0.f);
            smu[tid] = mu;
            srs[tid] = rsqrtf(var + p.eps);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // stored before this wave passes the first K-loop barrier
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = min(nw0 + j * 16 + 4 * g, p.N - 4);
            c4[j] = *reinterpret_cast<const f32x4*>(p.colsum + n);
            b4[j] = MODE == 0 ? *reinterpret_cast<const f32x4*>(p.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    for (int kt = 0; kt < nk; ++kt) {
        wait_vmcnt<(NBUF - 2) * (X3C ? 4 : 2) * NB>();     // my part of tile kt has landed (the younger tiles may be in flight)
        __builtin_amdgcn_s_barrier();              // ... and everyone's; every wave is done reading tile kt - 1
        DG_ISSUE(kt + NBUF - 1);
        const char* tA = smem + (kt % NBUF) * STAGE;
        if constexpr (X3C) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                bf16x8 fah[2], fal[2], fbh[2], fbl[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    fah[i] = ld_frag_kc<bf16>(tA, wm * 32 + i * 16 + l15, kk, g);
                    fal[i] = ld_frag_kc<bf16>(tA + TA, wm * 32 + i * 16 + l15, kk, g);
                    fbh[i] = ld_frag_kc<bf16>(tA + 2 * TA, wn * 32 + i * 16 + l15, kk, g);
                    fbl[i] = ld_frag_kc<bf16>(tA + 3 * TA, wn * 32 + i * 16 + l15, kk, g);
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        mma16(fbh[j], fah[i], acc[i][j]);
                        mma16(fbh[j], fal[i], acc[i][j]);
                        mma16(fbl[j], fah[i], acc[i][j]);
                    }
            }
            continue;
        }
        const char* tB = tA + TA;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                fa[i] = ld_frag_kc<bf16>(tA, wm * 32 + i * 16 + l15, kk, g);
                fb[i] = ld_frag_kc<bf16>(tB, wn * 32 + i * 16 + l15, kk, g);
            }
            // (swapped operands: a lane holds 4 consecutive columns of row l15)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) mma16(fb[j], fa[i], acc[i][j]);
        }
    }
#undef DG_ISSUE
    wait_vmcnt<0>();                               // the zero-fill tail requests
    if constexpr (MODE != 2) {
        // ---- LN-fold epilogue
        if (nk == 0) __syncthreads();              // (no K loop barrier has published smu / srs)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int rl = wm * 32 + i * 16 + l15, m = m0 + rl;
            const float mu = smu[rl], rs = srs[rl];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int n = nw0 + j * 16 + 4 * g;
                if (m >= p.M || n >= p.N) continue;
                f32x4 v;
                if constexpr (MODE == 1) {
                    // slab `split` of the consumer's fp32 input: the mean term rides on slab 0, the bias is the consumer's
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = rs * acc[i][j][r] - (split == 0 ? rs * mu * c4[j][r] : 0.f);
                    *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.C) + ((long)split * p.M + m) * p.ldc + n) = v;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        v[r] = rs * (acc[i][j][r] - mu * c4[j][r]) + b4[j][r];
                        if (p.act == MMTG_EPI_GELU) v[r] = gelu_new_t<bf16>(v[r]);
                    }
                    if (p.out_f32) {
                        *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.C) + (long)m * p.ldc + n) = v;
                    } else if constexpr (X3) {          // the activation as a plane pair: only the next product reads it
                        bf16x4 hi, lo;
#pragma unroll
                        for (int r = 0; r < 4; ++r) { hi[r] = (bf16)v[r]; lo[r] = (bf16)(v[r] - (float)hi[r]); }
                        bf16* dst = p.Cp + (long)m * p.ldcp + n;
                        *reinterpret_cast<bf16x4*>(dst) = hi;
                        *reinterpret_cast<bf16x4*>(dst + p.planeC) = lo;
                    } else {
                        const bf16x4 o = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
                        *reinterpret_cast<bf16x4*>(reinterpret_cast<bf16*>(p.C) + (long)m * p.ldc + n) = o;
                    }
                }
            }
        }

    } else {
        // ---- split-K reduced by the last-arriving wave (csrc/wgrad.hip), + bias + residual + row statistics
        const int S = p.splits;
        const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(p.ws, 0, p.ws_bytes, 0x00020000);
        const int slot0 = (t * S * (TB * TB) + wave * 1024 + lane * 4) * 4;        // byte offset of my lane in slot (t, 0)
        if (S > 1) {
            const int mine = slot0 + split * (TB * TB * 4);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) dg_st4_agent(rw, mine + (i * 2 + j) * 1024, acc[i][j]);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // every write-through store has been acknowledged
            unsigned* const cnt = p.cnt + (long)t * NW + wave;
            unsigned old = 0;
            if (lane == 0) old = atomicAdd(cnt, 1u);
            old = __builtin_amdgcn_readfirstlane(old);
            if (old != (unsigned)(S - 1)) return;
            // (re-armed for the next product: an agent-scope store in the persistent form, where no kernel boundary flushes it)
            if (lane == 0) *cnt = 0u;
        }
        // every split's partial (my own slot included: statically indexed registers, no scratch), all requested back to back:
        // one memory round trip for the whole reduction
        f32x4 prt[MAXS][4];        // (MAXS = most K splits the instantiation serves: 8 stand-alone, 4 in the register-capped persistent kernel)
#pragma unroll
        for (int s_ = 0; s_ < MAXS; ++s_) {
            const int se = s_ < S ? s_ : split;
#pragma unroll
            for (int q = 0; q < 4; ++q) prt[s_][q] = S > 1 ? dg_ld4_agent(rw, slot0 + se * (TB * TB * 4) + q * 1024) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = mw0 + i * 16 + l15;
            float r1 = 0.f, r2 = 0.f;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int n = nw0 + j * 16 + 4 * g;
                f32x4 sum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s_ = 0; s_ < MAXS; ++s_) {               // split order; mine from registers
                    const f32x4 v = s_ == split ? acc[i][j] : prt[s_][i * 2 + j];
                    if (s_ < S) sum += v;
                }
                if constexpr (X3) {
                    if (m < p.M && n < p.N) {
                        const f32x4 b4 = *reinterpret_cast<const f32x4*>(p.bias + n);
                        f32x4 xr = {0.f, 0.f, 0.f, 0.f};
                        if (p.type_ids) {
                            const f32x4 e0 = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p.emb_pos) + (long)*p.pos_ptr * p.ldr + n);
                            const f32x4 e1 = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p.emb_type) + p.type_ids[m] * p.ldr + n);
                            xr = e0 + e1;
                        } else if (p.resid) xr = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p.resid) + (long)m * p.ldr + n);
                        f32x4 f;
                        bf16x4 hi, lo;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            f[r] = sum[r] + b4[r];
                            if (p.act == MMTG_EPI_TANH) f[r] = tanh_t<bf16>(f[r]);
                            f[r] += xr[r];
                            r1 += f[r];
                            r2 += f[r] * f[r];
                            hi[r] = (bf16)f[r];
                            lo[r] = (bf16)(f[r] - (float)hi[r]);
                        }
                        if (p.C) *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.C) + (long)m * p.ldc + n) = f;
                        if (p.Cp) {
                            bf16* dst = p.Cp + (long)m * p.ldcp + n;
                            *reinterpret_cast<bf16x4*>(dst) = hi;
                            *reinterpret_cast<bf16x4*>(dst + p.planeC) = lo;
                        }
                    }
                    continue;
                }
                if (m < p.M && n < p.N) {
                    const f32x4 b4 = *reinterpret_cast<const f32x4*>(p.bias + n);
                    float xr[4];
                    if (p.type_ids) {
                        const bf16x4 e0 = *reinterpret_cast<const bf16x4*>(p.emb_pos + (long)*p.pos_ptr * p.ldr + n);
                        const bf16x4 e1 = *reinterpret_cast<const bf16x4*>(p.emb_type + p.type_ids[m] * p.ldr + n);
#pragma unroll
                        for (int r = 0; r < 4; ++r) xr[r] = (float)e0[r] + (float)e1[r];
                    } else {
                        bf16x4 x4;
                        x4 = *reinterpret_cast<const bf16x4*>(p.resid + (long)m * p.ldr + n);
#pragma unroll
                        for (int r = 0; r < 4; ++r) xr[r] = (float)x4[r];
                    }
                    bf16x4 o;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        o[r] = (bf16)(sum[r] + b4[r] + xr[r]);
                        const float f = (float)o[r];
                        r1 += f;
                        r2 += f * f;
                    }
                    *reinterpret_cast<bf16x4*>(reinterpret_cast<bf16*>(p.C) + (long)m * p.ldc + n) = o;
                }
            }
            // the row's 32 columns of this wave tile live in the four lane groups g: fold them
            r1 += __shfl_xor(r1, 16, 64); r2 += __shfl_xor(r2, 16, 64);
            r1 += __shfl_xor(r1, 32, 64); r2 += __shfl_xor(r2, 32, 64);
            if (g == 0 && m < p.M && nw0 < p.N && (!X3 || p.stats_out)) {
                float* dst = p.stats_out + ((long)m * DG_NP + (nw0 >> 5)) * 2;
                dst[0] = r1;
                dst[1] = r2;
            }
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(256, 2) void decode_gemm_kernel(DgArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];      // 4 stages | row statistics
    dg_tile<MODE, 4>(p, blockIdx.x, smem);
}
template <int MODE, bool COMB = false>
__global__ __launch_bounds__(256, 2) void decode_gemm_x3_kernel(DgArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];      // 4 stages of 16 KB (three passes) / 2 of 32 KB (combined) | row statistics
    dg_tile<MODE, (COMB ? 2 : 4), 8, true, COMB>(p, blockIdx.x, smem);
}

// x3 weight preparation, one wave per output row n of a K-contiguous weight given as a plane pair W = hi + lo ([N, K]):
//   W'[n, k] = gamma[k] W[n, k] re-split into a plane pair, c[n] = sum_k (W'_hi + W'_lo)[n, k] (of what the product multiplies),
//   bf[n] = bias[n] + sum_k beta[k] W[n, k]
__global__ __launch_bounds__(256) void ln_fold_x3_kernel(const bf16* __restrict__ W, long ldw, long planeW, const float* __restrict__ gamma,
        const float* __restrict__ beta, const float* __restrict__ bias, bf16* __restrict__ Wf, long ldf, long planeF, float* __restrict__ c,
        float* __restrict__ bf, int N, int K) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (n >= N) return;
    float sc = 0.f, sb = 0.f;
    for (int k = lane * 8; k < K; k += 512) {
        const bf16x8 wh = *reinterpret_cast<const bf16x8*>(W + (long)n * ldw + k);
        const bf16x8 wl = *reinterpret_cast<const bf16x8*>(W + planeW + (long)n * ldw + k);
        bf16x8 oh, ol;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float w = (float)wh[e] + (float)wl[e];
            const float f = gamma[k + e] * w;
            oh[e] = (bf16)f;
            ol[e] = (bf16)(f - (float)oh[e]);
            sc += (float)oh[e] + (float)ol[e];
            sb += beta[k + e] * w;
        }
        *reinterpret_cast<bf16x8*>(Wf + (long)n * ldf + k) = oh;
        *reinterpret_cast<bf16x8*>(Wf + planeF + (long)n * ldf + k) = ol;
    }
    sc = wave_sum(sc);
    sb = wave_sum(sb);
    if (lane == 0) { c[n] = sc; bf[n] = (bias ? bias[n] : 0.f) + sb; }
}

// W'[n, k] = gamma[k] W[n, k] (bf16), c[n] = sum_k W'[n, k] (of the ROUNDED values: what the product will multiply),
// bf[n] = bias[n] + sum_k beta[k] W[n, k]: one wave per output row
__global__ __launch_bounds__(256) void ln_fold_kernel(const bf16* __restrict__ W, long ldw, const float* __restrict__ gamma,
        const float* __restrict__ beta, const float* __restrict__ bias, bf16* __restrict__ Wf, float* __restrict__ c,
        float* __restrict__ bf, int N, int K) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (n >= N) return;
    float sc = 0.f, sb = 0.f;
    for (int k = lane * 8; k < K; k += 512) {
        const bf16x8 w = *reinterpret_cast<const bf16x8*>(W + (long)n * ldw + k);
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            o[e] = (bf16)(gamma[k + e] * (float)w[e]);
            sc += (float)o[e];
            sb += beta[k + e] * (float)w[e];
        }
        *reinterpret_cast<bf16x8*>(Wf + (long)n * ldw + k) = o;
    }
    sc = wave_sum(sc);
    sb = wave_sum(sb);
    if (lane == 0) { c[n] = sc; bf[n] = (bias ? bias[n] : 0.f) + sb; }
}

template <typename T>
__global__ __launch_bounds__(256) void decode_embed_add_kernel(const T* __restrict__ g, const T* __restrict__ wpe,
        const T* __restrict__ wte, const long long* __restrict__ type_ids, const int* __restrict__ pos_ptr,
        T* __restrict__ h, int D, float* __restrict__ stats) {
    __shared__ float red[8];
    const int b = blockIdx.x, pos = *pos_ptr;
    const long long ty = type_ids[b];
    float s1 = 0.f, s2 = 0.f;
    for (int d = threadIdx.x; d < D; d += 256) {
        const T o = (T)((float)g[(long)b * D + d] + (float)wpe[(long)pos * D + d] + (float)wte[ty * D + d]);
        h[(long)b * D + d] = o;
        s1 += (float)o;
        s2 += (float)o * (float)o;
    }
    if (stats) {        // LayerNorm statistics of the row as stored (fused decode path): partial 0 carries all of it
        s1 = wave_sum(s1);
        s2 = wave_sum(s2);
        if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = s1; red[4 + (threadIdx.x >> 6)] = s2; }
        __syncthreads();
        float* dst = stats + (long)b * DG_NP * 2;
        if (threadIdx.x == 0) { dst[0] = red[0] + red[1] + red[2] + red[3]; dst[1] = red[4] + red[5] + red[6] + red[7]; }
        else if (threadIdx.x < DG_NP * 2 && threadIdx.x >= 2) dst[threadIdx.x] = 0.f;
    }
}

// One wave per (b, head): append this token's K/V to the cache, then attend over keys 0..pos.
// Cache layout [B, nH, Tmax, 64].  Both passes over the cache use 16-byte vectors: a key's 64 channels are spread over
// OCT = 8 (bf16) / 16 (f32) adjacent lanes, so one wave-instruction reads 64 / OCT whole cache rows -- 1 KB, fully
// coalesced.  Scores: partial dot products folded across the OCT lanes; values: each lane accumulates its channel octet
// over its keys, the key groups are folded at the end.  Fixed summation order (ascending key per lane).
// Round 3: the K AND V rows of the first UN0 * KPI keys are requested at the very top, before the token's own q / k / v are
// even assembled from the c_attn slabs -- they depend on nothing this kernel computes -- so a step with a short prefix costs one
// memory round trip instead of three dependent ones (slabs -> scores -> values).  Branch-free: rows at or past `pos` are
// requested from the last valid row and replaced afterwards (key == pos: the token's own row, held in LDS exactly as stored).
// The KV cache rows are read once per token step and never again by this step: with `nt` (non-temporal) they need not displace the
// step's 193 MB of weights from the 256 MB Infinity Cache, which every step re-reads (A/B: MMTG_DECODE_KV_NT, profiles/r04_*).
// cross-lane folds of the score loop by DPP (full-rate VALU, no LDS crossbar: the __shfl_xor forms are a ds_bpermute + address
// arithmetic per step and sat on the per-chunk dependent chain).  fold_sum_lanes<OCT>: the sum over the OCT adjacent lanes of a key
// (quad swaps, then the mirror inside 8 / 16 lanes: every lane ends with the group's sum).  wave_max_of_groups<OCT>: the maximum
// over the whole wave of a value that is already uniform inside each group of OCT lanes; returned wave-uniform (readlane 63).
template <int CTRL, int ROWS = 0xF> __device__ __forceinline__ float dpp_keep(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, x), __builtin_bit_cast(int, x), CTRL, ROWS, 0xF, false));
}
template <int OCT> __device__ __forceinline__ float fold_sum_lanes(float a) {
    a += dpp_keep<0xB1>(a);                    // quad_perm [1,0,3,2]
    a += dpp_keep<0x4E>(a);                    // quad_perm [2,3,0,1]
    a += dpp_keep<0x141>(a);                   // row_half_mirror
    if constexpr (OCT == 16) a += dpp_keep<0x140>(a);      // row_mirror
    return a;
}
template <int OCT> __device__ __forceinline__ float wave_max_of_groups(float x) {
    if constexpr (OCT == 8) x = fmaxf(x, dpp_keep<0x140>(x));          // the row's two groups
    x = fmaxf(x, dpp_keep<0x142, 0xA>(x));     // row_bcast15 into rows 1, 3
    x = fmaxf(x, dpp_keep<0x143, 0xC>(x));     // row_bcast31 into rows 2, 3
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 63));
}

template <typename V, bool NT> __device__ __forceinline__ V ld_kv(const V* p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}

// bytes of LDS one (b, head) item needs: scores, key flags, q (f32), this token's k and v
template <typename T> constexpr int da_lds_bytes() { return 1024 * 4 + 1024 * 4 + 64 * 4 + 2 * 64 * (int)sizeof(T); }

// one 64-thread workgroup per (b, head)
// ROWS (beam search): the K / V rows of key j < pos are read from cache row rows[b * ldrows + j] (the ancestry table: which row of
// the batch wrote position j of this beam's history) instead of row b; the token's own K / V still go to row b, slot pos.  The
// table of the prefix is read into LDS (the first 4 KB, unused otherwise) in the pass that reads the key flags; the first two
// chunks' row indices are requested before their K / V (one dependent round trip more than the plain form).
template <typename T, bool NT = false, bool ROWS = false>
__device__ __forceinline__ void da_body(const T* __restrict__ qkv, T* __restrict__ kc, T* __restrict__ vc,
        const int* __restrict__ keep, long ldkeep, const int pos, T* __restrict__ out, const int B,
        int nH, int Tmax, const float* __restrict__ part, int splits, long slab, const float* __restrict__ bias,
        const int h, const int b, const int lane, char* lds, bf16* __restrict__ oplanes = nullptr, long oplane = 0,
        const int* __restrict__ rows = nullptr, long ldrows = 0) {
    typedef typename Vec16<T>::type V;
    constexpr int EPL = Vec16<T>::N, OCT = 64 / EPL, KPI = 64 / OCT;      // elements per lane, lanes per key, keys per instruction
    // (the SAME chunking in both forms: the first chunk's scores and the later chunks' come out of differently contracted
    //  loops, so moving the chunk boundary moves last bits -- the persistent step stays bit-equal to the per-launch one)
    constexpr int UN = 4, CH = UN * KPI;         // a chunk: UN keys per lane group = 32 keys (bf16) / 16 (f32)
    int* const srows = reinterpret_cast<int*>(lds);
    int* const skeep = reinterpret_cast<int*>(lds + 4096);
    float* const sq = reinterpret_cast<float*>(lds + 8192);
    T* const sk = reinterpret_cast<T*>(lds + 8192 + 256);
    T* const sv = sk + 64;
#define DA_SYNC() __syncthreads()
    const int D = nH * 64;
    const T* row = qkv + (long)b * 3 * D + h * 64;
    T* kbase = kc + (((long)b * nH + h) * Tmax) * 64;
    T* vbase = vc + (((long)b * nH + h) * Tmax) * 64;
    const int nkeys = pos + 1;
    const int oc = lane % OCT, kg = lane / OCT;
    const int last = pos > 0 ? pos - 1 : 0;
    // chunks 0 and 1 (K and V rows) are requested at the very top: they depend on nothing this kernel computes.  Branch-free:
    // rows at or past `pos` are requested from the last valid row and replaced (key == pos: the token's own row, from LDS) or masked
    V kA[UN], vA[UN], kB[UN], vB[UN];
    // ROWS: element offset of (cache row r, head h, key kr); r is clamped into the batch (a table is only ever read, never trusted)
    const int* const rrow = ROWS ? rows + (long)b * ldrows : nullptr;
    auto kv_off = [&](int r, int kr) -> long { return ((((long)min(max(r, 0), B - 1) * nH + h) * Tmax) + kr) * 64 + oc * EPL; };
    int rA[UN], rB[UN];
    if constexpr (ROWS) {
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int kA_ = u * KPI + kg, kB_ = CH + u * KPI + kg;
            rA[u] = rrow[kA_ < pos ? kA_ : last];
            rB[u] = rrow[kB_ < pos ? kB_ : last];
        }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
        const int key = u * KPI + kg, kr = key < pos ? key : last;
        if constexpr (ROWS) {
            kA[u] = ld_kv<V, NT>(reinterpret_cast<const V*>(kc + kv_off(rA[u], kr)));
            vA[u] = ld_kv<V, NT>(reinterpret_cast<const V*>(vc + kv_off(rA[u], kr)));
        } else {
            kA[u] = ld_kv<V, NT>(reinterpret_cast<const V*>(kbase + (long)kr * 64 + oc * EPL));
            vA[u] = ld_kv<V, NT>(reinterpret_cast<const V*>(vbase + (long)kr * 64 + oc * EPL));
        }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
        const int key = CH + u * KPI + kg, kr = key < pos ? key : last;
        if constexpr (ROWS) {
            kB[u] = ld_kv<V, NT>(reinterpret_cast<const V*>(kc + kv_off(rB[u], kr)));
            vB[u] = ld_kv<V, NT>(reinterpret_cast<const V*>(vc + kv_off(rB[u], kr)));
        } else {
            kB[u] = ld_kv<V, NT>(reinterpret_cast<const V*>(kbase + (long)kr * 64 + oc * EPL));
            vB[u] = ld_kv<V, NT>(reinterpret_cast<const V*>(vbase + (long)kr * 64 + oc * EPL));
        }
    }
    // the key-padding flags of the whole prefix in one coalesced pass, into LDS (round 3: the score loop used to read keep[]
    // from global memory key group by key group -- up to 16 DEPENDENT 4-byte loads, each a full memory round trip)
    // (the first 256 flags as four independent loads, stored after the slab sums; longer prefixes: a plain loop)
    int kp[4], rp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) kp[i] = keep[(long)b * ldkeep + min(lane + 64 * i, pos)];
    if constexpr (ROWS) {
#pragma unroll
        for (int i = 0; i < 4; ++i) rp[i] = rrow[min(lane + 64 * i, pos)];
    }
    asm volatile("" ::: "memory");      // compiler barrier: the requests above are ISSUED here (nothing waits for them yet)
    if (part) {
        // the c_attn product arrives as split-K slabs (MMTG_EPI_SPLIT): sum them in order, add the bias
        // and round to the storage type exactly as mmtg_splitk_finish would (saves that launch); up to four slabs are
        // requested together (one round trip), more in a plain loop
        const float* pr = part + (long)b * 3 * D + h * 64 + lane;
        float q = 0.f, k = 0.f, v = 0.f;
        const float bq = bias[h * 64 + lane], bk = bias[D + h * 64 + lane], bv = bias[2 * D + h * 64 + lane];
        float pq[4], pk[4], pv[4];
#pragma unroll
        for (int s_ = 0; s_ < 4; ++s_) {
            const long o = (long)(s_ < splits ? s_ : 0) * slab;
            pq[s_] = pr[o]; pk[s_] = pr[o + D]; pv[s_] = pr[o + 2 * D];
        }
#pragma unroll
        for (int s_ = 0; s_ < 4; ++s_)
            if (s_ < splits) { q += pq[s_]; k += pk[s_]; v += pv[s_]; }
        for (int s_ = 4; s_ < splits; ++s_) { q += pr[s_ * slab]; k += pr[s_ * slab + D]; v += pr[s_ * slab + 2 * D]; }
        q += bq; k += bk; v += bv;
        sq[lane] = (float)(T)q * 0.125f;
        sk[lane] = (T)k;
        sv[lane] = (T)v;
    } else {
        sq[lane] = (float)row[lane] * 0.125f;
        sk[lane] = row[D + lane];
        sv[lane] = row[2 * D + lane];
    }
    kbase[(long)pos * 64 + lane] = sk[lane];
    vbase[(long)pos * 64 + lane] = sv[lane];
#pragma unroll
    for (int i = 0; i < 4; ++i) skeep[lane + 64 * i] = kp[i];
    for (int key = lane + 256; key < nkeys; key += 64) skeep[key] = keep[(long)b * ldkeep + key];
    if constexpr (ROWS) {
#pragma unroll
        for (int i = 0; i < 4; ++i) srows[lane + 64 * i] = rp[i];
        for (int key = lane + 256; key < nkeys; key += 64) srows[key] = rrow[key];
    }
    DA_SYNC();
    float qv[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) qv[e] = sq[oc * EPL + e];
    const V knew = *reinterpret_cast<const V*>(sk + oc * EPL), vnew = *reinterpret_cast<const V*>(sv + oc * EPL);
    // ---- ONE pass over the cache (round 4): scores, running maximum / sum and the value accumulation per chunk of CH keys, all in
    // registers -- a lane group's eight (bf16) lanes all hold the score of the group's key after the fold, and the same lanes own the
    // channel octets of that key's value row, so no score ever goes through LDS.  Two chunks are always in flight (buffer c & 1 is
    // refilled with chunk c + 2 as soon as chunk c is consumed): the two-pass form walked the cache as K chunks, then softmax, then V
    // chunks -- up to five DEPENDENT memory round trips per layer at a full prefix against two here.
    float m_run = -INFINITY, sum = 0.f;
    float acc[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[e] = 0.f;
#define DA_STEP(KB_, VB_, K0_)                                                                                       \
    do {                                                                                                             \
        float a_[UN];                                                                                                \
        float cm_ = -INFINITY;                                                                                       \
        _Pragma("unroll") for (int u = 0; u < UN; ++u) {                                                             \
            const int key = (K0_) + u * KPI + kg;                                                                    \
            const bool isnew = key == pos;                                                                           \
            float a = 0.f;                                                                                           \
            _Pragma("unroll") for (int e = 0; e < EPL; ++e) {                                                        \
                a += qv[e] * (float)(isnew ? knew[e] : KB_[u][e]);                                                   \
                VB_[u][e] = isnew ? vnew[e] : VB_[u][e];                                                             \
            }                                                                                                        \
            a = fold_sum_lanes<OCT>(a);                                                                              \
            a_[u] = (key < nkeys && skeep[key < nkeys ? key : pos]) ? a : -INFINITY;                                 \
            cm_ = fmaxf(cm_, a_[u]);                                                                                 \
        }                                                                                                            \
        cm_ = wave_max_of_groups<OCT>(cm_);                                                                          \
        const float m_new = fmaxf(m_run, cm_);                                                                       \
        const float muse = m_new == -INFINITY ? 0.f : m_new;                                                         \
        const float alpha = expf(m_run - muse);                                                                      \
        sum *= alpha;                                                                                                \
        _Pragma("unroll") for (int e = 0; e < EPL; ++e) acc[e] *= alpha;                                             \
        _Pragma("unroll") for (int u = 0; u < UN; ++u) {                                                             \
            const float p = a_[u] == -INFINITY ? 0.f : expf(a_[u] - muse);                                           \
            sum += p;                                                                                                \
            _Pragma("unroll") for (int e = 0; e < EPL; ++e) acc[e] += p * (float)VB_[u][e];                          \
        }                                                                                                            \
        m_run = m_new;                                                                                               \
    } while (0)
#define DA_ISSUE(KB_, VB_, K0_)                                                                                      \
    do {                                                                                                             \
        _Pragma("unroll") for (int u = 0; u < UN; ++u) {                                                             \
            const int key = (K0_) + u * KPI + kg, kr = key < pos ? key : last;                                       \
            if constexpr (ROWS) {                                                                                    \
                const long o_ = kv_off(srows[kr], kr);                                                               \
                KB_[u] = ld_kv<V, NT>(reinterpret_cast<const V*>(kc + o_));                                          \
                VB_[u] = ld_kv<V, NT>(reinterpret_cast<const V*>(vc + o_));                                          \
            } else {                                                                                                 \
                KB_[u] = ld_kv<V, NT>(reinterpret_cast<const V*>(kbase + (long)kr * 64 + oc * EPL));                 \
                VB_[u] = ld_kv<V, NT>(reinterpret_cast<const V*>(vbase + (long)kr * 64 + oc * EPL));                 \
            }                                                                                                        \
        }                                                                                                            \
    } while (0)
#pragma unroll 1
    for (int k0 = 0; k0 < nkeys; k0 += 2 * CH) {
        DA_STEP(kA, vA, k0);
        if (k0 + 2 * CH < nkeys) DA_ISSUE(kA, vA, k0 + 2 * CH);
        if (k0 + CH < nkeys) {
            DA_STEP(kB, vB, k0 + CH);
            if (k0 + 3 * CH < nkeys) DA_ISSUE(kB, vB, k0 + 3 * CH);
        }
    }
#undef DA_STEP
#undef DA_ISSUE
    // fold over the key groups: every lane group holds the partial sums of ITS keys (the same value in its OCT lanes)
#pragma unroll
    for (int o = OCT; o < 64; o <<= 1) sum += __shfl_xor(sum, o, 64);
#pragma unroll
    for (int e = 0; e < EPL; ++e)
#pragma unroll
        for (int o = OCT; o < 64; o <<= 1) acc[e] += __shfl_xor(acc[e], o, 64);
    if (kg == 0) {
        const float inv = sum > 0.f ? 1.f / sum : 0.f;
        V o;
#pragma unroll
        for (int e = 0; e < EPL; ++e) o[e] = (T)(acc[e] * inv);
        if constexpr (EPL == 4) {
            if (oplanes) {        // x3: the context row as a (hi | lo) plane pair (attn.c_proj is its only reader)
                bf16x4 hi, lo;
#pragma unroll
                for (int e = 0; e < 4; ++e) { hi[e] = (bf16)(float)o[e]; lo[e] = (bf16)((float)o[e] - (float)hi[e]); }
                bf16* dst = oplanes + (long)b * D + h * 64 + oc * 4;
                *reinterpret_cast<bf16x4*>(dst) = hi;
                *reinterpret_cast<bf16x4*>(dst + oplane) = lo;
                return;
            }
        }
        *reinterpret_cast<V*>(out + (long)b * D + h * 64 + oc * EPL) = o;
    }
#undef DA_SYNC
}

template <typename T, bool NT = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3))) void decode_attn_kernel(const T* __restrict__ qkv, T* __restrict__ kc, T* __restrict__ vc,
        const int* __restrict__ keep, long ldkeep, const int* __restrict__ pos_ptr, T* __restrict__ out,
        int nH, int Tmax, const float* __restrict__ part, int splits, long slab, const float* __restrict__ bias,
        bf16* __restrict__ oplanes = nullptr, long oplane = 0) {
    __shared__ __attribute__((aligned(16))) char lds[da_lds_bytes<T>()];
    da_body<T, NT>(qkv, kc, vc, keep, ldkeep, *pos_ptr, out, (int)gridDim.y, nH, Tmax, part, splits, slab, bias,
                      (int)blockIdx.x, (int)blockIdx.y, (int)threadIdx.x, lds, oplanes, oplane);
}

// the same with the ancestry table of beam search (da_body ROWS): a kernel of its own, so the plain forms' code is unchanged
template <typename T, bool NT = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3))) void decode_attn_rows_kernel(T* __restrict__ kc, T* __restrict__ vc,
        const int* __restrict__ keep, long ldkeep, const int* __restrict__ rows, long ldrows, const int* __restrict__ pos_ptr,
        T* __restrict__ out, int nH, int Tmax, const float* __restrict__ part, int splits, long slab, const float* __restrict__ bias,
        bf16* __restrict__ oplanes, long oplane) {
    __shared__ __attribute__((aligned(16))) char lds[da_lds_bytes<T>()];
    da_body<T, NT, true>(nullptr, kc, vc, keep, ldkeep, *pos_ptr, out, (int)gridDim.y, nH, Tmax, part, splits, slab, bias,
                         (int)blockIdx.x, (int)blockIdx.y, (int)threadIdx.x, lds, oplanes, oplane, rows, ldrows);
}

// The selection kernels below end in one argument, the step's rule R: NoRule (the plain entries), FixedEnd (*_fixed), NgramBan
// (*_ngram), LineRule (*_lines), TemplateRule (*_tmpl), RhymeRule (*_rhyme) or RefrainRule (*_refrain).  A rule says which rows it holds (held) and, with R::ngram (the sentinel of penalize<true> is
// in use; bans() gives the NgramBan) and R::lines (PAD's slot is read; col() says what the line wants of a free column), which
// edits of the occurrence table the kernel makes after count_ids.
//
// Prefixed generation: row b with pos + 1 < fixed_end[b] sits on a column the host has written (a prefix token).  The rule holds
// the row: it leaves seq[b, pos + 1] alone and offers no beam candidates; the position is still published.

// what a line rule says of row b's free column j (uniform over the workgroup: every thread computes the same)
struct LineCol {
    bool force_pad;          // c >= hi: the row writes PAD, no logits consulted
    bool pad_ban;            // c < lo, or an end set whose members do not include the previous token
    const unsigned* mask;    // c == hi - 1 of a line with an end set: the set's bit row (else null)
};

struct NoRule {
    static constexpr bool ngram = false, lines = false, tmpl = false, rhyme = false, refrain = false;
    __device__ __forceinline__ bool held(int, int) const { return false; }
};

struct FixedEnd {
    const int* fixed_end;   // int32 [B]
    static constexpr bool ngram = false, lines = false, tmpl = false, rhyme = false, refrain = false;
    __device__ __forceinline__ bool held(int b, int pos) const { return pos + 1 < fixed_end[b]; }
};

// n-gram blocking (the *_ngram entries, include/mmtg_hip.h).  Its fixed_end is optional (null: no prefix).  After count_ids,
// ban_ngrams marks every id that would complete a content n-gram the row already holds with the sentinel count 0xFFFF (a banned id
// has occurred, so its slot is non-zero; no real count reaches 0xFFFF since MAXGEN < 65535), and the processing reads the sentinel
// as -inf (penalize<true>) with no extra LDS read per logit.
struct NgramBan {
    const int* fixed_end;   // int32 [B] or null
    int n;                  // 1 .. sent - 2
    int hist_cap;           // ints of dynamic LDS for the staged history (>= the longest history, min(ldseq - P, MAXGEN))
    static constexpr bool ngram = true, lines = false, tmpl = false, rhyme = false, refrain = false;
    __device__ __forceinline__ bool held(int b, int pos) const { return fixed_end && pos + 1 < fixed_end[b]; }
    __host__ __device__ __forceinline__ const NgramBan& bans() const { return *this; }
};

// PAD, [#START#], [#EOS#], [UNK], [SEP] are not content: they break n-grams
__device__ __forceinline__ bool ngram_content(int v) { return v != 0 && v != 1 && v != 2 && v != 100 && v != 102; }

// The ban rule for history g = gen[0..n) (the row's lyric columns before the one it fills) and n-gram size ng: with key
// g[n-ng+1 .. n-1] (empty for ng = 1), if n >= ng - 1 and the key is all content, every v = g[i+ng-1] (0 <= i <= n-ng) with
// g[i .. i+ng-1] all content and g[i .. i+ng-2] equal to the key is banned.  h: n ints of LDS; all threads of the block call.
__device__ __forceinline__ void ban_ngrams(unsigned* cnt, int* h, int V, const long long* gen, int n, int ng, int tid) {
    for (int i = tid; i < n; i += 256) h[i] = (int)gen[i];
    __syncthreads();
    const int k0 = n - ng + 1;                             // first key column
    bool key_ok = k0 >= 0;
    for (int k = k0; key_ok && k < n; ++k) key_ok = ngram_content(h[k]);
    if (key_ok) {
        for (int i = tid; i <= n - ng; i += 256) {        // window g[i .. i+ng-1]: a key match makes its columns content
            const int v = h[i + ng - 1];
            bool hit = ngram_content(v) && v > 0 && v < V;
            for (int k = 0; hit && k < ng - 1; ++k) hit = h[i + k] == h[k0 + k];
            if (hit) atomicOr(cnt + (v >> 1), 0xFFFFu << (16 * (v & 1)));
        }
    }
    __syncthreads();
}

// Line-length bounds and line-end sets (the *_lines entries, include/mmtg_hip.h): an NgramBan whose n may be 0 (no n-gram bans;
// the line bans use its sentinel) plus the per-row, per-line tables.  Lyric index j sits on line l = j / sent at content column
// c = j % sent - 1; a line past n_lines is unconstrained (lo 0, hi sent - 2, no set).
struct LineRule {
    NgramBan ng;                   // fixed_end optional; n = 0: no n-gram bans (hist_cap 0)
    const unsigned char* lo;       // [B, n_lines]
    const unsigned char* hi;       // [B, n_lines], lo <= hi <= sent - 2
    const short* set_of;           // [B, n_lines] row of `sets` (-1: no end set), or null
    const unsigned* sets;          // [n_sets, words] bit v of a row: content id v is in the set
    int n_lines, n_sets, words;    // words >= ceil(V / 32)
    static constexpr bool ngram = true, lines = true, tmpl = false, rhyme = false, refrain = false;
    __device__ __forceinline__ bool held(int b, int pos) const { return ng.held(b, pos); }
    __host__ __device__ __forceinline__ const NgramBan& bans() const { return ng; }

    __device__ __forceinline__ LineCol col(int b, int j, int sent, const long long* gen) const {
        LineCol lc = {false, false, nullptr};
        const int l = j / sent, c = j % sent - 1;
        if (l >= n_lines) return lc;
        const long at = (long)b * n_lines + l;
        const int lo_ = lo[at], hi_ = hi[at];
        const int s = set_of ? (int)set_of[at] : -1;
        lc.force_pad = c >= hi_;
        lc.pad_ban = c < lo_;
        if (s >= 0 && s < n_sets && !lc.force_pad) {
            const unsigned* m = sets + (long)s * words;
            const long long prev = gen[j - 1];
            const bool in = prev >= 0 && prev < 32LL * words && ((m[prev >> 5] >> (prev & 31)) & 1u);
            lc.pad_ban = lc.pad_ban || !in;
            if (c == hi_ - 1) lc.mask = m;
        }
        return lc;
    }
};

// The line bans as edits of the occurrence table, after count_ids / ban_ngrams (all threads of the block call): at the end-set
// column every id outside the set gets the sentinel 0xFFFF (the specials among them are -inf anyway); PAD's slot, which the plain
// forms never read, is set to 0 (no penalty, as ever) or to the sentinel (PAD banned).  The logit loops of the LN forms read PAD's
// slot like any other, so the rule costs them nothing per logit.  (Thread 0 owns word 0 in both loops: no barrier between them.)
__device__ __forceinline__ void ban_line(unsigned* cnt, int V, const LineCol& lc, int tid) {
    if (lc.mask)
        for (int i = tid; i < (V + 1) / 2; i += 256) {          // word i: ids 2 i and 2 i + 1 = bits 2 (i & 15), + 1 of mask word i / 16
            const unsigned two = (lc.mask[i >> 4] >> (2 * (i & 15))) & 3u;
            cnt[i] |= ((two & 1u) ? 0u : 0xFFFFu) | ((two & 2u) ? 0u : 0xFFFF0000u);
        }
    if (tid == 0) cnt[0] = (cnt[0] & 0xFFFF0000u) | (lc.pad_ban ? 0xFFFFu : 0u);
    __syncthreads();
}

// Line templates (the *_tmpl entries, include/mmtg_hip.h): a LineRule plus one symbol per row, line and content column.  tmpl is
// int32 [B, n_lines, sent - 2]: v >= 0 a given id (the row writes it, no logits consulted), -1 free, v <= -2 the class -2 - v, a row
// of the line rule's own `sets` (every id outside it gets the sentinel).  Closed / open templates need no field: the host folds
// them into lo / hi, so a column with a symbol always has c < lo <= hi (never a full line's PAD).
struct TmplCol {
    int given;               // >= 0: the row writes this id (else -1)
    const unsigned* cls;     // a class column: the class's bit row (else null)
};

struct TemplateRule {
    LineRule ln;
    const int* table;              // [B, n_lines, sent - 2]
    static constexpr bool ngram = true, lines = true, tmpl = true, rhyme = false, refrain = false;
    __device__ __forceinline__ bool held(int b, int pos) const { return ln.held(b, pos); }
    __host__ __device__ __forceinline__ const NgramBan& bans() const { return ln.ng; }
    __device__ __forceinline__ LineCol col(int b, int j, int sent, const long long* gen) const { return ln.col(b, j, sent, gen); }

    __device__ __forceinline__ TmplCol sym(int b, int j, int sent) const {
        TmplCol tc = {-1, nullptr};
        const int l = j / sent, c = j % sent - 1;
        if (l >= ln.n_lines || c < 0 || c >= sent - 2) return tc;
        const int v = table[((long)b * ln.n_lines + l) * (sent - 2) + c];
        if (v >= 0) tc.given = v;
        else if (v <= -2 && -2 - v < ln.n_sets) tc.cls = ln.sets + (long)(-2 - v) * ln.words;
        return tc;
    }
};

// ban_line with a class column's mask beside the end set's (either may be null; both: an id survives only if both admit it).  The
// masks are read from global memory in the one pass over the count words; nothing is staged.
__device__ __forceinline__ void ban_line_tmpl(unsigned* cnt, int V, const LineCol& lc, const unsigned* cls, int tid) {
    if (lc.mask || cls)
        for (int i = tid; i < (V + 1) / 2; i += 256) {
            unsigned m = 0xFFFFFFFFu;
            if (lc.mask) m &= lc.mask[i >> 4];
            if (cls) m &= cls[i >> 4];
            const unsigned two = (m >> (2 * (i & 15))) & 3u;
            cnt[i] |= ((two & 1u) ? 0u : 0xFFFFu) | ((two & 2u) ? 0u : 0xFFFF0000u);
        }
    if (tid == 0) cnt[0] = (cnt[0] & 0xFFFF0000u) | (lc.pad_ban ? 0xFFFFu : 0u);
    __syncthreads();
}

// Rhyme schemes (the *_rhyme entries, include/mmtg_hip.h): a TemplateRule (its table may be null: no templates) whose end set, on
// a follower line, is found at run time.  lead[b, l] is the line whose last content id t decides line l's rhyme (-1: no follower);
// class_of[t] is t's class, a row of the line rule's own `sets` (-1: none).  A leader is an ordinary line with a static end set (the
// union of the classes), so only followers are new here; a follower whose leader gave no class is an ordinary line.
struct RhymeRule {
    TemplateRule tm;               // tm.table may be null
    const short* class_of;         // [V] row of `sets`, or -1
    const signed char* lead;       // [B, n_lines] the leader's line (< l), or -1
    int distinct;                  // a follower may not end on an id an earlier line of its group ends on
    int V;
    static constexpr bool ngram = true, lines = true, tmpl = true, rhyme = true, refrain = false;
    __device__ __forceinline__ bool held(int b, int pos) const { return tm.held(b, pos); }
    __host__ __device__ __forceinline__ const NgramBan& bans() const { return tm.ln.ng; }
    __device__ __forceinline__ TmplCol sym(int b, int j, int sent) const {
        return tm.table ? tm.sym(b, j, sent) : TmplCol{-1, nullptr};
    }

    // the last content id of line r of the row (0: the line is empty); at most sent - 2 reads, every thread the same
    __device__ __forceinline__ int line_end(int r, int sent, const long long* gen) const {
        long long t = 0;
        for (int q = r * sent + 1; q < r * sent + sent - 1; ++q) {
            const long long v = gen[q];
            if (v != 0) t = v;
        }
        return t > 0 && t < V ? (int)t : 0;
    }

    // row b's leader of line l, or -1 (a leader lies before its follower, so its line is complete when the follower is written)
    __device__ __forceinline__ int leader(int b, int l) const {
        const int r = lead[(long)b * tm.ln.n_lines + l];
        return r >= 0 && r < l ? r : -1;
    }

    // LineRule::col with a follower's set index taken from class_of[t]; *rhymes: the column is a follower's and its leader gave a class
    __device__ __forceinline__ LineCol col(int b, int j, int sent, const long long* gen, bool* rhymes) const {
        const LineRule& ln = tm.ln;
        const int l = j / sent, c = j % sent - 1;
        const int r = l < ln.n_lines ? leader(b, l) : -1;
        *rhymes = false;
        if (r < 0) return ln.col(b, j, sent, gen);
        LineCol lc = {false, false, nullptr};
        const long at = (long)b * ln.n_lines + l;
        const int lo_ = ln.lo[at], hi_ = ln.hi[at];
        lc.force_pad = c >= hi_;
        lc.pad_ban = c < lo_;
        if (lc.force_pad) return lc;
        const int t = line_end(r, sent, gen);
        const int s = t ? (int)class_of[t] : -1;
        if (s >= 0 && s < ln.n_sets) {
            const unsigned* m = ln.sets + (long)s * ln.words;
            const long long prev = gen[j - 1];
            const bool in = prev >= 0 && prev < 32LL * ln.words && ((m[prev >> 5] >> (prev & 31)) & 1u);
            lc.pad_ban = lc.pad_ban || !in;
            if (c == hi_ - 1) lc.mask = m;
            *rhymes = true;
        }
        return lc;
    }

    // rhyme_distinct, after ban_line_tmpl on a column col() said rhymes: thread m < l looks at line m; if it is of the follower's
    // group, its end id loses its place in the set -- the sentinel at the mask column, and PAD's sentinel where it is the previous
    // token.  All threads of the block call (rhymes is uniform over the block).
    __device__ __forceinline__ void ban_distinct(unsigned* cnt, int b, int j, int sent, const long long* gen, const LineCol& lc,
                                                 bool rhymes, int tid) const {
        const LineRule& ln = tm.ln;
        if (!distinct || !rhymes) return;
        const int l = j / sent, r = leader(b, l);
        if (tid < l && (tid == r || lead[(long)b * ln.n_lines + tid] == r)) {
            const int t = line_end(tid, sent, gen);
            if (t) {
                if (lc.mask) atomicOr(cnt + (t >> 1), 0xFFFFu << (16 * (t & 1)));
                if (gen[j - 1] == t) atomicOr(cnt, 0xFFFFu);
            }
        }
        __syncthreads();
    }
};

// Refrain schemes (the *_refrain entries, include/mmtg_hip.h): a RhymeRule plus src[b, l], the line whose text line l of row b repeats
// (-1: line l is no copy).  On a copy column the row writes the id its own history holds at the same column of the source line, before
// every other test but the held prefix and the cadence; everywhere else the rule is rh's.  rh's own tables may be the "no rule" forms:
// lo / hi null (no line rule at all; n_lines is still the width of src) and lead null (no rhyme scheme).
struct RefrainRule {
    RhymeRule rh;
    const signed char* src;        // [B, n_lines] the source's line (< l), or -1
    static constexpr bool ngram = true, lines = true, tmpl = true, rhyme = true, refrain = true;
    __device__ __forceinline__ bool held(int b, int pos) const { return rh.held(b, pos); }
    __host__ __device__ __forceinline__ const NgramBan& bans() const { return rh.bans(); }
    __device__ __forceinline__ TmplCol sym(int b, int j, int sent) const { return rh.sym(b, j, sent); }
    __device__ __forceinline__ LineCol col(int b, int j, int sent, const long long* gen, bool* rhymes) const {
        if (rh.lead) return rh.col(b, j, sent, gen, rhymes);
        *rhymes = false;
        return rh.tm.ln.lo ? rh.tm.ln.col(b, j, sent, gen) : LineCol{false, false, nullptr};
    }
    __device__ __forceinline__ void ban_distinct(unsigned* cnt, int b, int j, int sent, const long long* gen, const LineCol& lc,
                                                 bool rhymes, int tid) const {
        rh.ban_distinct(cnt, b, j, sent, gen, lc, rhymes, tid);         // (rhymes is false without a lead table)
    }

    // the lyric index row b copies into index j (the same column of its source line; < j), or -1: no copy column
    __device__ __forceinline__ int copy_from(int b, int j, int sent) const {
        const int l = j / sent;
        if (l >= rh.tm.ln.n_lines) return -1;
        const int r = src[(long)b * rh.tm.ln.n_lines + l];
        return r >= 0 && r < l ? j - (l - r) * sent : -1;
    }
};

// logits processor + arg-max + forced-token cadence + append (generate.py:117-142), device-driven.
template <typename R>
__global__ __launch_bounds__(256) void decode_select_kernel(const float* __restrict__ logits, long ldl, int V,
        long long* __restrict__ seq, long ldseq, const int* __restrict__ pos_ptr, int P, int sent,
        float temperature, float rep_penalty, int have_logits, int top_k, float top_p,
        const float* __restrict__ uniforms, long ldu, int* __restrict__ pos_next, R rule) {
    extern __shared__ unsigned cnt[];
    __shared__ float sval[4];
    __shared__ int sidx[4];
    const int b = blockIdx.x, tid = threadIdx.x, pos = *pos_ptr;
    // the step's last kernel also publishes the next position -- into the OTHER slot of the decoder's position pair (every
    // kernel of this step reads *pos_ptr; nobody reads *pos_next before the next step), which replaces a one-thread launch
    if (pos_next && b == 0 && tid == 0) *pos_next = pos + 1;
    if (rule.held(b, pos)) return;
    const int j = pos + 1 - P;                 // lyric index of the token to append
    if (j < 1) return;                         // still inside the prompt / the initial [#START#]
    long long* gen = seq + (long)b * ldseq + P;
    if (j > 1 && (j + 1) % sent == 0) { if (tid == 0) gen[j] = 2; return; }     // [#EOS#]
    if (j > 1 && (j + 1) % sent == 1) { if (tid == 0) gen[j] = 1; return; }     // [#START#]
    if constexpr (R::refrain) {                // a copy column: the id the row's own history holds there in the source line, literally
        const int q = rule.copy_from(b, j, sent);
        if (q >= 0) { const long long v = gen[q]; if (tid == 0) gen[j] = v; return; }
    }
    if (!have_logits) return;
    const int n = min(j, MAXGEN);
    if (gen[n - 1] == 0) { if (tid == 0) gen[j] = 0; return; }                   // sticky PAD
    LineCol lc = {false, false, nullptr};
    [[maybe_unused]] bool rhymes = false;
    if constexpr (R::lines) {
        if constexpr (R::rhyme) lc = rule.col(b, j, sent, gen, &rhymes);
        else lc = rule.col(b, j, sent, gen);
        if (lc.force_pad) { if (tid == 0) gen[j] = 0; return; }                  // the line is full: PAD, as sticky PAD writes it
    }
    TmplCol tc = {-1, nullptr};
    if constexpr (R::tmpl) {
        tc = rule.sym(b, j, sent);
        if (tc.given >= 0) { if (tid == 0) gen[j] = tc.given; return; }          // a given column: its id, as a full line writes PAD
    }
    count_ids(cnt, V, gen, n, tid);
    if constexpr (R::ngram) {  // after the (V + 1) / 2 count words and, when sampling, the V-float row image
        const NgramBan ng = rule.bans();
        if (!R::lines || ng.n > 0)
            ban_ngrams(cnt, reinterpret_cast<int*>(cnt + (V + 1) / 2 + (uniforms ? V : 0)), V, gen, min(n, ng.hist_cap), ng.n, tid);
    }
    if constexpr (R::tmpl) ban_line_tmpl(cnt, V, lc, tc.cls, tid);
    else if constexpr (R::lines) ban_line(cnt, V, lc, tid);
    if constexpr (R::rhyme) rule.ban_distinct(cnt, b, j, sent, gen, lc, rhymes, tid);
    if (uniforms) {            // stochastic: uniforms[pos, b] drives the draw (top_k == 1 and top_p == 0 is the greedy path)
        float* px = reinterpret_cast<float*>(cnt + (V + 1) / 2);
        int pick;
        if constexpr (R::tmpl)     // (sample_row's comment: an instantiation of its own, inlined by force; the rhyme form's too)
            [[clang::always_inline]] pick = sample_row<true, true, true>(logits + (long)b * ldl, V, cnt, px, temperature, rep_penalty, top_k,
                                                                         top_p, uniforms[(long)pos * ldu + b], tid, nullptr);
        else
            pick = sample_row<R::ngram, R::lines>(logits + (long)b * ldl, V, cnt, px, temperature, rep_penalty, top_k, top_p,
                                                  uniforms[(long)pos * ldu + b], tid, nullptr);
        if (tid == 0) gen[j] = pick;
        return;
    }
    float best;
    int besti;
    scan_row<R::ngram, R::lines>(logits + (long)b * ldl, V, cnt, temperature, rep_penalty, tid, best, besti);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(besti, o, 64);
        if (ov > best || (ov == best && oi < besti)) { best = ov; besti = oi; }
    }
    if ((tid & 63) == 0) { sval[tid >> 6] = best; sidx[tid >> 6] = besti; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w)
            if (sval[w] > best || (sval[w] == best && sidx[w] < besti)) { best = sval[w]; besti = sidx[w]; }
        gen[j] = besti == 0x7fffffff ? 0 : besti;
    }
}

// decode_select_kernel<RefrainRule>'s sampling path with sample_row_warp for the draw (mmtg_decode_sample_warp): a kernel of its
// own over the most general rule, whose "no rule" forms serve every generation, so the kernels above stay what they were.  Always
// with logits and uniforms (a step without the head runs the entry it always ran).
__global__ __launch_bounds__(256) void decode_select_warp_kernel(const float* __restrict__ logits, long ldl, int V,
        long long* __restrict__ seq, long ldseq, const int* __restrict__ pos_ptr, int P, int sent,
        float temperature, float rep_penalty, int top_k, float top_p, float min_p, float typical_p, float epsilon_cutoff,
        float eta_cutoff, const float* __restrict__ uniforms, long ldu, int* __restrict__ pos_next, RefrainRule rule) {
    extern __shared__ unsigned cnt[];
    const int b = blockIdx.x, tid = threadIdx.x, pos = *pos_ptr;
    if (pos_next && b == 0 && tid == 0) *pos_next = pos + 1;
    if (rule.held(b, pos)) return;
    const int j = pos + 1 - P;                 // lyric index of the token to append
    if (j < 1) return;                         // still inside the prompt / the initial [#START#]
    long long* gen = seq + (long)b * ldseq + P;
    if (j > 1 && (j + 1) % sent == 0) { if (tid == 0) gen[j] = 2; return; }     // [#EOS#]
    if (j > 1 && (j + 1) % sent == 1) { if (tid == 0) gen[j] = 1; return; }     // [#START#]
    const int q = rule.copy_from(b, j, sent);
    if (q >= 0) { const long long v = gen[q]; if (tid == 0) gen[j] = v; return; }
    const int n = min(j, MAXGEN);
    if (gen[n - 1] == 0) { if (tid == 0) gen[j] = 0; return; }                   // sticky PAD
    bool rhymes = false;
    const LineCol lc = rule.col(b, j, sent, gen, &rhymes);
    if (lc.force_pad) { if (tid == 0) gen[j] = 0; return; }
    const TmplCol tc = rule.sym(b, j, sent);
    if (tc.given >= 0) { if (tid == 0) gen[j] = tc.given; return; }
    count_ids(cnt, V, gen, n, tid);
    const NgramBan ng = rule.bans();
    if (ng.n > 0) ban_ngrams(cnt, reinterpret_cast<int*>(cnt + (V + 1) / 2 + V), V, gen, min(n, ng.hist_cap), ng.n, tid);
    ban_line_tmpl(cnt, V, lc, tc.cls, tid);
    rule.ban_distinct(cnt, b, j, sent, gen, lc, rhymes, tid);
    float* px = reinterpret_cast<float*>(cnt + (V + 1) / 2);
    const int pick = sample_row_warp<true, true>(logits + (long)b * ldl, V, cnt, px, temperature, rep_penalty, top_k, top_p, min_p,
                                                 typical_p, epsilon_cutoff, eta_cutoff, uniforms[(long)pos * ldu + b], tid, nullptr);
    if (tid == 0) gen[j] = pick;
}

// decode_select_warp_kernel with the Mirostat stage (mmtg_decode_sample_mirostat).  mu[b] changes only on a column the row
// draws: every early return leaves it alone.
__global__ __launch_bounds__(256) void decode_select_mirostat_kernel(const float* __restrict__ logits, long ldl, int V,
        long long* __restrict__ seq, long ldseq, const int* __restrict__ pos_ptr, int P, int sent,
        float temperature, float rep_penalty, int top_k, float top_p, float min_p, float typical_p, float epsilon_cutoff,
        float eta_cutoff, float tau, float eta, float* mu, const float* __restrict__ uniforms, long ldu, int* __restrict__ pos_next,
        RefrainRule rule) {
    extern __shared__ unsigned cnt[];
    const int b = blockIdx.x, tid = threadIdx.x, pos = *pos_ptr;
    if (pos_next && b == 0 && tid == 0) *pos_next = pos + 1;
    if (rule.held(b, pos)) return;
    const int j = pos + 1 - P;                 // lyric index of the token to append
    if (j < 1) return;                         // still inside the prompt / the initial [#START#]
    long long* gen = seq + (long)b * ldseq + P;
    if (j > 1 && (j + 1) % sent == 0) { if (tid == 0) gen[j] = 2; return; }     // [#EOS#]
    if (j > 1 && (j + 1) % sent == 1) { if (tid == 0) gen[j] = 1; return; }     // [#START#]
    const int q = rule.copy_from(b, j, sent);
    if (q >= 0) { const long long v = gen[q]; if (tid == 0) gen[j] = v; return; }
    const int n = min(j, MAXGEN);
    if (gen[n - 1] == 0) { if (tid == 0) gen[j] = 0; return; }                   // sticky PAD
    bool rhymes = false;
    const LineCol lc = rule.col(b, j, sent, gen, &rhymes);
    if (lc.force_pad) { if (tid == 0) gen[j] = 0; return; }
    const TmplCol tc = rule.sym(b, j, sent);
    if (tc.given >= 0) { if (tid == 0) gen[j] = tc.given; return; }
    const float mub = mu[b];
    count_ids(cnt, V, gen, n, tid);
    const NgramBan ng = rule.bans();
    if (ng.n > 0) ban_ngrams(cnt, reinterpret_cast<int*>(cnt + (V + 1) / 2 + V), V, gen, min(n, ng.hist_cap), ng.n, tid);
    ban_line_tmpl(cnt, V, lc, tc.cls, tid);
    rule.ban_distinct(cnt, b, j, sent, gen, lc, rhymes, tid);
    float* px = reinterpret_cast<float*>(cnt + (V + 1) / 2);
    float s;
    const int pick = sample_row_warp<true, true, true>(logits + (long)b * ldl, V, cnt, px, temperature, rep_penalty, top_k, top_p, min_p,
                                                       typical_p, epsilon_cutoff, eta_cutoff, uniforms[(long)pos * ldu + b], tid, nullptr,
                                                       mub, &s);
    if (tid == 0) { gen[j] = pick; mu[b] = mub - eta * (s - tau); }
}

__global__ void decode_advance_kernel(int* pos_ptr) { *pos_ptr += 1; }

// ------------------------------------------------------------------ beam search (the selection step of BeamDecoder)
// Rows b0 .. b0 + nb - 1 of the batch are the nb beams of prompt b0 / nb.  Two launches replace decode_select:
//   candidates (one workgroup per row): the row's processed logits x exactly as decode_select computes them (per-occurrence
//     penalty, temperature, bans; cut at V), log_softmax(x) in fp32, and the row's top nb (log-probability, id) pairs ordered by
//     x descending, then id ascending.  A sticky-PAD row offers PAD at log-probability 0 (then -inf fillers).
//   merge (one workgroup per prompt): candidate (parent p, rank k) scores scores[p] + logp; the prompt keeps its nb best by
//     (score descending, parent ascending, rank ascending), reorders its rows of seq / keep / the ancestry table in place (staged
//     through LDS), appends the tokens and points rows[b, pos + 1] at b.  Forced positions keep every beam (identity) and append
//     the forced token; the scores are unchanged there.
constexpr int BEAM_MAX = 16;
constexpr int BEAM_TW = 64;        // columns of seq / keep / rows staged per pass of the reorder

__device__ __forceinline__ bool beam_forced(int j, int sent) { return j > 1 && ((j + 1) % sent == 0 || (j + 1) % sent == 1); }

template <typename R>
__global__ __launch_bounds__(256) void beam_candidates_kernel(const float* __restrict__ logits, long ldl, int V,
        const long long* __restrict__ seq, long ldseq, const int* __restrict__ pos_ptr, int P, int sent,
        float temperature, float rep_penalty, int nb, float* __restrict__ cand_val, int* __restrict__ cand_id, R rule) {
    extern __shared__ unsigned cnt[];          // (V + 1) / 2 count words | V processed logits
    float* const px = reinterpret_cast<float*>(cnt + (V + 1) / 2);
    __shared__ float sval[4], sx[BEAM_MAX];
    __shared__ int sidx[4], si[BEAM_MAX];
    const int b = blockIdx.x, tid = threadIdx.x, pos = *pos_ptr;
    const int j = pos + 1 - P;
    if (j < 1 || beam_forced(j, sent)) return;             // the merge appends the forced token without candidates
    if (rule.held(b, pos)) return;                         // a prefix column: nothing to offer (the merge keeps the prompt)
    float* const cv = cand_val + (long)b * nb;
    int* const ci = cand_id + (long)b * nb;
    const long long* gen = seq + (long)b * ldseq + P;
    if constexpr (R::refrain) {                            // a copy column: the source's id with the score unchanged, as a given id
        const int q = rule.copy_from(b, j, sent);
        if (q >= 0) {
            const int v = (int)gen[q];
            if (tid < nb) { cv[tid] = tid == 0 ? 0.f : -INFINITY; ci[tid] = tid == 0 ? v : 0; }
            return;
        }
    }
    const int n = min(j, MAXGEN);
    if (gen[n - 1] == 0) {                                 // sticky PAD: PAD with the score unchanged
        if (tid < nb) { cv[tid] = tid == 0 ? 0.f : -INFINITY; ci[tid] = 0; }
        return;
    }
    LineCol lc = {false, false, nullptr};
    [[maybe_unused]] bool rhymes = false;
    if constexpr (R::lines) {
        if constexpr (R::rhyme) lc = rule.col(b, j, sent, gen, &rhymes);
        else lc = rule.col(b, j, sent, gen);
        if (lc.force_pad) {                                // the line is full: PAD with the score unchanged, as sticky PAD offers it
            if (tid < nb) { cv[tid] = tid == 0 ? 0.f : -INFINITY; ci[tid] = 0; }
            return;
        }
    }
    TmplCol tc = {-1, nullptr};
    if constexpr (R::tmpl) {
        tc = rule.sym(b, j, sent);
        if (tc.given >= 0) {                               // a given column: its id with the score unchanged
            if (tid < nb) { cv[tid] = tid == 0 ? 0.f : -INFINITY; ci[tid] = tid == 0 ? tc.given : 0; }
            return;
        }
    }
    count_ids(cnt, V, gen, n, tid);
    if constexpr (R::ngram) {  // after the count words and the V processed logits
        const NgramBan ng = rule.bans();
        if (!R::lines || ng.n > 0) ban_ngrams(cnt, reinterpret_cast<int*>(px + V), V, gen, min(n, ng.hist_cap), ng.n, tid);
    }
    if constexpr (R::tmpl) ban_line_tmpl(cnt, V, lc, tc.cls, tid);
    else if constexpr (R::lines) ban_line(cnt, V, lc, tid);
    if constexpr (R::rhyme) rule.ban_distinct(cnt, b, j, sent, gen, lc, rhymes, tid);
    const float* row = logits + (long)b * ldl;
    float mx = -INFINITY;
    for (int v = tid; v < V; v += 256) {
        float x = row[v];
        if ((R::lines || v != 0) && v != 102) {
            const int c = (cnt[v >> 1] >> (16 * (v & 1))) & 0xFFFF;
            x = penalize<R::ngram>(x, c, rep_penalty);
        }
        x = x / temperature;
        if (v == 1 || v == 2 || v == 100 || v == 102) x = -INFINITY;
        px[v] = x;
        mx = fmaxf(mx, x);
    }
    mx = wave_max(mx);
    if ((tid & 63) == 0) sval[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(sval[0], sval[1]), fmaxf(sval[2], sval[3]));
    float sum = 0.f;
    for (int v = tid; v < V; v += 256) sum += expf(px[v] - mx);
    sum = wave_sum(sum);
    __syncthreads();
    if ((tid & 63) == 0) sval[tid >> 6] = sum;
    __syncthreads();
    const float lsum = logf(sval[0] + sval[1] + sval[2] + sval[3]);
    // nb rounds of the block arg-max (lowest id wins ties); a taken id is marked NaN, which no comparison selects again
    for (int r = 0; r < nb; ++r) {
        __syncthreads();
        float best = -INFINITY;
        int besti = 0x7fffffff;
        for (int v = tid; v < V; v += 256) {
            const float x = px[v];
            if (x > best || (x == best && v < besti)) { best = x; besti = v; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(besti, o, 64);
            if (ov > best || (ov == best && oi < besti)) { best = ov; besti = oi; }
        }
        if ((tid & 63) == 0) { sval[tid >> 6] = best; sidx[tid >> 6] = besti; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < 4; ++w)
                if (sval[w] > best || (sval[w] == best && sidx[w] < besti)) { best = sval[w]; besti = sidx[w]; }
            sx[r] = best;
            si[r] = besti;
            if (besti >= 0 && besti < V) px[besti] = __int_as_float(0x7fc00000);
        }
    }
    __syncthreads();
    if (tid < nb) {
        const float x = sx[tid];
        const bool ok = si[tid] >= 0 && si[tid] < V && x > -INFINITY && mx > -INFINITY;
        cv[tid] = ok ? (x - mx) - lsum : -INFINITY;        // log_softmax(x)[v] = (x - max) - log(sum exp(x - max))
        ci[tid] = ok ? si[tid] : 0;
    }
}

template <typename R>
__global__ __launch_bounds__(256) void beam_merge_kernel(const float* __restrict__ cand_val, const int* __restrict__ cand_id,
        float* __restrict__ scores, long long* __restrict__ seq, long ldseq, int* __restrict__ keep, long ldkeep,
        int* __restrict__ rows, long ldrows, const int* __restrict__ pos_ptr, int P, int sent, int nb, int* __restrict__ pos_next,
        R rule) {
    __shared__ float sc[BEAM_MAX * BEAM_MAX];
    __shared__ float s_sc[BEAM_MAX];
    __shared__ int s_par[BEAM_MAX], s_tok[BEAM_MAX];
    __shared__ long long st_seq[BEAM_MAX][BEAM_TW];
    __shared__ int st_keep[BEAM_MAX][BEAM_TW], st_rows[BEAM_MAX][BEAM_TW];
    const int g = blockIdx.x, tid = threadIdx.x, pos = *pos_ptr, b0 = g * nb;
    if (pos_next && g == 0 && tid == 0) *pos_next = pos + 1;
    const int j = pos + 1 - P;
    const bool next_ok = pos + 1 < ldrows;
    if (rule.held(b0, pos)) {                               // the prompt's prefix column (one prefix per prompt): keep every beam,
        if (tid < nb && next_ok) rows[(long)(b0 + tid) * ldrows + pos + 1] = b0 + tid;       // its score and its host-written token
        return;
    }
    if (j < 1 || beam_forced(j, sent) || !cand_val) {      // identity: the forced token (if any), every beam keeps its own row
        if (tid < nb) {
            const long b = b0 + tid;
            if (j >= 1 && beam_forced(j, sent)) seq[b * ldseq + pos + 1] = (j + 1) % sent == 0 ? 2 : 1;
            if (next_ok) rows[b * ldrows + pos + 1] = (int)b;
        }
        return;
    }
    const int nc = nb * nb;
    float my = -INFINITY;
    int mp = 0, mk = 0;
    if (tid < nc) {
        mp = tid / nb;
        mk = tid - mp * nb;
        my = scores[b0 + mp] + cand_val[(long)(b0 + mp) * nb + mk];
        if (my != my) my = -INFINITY;                      // (a strict total order: every place below is taken once)
        sc[tid] = my;
    }
    __syncthreads();
    if (tid < nc) {
        // candidate o = (parent o / nb, rank o % nb): (parent, rank) ascending is o ascending
        int place = 0;
        for (int o = 0; o < nc; ++o) {
            const float so = sc[o];
            place += (so > my) || (so == my && o < tid);
        }
        if (place < nb) { s_par[place] = mp; s_tok[place] = cand_id[(long)(b0 + mp) * nb + mk]; s_sc[place] = my; }
    }
    __syncthreads();
    bool ident = true;
    for (int r = 0; r < nb; ++r) ident = ident && s_par[r] == r;
    if (!ident) {
        for (int c0 = 0; c0 <= pos; c0 += BEAM_TW) {
            const int w = min(BEAM_TW, pos + 1 - c0);
            for (int e = tid; e < nb * BEAM_TW; e += 256) {
                const int r = e / BEAM_TW, c = e - r * BEAM_TW;
                if (c < w) {
                    const long b = b0 + r;
                    st_seq[r][c] = seq[b * ldseq + c0 + c];
                    st_keep[r][c] = keep[b * ldkeep + c0 + c];
                    st_rows[r][c] = rows[b * ldrows + c0 + c];
                }
            }
            __syncthreads();
            for (int e = tid; e < nb * BEAM_TW; e += 256) {
                const int r = e / BEAM_TW, c = e - r * BEAM_TW;
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
        seq[b * ldseq + pos + 1] = s_tok[tid];
        if (next_ok) rows[b * ldrows + pos + 1] = (int)b;
    }
}

// Diverse beams (the *_merge_groups entries, include/mmtg_hip.h): the prompt's nb beams are G groups of s = nb / G rows, served in
// order.  Round g ranks the s * nb candidates whose parent is one of group g's rows by sel = base - lambda * n(v), n(v) = the live
// slots (score above -inf) earlier rounds filled with the content id v at this step, and keeps the s best by (sel descending,
// parent ascending, rank ascending) with the score base.  The s best after the penalty lie among each parent's nb best before it
// (at most nb - s ids are penalised), so the candidates kernels' tables are enough.  Held prompts, forced columns and null
// candidates do what beam_merge_kernel does; G = 1 is beam_merge_kernel's selection (n is 0 throughout).
template <typename R>
__global__ __launch_bounds__(256) void beam_merge_groups_kernel(const float* __restrict__ cand_val, const int* __restrict__ cand_id,
        float* __restrict__ scores, long long* __restrict__ seq, long ldseq, int* __restrict__ keep, long ldkeep,
        int* __restrict__ rows, long ldrows, const int* __restrict__ pos_ptr, int P, int sent, int nb, int* __restrict__ pos_next,
        int groups, float lambda, R rule) {
    __shared__ float sc[BEAM_MAX * BEAM_MAX];
    __shared__ float s_sc[BEAM_MAX];
    __shared__ int s_par[BEAM_MAX], s_tok[BEAM_MAX];
    __shared__ long long st_seq[BEAM_MAX][BEAM_TW];
    __shared__ int st_keep[BEAM_MAX][BEAM_TW], st_rows[BEAM_MAX][BEAM_TW];
    const int g = blockIdx.x, tid = threadIdx.x, pos = *pos_ptr, b0 = g * nb;
    if (pos_next && g == 0 && tid == 0) *pos_next = pos + 1;
    const int j = pos + 1 - P;
    const bool next_ok = pos + 1 < ldrows;
    if (rule.held(b0, pos)) {
        if (tid < nb && next_ok) rows[(long)(b0 + tid) * ldrows + pos + 1] = b0 + tid;
        return;
    }
    if (j < 1 || beam_forced(j, sent) || !cand_val) {
        if (tid < nb) {
            const long b = b0 + tid;
            if (j >= 1 && beam_forced(j, sent)) seq[b * ldseq + pos + 1] = (j + 1) % sent == 0 ? 2 : 1;
            if (next_ok) rows[b * ldrows + pos + 1] = (int)b;
        }
        return;
    }
    const int nc = nb * nb, gs = nb / groups, gc = gs * nb;   // candidates in all, rows and candidates of one group
    float base = -INFINITY;
    int mp = 0, mk = 0, mv = 0;
    if (tid < nc) {
        mp = tid / nb;
        mk = tid - mp * nb;
        base = scores[b0 + mp] + cand_val[(long)(b0 + mp) * nb + mk];
        if (base != base) base = -INFINITY;
        mv = cand_id[(long)(b0 + mp) * nb + mk];
    }
    const bool content = ngram_content(mv);
    for (int r = 0; r < groups; ++r) {
        const int c0 = r * gc, r0 = r * gs;                    // the round's first candidate and first slot
        const bool mine = tid >= c0 && tid < c0 + gc;
        float sel = base;
        if (mine) {
            int n = 0;
            if (content)
                for (int q = 0; q < r0; ++q) n += s_tok[q] == mv && s_sc[q] > -INFINITY;
            if (n) {
#pragma clang fp contract(off)
                const float pen = lambda * (float)n;           // (two roundings, as a host restatement in fp32 has them)
                sel = base - pen;
            }
            sc[tid] = sel;
        }
        __syncthreads();
        if (mine) {
            int place = 0;
            for (int o = c0; o < c0 + gc; ++o) {
                const float so = sc[o];
                place += (so > sel) || (so == sel && o < tid);
            }
            if (place < gs) { s_par[r0 + place] = mp; s_tok[r0 + place] = mv; s_sc[r0 + place] = base; }
        }
        __syncthreads();
    }
    bool ident = true;
    for (int r = 0; r < nb; ++r) ident = ident && s_par[r] == r;
    if (!ident) {
        for (int c0 = 0; c0 <= pos; c0 += BEAM_TW) {
            const int w = min(BEAM_TW, pos + 1 - c0);
            for (int e = tid; e < nb * BEAM_TW; e += 256) {
                const int r = e / BEAM_TW, c = e - r * BEAM_TW;
                if (c < w) {
                    const long b = b0 + r;
                    st_seq[r][c] = seq[b * ldseq + c0 + c];
                    st_keep[r][c] = keep[b * ldkeep + c0 + c];
                    st_rows[r][c] = rows[b * ldrows + c0 + c];
                }
            }
            __syncthreads();
            for (int e = tid; e < nb * BEAM_TW; e += 256) {
                const int r = e / BEAM_TW, c = e - r * BEAM_TW;
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
        seq[b * ldseq + pos + 1] = s_tok[tid];
        if (next_ok) rows[b * ldrows + pos + 1] = (int)b;
    }
}

// Keyword-constrained beams (the *_kw entries, include/mmtg_hip.h): a prompt carries K <= KW_MAX phrases of 1 .. KW_LEN content
// ids its lyric should contain somewhere.  The candidates kernel offers W = nb + K slots per row -- the top nb as ever, then one
// slot per keyword with the phrase's next id -- and the bank of every slot, bank(h + [id]) = the lengths of the keywords met in the
// history plus the longest partial phrase it ends in; the merge shares the nb places among the banks.  The bank is a function of
// the history alone, recomputed at every step: nothing is carried from step to step or reordered with the beams.
constexpr int KW_MAX = 8, KW_LEN = 4;

struct Keywords {
    const int* phrases;          // int32 [prompts, KW_MAX, KW_LEN]
    const signed char* lens;     // int8 [prompts, KW_MAX]; a length outside 1 .. cap makes its keyword inert (no slot, no bank)
    int K;                       // keywords per prompt, 0 .. KW_MAX
    int cap;                     // the longest phrase of the call, 1 .. KW_LEN
    int* cand_bank;              // int32 [B, nb + K]
};

// tail: the last KW_LEN - 1 ids of the history h, oldest first (-1 before the row's start).  The id d places before the end of
// h + [t] (APP) or of h itself (d = 0: the last one)
template <bool APP>
__device__ __forceinline__ int kw_at(const int* tail, int t, int d) {
    return APP ? (d == 0 ? t : tail[KW_LEN - 1 - d]) : tail[KW_LEN - 2 - d];
}

// the largest m <= top with the last m ids of h + [t] (APP; top <= KW_LEN) or of h (top < KW_LEN) equal to ph[0..m), 0 if none
template <bool APP>
__device__ __forceinline__ int kw_match(const int* ph, int top, const int* tail, int t) {
    int best = 0;
    for (int m = 1; m <= top; ++m) {
        bool eq = true;
        for (int k = 0; k < m; ++k) eq = eq && kw_at<APP>(tail, t, m - 1 - k) == ph[k];
        if (eq) best = m;
    }
    return best;
}

// the id an unmet keyword of length L offers after h: phrase[m], m its progress (the longest proper prefix of the phrase h ends in)
__device__ __forceinline__ int kw_offer(const int* ph, int L, const int* tail) { return ph[kw_match<false>(ph, L - 1, tail, 0)]; }

// bank(h + [t]) from met(h) and the last ids of h: a keyword of met(h), or one the window ending in t completes, counts its
// length; of the others the longest progress counts
__device__ __forceinline__ int kw_bank(const int (*ph)[KW_LEN], const int* len, int K, unsigned met, const int* tail, int t) {
    int bank = 0, prog = 0;
    for (int q = 0; q < K; ++q) {
        const int L = len[q];
        if (L < 1) continue;
        if ((met >> q) & 1u) { bank += L; continue; }
        const int m = kw_match<true>(ph[q], L, tail, t);
        if (m == L) bank += L;
        else prog = max(prog, m);
    }
    return bank + prog;
}

// beam_candidates_kernel<RhymeRule> (its processing, line by line; the rule's tables may be empty: n_lines 0 constrains nothing)
// with the keyword slots and the banks.  A kernel of its own, so that the forms without keywords keep their code (a template, as
// they are: R is RhymeRule, the one form that serves every rule or none).
template <typename R>
__global__ __launch_bounds__(256) void beam_candidates_kw_kernel(const float* __restrict__ logits, long ldl, int V,
        const long long* __restrict__ seq, long ldseq, const int* __restrict__ pos_ptr, int P, int sent,
        float temperature, float rep_penalty, int nb, float* __restrict__ cand_val, int* __restrict__ cand_id, R rule,
        Keywords kw) {
    static_assert(R::rhyme, "the keyword candidates are built over the rhyme form");
    extern __shared__ unsigned cnt[];          // (V + 1) / 2 count words | V processed logits | the n-gram form's history
    float* const px = reinterpret_cast<float*>(cnt + (V + 1) / 2);
    __shared__ float sval[4], sx[BEAM_MAX];
    __shared__ int sidx[4], si[BEAM_MAX];
    __shared__ int s_ph[KW_MAX][KW_LEN], s_len[KW_MAX], s_tail[KW_LEN - 1];
    __shared__ unsigned s_met;
    const int b = blockIdx.x, tid = threadIdx.x, pos = *pos_ptr;
    const int j = pos + 1 - P;
    if (j < 1 || beam_forced(j, sent)) return;
    if (rule.held(b, pos)) return;
    const int K = kw.K, W = nb + K;
    float* const cv = cand_val + (long)b * W;
    int* const ci = cand_id + (long)b * W;
    int* const cb = kw.cand_bank + (long)b * W;
    const long long* gen = seq + (long)b * ldseq + P;
    const int n = min(j, MAXGEN);
    // the prompt's phrases, the history's last ids and the met mask: thread i looks at the windows that start at column i
    const long kw0 = (long)(b / nb) * KW_MAX;
    if (tid < KW_MAX * KW_LEN) s_ph[tid / KW_LEN][tid % KW_LEN] = tid / KW_LEN < K ? kw.phrases[kw0 * KW_LEN + tid] : -1;
    if (tid < KW_MAX) {
        const int L = tid < K ? (int)kw.lens[kw0 + tid] : 0;
        s_len[tid] = L >= 1 && L <= kw.cap ? L : 0;
    }
    if (tid < KW_LEN - 1) {
        const int c = j - (KW_LEN - 1) + tid;
        s_tail[tid] = c >= 0 ? (int)gen[c] : -1;
    }
    if (tid == 0) s_met = 0u;
    __syncthreads();
    for (int i = tid; i < j; i += 256) {
        unsigned hit = 0u;
        for (int q = 0; q < K; ++q) {
            const int L = s_len[q];
            bool eq = L >= 1 && i + L <= j;
            for (int k = 0; eq && k < L; ++k) eq = gen[i + k] == (long long)s_ph[q][k];
            if (eq) hit |= 1u << q;
        }
        if (hit) atomicOr(&s_met, hit);
    }
    __syncthreads();
    const unsigned met = s_met;
    int one = -1;                                          // >= 0: the row offers this id alone, with the score unchanged
    if (gen[n - 1] == 0) one = 0;                          // sticky PAD
    bool rhymes = false;
    LineCol lc = {false, false, nullptr};
    TmplCol tc = {-1, nullptr};
    if (one < 0) {
        lc = rule.col(b, j, sent, gen, &rhymes);
        if (lc.force_pad) one = 0;                         // the line is full
    }
    if (one < 0) {
        tc = rule.sym(b, j, sent);
        if (tc.given >= 0) one = tc.given;                 // a given column (it may complete a phrase)
    }
    if (one >= 0) {
        if (tid < W) {
            cv[tid] = tid == 0 ? 0.f : -INFINITY;
            ci[tid] = tid == 0 ? one : 0;
            cb[tid] = tid == 0 ? kw_bank(s_ph, s_len, K, met, s_tail, one) : 0;
        }
        return;
    }
    count_ids(cnt, V, gen, n, tid);
    const NgramBan ng = rule.bans();
    if (ng.n > 0) ban_ngrams(cnt, reinterpret_cast<int*>(px + V), V, gen, min(n, ng.hist_cap), ng.n, tid);
    ban_line_tmpl(cnt, V, lc, tc.cls, tid);
    rule.ban_distinct(cnt, b, j, sent, gen, lc, rhymes, tid);
    const float* row = logits + (long)b * ldl;
    float mx = -INFINITY;
    for (int v = tid; v < V; v += 256) {
        float x = row[v];
        if (v != 102) {
            const int c = (cnt[v >> 1] >> (16 * (v & 1))) & 0xFFFF;
            x = penalize<true>(x, c, rep_penalty);
        }
        x = x / temperature;
        if (v == 1 || v == 2 || v == 100 || v == 102) x = -INFINITY;
        px[v] = x;
        mx = fmaxf(mx, x);
    }
    mx = wave_max(mx);
    if ((tid & 63) == 0) sval[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(sval[0], sval[1]), fmaxf(sval[2], sval[3]));
    float sum = 0.f;
    for (int v = tid; v < V; v += 256) sum += expf(px[v] - mx);
    sum = wave_sum(sum);
    __syncthreads();
    if ((tid & 63) == 0) sval[tid >> 6] = sum;
    __syncthreads();
    const float lsum = logf(sval[0] + sval[1] + sval[2] + sval[3]);
    for (int r = 0; r < nb; ++r) {
        __syncthreads();
        float best = -INFINITY;
        int besti = 0x7fffffff;
        for (int v = tid; v < V; v += 256) {
            const float x = px[v];
            if (x > best || (x == best && v < besti)) { best = x; besti = v; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(besti, o, 64);
            if (ov > best || (ov == best && oi < besti)) { best = ov; besti = oi; }
        }
        if ((tid & 63) == 0) { sval[tid >> 6] = best; sidx[tid >> 6] = besti; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < 4; ++w)
                if (sval[w] > best || (sval[w] == best && sidx[w] < besti)) { best = sval[w]; besti = sidx[w]; }
            sx[r] = best;
            si[r] = besti;
            if (besti >= 0 && besti < V) px[besti] = __int_as_float(0x7fc00000);
        }
    }
    __syncthreads();
    if (tid < nb) {
        const float x = sx[tid];
        const bool ok = si[tid] >= 0 && si[tid] < V && x > -INFINITY && mx > -INFINITY;
        cv[tid] = ok ? (x - mx) - lsum : -INFINITY;
        ci[tid] = ok ? si[tid] : 0;
        cb[tid] = ok ? kw_bank(s_ph, s_len, K, met, s_tail, si[tid]) : 0;
    } else if (tid < W) {
        // keyword q's slot: the phrase's next id, unless the keyword is met, the id is banned (-inf), among the top nb (marked NaN
        // by the rounds above) or offered by an earlier keyword's slot (an earlier unmet keyword with the same next id: were that
        // slot dead for a ban or for the top nb, this one would be too)
        const int q = tid - nb, L = s_len[q];
        float val = -INFINITY;
        int id = 0, bank = 0;
        if (L >= 1 && !((met >> q) & 1u)) {
            const int t = kw_offer(s_ph[q], L, s_tail);
            bool dup = false;
            for (int e = 0; e < q; ++e) dup = dup || (s_len[e] >= 1 && !((met >> e) & 1u) && kw_offer(s_ph[e], s_len[e], s_tail) == t);
            if (t > 0 && t < V && !dup) {
                const float x = px[t];
                if (x > -INFINITY && mx > -INFINITY) {
                    val = (x - mx) - lsum;
                    id = t;
                    bank = kw_bank(s_ph, s_len, K, met, s_tail, t);
                }
            }
        }
        cv[tid] = val;
        ci[tid] = id;
        cb[tid] = bank;
    }
}

// beam_merge_kernel over W = nb + K candidates per parent and their banks (candidate o = p * W + k, one per thread).  A live
// candidate (base above -inf) has the rank r it holds inside its own bank by (base descending, o ascending); the live ones are
// ordered by (r ascending, bank descending) -- the best of every bank, highest bank first, then the second best of every bank --
// the dead ones follow in o order, and the first nb are kept with the score base.  With every bank equal that is the plain order.
template <typename R>
__global__ __launch_bounds__(256) void beam_merge_kw_kernel(const float* __restrict__ cand_val, const int* __restrict__ cand_id,
        const int* __restrict__ cand_bank, float* __restrict__ scores, long long* __restrict__ seq, long ldseq,
        int* __restrict__ keep, long ldkeep, int* __restrict__ rows, long ldrows, const int* __restrict__ pos_ptr, int P, int sent,
        int nb, int* __restrict__ pos_next, int K, R rule) {
    __shared__ float sc[BEAM_MAX * BEAM_MAX];
    __shared__ int s_bank[BEAM_MAX * BEAM_MAX], s_rank[BEAM_MAX * BEAM_MAX];
    __shared__ float s_sc[BEAM_MAX];
    __shared__ int s_par[BEAM_MAX], s_tok[BEAM_MAX];
    __shared__ long long st_seq[BEAM_MAX][BEAM_TW];
    __shared__ int st_keep[BEAM_MAX][BEAM_TW], st_rows[BEAM_MAX][BEAM_TW];
    const int g = blockIdx.x, tid = threadIdx.x, pos = *pos_ptr, b0 = g * nb;
    if (pos_next && g == 0 && tid == 0) *pos_next = pos + 1;
    const int j = pos + 1 - P;
    const bool next_ok = pos + 1 < ldrows;
    if (rule.held(b0, pos)) {
        if (tid < nb && next_ok) rows[(long)(b0 + tid) * ldrows + pos + 1] = b0 + tid;
        return;
    }
    if (j < 1 || beam_forced(j, sent) || !cand_val) {
        if (tid < nb) {
            const long b = b0 + tid;
            if (j >= 1 && beam_forced(j, sent)) seq[b * ldseq + pos + 1] = (j + 1) % sent == 0 ? 2 : 1;
            if (next_ok) rows[b * ldrows + pos + 1] = (int)b;
        }
        return;
    }
    constexpr int DEAD = 0x7fffffff;
    const int W = nb + K, nc = nb * W;                          // nc <= 256 (the entry checks)
    float my = -INFINITY;
    int mp = 0, mk = 0, bank = 0;
    if (tid < nc) {
        mp = tid / W;
        mk = tid - mp * W;
        my = scores[b0 + mp] + cand_val[(long)(b0 + mp) * W + mk];
        if (my != my) my = -INFINITY;
        bank = cand_bank[(long)(b0 + mp) * W + mk];
        sc[tid] = my;
        s_bank[tid] = bank;
    }
    __syncthreads();
    const bool live = my > -INFINITY;
    int r = DEAD;
    if (tid < nc) {
        if (live) {
            r = 0;
            for (int o = 0; o < nc; ++o) {
                const float so = sc[o];
                r += s_bank[o] == bank && ((so > my) || (so == my && o < tid));      // (so >= my is live)
            }
        }
        s_rank[tid] = r;
    }
    __syncthreads();
    if (tid < nc) {
        int place = 0;
        for (int o = 0; o < nc; ++o) {
            const int ro = s_rank[o];
            place += live ? (ro < r || (ro == r && s_bank[o] > bank)) : (ro != DEAD || o < tid);
        }
        if (place < nb) { s_par[place] = mp; s_tok[place] = cand_id[(long)(b0 + mp) * W + mk]; s_sc[place] = my; }
    }
    __syncthreads();
    bool ident = true;
    for (int q = 0; q < nb; ++q) ident = ident && s_par[q] == q;
    if (!ident) {
        for (int c0 = 0; c0 <= pos; c0 += BEAM_TW) {
            const int w = min(BEAM_TW, pos + 1 - c0);
            for (int e = tid; e < nb * BEAM_TW; e += 256) {
                const int q = e / BEAM_TW, c = e - q * BEAM_TW;
                if (c < w) {
                    const long b = b0 + q;
                    st_seq[q][c] = seq[b * ldseq + c0 + c];
                    st_keep[q][c] = keep[b * ldkeep + c0 + c];
                    st_rows[q][c] = rows[b * ldrows + c0 + c];
                }
            }
            __syncthreads();
            for (int e = tid; e < nb * BEAM_TW; e += 256) {
                const int q = e / BEAM_TW, c = e - q * BEAM_TW;
                if (c < w) {
                    const long b = b0 + q;
                    const int p = s_par[q];
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
        seq[b * ldseq + pos + 1] = s_tok[tid];
        if (next_ok) rows[b * ldrows + pos + 1] = (int)b;
    }
}

}  // namespace

extern "C" int mmtg_decode_embed(int dtype, const void* table, const long long* seq, long ldseq, const void* c, void* x,
                                 const int* pos_ptr, const long long* tpw_type, const long long* tpw_mask,
                                 long long* type_out, int* keep, long ldkeep, int B, int P, int S, int E, int two_sents,
                                 int V, int sent, int max_sent_num, void* stream) {
    MMTG_REQUIRE(table && seq && c && x && pos_ptr && tpw_type && tpw_mask && type_out && keep, "decode_embed: null pointer");
    MMTG_REQUIRE(B > 0 && E % 8 == 0 && sent > 1 && max_sent_num > 1, "decode_embed: bad sizes");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_DECODE, s, (double)B * E, (dtype == MMTG_F32 ? 12.0 : 6.0) * B * E);
    if (dtype == MMTG_F32)
        hipLaunchKernelGGL(decode_embed_kernel<float>, dim3(B), dim3(256), 0, s, (const float*)table, seq, ldseq, (const float*)c, (float*)x, pos_ptr, tpw_type, tpw_mask, type_out, keep, ldkeep, P, S, E, two_sents, V, sent, max_sent_num);
    else if (dtype == MMTG_BF16)
        hipLaunchKernelGGL(decode_embed_kernel<bf16>, dim3(B), dim3(256), 0, s, (const bf16*)table, seq, ldseq, (const bf16*)c, (bf16*)x, pos_ptr, tpw_type, tpw_mask, type_out, keep, ldkeep, P, S, E, two_sents, V, sent, max_sent_num);
    else MMTG_FAIL(MMTG_ERR_BAD_ARG, "decode_embed: bad dtype");
    MMTG_LAUNCH_CHECK("decode_embed");
    return MMTG_OK;
}

extern "C" int mmtg_decode_embed_add(int dtype, const void* g, const void* wpe, const void* wte, const long long* type_ids,
                                     const int* pos_ptr, void* h, int B, int D, float* stats, void* stream) {
    MMTG_REQUIRE(g && wpe && wte && type_ids && pos_ptr && h && B > 0 && D > 0, "decode_embed_add: bad args");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_DECODE, s, 2.0 * B * D, (dtype == MMTG_F32 ? 16.0 : 8.0) * B * D);
    if (dtype == MMTG_F32)
        hipLaunchKernelGGL(decode_embed_add_kernel<float>, dim3(B), dim3(256), 0, s, (const float*)g, (const float*)wpe, (const float*)wte, type_ids, pos_ptr, (float*)h, D, stats);
    else if (dtype == MMTG_BF16)
        hipLaunchKernelGGL(decode_embed_add_kernel<bf16>, dim3(B), dim3(256), 0, s, (const bf16*)g, (const bf16*)wpe, (const bf16*)wte, type_ids, pos_ptr, (bf16*)h, D, stats);
    else MMTG_FAIL(MMTG_ERR_BAD_ARG, "decode_embed_add: bad dtype");
    MMTG_LAUNCH_CHECK("decode_embed_add");
    return MMTG_OK;
}

extern "C" int mmtg_decode_attn(int dtype, const void* qkv, void* kcache, void* vcache, const int* keep, long ldkeep,
                                const int* pos_ptr, void* out, int B, int nH, int dh, int Tmax, void* stream) {
    MMTG_REQUIRE(qkv && kcache && vcache && keep && pos_ptr && out, "decode_attn: null pointer");
    MMTG_REQUIRE(dh == 64 && B > 0 && nH > 0 && Tmax > 0 && Tmax <= 1024, "decode_attn: head dim 64, Tmax <= 1024");
    hipStream_t s = (hipStream_t)stream;
    const double esz = dtype == MMTG_F32 ? 4 : 2;
    ProfScope prof(MMTG_PROF_DECODE, s, 4.0 * B * nH * (double)Tmax * dh, esz * 2.0 * B * nH * (double)Tmax * dh);
    dim3 grid(nH, B), block(64);
    if (dtype == MMTG_F32)
        hipLaunchKernelGGL(decode_attn_kernel<float>, grid, block, 0, s, (const float*)qkv, (float*)kcache, (float*)vcache, keep, ldkeep, pos_ptr, (float*)out, nH, Tmax, nullptr, 0, 0, nullptr);
    else if (dtype == MMTG_BF16)
        hipLaunchKernelGGL(decode_attn_kernel<bf16>, grid, block, 0, s, (const bf16*)qkv, (bf16*)kcache, (bf16*)vcache, keep, ldkeep, pos_ptr, (bf16*)out, nH, Tmax, nullptr, 0, 0, nullptr);
    else MMTG_FAIL(MMTG_ERR_BAD_ARG, "decode_attn: bad dtype");
    MMTG_LAUNCH_CHECK("decode_attn");
    return MMTG_OK;
}

extern "C" int mmtg_decode_attn_split(int dtype, const float* part, int splits, const float* bias, void* kcache, void* vcache,
                                      const int* keep, long ldkeep, const int* pos_ptr, void* out, int B, int nH, int dh, int Tmax,
                                      void* stream) {
    MMTG_REQUIRE(part && bias && splits > 0 && kcache && vcache && keep && pos_ptr && out, "decode_attn_split: null pointer");
    MMTG_REQUIRE(dh == 64 && B > 0 && nH > 0 && Tmax > 0 && Tmax <= 1024, "decode_attn_split: head dim 64, Tmax <= 1024");
    hipStream_t s = (hipStream_t)stream;
    const double esz = dtype == MMTG_F32 ? 4 : 2;
    ProfScope prof(MMTG_PROF_DECODE, s, 4.0 * B * nH * (double)Tmax * dh, esz * 2.0 * B * nH * (double)Tmax * dh);
    dim3 grid(nH, B), block(64);
    const long slab = (long)B * 3 * nH * 64;
    if (dtype == MMTG_F32)
        hipLaunchKernelGGL(decode_attn_kernel<float>, grid, block, 0, s, (const float*)nullptr, (float*)kcache, (float*)vcache, keep, ldkeep, pos_ptr, (float*)out, nH, Tmax, part, splits, slab, bias);
    else if (dtype == MMTG_BF16) {
        static const bool kv_nt = !getenv("MMTG_DECODE_KV_NT") || atoi(getenv("MMTG_DECODE_KV_NT")) != 0;      // default on (700 vs 721 us per token step; =0 for the A/B)
        if (kv_nt) hipLaunchKernelGGL((decode_attn_kernel<bf16, true>), grid, block, 0, s, (const bf16*)nullptr, (bf16*)kcache, (bf16*)vcache, keep, ldkeep, pos_ptr, (bf16*)out, nH, Tmax, part, splits, slab, bias);
        else hipLaunchKernelGGL(decode_attn_kernel<bf16>, grid, block, 0, s, (const bf16*)nullptr, (bf16*)kcache, (bf16*)vcache, keep, ldkeep, pos_ptr, (bf16*)out, nH, Tmax, part, splits, slab, bias);
    } else MMTG_FAIL(MMTG_ERR_BAD_ARG, "decode_attn_split: bad dtype");
    MMTG_LAUNCH_CHECK("decode_attn_split");
    return MMTG_OK;
}

extern "C" int mmtg_decode_attn_split_rows(int dtype, const float* part, int splits, const float* bias, void* kcache, void* vcache,
                                           const int* keep, long ldkeep, const int* rows, long ldrows, const int* pos_ptr, void* out,
                                           int B, int nH, int dh, int Tmax, void* stream) {
    MMTG_REQUIRE(part && bias && splits > 0 && kcache && vcache && keep && rows && pos_ptr && out, "decode_attn_split_rows: null pointer");
    MMTG_REQUIRE(dh == 64 && B > 0 && nH > 0 && Tmax > 0 && Tmax <= 1024 && ldrows >= Tmax,
                 "decode_attn_split_rows: head dim 64, Tmax <= 1024, the ancestry table [B, ldrows >= Tmax]");
    hipStream_t s = (hipStream_t)stream;
    const double esz = dtype == MMTG_F32 ? 4 : 2;
    ProfScope prof(MMTG_PROF_DECODE, s, 4.0 * B * nH * (double)Tmax * dh, esz * 2.0 * B * nH * (double)Tmax * dh);
    dim3 grid(nH, B), block(64);
    const long slab = (long)B * 3 * nH * 64;
    if (dtype == MMTG_F32)
        hipLaunchKernelGGL(decode_attn_rows_kernel<float>, grid, block, 0, s, (float*)kcache, (float*)vcache, keep, ldkeep, rows, ldrows, pos_ptr,
                           (float*)out, nH, Tmax, part, splits, slab, bias, (bf16*)nullptr, 0L);
    else if (dtype == MMTG_BF16) {
        static const bool kv_nt = !getenv("MMTG_DECODE_KV_NT") || atoi(getenv("MMTG_DECODE_KV_NT")) != 0;      // as mmtg_decode_attn_split
        if (kv_nt) hipLaunchKernelGGL((decode_attn_rows_kernel<bf16, true>), grid, block, 0, s, (bf16*)kcache, (bf16*)vcache, keep, ldkeep, rows, ldrows,
                                      pos_ptr, (bf16*)out, nH, Tmax, part, splits, slab, bias, (bf16*)nullptr, 0L);
        else hipLaunchKernelGGL((decode_attn_rows_kernel<bf16, false>), grid, block, 0, s, (bf16*)kcache, (bf16*)vcache, keep, ldkeep, rows, ldrows,
                                pos_ptr, (bf16*)out, nH, Tmax, part, splits, slab, bias, (bf16*)nullptr, 0L);
    } else MMTG_FAIL(MMTG_ERR_BAD_ARG, "decode_attn_split_rows: bad dtype");
    MMTG_LAUNCH_CHECK("decode_attn_split_rows");
    return MMTG_OK;
}

// ---- the selection entries: one launch helper per kernel, taking the entry's rule (NoRule{} for the plain ones)

// dynamic LDS of a selection launch: the count words, the V-float row image (sampling, beam candidates), the rule's staged history
template <typename R>
static size_t select_lds(int V, bool row_image, const R& rule) {
    size_t shm = (size_t)((V + 1) / 2) * 4 + (row_image ? (size_t)V * 4 : 0);
    if constexpr (R::ngram) shm += (size_t)rule.bans().hist_cap * 4;
    return shm;
}

template <typename R>
static int decode_select_launch(const char* what, const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                                int P, int sent, float temperature, float rep_penalty, int top_k, float top_p,
                                const float* uniforms, long ldu, int B, int* pos_next, void* stream, R rule) {
    MMTG_REQUIRE(seq && pos_ptr && B > 0 && sent > 1, "%s: bad args", what);
    MMTG_REQUIRE(pos_next != pos_ptr, "%s: pos_next must not alias pos_ptr (blocks read the position while block 0 writes the next)", what);
    MMTG_REQUIRE(!logits || (V > 0 && ldl >= V && temperature > 0.f && rep_penalty > 0.f), "%s: bad logits args", what);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_DECODE, s, 4.0 * B * V, 4.0 * B * V);
    MMTG_REQUIRE(!logits || V <= (uniforms ? 24000 : 30000), "%s: vocabulary of %d exceeds the LDS tables", what, V);
    const size_t shm = logits ? select_lds(V, uniforms != nullptr, rule) : 0;
    static bool attr_done = false;
    if (!attr_done) {
        if (hipFuncSetAttribute((const void*)decode_select_kernel<R>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096) != hipSuccess)
            MMTG_FAIL(MMTG_ERR_HIP, "%s: cannot raise dynamic LDS", what);
        attr_done = true;
    }
    hipLaunchKernelGGL(decode_select_kernel<R>, dim3(B), dim3(256), shm, s, logits, ldl, V, seq, ldseq,
                       pos_ptr, P, sent, temperature, rep_penalty, logits != nullptr, top_k, top_p, logits ? uniforms : nullptr, ldu, pos_next, rule);
    MMTG_LAUNCH_CHECK(what);
    return MMTG_OK;
}

template <typename R>
static int beam_candidates_launch(const char* what, const float* logits, long ldl, int V, const long long* seq, long ldseq,
                                  const int* pos_ptr, int P, int sent, float temperature, float rep_penalty, int nb, float* cand_val,
                                  int* cand_id, int B, void* stream, R rule) {
    MMTG_REQUIRE(nb >= 1 && nb <= BEAM_MAX, "%s: %d beams per prompt (1..%d)", what, nb, BEAM_MAX);
    MMTG_REQUIRE(logits && seq && pos_ptr && cand_val && cand_id && B > 0 && sent > 1 && V > 0 && ldl >= V,
                 "%s: bad args", what);
    MMTG_REQUIRE(temperature > 0.f && rep_penalty > 0.f, "%s: temperature / penalty must be > 0", what);
    MMTG_REQUIRE(V <= 24000, "%s: vocabulary of %d exceeds the LDS row image (24000)", what, V);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_DECODE, s, 4.0 * B * V, 4.0 * B * V);
    static bool attr_done = false;
    if (!attr_done) {
        if (hipFuncSetAttribute((const void*)beam_candidates_kernel<R>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096) != hipSuccess)
            MMTG_FAIL(MMTG_ERR_HIP, "%s: cannot raise dynamic LDS", what);
        attr_done = true;
    }
    hipLaunchKernelGGL(beam_candidates_kernel<R>, dim3(B), dim3(256), select_lds(V, true, rule), s, logits, ldl, V, seq, ldseq, pos_ptr, P, sent,
                       temperature, rep_penalty, nb, cand_val, cand_id, rule);
    MMTG_LAUNCH_CHECK(what);
    return MMTG_OK;
}

template <typename R>
static int beam_merge_launch(const char* what, const float* cand_val, const int* cand_id, float* scores, long long* seq, long ldseq, int* keep,
                             long ldkeep, int* rows, long ldrows, const int* pos_ptr, int P, int sent, int nb, int n_prompts,
                             int* pos_next, void* stream, R rule) {
    MMTG_REQUIRE(nb >= 1 && nb <= BEAM_MAX, "%s: %d beams per prompt (1..%d)", what, nb, BEAM_MAX);
    MMTG_REQUIRE(scores && seq && keep && rows && pos_ptr && n_prompts > 0 && sent > 1 && ldrows > 0 && (!cand_val || cand_id),
                 "%s: bad args", what);
    MMTG_REQUIRE(pos_next != pos_ptr, "%s: pos_next must not alias pos_ptr", what);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_DECODE, s, (double)n_prompts * nb * nb, 32.0 * n_prompts * nb * (double)ldrows);
    hipLaunchKernelGGL(beam_merge_kernel<R>, dim3(n_prompts), dim3(256), 0, s, cand_val, cand_id, scores, seq, ldseq, keep, ldkeep, rows,
                       ldrows, pos_ptr, P, sent, nb, pos_next, rule);
    MMTG_LAUNCH_CHECK(what);
    return MMTG_OK;
}

// (the grouped merge: groups divides nb, the penalty is finite and >= 0; the plain merge's checks besides)
template <typename R>
static int beam_merge_groups_launch(const char* what, const float* cand_val, const int* cand_id, float* scores, long long* seq, long ldseq,
                                    int* keep, long ldkeep, int* rows, long ldrows, const int* pos_ptr, int P, int sent, int nb,
                                    int n_prompts, int* pos_next, int groups, float diversity_penalty, void* stream, R rule) {
    MMTG_REQUIRE(nb >= 1 && nb <= BEAM_MAX, "%s: %d beams per prompt (1..%d)", what, nb, BEAM_MAX);
    MMTG_REQUIRE(groups >= 1 && nb % groups == 0, "%s: %d groups do not divide %d beams", what, groups, nb);
    MMTG_REQUIRE(diversity_penalty >= 0.f && diversity_penalty < INFINITY, "%s: diversity penalty must be finite and >= 0", what);
    MMTG_REQUIRE(scores && seq && keep && rows && pos_ptr && n_prompts > 0 && sent > 1 && ldrows > 0 && (!cand_val || cand_id),
                 "%s: bad args", what);
    MMTG_REQUIRE(pos_next != pos_ptr, "%s: pos_next must not alias pos_ptr", what);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_DECODE, s, (double)n_prompts * nb * nb, 32.0 * n_prompts * nb * (double)ldrows);
    hipLaunchKernelGGL(beam_merge_groups_kernel<R>, dim3(n_prompts), dim3(256), 0, s, cand_val, cand_id, scores, seq, ldseq, keep, ldkeep,
                       rows, ldrows, pos_ptr, P, sent, nb, pos_next, groups, diversity_penalty, rule);
    MMTG_LAUNCH_CHECK(what);
    return MMTG_OK;
}

// (what every sample_* entry asks of its own arguments)
static int sample_args_check(const char* what, const float* uniforms, long ldu, int B, int top_k, float top_p) {
    MMTG_REQUIRE(uniforms && ldu >= B && top_k >= 0 && top_p >= 0.f, "%s: uniforms [positions, ldu >= B], top_k >= 0, top_p >= 0", what);
    return MMTG_OK;
}

// (the checks every *_ngram entry makes before its launch; the history fits MAXGEN ints of LDS, which the V limits leave room for)
static int ngram_check(const char* what, const float* logits, long ldseq, int P, int sent, int ngram, int* hist_cap) {
    MMTG_REQUIRE(logits, "%s: the n-gram form needs logits", what);
    MMTG_REQUIRE(sent > 2 && ngram >= 1 && ngram <= sent - 2, "%s: n-gram size %d outside 1..%d (sent - 2)", what, ngram, sent - 2);
    MMTG_REQUIRE(ldseq > P && P >= 0, "%s: bad sequence layout (ldseq %ld, P %d)", what, ldseq, P);
    *hist_cap = (int)(ldseq - P < MAXGEN ? ldseq - P : MAXGEN);
    return MMTG_OK;
}

// (the checks every *_lines entry makes before its launch, and its rule; ngram 0 stages no history)
static int lines_check(const char* what, const float* logits, int V, long ldseq, int P, int sent, const int* fixed_end, int ngram,
                       const unsigned char* lo, const unsigned char* hi, int n_lines, const unsigned* sets, int n_sets,
                       const short* set_of, LineRule* lr) {
    MMTG_REQUIRE(logits, "%s: the line form needs logits", what);
    MMTG_REQUIRE(sent > 2 && ngram >= 0 && ngram <= sent - 2, "%s: n-gram size %d outside 0..%d (sent - 2)", what, ngram, sent - 2);
    MMTG_REQUIRE(lo && hi && n_lines >= 1, "%s: lo / hi [B, n_lines >= 1] needed (n_lines %d)", what, n_lines);
    MMTG_REQUIRE(n_sets >= 0 && (n_sets > 0) == (sets != nullptr) && (n_sets > 0) == (set_of != nullptr),
                 "%s: end sets need sets, set_of and n_sets > 0 together (n_sets %d)", what, n_sets);
    int cap = 0;
    if (ngram > 0) {
        if (int e = ngram_check(what, logits, ldseq, P, sent, ngram, &cap)) return e;
    } else MMTG_REQUIRE(ldseq > P && P >= 0, "%s: bad sequence layout (ldseq %ld, P %d)", what, ldseq, P);
    *lr = LineRule{NgramBan{fixed_end, ngram, cap}, lo, hi, set_of, sets, n_lines, n_sets, (V + 31) / 32};
    return MMTG_OK;
}

extern "C" int mmtg_decode_select(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                                  int P, int sent, float temperature, float rep_penalty, int B, int* pos_next, void* stream) {
    return decode_select_launch("decode_select", logits, ldl, V, seq, ldseq, pos_ptr, P, sent, temperature, rep_penalty, 1, 0.f, nullptr, 0, B,
                                pos_next, stream, NoRule{});
}

extern "C" int mmtg_decode_sample(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                                  int P, int sent, float temperature, float rep_penalty, int top_k, float top_p,
                                  const float* uniforms, long ldu, int B, int* pos_next, void* stream) {
    if (int e = sample_args_check("decode_sample", uniforms, ldu, B, top_k, top_p)) return e;
    return decode_select_launch("decode_select", logits, ldl, V, seq, ldseq, pos_ptr, P, sent, temperature, rep_penalty, top_k, top_p, uniforms,
                                ldu, B, pos_next, stream, NoRule{});
}

extern "C" int mmtg_decode_advance(int* pos_ptr, void* stream) {
    MMTG_REQUIRE(pos_ptr, "decode_advance: null pointer");
    hipLaunchKernelGGL(decode_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, pos_ptr);
    MMTG_LAUNCH_CHECK("decode_advance");
    return MMTG_OK;
}

extern "C" int mmtg_decode_beam_candidates(const float* logits, long ldl, int V, const long long* seq, long ldseq, const int* pos_ptr,
                                           int P, int sent, float temperature, float rep_penalty, int nb, float* cand_val, int* cand_id,
                                           int B, void* stream) {
    return beam_candidates_launch("decode_beam_candidates", logits, ldl, V, seq, ldseq, pos_ptr, P, sent, temperature, rep_penalty, nb,
                                  cand_val, cand_id, B, stream, NoRule{});
}

extern "C" int mmtg_decode_beam_merge(const float* cand_val, const int* cand_id, float* scores, long long* seq, long ldseq, int* keep,
                                      long ldkeep, int* rows, long ldrows, const int* pos_ptr, int P, int sent, int nb, int n_prompts,
                                      int* pos_next, void* stream) {
    return beam_merge_launch("decode_beam_merge", cand_val, cand_id, scores, seq, ldseq, keep, ldkeep, rows, ldrows, pos_ptr, P, sent, nb,
                             n_prompts, pos_next, stream, NoRule{});
}

extern "C" int mmtg_decode_select_fixed(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                                        int P, int sent, float temperature, float rep_penalty, int B, int* pos_next, const int* fixed_end,
                                        void* stream) {
    MMTG_REQUIRE(fixed_end, "decode_select_fixed: null fixed_end");
    return decode_select_launch("decode_select_fixed", logits, ldl, V, seq, ldseq, pos_ptr, P, sent, temperature, rep_penalty, 1, 0.f, nullptr,
                                0, B, pos_next, stream, FixedEnd{fixed_end});
}

extern "C" int mmtg_decode_sample_fixed(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                                        int P, int sent, float temperature, float rep_penalty, int top_k, float top_p,
                                        const float* uniforms, long ldu, int B, int* pos_next, const int* fixed_end, void* stream) {
    MMTG_REQUIRE(fixed_end, "decode_sample_fixed: null fixed_end");
    if (int e = sample_args_check("decode_sample_fixed", uniforms, ldu, B, top_k, top_p)) return e;
    return decode_select_launch("decode_select_fixed", logits, ldl, V, seq, ldseq, pos_ptr, P, sent, temperature, rep_penalty, top_k, top_p,
                                uniforms, ldu, B, pos_next, stream, FixedEnd{fixed_end});
}

extern "C" int mmtg_decode_beam_candidates_fixed(const float* logits, long ldl, int V, const long long* seq, long ldseq, const int* pos_ptr,
                                                 int P, int sent, float temperature, float rep_penalty, int nb, float* cand_val, int* cand_id,
                                                 int B, const int* fixed_end, void* stream) {
    MMTG_REQUIRE(fixed_end, "decode_beam_candidates_fixed: null fixed_end");
    return beam_candidates_launch("decode_beam_candidates_fixed", logits, ldl, V, seq, ldseq, pos_ptr, P, sent, temperature, rep_penalty,
                                  nb, cand_val, cand_id, B, stream, FixedEnd{fixed_end});
}

extern "C" int mmtg_decode_beam_merge_fixed(const float* cand_val, const int* cand_id, float* scores, long long* seq, long ldseq, int* keep,
                                            long ldkeep, int* rows, long ldrows, const int* pos_ptr, int P, int sent, int nb, int n_prompts,
                                            int* pos_next, const int* fixed_end, void* stream) {
    MMTG_REQUIRE(fixed_end, "decode_beam_merge_fixed: null fixed_end");
    return beam_merge_launch("decode_beam_merge_fixed", cand_val, cand_id, scores, seq, ldseq, keep, ldkeep, rows, ldrows, pos_ptr, P, sent,
                             nb, n_prompts, pos_next, stream, FixedEnd{fixed_end});
}

extern "C" int mmtg_decode_beam_merge_groups(const float* cand_val, const int* cand_id, float* scores, long long* seq, long ldseq, int* keep,
                                             long ldkeep, int* rows, long ldrows, const int* pos_ptr, int P, int sent, int nb, int n_prompts,
                                             int* pos_next, int groups, float diversity_penalty, void* stream) {
    return beam_merge_groups_launch("decode_beam_merge_groups", cand_val, cand_id, scores, seq, ldseq, keep, ldkeep, rows, ldrows, pos_ptr, P,
                                    sent, nb, n_prompts, pos_next, groups, diversity_penalty, stream, NoRule{});
}

extern "C" int mmtg_decode_beam_merge_groups_fixed(const float* cand_val, const int* cand_id, float* scores, long long* seq, long ldseq,
                                                   int* keep, long ldkeep, int* rows, long ldrows, const int* pos_ptr, int P, int sent, int nb,
                                                   int n_prompts, int* pos_next, const int* fixed_end, int groups, float diversity_penalty,
                                                   void* stream) {
    MMTG_REQUIRE(fixed_end, "decode_beam_merge_groups_fixed: null fixed_end");
    return beam_merge_groups_launch("decode_beam_merge_groups_fixed", cand_val, cand_id, scores, seq, ldseq, keep, ldkeep, rows, ldrows,
                                    pos_ptr, P, sent, nb, n_prompts, pos_next, groups, diversity_penalty, stream, FixedEnd{fixed_end});
}

extern "C" int mmtg_decode_select_ngram(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                                        int P, int sent, float temperature, float rep_penalty, int B, int* pos_next, const int* fixed_end,
                                        int ngram, void* stream) {
    int cap = 0;
    if (int e = ngram_check("decode_select_ngram", logits, ldseq, P, sent, ngram, &cap)) return e;
    return decode_select_launch("decode_select_ngram", logits, ldl, V, seq, ldseq, pos_ptr, P, sent, temperature, rep_penalty, 1, 0.f, nullptr,
                                0, B, pos_next, stream, NgramBan{fixed_end, ngram, cap});
}

extern "C" int mmtg_decode_sample_ngram(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                                        int P, int sent, float temperature, float rep_penalty, int top_k, float top_p,
                                        const float* uniforms, long ldu, int B, int* pos_next, const int* fixed_end, int ngram,
                                        void* stream) {
    int cap = 0;
    if (int e = ngram_check("decode_sample_ngram", logits, ldseq, P, sent, ngram, &cap)) return e;
    if (int e = sample_args_check("decode_sample_ngram", uniforms, ldu, B, top_k, top_p)) return e;
    return decode_select_launch("decode_sample_ngram", logits, ldl, V, seq, ldseq, pos_ptr, P, sent, temperature, rep_penalty, top_k, top_p,
                                uniforms, ldu, B, pos_next, stream, NgramBan{fixed_end, ngram, cap});
}

extern "C" int mmtg_decode_beam_candidates_ngram(const float* logits, long ldl, int V, const long long* seq, long ldseq, const int* pos_ptr,
                                                 int P, int sent, float temperature, float rep_penalty, int nb, float* cand_val, int* cand_id,
                                                 int B, const int* fixed_end, int ngram, void* stream) {
    int cap = 0;
    if (int e = ngram_check("decode_beam_candidates_ngram", logits, ldseq, P, sent, ngram, &cap)) return e;
    return beam_candidates_launch("decode_beam_candidates_ngram", logits, ldl, V, seq, ldseq, pos_ptr, P, sent, temperature, rep_penalty,
                                  nb, cand_val, cand_id, B, stream, NgramBan{fixed_end, ngram, cap});
}

extern "C" int mmtg_decode_select_lines(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                                        int P, int sent, float temperature, float rep_penalty, int B, int* pos_next, const int* fixed_end,
                                        int ngram, const unsigned char* lo, const unsigned char* hi, int n_lines, const unsigned* sets,
                                        int n_sets, const short* set_of, void* stream) {
    LineRule lr;
    if (int e = lines_check("decode_select_lines", logits, V, ldseq, P, sent, fixed_end, ngram, lo, hi, n_lines, sets, n_sets, set_of, &lr))
        return e;
    return decode_select_launch("decode_select_lines", logits, ldl, V, seq, ldseq, pos_ptr, P, sent, temperature, rep_penalty, 1, 0.f, nullptr,
                                0, B, pos_next, stream, lr);
}

extern "C" int mmtg_decode_sample_lines(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                                        int P, int sent, float temperature, float rep_penalty, int top_k, float top_p,
                                        const float* uniforms, long ldu, int B, int* pos_next, const int* fixed_end, int ngram,
                                        const unsigned char* lo, const unsigned char* hi, int n_lines, const unsigned* sets, int n_sets,
                                        const short* set_of, void* stream) {
    LineRule lr;
    if (int e = lines_check("decode_sample_lines", logits, V, ldseq, P, sent, fixed_end, ngram, lo, hi, n_lines, sets, n_sets, set_of, &lr))
        return e;
    if (int e = sample_args_check("decode_sample_lines", uniforms, ldu, B, top_k, top_p)) return e;
    return decode_select_launch("decode_sample_lines", logits, ldl, V, seq, ldseq, pos_ptr, P, sent, temperature, rep_penalty, top_k, top_p,
                                uniforms, ldu, B, pos_next, stream, lr);
}

extern "C" int mmtg_decode_beam_candidates_lines(const float* logits, long ldl, int V, const long long* seq, long ldseq, const int* pos_ptr,
                                                 int P, int sent, float temperature, float rep_penalty, int nb, float* cand_val, int* cand_id,
                                                 int B, const int* fixed_end, int ngram, const unsigned char* lo, const unsigned char* hi,
                                                 int n_lines, const unsigned* sets, int n_sets, const short* set_of, void* stream) {
    LineRule lr;
    if (int e = lines_check("decode_beam_candidates_lines", logits, V, ldseq, P, sent, fixed_end, ngram, lo, hi, n_lines, sets, n_sets,
                            set_of, &lr))
        return e;
    return beam_candidates_launch("decode_beam_candidates_lines", logits, ldl, V, seq, ldseq, pos_ptr, P, sent, temperature, rep_penalty,
                                  nb, cand_val, cand_id, B, stream, lr);
}

// (a *_tmpl entry's checks: its *_lines namesake's, and the table)
static int tmpl_check(const char* what, const float* logits, int V, long ldseq, int P, int sent, const int* fixed_end, int ngram,
                      const unsigned char* lo, const unsigned char* hi, int n_lines, const unsigned* sets, int n_sets,
                      const short* set_of, const int* tmpl, TemplateRule* tr) {
    LineRule lr;
    if (int e = lines_check(what, logits, V, ldseq, P, sent, fixed_end, ngram, lo, hi, n_lines, sets, n_sets, set_of, &lr)) return e;
    MMTG_REQUIRE(tmpl, "%s: the template table [B, n_lines, sent - 2] is needed", what);
    *tr = TemplateRule{lr, tmpl};
    return MMTG_OK;
}

extern "C" int mmtg_decode_select_tmpl(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                                       int P, int sent, float temperature, float rep_penalty, int B, int* pos_next, const int* fixed_end,
                                       int ngram, const unsigned char* lo, const unsigned char* hi, int n_lines, const unsigned* sets,
                                       int n_sets, const short* set_of, const int* tmpl, void* stream) {
    TemplateRule tr;
    if (int e = tmpl_check("decode_select_tmpl", logits, V, ldseq, P, sent, fixed_end, ngram, lo, hi, n_lines, sets, n_sets, set_of, tmpl, &tr))
        return e;
    return decode_select_launch("decode_select_tmpl", logits, ldl, V, seq, ldseq, pos_ptr, P, sent, temperature, rep_penalty, 1, 0.f, nullptr,
                                0, B, pos_next, stream, tr);
}

extern "C" int mmtg_decode_sample_tmpl(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                                       int P, int sent, float temperature, float rep_penalty, int top_k, float top_p,
                                       const float* uniforms, long ldu, int B, int* pos_next, const int* fixed_end, int ngram,
                                       const unsigned char* lo, const unsigned char* hi, int n_lines, const unsigned* sets, int n_sets,
                                       const short* set_of, const int* tmpl, void* stream) {
    TemplateRule tr;
    if (int e = tmpl_check("decode_sample_tmpl", logits, V, ldseq, P, sent, fixed_end, ngram, lo, hi, n_lines, sets, n_sets, set_of, tmpl, &tr))
        return e;
    if (int e = sample_args_check("decode_sample_tmpl", uniforms, ldu, B, top_k, top_p)) return e;
    return decode_select_launch("decode_sample_tmpl", logits, ldl, V, seq, ldseq, pos_ptr, P, sent, temperature, rep_penalty, top_k, top_p,
                                uniforms, ldu, B, pos_next, stream, tr);
}

extern "C" int mmtg_decode_beam_candidates_tmpl(const float* logits, long ldl, int V, const long long* seq, long ldseq, const int* pos_ptr,
                                                int P, int sent, float temperature, float rep_penalty, int nb, float* cand_val, int* cand_id,
                                                int B, const int* fixed_end, int ngram, const unsigned char* lo, const unsigned char* hi,
                                                int n_lines, const unsigned* sets, int n_sets, const short* set_of, const int* tmpl,
                                                void* stream) {
    TemplateRule tr;
    if (int e = tmpl_check("decode_beam_candidates_tmpl", logits, V, ldseq, P, sent, fixed_end, ngram, lo, hi, n_lines, sets, n_sets,
                           set_of, tmpl, &tr))
        return e;
    return beam_candidates_launch("decode_beam_candidates_tmpl", logits, ldl, V, seq, ldseq, pos_ptr, P, sent, temperature, rep_penalty,
                                  nb, cand_val, cand_id, B, stream, tr);
}

// (a *_rhyme entry's checks: its *_lines namesake's -- the template table is optional here -- and the rhyme tables)
static int rhyme_check(const char* what, const float* logits, int V, long ldseq, int P, int sent, const int* fixed_end, int ngram,
                       const unsigned char* lo, const unsigned char* hi, int n_lines, const unsigned* sets, int n_sets,
                       const short* set_of, const int* tmpl, const short* class_of, const signed char* lead, int distinct,
                       RhymeRule* rr) {
    LineRule lr;
    if (int e = lines_check(what, logits, V, ldseq, P, sent, fixed_end, ngram, lo, hi, n_lines, sets, n_sets, set_of, &lr)) return e;
    MMTG_REQUIRE(class_of && lead, "%s: class_of [V] and lead [B, n_lines] are needed", what);
    MMTG_REQUIRE(n_sets > 0, "%s: rhyme classes are rows of sets (n_sets %d)", what, n_sets);
    MMTG_REQUIRE(n_lines <= 128, "%s: %d lines, a leader's line index must fit a signed char (128)", what, n_lines);
    MMTG_REQUIRE(distinct == 0 || distinct == 1, "%s: distinct is 0 or 1 (got %d)", what, distinct);
    *rr = RhymeRule{TemplateRule{lr, tmpl}, class_of, lead, distinct, V};
    return MMTG_OK;
}

extern "C" int mmtg_decode_select_rhyme(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                                        int P, int sent, float temperature, float rep_penalty, int B, int* pos_next, const int* fixed_end,
                                        int ngram, const unsigned char* lo, const unsigned char* hi, int n_lines, const unsigned* sets,
                                        int n_sets, const short* set_of, const int* tmpl, const short* class_of,
                                        const signed char* lead, int distinct, void* stream) {
    RhymeRule rr;
    if (int e = rhyme_check("decode_select_rhyme", logits, V, ldseq, P, sent, fixed_end, ngram, lo, hi, n_lines, sets, n_sets, set_of, tmpl,
                            class_of, lead, distinct, &rr))
        return e;
    return decode_select_launch("decode_select_rhyme", logits, ldl, V, seq, ldseq, pos_ptr, P, sent, temperature, rep_penalty, 1, 0.f, nullptr,
                                0, B, pos_next, stream, rr);
}

extern "C" int mmtg_decode_sample_rhyme(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                                        int P, int sent, float temperature, float rep_penalty, int top_k, float top_p,
                                        const float* uniforms, long ldu, int B, int* pos_next, const int* fixed_end, int ngram,
                                        const unsigned char* lo, const unsigned char* hi, int n_lines, const unsigned* sets, int n_sets,
                                        const short* set_of, const int* tmpl, const short* class_of, const signed char* lead,
                                        int distinct, void* stream) {
    RhymeRule rr;
    if (int e = rhyme_check("decode_sample_rhyme", logits, V, ldseq, P, sent, fixed_end, ngram, lo, hi, n_lines, sets, n_sets, set_of, tmpl,
                            class_of, lead, distinct, &rr))
        return e;
    if (int e = sample_args_check("decode_sample_rhyme", uniforms, ldu, B, top_k, top_p)) return e;
    return decode_select_launch("decode_sample_rhyme", logits, ldl, V, seq, ldseq, pos_ptr, P, sent, temperature, rep_penalty, top_k, top_p,
                                uniforms, ldu, B, pos_next, stream, rr);
}

extern "C" int mmtg_decode_beam_candidates_rhyme(const float* logits, long ldl, int V, const long long* seq, long ldseq, const int* pos_ptr,
                                                 int P, int sent, float temperature, float rep_penalty, int nb, float* cand_val, int* cand_id,
                                                 int B, const int* fixed_end, int ngram, const unsigned char* lo, const unsigned char* hi,
                                                 int n_lines, const unsigned* sets, int n_sets, const short* set_of, const int* tmpl,
                                                 const short* class_of, const signed char* lead, int distinct, void* stream) {
    RhymeRule rr;
    if (int e = rhyme_check("decode_beam_candidates_rhyme", logits, V, ldseq, P, sent, fixed_end, ngram, lo, hi, n_lines, sets, n_sets,
                            set_of, tmpl, class_of, lead, distinct, &rr))
        return e;
    return beam_candidates_launch("decode_beam_candidates_rhyme", logits, ldl, V, seq, ldseq, pos_ptr, P, sent, temperature, rep_penalty,
                                  nb, cand_val, cand_id, B, stream, rr);
}

// (a *_refrain entry's checks: src, and the rhyme form's tables where they are given -- lo / hi null: no line rule, then every other
// table is null too; class_of / lead null: no rhyme scheme.  Logits are not asked for here: the select entry runs without them)
static int refrain_check(const char* what, int V, long ldseq, int P, int sent, const int* fixed_end, int ngram, const unsigned char* lo,
                         const unsigned char* hi, int n_lines, const unsigned* sets, int n_sets, const short* set_of, const int* tmpl,
                         const short* class_of, const signed char* lead, int distinct, const signed char* src, RefrainRule* rf) {
    MMTG_REQUIRE(src, "%s: src [B, n_lines] is needed", what);
    MMTG_REQUIRE(n_lines >= 1 && n_lines <= 128, "%s: %d lines, a source's line index must fit a signed char (1..128)", what, n_lines);
    MMTG_REQUIRE(sent > 2 && ngram >= 0 && ngram <= sent - 2, "%s: n-gram size %d outside 0..%d (sent - 2)", what, ngram, sent - 2);
    MMTG_REQUIRE(ldseq > P && P >= 0 && V >= 0, "%s: bad sequence layout (ldseq %ld, P %d)", what, ldseq, P);
    MMTG_REQUIRE((lo != nullptr) == (hi != nullptr), "%s: lo and hi come together", what);
    MMTG_REQUIRE(n_sets >= 0 && (n_sets > 0) == (sets != nullptr) && (n_sets > 0) == (set_of != nullptr),
                 "%s: end sets need sets, set_of and n_sets > 0 together (n_sets %d)", what, n_sets);
    MMTG_REQUIRE(lo || (!sets && !tmpl && !class_of && !lead), "%s: line tables without lo / hi", what);
    MMTG_REQUIRE((class_of != nullptr) == (lead != nullptr), "%s: class_of [V] and lead [B, n_lines] come together", what);
    MMTG_REQUIRE(!lead || n_sets > 0, "%s: rhyme classes are rows of sets (n_sets %d)", what, n_sets);
    MMTG_REQUIRE(distinct == 0 || (distinct == 1 && lead), "%s: distinct is 0 or, with a rhyme scheme, 1 (got %d)", what, distinct);
    const int cap = ngram > 0 ? (int)(ldseq - P < MAXGEN ? ldseq - P : MAXGEN) : 0;
    *rf = RefrainRule{RhymeRule{TemplateRule{LineRule{NgramBan{fixed_end, ngram, cap}, lo, hi, set_of, sets, n_lines, n_sets, (V + 31) / 32},
                                             tmpl}, class_of, lead, distinct, V}, src};
    return MMTG_OK;
}

extern "C" int mmtg_decode_select_refrain(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                                          int P, int sent, float temperature, float rep_penalty, int B, int* pos_next, const int* fixed_end,
                                          int ngram, const unsigned char* lo, const unsigned char* hi, int n_lines, const unsigned* sets,
                                          int n_sets, const short* set_of, const int* tmpl, const short* class_of,
                                          const signed char* lead, int distinct, const signed char* src, void* stream) {
    RefrainRule rf;
    if (int e = refrain_check("decode_select_refrain", V, ldseq, P, sent, fixed_end, ngram, lo, hi, n_lines, sets, n_sets, set_of, tmpl,
                              class_of, lead, distinct, src, &rf))
        return e;
    return decode_select_launch("decode_select_refrain", logits, ldl, V, seq, ldseq, pos_ptr, P, sent, temperature, rep_penalty, 1, 0.f,
                                nullptr, 0, B, pos_next, stream, rf);
}

extern "C" int mmtg_decode_sample_refrain(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                                          int P, int sent, float temperature, float rep_penalty, int top_k, float top_p,
                                          const float* uniforms, long ldu, int B, int* pos_next, const int* fixed_end, int ngram,
                                          const unsigned char* lo, const unsigned char* hi, int n_lines, const unsigned* sets, int n_sets,
                                          const short* set_of, const int* tmpl, const short* class_of, const signed char* lead,
                                          int distinct, const signed char* src, void* stream) {
    RefrainRule rf;
    MMTG_REQUIRE(logits, "decode_sample_refrain: a draw needs logits");
    if (int e = refrain_check("decode_sample_refrain", V, ldseq, P, sent, fixed_end, ngram, lo, hi, n_lines, sets, n_sets, set_of, tmpl,
                              class_of, lead, distinct, src, &rf))
        return e;
    if (int e = sample_args_check("decode_sample_refrain", uniforms, ldu, B, top_k, top_p)) return e;
    return decode_select_launch("decode_sample_refrain", logits, ldl, V, seq, ldseq, pos_ptr, P, sent, temperature, rep_penalty, top_k, top_p,
                                uniforms, ldu, B, pos_next, stream, rf);
}

extern "C" int mmtg_decode_sample_warp(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                                       int P, int sent, float temperature, float rep_penalty, int top_k, float top_p, float min_p,
                                       float typical_p, float epsilon_cutoff, float eta_cutoff, const float* uniforms, long ldu, int B,
                                       int* pos_next, const int* fixed_end, int ngram, const unsigned char* lo, const unsigned char* hi,
                                       int n_lines, const unsigned* sets, int n_sets, const short* set_of, const int* tmpl,
                                       const short* class_of, const signed char* lead, int distinct, const signed char* src,
                                       void* stream) {
    RefrainRule rf;
    MMTG_REQUIRE(logits, "decode_sample_warp: a draw needs logits");
    if (int e = refrain_check("decode_sample_warp", V, ldseq, P, sent, fixed_end, ngram, lo, hi, n_lines, sets, n_sets, set_of, tmpl,
                              class_of, lead, distinct, src, &rf))
        return e;
    if (int e = sample_args_check("decode_sample_warp", uniforms, ldu, B, top_k, top_p)) return e;
    if (int e = warp_args_check("decode_sample_warp", min_p, typical_p, epsilon_cutoff, eta_cutoff)) return e;
    MMTG_REQUIRE(seq && pos_ptr && B > 0, "decode_sample_warp: bad args");
    MMTG_REQUIRE(pos_next != pos_ptr, "decode_sample_warp: pos_next must not alias pos_ptr (blocks read the position while block 0 writes the next)");
    MMTG_REQUIRE(V > 0 && ldl >= V && temperature > 0.f && rep_penalty > 0.f, "decode_sample_warp: bad logits args");
    MMTG_REQUIRE(V <= 24000, "decode_sample_warp: vocabulary of %d exceeds the LDS tables", V);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_DECODE, s, 40.0 * B * V, 4.0 * B * V);
    static bool attr_done = false;
    if (!attr_done) {
        if (hipFuncSetAttribute((const void*)decode_select_warp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096) != hipSuccess)
            MMTG_FAIL(MMTG_ERR_HIP, "decode_sample_warp: cannot raise dynamic LDS");
        attr_done = true;
    }
    hipLaunchKernelGGL(decode_select_warp_kernel, dim3(B), dim3(256), select_lds(V, true, rf), s, logits, ldl, V, seq, ldseq, pos_ptr, P,
                       sent, temperature, rep_penalty, top_k, top_p, min_p, typical_p, epsilon_cutoff, eta_cutoff, uniforms, ldu, pos_next,
                       rf);
    MMTG_LAUNCH_CHECK("decode_sample_warp");
    return MMTG_OK;
}

extern "C" int mmtg_decode_sample_mirostat(const float* logits, long ldl, int V, long long* seq, long ldseq, const int* pos_ptr,
                                           int P, int sent, float temperature, float rep_penalty, int top_k, float top_p, float min_p,
                                           float typical_p, float epsilon_cutoff, float eta_cutoff, const float* uniforms, long ldu,
                                           int B, int* pos_next, const int* fixed_end, int ngram, const unsigned char* lo,
                                           const unsigned char* hi, int n_lines, const unsigned* sets, int n_sets, const short* set_of,
                                           const int* tmpl, const short* class_of, const signed char* lead, int distinct,
                                           const signed char* src, float mirostat_tau, float mirostat_eta, float* mu, void* stream) {
    RefrainRule rf;
    if (int e = mirostat_args_check("decode_sample_mirostat", mirostat_tau, mirostat_eta, mu)) return e;
    MMTG_REQUIRE(logits, "decode_sample_mirostat: a draw needs logits");
    if (int e = refrain_check("decode_sample_mirostat", V, ldseq, P, sent, fixed_end, ngram, lo, hi, n_lines, sets, n_sets, set_of, tmpl,
                              class_of, lead, distinct, src, &rf))
        return e;
    if (int e = sample_args_check("decode_sample_mirostat", uniforms, ldu, B, top_k, top_p)) return e;
    if (int e = warp_args_check("decode_sample_mirostat", min_p, typical_p, epsilon_cutoff, eta_cutoff)) return e;
    MMTG_REQUIRE(seq && pos_ptr && B > 0, "decode_sample_mirostat: bad args");
    MMTG_REQUIRE(pos_next != pos_ptr, "decode_sample_mirostat: pos_next must not alias pos_ptr (blocks read the position while block 0 writes the next)");
    MMTG_REQUIRE(V > 0 && ldl >= V && temperature > 0.f && rep_penalty > 0.f, "decode_sample_mirostat: bad logits args");
    MMTG_REQUIRE(V <= 24000, "decode_sample_mirostat: vocabulary of %d exceeds the LDS tables", V);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_DECODE, s, 44.0 * B * V, 4.0 * B * V);
    static bool attr_done = false;
    if (!attr_done) {
        if (hipFuncSetAttribute((const void*)decode_select_mirostat_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096) != hipSuccess)
            MMTG_FAIL(MMTG_ERR_HIP, "decode_sample_mirostat: cannot raise dynamic LDS");
        attr_done = true;
    }
    hipLaunchKernelGGL(decode_select_mirostat_kernel, dim3(B), dim3(256), select_lds(V, true, rf), s, logits, ldl, V, seq, ldseq, pos_ptr,
                       P, sent, temperature, rep_penalty, top_k, top_p, min_p, typical_p, epsilon_cutoff, eta_cutoff, mirostat_tau,
                       mirostat_eta, mu, uniforms, ldu, pos_next, rf);
    MMTG_LAUNCH_CHECK("decode_sample_mirostat");
    return MMTG_OK;
}

extern "C" int mmtg_decode_beam_candidates_refrain(const float* logits, long ldl, int V, const long long* seq, long ldseq,
                                                   const int* pos_ptr, int P, int sent, float temperature, float rep_penalty, int nb,
                                                   float* cand_val, int* cand_id, int B, const int* fixed_end, int ngram,
                                                   const unsigned char* lo, const unsigned char* hi, int n_lines, const unsigned* sets,
                                                   int n_sets, const short* set_of, const int* tmpl, const short* class_of,
                                                   const signed char* lead, int distinct, const signed char* src, void* stream) {
    RefrainRule rf;
    if (int e = refrain_check("decode_beam_candidates_refrain", V, ldseq, P, sent, fixed_end, ngram, lo, hi, n_lines, sets, n_sets, set_of,
                              tmpl, class_of, lead, distinct, src, &rf))
        return e;
    return beam_candidates_launch("decode_beam_candidates_refrain", logits, ldl, V, seq, ldseq, pos_ptr, P, sent, temperature, rep_penalty,
                                  nb, cand_val, cand_id, B, stream, rf);
}

// (what every *_kw entry asks of K and nb: one merge workgroup holds a candidate per thread)
static int kw_check(const char* what, int nb, int K) {
    MMTG_REQUIRE(nb >= 1 && nb <= BEAM_MAX, "%s: %d beams per prompt (1..%d)", what, nb, BEAM_MAX);
    MMTG_REQUIRE(K >= 0 && K <= KW_MAX, "%s: %d keywords per prompt (0..%d)", what, K, KW_MAX);
    MMTG_REQUIRE(nb * (nb + K) <= 256, "%s: %d beams x (%d beams + %d keywords) candidates exceed the merge workgroup (256)", what, nb, nb, K);
    return MMTG_OK;
}

extern "C" int mmtg_decode_beam_candidates_kw(const float* logits, long ldl, int V, const long long* seq, long ldseq, const int* pos_ptr,
                                              int P, int sent, float temperature, float rep_penalty, int nb, float* cand_val, int* cand_id,
                                              int B, const int* fixed_end, int ngram, const unsigned char* lo, const unsigned char* hi,
                                              int n_lines, const unsigned* sets, int n_sets, const short* set_of, const int* tmpl,
                                              const short* class_of, const signed char* lead, int distinct, const int* phrases,
                                              const signed char* phrase_len, int K, int phrase_cap, int* cand_bank, void* stream) {
    const char* what = "decode_beam_candidates_kw";
    if (int e = kw_check(what, nb, K)) return e;
    MMTG_REQUIRE(cand_bank, "%s: null cand_bank", what);
    MMTG_REQUIRE(K == 0 || (phrases && phrase_len), "%s: phrases [prompts, %d, %d] and phrase_len [prompts, %d] are needed", what, KW_MAX,
                 KW_LEN, KW_MAX);
    MMTG_REQUIRE(K == 0 || (phrase_cap >= 1 && phrase_cap <= KW_LEN), "%s: phrase length %d outside 1..%d", what, phrase_cap, KW_LEN);
    MMTG_REQUIRE(logits && seq && pos_ptr && cand_val && cand_id && B > 0 && B % nb == 0 && sent > 2 && V > 0 && ldl >= V, "%s: bad args", what);
    MMTG_REQUIRE(temperature > 0.f && rep_penalty > 0.f, "%s: temperature / penalty must be > 0", what);
    MMTG_REQUIRE(V <= 24000, "%s: vocabulary of %d exceeds the LDS row image (24000)", what, V);
    RhymeRule rr;
    if (n_lines == 0) {         // no line rule at all: the rhyme form with empty tables constrains nothing (every line is past n_lines)
        MMTG_REQUIRE(!lo && !hi && !sets && !set_of && !tmpl && !class_of && !lead && n_sets == 0 && distinct == 0,
                     "%s: line tables without lines (n_lines 0)", what);
        MMTG_REQUIRE(ngram >= 0 && ngram <= sent - 2, "%s: n-gram size %d outside 0..%d (sent - 2)", what, ngram, sent - 2);
        int cap = 0;
        if (ngram > 0) {
            if (int e = ngram_check(what, logits, ldseq, P, sent, ngram, &cap)) return e;
        } else MMTG_REQUIRE(ldseq > P && P >= 0, "%s: bad sequence layout (ldseq %ld, P %d)", what, ldseq, P);
        rr = RhymeRule{TemplateRule{LineRule{NgramBan{fixed_end, ngram, cap}, nullptr, nullptr, nullptr, nullptr, 0, 0, (V + 31) / 32}, nullptr},
                       nullptr, nullptr, 0, V};
    } else {                    // the *_rhyme entry's tables, except that the classes may be absent when no line has a leader
        LineRule lr;
        if (int e = lines_check(what, logits, V, ldseq, P, sent, fixed_end, ngram, lo, hi, n_lines, sets, n_sets, set_of, &lr)) return e;
        MMTG_REQUIRE(class_of && lead, "%s: class_of [V] and lead [B, n_lines] are needed", what);
        MMTG_REQUIRE(n_lines <= 128, "%s: %d lines, a leader's line index must fit a signed char (128)", what, n_lines);
        MMTG_REQUIRE(distinct == 0 || distinct == 1, "%s: distinct is 0 or 1 (got %d)", what, distinct);
        rr = RhymeRule{TemplateRule{lr, tmpl}, class_of, lead, distinct, V};
    }
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_DECODE, s, 4.0 * B * V, 4.0 * B * V);
    static bool attr_done = false;
    if (!attr_done) {
        if (hipFuncSetAttribute((const void*)beam_candidates_kw_kernel<RhymeRule>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096) != hipSuccess)
            MMTG_FAIL(MMTG_ERR_HIP, "%s: cannot raise dynamic LDS", what);
        attr_done = true;
    }
    hipLaunchKernelGGL(beam_candidates_kw_kernel<RhymeRule>, dim3(B), dim3(256), select_lds(V, true, rr), s, logits, ldl, V, seq, ldseq, pos_ptr, P, sent,
                       temperature, rep_penalty, nb, cand_val, cand_id, rr, Keywords{phrases, phrase_len, K, K ? phrase_cap : 0, cand_bank});
    MMTG_LAUNCH_CHECK(what);
    return MMTG_OK;
}

template <typename R>
static int beam_merge_kw_launch(const char* what, const float* cand_val, const int* cand_id, const int* cand_bank, float* scores,
                                long long* seq, long ldseq, int* keep, long ldkeep, int* rows, long ldrows, const int* pos_ptr, int P,
                                int sent, int nb, int n_prompts, int* pos_next, int K, void* stream, R rule) {
    if (int e = kw_check(what, nb, K)) return e;
    MMTG_REQUIRE(scores && seq && keep && rows && pos_ptr && n_prompts > 0 && sent > 1 && ldrows > 0 && (!cand_val || (cand_id && cand_bank)),
                 "%s: bad args", what);
    MMTG_REQUIRE(pos_next != pos_ptr, "%s: pos_next must not alias pos_ptr", what);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_DECODE, s, (double)n_prompts * nb * (nb + K), 32.0 * n_prompts * nb * (double)ldrows);
    hipLaunchKernelGGL(beam_merge_kw_kernel<R>, dim3(n_prompts), dim3(256), 0, s, cand_val, cand_id, cand_bank, scores, seq, ldseq, keep, ldkeep,
                       rows, ldrows, pos_ptr, P, sent, nb, pos_next, K, rule);
    MMTG_LAUNCH_CHECK(what);
    return MMTG_OK;
}

extern "C" int mmtg_decode_beam_merge_kw(const float* cand_val, const int* cand_id, const int* cand_bank, float* scores, long long* seq,
                                         long ldseq, int* keep, long ldkeep, int* rows, long ldrows, const int* pos_ptr, int P, int sent,
                                         int nb, int n_prompts, int* pos_next, int K, void* stream) {
    return beam_merge_kw_launch("decode_beam_merge_kw", cand_val, cand_id, cand_bank, scores, seq, ldseq, keep, ldkeep, rows, ldrows, pos_ptr, P,
                                sent, nb, n_prompts, pos_next, K, stream, NoRule{});
}

extern "C" int mmtg_decode_beam_merge_kw_fixed(const float* cand_val, const int* cand_id, const int* cand_bank, float* scores, long long* seq,
                                               long ldseq, int* keep, long ldkeep, int* rows, long ldrows, const int* pos_ptr, int P,
                                               int sent, int nb, int n_prompts, int* pos_next, const int* fixed_end, int K, void* stream) {
    MMTG_REQUIRE(fixed_end, "decode_beam_merge_kw_fixed: null fixed_end");
    return beam_merge_kw_launch("decode_beam_merge_kw_fixed", cand_val, cand_id, cand_bank, scores, seq, ldseq, keep, ldkeep, rows, ldrows,
                                pos_ptr, P, sent, nb, n_prompts, pos_next, K, stream, FixedEnd{fixed_end});
}

extern "C" int mmtg_ln_fold_weights(const void* W, long ldw, const float* gamma, const float* beta, const float* bias, void* Wf,
                                    float* colsum, float* bias_f, int N, int K, void* stream) {
    MMTG_REQUIRE(W && gamma && beta && Wf && colsum && bias_f && N > 0 && K > 0 && K % 8 == 0 && ldw % 8 == 0 && ldw >= K,
                 "ln_fold_weights: bad arguments (K, ldw multiples of 8)");
    MMTG_REQUIRE(MMTG_ALIGNED16(W) && MMTG_ALIGNED16(Wf), "ln_fold_weights: 16-byte alignment");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_MISC, s, 3.0 * N * (double)K, 4.0 * N * (double)K);
    hipLaunchKernelGGL(ln_fold_kernel, dim3(cdiv(N, 4)), dim3(256), 0, s, (const bf16*)W, ldw, gamma, beta, bias, (bf16*)Wf, colsum, bias_f, N, K);
    MMTG_LAUNCH_CHECK("ln_fold_weights");
    return MMTG_OK;
}

static int dg_fill(DgArgs& a, int mode, int M, int N, int K, const void* A, long lda, const void* W, long ldw, void* C, long ldc,
                   const float* bias, const float* colsum, const float* stats_in, int np_in, float eps, int act,
                   int out_f32, const void* resid, long ldr, float* stats_out, int splits, float* ws, long ws_floats,
                   unsigned* counters, long n_counters, const void* emb_pos, const void* emb_type,
                   const long long* type_ids, const int* pos_ptr) {
    MMTG_REQUIRE(mode >= 0 && mode <= 2, "decode_gemm: mode 0 (LN-fold), 1 (LN-fold slabs) or 2 (in-kernel split-K reduce)");
    MMTG_REQUIRE(M > 0 && N > 0 && K > 0 && A && W && C, "decode_gemm: bad arguments");
    MMTG_REQUIRE(K % 8 == 0 && lda % 8 == 0 && ldw % 8 == 0 && N % 4 == 0 && ldc % 4 == 0, "decode_gemm: K, lda, ldw multiples of 8; N, ldc of 4");
    MMTG_REQUIRE(MMTG_ALIGNED16(A) && MMTG_ALIGNED16(W) && MMTG_ALIGNED16(C), "decode_gemm: 16-byte alignment");
    if (splits < 1) splits = 1;
    memset(&a, 0, sizeof(a));
    a.A = (const bf16*)A; a.W = (const bf16*)W; a.C = C; a.lda = lda; a.ldw = ldw; a.ldc = ldc; a.ldr = ldr;
    a.M = M; a.N = N; a.K = K;
    a.kper = cdiv(cdiv(K, splits), 64) * 64;
    a.splits = cdiv(K, a.kper);
    a.tiles_n = cdiv(N, 64);
    a.ntiles = cdiv(M, 64) * a.tiles_n;
    const long bytesA = ((long)(M - 1) * lda + K) * 2, bytesW = ((long)(N - 1) * ldw + K) * 2;
    MMTG_REQUIRE(bytesA < 0x7FFFFF00L && bytesW < 0x7FFFFF00L, "decode_gemm: operands must stay below 2 GiB");
    a.bytesA = (int)bytesA; a.bytesW = (int)bytesW;
    a.bias = bias; a.colsum = colsum; a.stats_in = stats_in; a.np_in = np_in; a.eps = eps; a.inv_k = 1.0f / (float)K;
    a.act = act; a.out_f32 = out_f32; a.resid = (const bf16*)resid; a.stats_out = stats_out; a.ws = ws; a.cnt = counters;
    a.ws_bytes = (int)(ws_floats < (1L << 29) ? ws_floats * 4 : 0x7FFFFFF0L);
    if (mode != 2) {
        MMTG_REQUIRE(colsum && stats_in && np_in >= 1 && np_in <= DG_NP && MMTG_ALIGNED16(stats_in) && MMTG_ALIGNED16(colsum),
                     "decode_gemm: LN-fold needs the weight column sums and the row statistics ([M][%d][2] floats, np_in partials)", DG_NP);
        MMTG_REQUIRE(mode == 1 || (bias && MMTG_ALIGNED16(bias) && a.splits == 1), "decode_gemm: mode 0 is a single K slice with the folded bias");
        MMTG_REQUIRE(mode == 0 || out_f32 == 1, "decode_gemm: mode 1 writes fp32 slabs [splits][M][ldc]");
        MMTG_REQUIRE(act == MMTG_EPI_NONE || act == MMTG_EPI_GELU, "decode_gemm: activation NONE or GELU");
    } else {
        MMTG_REQUIRE(!type_ids || (emb_pos && emb_type && pos_ptr && !resid), "decode_gemm: the embedding residual takes wpe, wte, type ids and the position (and no resid)");
        a.emb_pos = (const bf16*)emb_pos; a.emb_type = (const bf16*)emb_type; a.type_ids = type_ids; a.pos_ptr = pos_ptr;
        MMTG_REQUIRE(bias && (resid || type_ids) && stats_out && N % 32 == 0 && N / 32 <= DG_NP && ldr % 4 == 0 && MMTG_ALIGNED16(bias),
                     "decode_gemm: the reduce mode needs bias, residual and the statistics output; N a multiple of 32, at most %d", 32 * DG_NP);
        MMTG_REQUIRE(a.splits <= 8, "decode_gemm: at most 8 K splits in the reduce mode");
        MMTG_REQUIRE(a.splits == 1 || (ws && counters && ws_floats >= (long)a.ntiles * a.splits * 4096 && n_counters >= (long)a.ntiles * 4),
                     "decode_gemm: split products need %ld workspace floats and %ld zeroed counters", (long)a.ntiles * a.splits * 4096, (long)a.ntiles * 4);
    }
    return MMTG_OK;
}

extern "C" int mmtg_decode_gemm(int mode, int M, int N, int K, const void* A, long lda, const void* W, long ldw, void* C, long ldc,
                                const float* bias, const float* colsum, const float* stats_in, int np_in, float eps, int act,
                                int out_f32, const void* resid, long ldr, float* stats_out, int splits, float* ws, long ws_floats,
                                unsigned* counters, long n_counters, const void* emb_pos, const void* emb_type,
                                const long long* type_ids, const int* pos_ptr, void* stream) {
    DgArgs a;
    int rc_ = dg_fill(a, mode, M, N, K, A, lda, W, ldw, C, ldc, bias, colsum, stats_in, np_in, eps, act, out_f32, resid, ldr, stats_out, splits,
                      ws, ws_floats, counters, n_counters, emb_pos, emb_type, type_ids, pos_ptr);
    if (rc_) return rc_;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_GEMM_BF16, s, 2.0 * M * N * (double)K, 2.0 * ((double)M * K + (double)N * K) + (out_f32 ? 4.0 : 2.0) * (double)M * N);
    const size_t shm = 4 * 2 * 64 * 128 + 2 * 64 * 4;
    static bool attr_done = false;
    if (!attr_done) {
        if (hipFuncSetAttribute((const void*)decode_gemm_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm) != hipSuccess ||
            hipFuncSetAttribute((const void*)decode_gemm_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm) != hipSuccess ||
            hipFuncSetAttribute((const void*)decode_gemm_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm) != hipSuccess)
            MMTG_FAIL(MMTG_ERR_HIP, "decode_gemm: cannot raise dynamic LDS");
        attr_done = true;
    }
    const dim3 grid(a.ntiles * a.splits), block(256);
    if (mode == 0) hipLaunchKernelGGL(decode_gemm_kernel<0>, grid, block, shm, s, a);
    else if (mode == 1) hipLaunchKernelGGL(decode_gemm_kernel<1>, grid, block, shm, s, a);
    else hipLaunchKernelGGL(decode_gemm_kernel<2>, grid, block, shm, s, a);
    MMTG_LAUNCH_CHECK("decode_gemm");
    return MMTG_OK;
}

// ------------------------------------------------------------------ split-precision token step (round 5)
// The same fused products on (hi | lo) plane pairs: fp32 residual stream, fp32 KV cache, fp32 logits -- the decode step whose
// greedy ids equal the reference's (generate.py:117-142 in fp32 arithmetic) at a multiple of the exact-fp32 kernels' speed.
extern "C" int mmtg_decode_gemm_x3(int mode, int M, int N, int K, const void* A, long lda, long planeA, const void* W, long ldw, long planeW,
                                   float* C, long ldc, void* Cp, long ldcp, long planeC, const float* bias, const float* colsum,
                                   const float* stats_in, int np_in, float eps, int act, const float* resid, long ldr, float* stats_out,
                                   int splits, float* ws, long ws_floats, unsigned* counters, long n_counters, const float* emb_pos,
                                   const float* emb_type, const long long* type_ids, const int* pos_ptr, void* stream) {
    MMTG_REQUIRE(mode >= 0 && mode <= 2, "decode_gemm_x3: mode 0 (LN-fold), 1 (LN-fold slabs) or 2 (in-kernel split-K reduce)");
    MMTG_REQUIRE(M > 0 && N > 0 && K > 0 && A && W && (C || Cp), "decode_gemm_x3: bad arguments");
    MMTG_REQUIRE(K % 64 == 0 && lda % 8 == 0 && ldw % 8 == 0 && N % 4 == 0 && planeA % 8 == 0 && planeW % 8 == 0,
                 "decode_gemm_x3: K a multiple of 64; lda, ldw, plane distances of 8; N of 4");
    MMTG_REQUIRE(MMTG_ALIGNED16(A) && MMTG_ALIGNED16(W) && MMTG_ALIGNED16(C) && MMTG_ALIGNED16(Cp) && (!C || ldc % 4 == 0) && (!Cp || (ldcp % 4 == 0 && planeC % 4 == 0)),
                 "decode_gemm_x3: 16-byte alignment");
    MMTG_REQUIRE(planeA >= (long)(M - 1) * lda + K && planeW >= (long)(N - 1) * ldw + K && (!Cp || planeC >= (long)(M - 1) * ldcp + N),
                 "decode_gemm_x3: a lo plane must lie behind its hi plane");
    if (splits < 1) splits = 1;
    DgArgs a;
    memset(&a, 0, sizeof(a));
    a.A = (const bf16*)A; a.W = (const bf16*)W; a.C = C; a.lda = lda; a.ldw = ldw; a.ldc = ldc; a.ldr = ldr;
    a.Cp = (bf16*)Cp; a.ldcp = ldcp; a.planeC = planeC;
    a.M = M; a.N = N; a.K = K;
    a.kper = cdiv(cdiv(K, splits), 64) * 64;
    a.splits = cdiv(K, a.kper);
    a.tiles_n = cdiv(N, 64);
    a.ntiles = cdiv(M, 64) * a.tiles_n;
    const long bytesA = (planeA + (long)(M - 1) * lda + K) * 2, bytesW = (planeW + (long)(N - 1) * ldw + K) * 2;
    MMTG_REQUIRE(bytesA < 0x7FFFFF00L && bytesW < 0x7FFFFF00L, "decode_gemm_x3: plane pairs must stay below 2 GiB");
    a.bytesA = (int)bytesA; a.bytesW = (int)bytesW; a.planeA = (int)(planeA * 2); a.planeW = (int)(planeW * 2);
    a.bias = bias; a.colsum = colsum; a.stats_in = stats_in; a.np_in = np_in; a.eps = eps; a.inv_k = 1.0f / (float)K;
    a.act = act; a.out_f32 = C != nullptr; a.resid = (const bf16*)resid; a.stats_out = stats_out; a.ws = ws; a.cnt = counters;
    a.ws_bytes = (int)(ws_floats < (1L << 29) ? ws_floats * 4 : 0x7FFFFFF0L);
    if (mode != 2) {
        MMTG_REQUIRE(colsum && stats_in && np_in >= 1 && np_in <= DG_NP && MMTG_ALIGNED16(stats_in) && MMTG_ALIGNED16(colsum),
                     "decode_gemm_x3: LN-fold needs the weight column sums and the row statistics ([M][%d][2] floats, np_in partials)", DG_NP);
        MMTG_REQUIRE(mode == 1 || (bias && MMTG_ALIGNED16(bias) && a.splits == 1), "decode_gemm_x3: mode 0 is a single K slice with the folded bias");
        MMTG_REQUIRE(mode == 0 || (C && !Cp), "decode_gemm_x3: mode 1 writes fp32 slabs [splits][M][ldc]");
        MMTG_REQUIRE(mode == 1 || ((C != nullptr) != (Cp != nullptr)), "decode_gemm_x3: mode 0 writes fp32 rows OR a plane pair");
        MMTG_REQUIRE(act == MMTG_EPI_NONE || act == MMTG_EPI_GELU, "decode_gemm_x3: LN-fold activation NONE or GELU");
    } else {
        MMTG_REQUIRE(!type_ids || (emb_pos && emb_type && pos_ptr && !resid), "decode_gemm_x3: the embedding residual takes wpe, wte, type ids and the position (and no resid)");
        a.emb_pos = (const bf16*)emb_pos; a.emb_type = (const bf16*)emb_type; a.type_ids = type_ids; a.pos_ptr = pos_ptr;
        MMTG_REQUIRE(bias && MMTG_ALIGNED16(bias) && N % 32 == 0 && ldr % 4 == 0 && (!stats_out || N / 32 <= DG_NP),
                     "decode_gemm_x3: the reduce mode needs a bias; N a multiple of 32 (at most %d with statistics)", 32 * DG_NP);
        MMTG_REQUIRE(act == MMTG_EPI_NONE || act == MMTG_EPI_TANH, "decode_gemm_x3: reduce-mode activation NONE or TANH (before the residual)");
        MMTG_REQUIRE(a.splits <= 8, "decode_gemm_x3: at most 8 K splits in the reduce mode");
        MMTG_REQUIRE(a.splits == 1 || (ws && counters && ws_floats >= (long)a.ntiles * a.splits * 4096 && n_counters >= (long)a.ntiles * 4),
                     "decode_gemm_x3: split products need %ld workspace floats and %ld zeroed counters", (long)a.ntiles * a.splits * 4096, (long)a.ntiles * 4);
    }
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_GEMM_BF16, s, 2.0 * M * N * (double)K, 4.0 * ((double)M * K + (double)N * K + (double)M * N));
    const size_t shm = 4 * 2 * 64 * 128 + 2 * 64 * 4;        // (both forms: 4 x 16 KB or 2 x 32 KB)
    // MMTG_DECODE_X3_COMBINED (A/B switch): 1 = one K loop over combined stages, 0 = three passes over 16 KB stages
    static const int comb = getenv("MMTG_DECODE_X3_COMBINED") ? atoi(getenv("MMTG_DECODE_X3_COMBINED")) : 1;
    static bool attr_done = false;
    if (!attr_done) {
        if (hipFuncSetAttribute((const void*)decode_gemm_x3_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm) != hipSuccess ||
            hipFuncSetAttribute((const void*)decode_gemm_x3_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm) != hipSuccess ||
            hipFuncSetAttribute((const void*)decode_gemm_x3_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm) != hipSuccess ||
            hipFuncSetAttribute((const void*)decode_gemm_x3_kernel<0, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm) != hipSuccess ||
            hipFuncSetAttribute((const void*)decode_gemm_x3_kernel<1, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm) != hipSuccess ||
            hipFuncSetAttribute((const void*)decode_gemm_x3_kernel<2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm) != hipSuccess)
            MMTG_FAIL(MMTG_ERR_HIP, "decode_gemm_x3: cannot raise dynamic LDS");
        attr_done = true;
    }
    const dim3 grid(a.ntiles * a.splits), block(256);
    if (comb) {
        if (mode == 0) hipLaunchKernelGGL((decode_gemm_x3_kernel<0, true>), grid, block, shm, s, a);
        else if (mode == 1) hipLaunchKernelGGL((decode_gemm_x3_kernel<1, true>), grid, block, shm, s, a);
        else hipLaunchKernelGGL((decode_gemm_x3_kernel<2, true>), grid, block, shm, s, a);
    } else if (mode == 0) hipLaunchKernelGGL(decode_gemm_x3_kernel<0>, grid, block, shm, s, a);
    else if (mode == 1) hipLaunchKernelGGL(decode_gemm_x3_kernel<1>, grid, block, shm, s, a);
    else hipLaunchKernelGGL(decode_gemm_x3_kernel<2>, grid, block, shm, s, a);
    MMTG_LAUNCH_CHECK("decode_gemm_x3");
    return MMTG_OK;
}

extern "C" int mmtg_ln_fold_weights_x3(const void* W, long ldw, long planeW, const float* gamma, const float* beta, const float* bias,
                                       void* Wf, long ldf, long planeF, float* colsum, float* bias_f, int N, int K, void* stream) {
    MMTG_REQUIRE(W && gamma && beta && Wf && colsum && bias_f && N > 0 && K > 0 && K % 8 == 0 && ldw % 8 == 0 && ldw >= K && ldf % 8 == 0 && ldf >= K &&
                 planeW % 8 == 0 && planeF % 8 == 0, "ln_fold_weights_x3: bad arguments (K, leading dimensions, plane distances multiples of 8)");
    MMTG_REQUIRE(MMTG_ALIGNED16(W) && MMTG_ALIGNED16(Wf), "ln_fold_weights_x3: 16-byte alignment");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_MISC, s, 5.0 * N * (double)K, 8.0 * N * (double)K);
    hipLaunchKernelGGL(ln_fold_x3_kernel, dim3(cdiv(N, 4)), dim3(256), 0, s, (const bf16*)W, ldw, planeW, gamma, beta, bias, (bf16*)Wf, ldf, planeF,
                       colsum, bias_f, N, K);
    MMTG_LAUNCH_CHECK("ln_fold_weights_x3");
    return MMTG_OK;
}

extern "C" int mmtg_decode_attn_split_x3(const float* part, int splits, const float* bias, float* kcache, float* vcache, const int* keep,
                                         long ldkeep, const int* pos_ptr, void* out_planes, long plane, int B, int nH, int dh, int Tmax,
                                         void* stream) {
    MMTG_REQUIRE(part && bias && splits > 0 && kcache && vcache && keep && pos_ptr && out_planes, "decode_attn_split_x3: null pointer");
    MMTG_REQUIRE(dh == 64 && B > 0 && nH > 0 && Tmax > 0 && Tmax <= 1024 && plane % 4 == 0 && plane >= (long)B * nH * 64 && (((uintptr_t)out_planes) & 7) == 0,
                 "decode_attn_split_x3: head dim 64, Tmax <= 1024, the lo plane behind the hi plane");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_DECODE, s, 4.0 * B * nH * (double)Tmax * dh, 8.0 * B * nH * (double)Tmax * dh);
    const long slab = (long)B * 3 * nH * 64;
    static const bool kv_nt = !getenv("MMTG_DECODE_KV_NT") || atoi(getenv("MMTG_DECODE_KV_NT")) != 0;
    if (kv_nt) hipLaunchKernelGGL((decode_attn_kernel<float, true>), dim3(nH, B), dim3(64), 0, s, (const float*)nullptr, kcache, vcache, keep, ldkeep, pos_ptr,
                                  (float*)nullptr, nH, Tmax, part, splits, slab, bias, (bf16*)out_planes, plane);
    else hipLaunchKernelGGL((decode_attn_kernel<float, false>), dim3(nH, B), dim3(64), 0, s, (const float*)nullptr, kcache, vcache, keep, ldkeep, pos_ptr,
                            (float*)nullptr, nH, Tmax, part, splits, slab, bias, (bf16*)out_planes, plane);
    MMTG_LAUNCH_CHECK("decode_attn_split_x3");
    return MMTG_OK;
}

extern "C" int mmtg_decode_embed_x3(const float* table, const long long* seq, long ldseq, const float* c, void* x_planes, long plane,
                                    const int* pos_ptr, const long long* tpw_type, const long long* tpw_mask, long long* type_out, int* keep,
                                    long ldkeep, int B, int P, int S, int E, int two_sents, int V, int sent, int max_sent_num, void* stream) {
    MMTG_REQUIRE(table && seq && c && x_planes && pos_ptr && tpw_type && tpw_mask && type_out && keep, "decode_embed_x3: null pointer");
    MMTG_REQUIRE(B > 0 && E % 8 == 0 && sent > 1 && max_sent_num > 1 && plane % 4 == 0 && plane >= (long)B * E && (((uintptr_t)x_planes) & 7) == 0,
                 "decode_embed_x3: bad sizes");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_DECODE, s, (double)B * E, 12.0 * B * E);
    hipLaunchKernelGGL(decode_embed_kernel<float>, dim3(B), dim3(256), 0, s, table, seq, ldseq, c, (float*)nullptr, pos_ptr, tpw_type, tpw_mask, type_out, keep,
                       ldkeep, P, S, E, two_sents, V, sent, max_sent_num, (bf16*)x_planes, plane);
    MMTG_LAUNCH_CHECK("decode_embed_x3");
    return MMTG_OK;
}

extern "C" int mmtg_decode_attn_split_x3_rows(const float* part, int splits, const float* bias, float* kcache, float* vcache, const int* keep,
                                              long ldkeep, const int* rows, long ldrows, const int* pos_ptr, void* out_planes, long plane, int B,
                                              int nH, int dh, int Tmax, void* stream) {
    MMTG_REQUIRE(part && bias && splits > 0 && kcache && vcache && keep && rows && pos_ptr && out_planes, "decode_attn_split_x3_rows: null pointer");
    MMTG_REQUIRE(dh == 64 && B > 0 && nH > 0 && Tmax > 0 && Tmax <= 1024 && ldrows >= Tmax && plane % 4 == 0 && plane >= (long)B * nH * 64 &&
                 (((uintptr_t)out_planes) & 7) == 0,
                 "decode_attn_split_x3_rows: head dim 64, Tmax <= 1024, the ancestry table [B, ldrows >= Tmax], the lo plane behind the hi plane");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_DECODE, s, 4.0 * B * nH * (double)Tmax * dh, 8.0 * B * nH * (double)Tmax * dh);
    const long slab = (long)B * 3 * nH * 64;
    static const bool kv_nt = !getenv("MMTG_DECODE_KV_NT") || atoi(getenv("MMTG_DECODE_KV_NT")) != 0;
    if (kv_nt) hipLaunchKernelGGL((decode_attn_rows_kernel<float, true>), dim3(nH, B), dim3(64), 0, s, kcache, vcache, keep, ldkeep, rows, ldrows, pos_ptr,
                                  (float*)nullptr, nH, Tmax, part, splits, slab, bias, (bf16*)out_planes, plane);
    else hipLaunchKernelGGL((decode_attn_rows_kernel<float, false>), dim3(nH, B), dim3(64), 0, s, kcache, vcache, keep, ldkeep, rows, ldrows, pos_ptr,
                            (float*)nullptr, nH, Tmax, part, splits, slab, bias, (bf16*)out_planes, plane);
    MMTG_LAUNCH_CHECK("decode_attn_split_x3_rows");
    return MMTG_OK;
}

// ------------------------------------------------------------------ token log-probabilities (GreedyDecoder with return_logprobs=)
// One workgroup per row, launched after the step's selection entry on the same stream: the log-probability the model gives the id
// the step has just placed, log_softmax of the RAW logits (no penalty, no temperature, no bans; cut at V) at seq[b, pos + 1].  The
// kernel knows nothing of the selection's rule -- it scores whatever the column holds (a pick, a draw, a given id, a PAD, a held
// prefix id) -- so it is one kernel of its own behind all twelve selection forms, which stay the code they were
// (profiles/r14_logprob_decode_disassembly_diff.txt).  It reads *pos_ptr, which the selection leaves alone (it publishes the next
// position into the pair's other word).
namespace {

// (max, sum of exp(x - max)) of two parts as one; a part whose max is -inf holds nothing, and two such parts stay (-inf, 0)
__device__ __forceinline__ void lse_merge(float& m, float& s, float om, float os) {
    const float nm = fmaxf(m, om);
    s = nm == -INFINITY ? 0.f : s * expf(m - nm) + os * expf(om - nm);
    m = nm;
}

// scan_row's load shape: 16-byte aligned rows as float4, all of a pass's loads (up to 16 per thread) requested before the first is
// used; each pass folds its own (max, sum) into the thread's running pair.  The tail and unaligned rows go one logit at a time.
// -inf entries add 0 to the sum.  Fixed order throughout: the result is bit-reproducible.
// (UN, the loads per thread and pass, is a template parameter so that the kernel is emitted where it is instantiated, behind every
// other function of the code object: a plain kernel is emitted among the first, and the calls that cross it get other offsets)
template <int UN>
__global__ __launch_bounds__(256) void decode_logprob_kernel(const float* __restrict__ logits, long ldl, int V,
        const long long* __restrict__ seq, long ldseq, const int* __restrict__ pos_ptr, int P, float* __restrict__ out, long ldo,
        int ncols) {
    __shared__ float sm[4];
    __shared__ float ss[4];
    const int b = blockIdx.x, tid = threadIdx.x, pos = *pos_ptr;
    const int j = pos + 1 - P;                 // lyric index of the token the step has placed
    if (j < 0 || j >= ncols || pos + 1 >= ldseq) return;
    const long long v = seq[(long)b * ldseq + pos + 1];
    if (v < 0 || v >= V) return;
    const float* row = logits + (long)b * ldl;
    float m = -INFINITY, s = 0.f;
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
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o, 64);
        const float os = __shfl_xor(s, o, 64);
        lse_merge(m, s, om, os);
    }
    if ((tid & 63) == 0) { sm[tid >> 6] = m; ss[tid >> 6] = s; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) lse_merge(m, s, sm[w], ss[w]);
        // a row whose maximum is -inf has no distribution: -inf, never NaN; a chosen -inf entry gives -inf by the arithmetic
        out[(long)b * ldo + j] = m == -INFINITY ? -INFINITY : row[v] - m - logf(s);
    }
}

}  // namespace

extern "C" int mmtg_decode_logprob(const float* logits, long ldl, int V, const long long* seq, long ldseq, const int* pos_ptr, int P,
                                   float* out, long ldo, int ncols, int B, void* stream) {
    MMTG_REQUIRE(logits && seq && pos_ptr && out, "decode_logprob: null pointer");
    MMTG_REQUIRE(B > 0 && V > 0 && ldl >= V && P >= 0 && ldseq > P && ncols > 0 && ldo >= ncols,
                 "decode_logprob: logits [B, ldl >= V], seq [B, ldseq > P], out [B, ldo >= ncols > 0] (B %d, V %d, ldl %ld, P %d, ldseq %ld, "
                 "ncols %d, ldo %ld)", B, V, ldl, P, ldseq, ncols, ldo);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_DECODE, s, 2.0 * B * V, 4.0 * B * V);
    hipLaunchKernelGGL(decode_logprob_kernel<16>, dim3(B), dim3(256), 0, s, logits, ldl, V, seq, ldseq, pos_ptr, P, out, ldo, ncols);
    MMTG_LAUNCH_CHECK("decode_logprob");
    return MMTG_OK;
}

// ------------------------------------------------------------------ stochastic beam search (StochasticBeamDecoder)
// The candidates of mmtg_decode_gumbel_candidates (include/mmtg_hip.h states the rule; the merge is csrc/decode_stochastic.hip).
// beam_candidates_kernel<RefrainRule> with Gumbel noise: the row's nb largest t_v = log_softmax(x)[v] + n_v, each with its
// log-probability and the perturbed value of the child, conditioned on the row's own.  One kernel over the most general rule, whose
// "no rule" forms serve every generation, as decode_select_warp_kernel is; a template, so that it is emitted behind every other
// function of the code object and the kernels above stay the code they were.
// LDS: the count words and ONE V-float image, which holds x and then t (select_lds(V, true, rule), what the beam candidates ask
// for).  lp is not kept beside t: the nb winners' are recomputed from the logits by the beam kernel's own expressions, so cand_val
// has the bits that kernel gives the id, and the footprint stays at 80 KB for V = 13317 instead of 133 KB.
namespace {

// log(1 - exp(a)) for a <= 0 (Maechler 2012): log1mexp(0) = -inf
__device__ __forceinline__ float gumbel_log1mexp(float a) { return a > -0.69314718f ? logf(-expm1f(a)) : log1pf(-expf(a)); }

template <typename R>
__global__ __launch_bounds__(256) void gumbel_candidates_kernel(const float* __restrict__ logits, long ldl, int V,
        const long long* __restrict__ seq, long ldseq, const int* __restrict__ pos_ptr, int P, int sent,
        float temperature, float rep_penalty, int nb, float* __restrict__ cand_val, int* __restrict__ cand_id,
        const float* __restrict__ scores, const float* __restrict__ gum, const unsigned* __restrict__ row_seed,
        float* __restrict__ cand_g, R rule) {
    extern __shared__ unsigned cnt[];          // (V + 1) / 2 count words | V floats: the processed logits, then t
    float* const px = reinterpret_cast<float*>(cnt + (V + 1) / 2);
    __shared__ float sval[4], sx[BEAM_MAX];
    __shared__ int sidx[4], si[BEAM_MAX];
    const int b = blockIdx.x, tid = threadIdx.x, pos = *pos_ptr;
    const int j = pos + 1 - P;
    if (j < 1 || beam_forced(j, sent)) return;             // the merge appends the forced token without candidates
    if (rule.held(b, pos)) return;                         // a prefix column: nothing to offer (the merge keeps the prompt)
    float* const cv = cand_val + (long)b * nb;
    float* const cg = cand_g + (long)b * nb;
    int* const ci = cand_id + (long)b * nb;
    const float gb = gum[b], sb = scores[b];
    if (!(gb > -INFINITY) || !(sb > -INFINITY)) {          // a dead row offers nothing (NaN counts as dead)
        if (tid < nb) { cv[tid] = -INFINITY; cg[tid] = -INFINITY; ci[tid] = 0; }
        return;
    }
    const long long* gen = seq + (long)b * ldseq + P;
    // the single-choice columns: slot 0 alone, at log-probability 0, with the row's own perturbed value (probability 1)
    int only = -1;
    const int q = rule.copy_from(b, j, sent);
    const int n = min(j, MAXGEN);
    LineCol lc = {false, false, nullptr};
    bool rhymes = false;
    TmplCol tc = {-1, nullptr};
    if (q >= 0) only = (int)gen[q];                        // a refrain's copy
    else if (gen[n - 1] == 0) only = 0;                    // sticky PAD
    else {
        lc = rule.col(b, j, sent, gen, &rhymes);
        if (lc.force_pad) only = 0;                        // a full line's PAD
        else {
            tc = rule.sym(b, j, sent);
            if (tc.given >= 0) only = tc.given;            // a template's given id
        }
    }
    if (q >= 0 || only >= 0) {
        if (tid < nb) { cv[tid] = tid == 0 ? 0.f : -INFINITY; cg[tid] = tid == 0 ? gb : -INFINITY; ci[tid] = tid == 0 ? only : 0; }
        return;
    }
    count_ids(cnt, V, gen, n, tid);
    const NgramBan ng = rule.bans();
    if (ng.n > 0) ban_ngrams(cnt, reinterpret_cast<int*>(px + V), V, gen, min(n, ng.hist_cap), ng.n, tid);
    ban_line_tmpl(cnt, V, lc, tc.cls, tid);
    rule.ban_distinct(cnt, b, j, sent, gen, lc, rhymes, tid);
    const float* row = logits + (long)b * ldl;
    float mx = -INFINITY;
    for (int v = tid; v < V; v += 256) {                   // (beam_candidates_kernel's expressions, in its order: cand_val's bits)
        float x = row[v];
        if (v != 102) {
            const int c = (cnt[v >> 1] >> (16 * (v & 1))) & 0xFFFF;
            x = penalize<true>(x, c, rep_penalty);
        }
        x = x / temperature;
        if (v == 1 || v == 2 || v == 100 || v == 102) x = -INFINITY;
        px[v] = x;
        mx = fmaxf(mx, x);
    }
    mx = wave_max(mx);
    if ((tid & 63) == 0) sval[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(sval[0], sval[1]), fmaxf(sval[2], sval[3]));
    if (!(mx > -INFINITY)) {                               // every id banned: nothing to offer, as a dead row
        if (tid < nb) { cv[tid] = -INFINITY; cg[tid] = -INFINITY; ci[tid] = 0; }
        return;
    }
    float sum = 0.f;
    for (int v = tid; v < V; v += 256) sum += expf(px[v] - mx);
    sum = wave_sum(sum);
    __syncthreads();
    if ((tid & 63) == 0) sval[tid >> 6] = sum;
    __syncthreads();
    const float lsum = logf(sval[0] + sval[1] + sval[2] + sval[3]);
    // t_v = lp_v + n_v in place of x_v (a thread rewrites the entries it wrote); -inf stays -inf: the noise is finite
    const unsigned hs = hash_u32(row_seed[b], (unsigned)pos);
    float zt = -INFINITY;
    for (int v = tid; v < V; v += 256) {
        const float x = px[v];
        float t = -INFINITY;
        if (x > -INFINITY) {
            const unsigned h = hash_u32(hs, (unsigned)v);
            const float u = ((float)(h >> 9) + 0.5f) * 1.1920928955078125e-07f;          // 2^-23: exact, inside (0, 1)
            t = ((x - mx) - lsum) + -logf(-logf(u));
        }
        px[v] = t;
        zt = fmaxf(zt, t);
    }
    zt = wave_max(zt);
    __syncthreads();                                       // (sval's sums are read)
    if ((tid & 63) == 0) sval[tid >> 6] = zt;
    __syncthreads();
    zt = fmaxf(fmaxf(sval[0], sval[1]), fmaxf(sval[2], sval[3]));
    // nb rounds of the block arg-max over t (lowest id wins ties); a taken id is marked NaN, which no comparison selects again
    for (int r = 0; r < nb; ++r) {
        __syncthreads();
        float best = -INFINITY;
        int besti = 0x7fffffff;
        for (int v = tid; v < V; v += 256) {
            const float x = px[v];
            if (x > best || (x == best && v < besti)) { best = x; besti = v; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(besti, o, 64);
            if (ov > best || (ov == best && oi < besti)) { best = ov; besti = oi; }
        }
        if ((tid & 63) == 0) { sval[tid >> 6] = best; sidx[tid >> 6] = besti; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < 4; ++w)
                if (sval[w] > best || (sval[w] == best && sidx[w] < besti)) { best = sval[w]; besti = sidx[w]; }
            sx[r] = best;
            si[r] = besti;
            if (besti >= 0 && besti < V) px[besti] = __int_as_float(0x7fc00000);
        }
    }
    __syncthreads();
    if (tid < nb) {
        const float t = sx[tid];
        const int v = si[tid];
        const bool ok = v >= 0 && v < V && t > -INFINITY;
        float lp = -INFINITY, g = -INFINITY;
        if (ok) {
            float x = row[v];                              // the winner's log-probability again, from the logits
            if (v != 102) {
                const int c = (cnt[v >> 1] >> (16 * (v & 1))) & 0xFFFF;
                x = penalize<true>(x, c, rep_penalty);
            }
            x = x / temperature;
            lp = (x - mx) - lsum;
            const float G = sb + t;
            const float w = (gb - G) + gumbel_log1mexp(t - zt);
            g = gb - fmaxf(0.f, w) - log1pf(expf(-fabsf(w)));
        }
        cv[tid] = lp;
        cg[tid] = g;
        ci[tid] = ok ? v : 0;
    }
}

}  // namespace

extern "C" int mmtg_decode_gumbel_candidates(const float* logits, long ldl, int V, const long long* seq, long ldseq,
                                             const int* pos_ptr, int P, int sent, float temperature, float rep_penalty, int nb,
                                             float* cand_val, int* cand_id, int B, const int* fixed_end, int ngram,
                                             const unsigned char* lo, const unsigned char* hi, int n_lines, const unsigned* sets,
                                             int n_sets, const short* set_of, const int* tmpl, const short* class_of,
                                             const signed char* lead, int distinct, const signed char* src, const float* scores,
                                             const float* gum, const unsigned* row_seed, float* cand_g, void* stream) {
    const char* what = "decode_gumbel_candidates";
    RefrainRule rf;
    MMTG_REQUIRE(nb >= 1 && nb <= BEAM_MAX, "%s: nb = %d rows per prompt (1..%d)", what, nb, BEAM_MAX);
    MMTG_REQUIRE(scores, "%s: scores [B] is null", what);
    MMTG_REQUIRE(gum, "%s: gum [B] is null", what);
    MMTG_REQUIRE(row_seed, "%s: row_seed [B] is null", what);
    MMTG_REQUIRE(cand_g, "%s: cand_g [B, nb] is null", what);
    if (int e = refrain_check(what, V, ldseq, P, sent, fixed_end, ngram, lo, hi, n_lines, sets, n_sets, set_of, tmpl, class_of, lead,
                              distinct, src, &rf))
        return e;
    MMTG_REQUIRE(logits && seq && pos_ptr && cand_val && cand_id && B > 0 && V > 0 && ldl >= V, "%s: bad args", what);
    MMTG_REQUIRE(temperature > 0.f && rep_penalty > 0.f, "%s: temperature / penalty must be > 0", what);
    MMTG_REQUIRE(V <= 24000, "%s: vocabulary of %d exceeds the LDS row image (24000)", what, V);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(MMTG_PROF_DECODE, s, 60.0 * B * V, 4.0 * B * V);
    static bool attr_done = false;
    if (!attr_done) {
        if (hipFuncSetAttribute((const void*)gumbel_candidates_kernel<RefrainRule>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                160 * 1024 - 4096) != hipSuccess)
            MMTG_FAIL(MMTG_ERR_HIP, "%s: cannot raise dynamic LDS", what);
        attr_done = true;
    }
    hipLaunchKernelGGL(gumbel_candidates_kernel<RefrainRule>, dim3(B), dim3(256), select_lds(V, true, rf), s, logits, ldl, V, seq, ldseq,
                       pos_ptr, P, sent, temperature, rep_penalty, nb, cand_val, cand_id, scores, gum, row_seed, cand_g, rf);
    MMTG_LAUNCH_CHECK(what);
    return MMTG_OK;
}
