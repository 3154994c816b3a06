// truncate.hip — min_p and typical_p (llama.cpp's truncation samplers, which Ollama exposes as options.min_p and
// options.typical_p) applied to the logits on the device, inside the same (captured) decode step as the sampler.
//
// One kernel, launched AFTER the penalty kernel and the logprob pre-kernel and BEFORE the sampler (sampler.hip), one
// workgroup per slot with the sampler's row_of_slot / first-n-slots addressing, its liveness test (empty, parked and
// DONE slots, and slots with row_of_slot < 0, are skipped) and its legal set (next[s][v] >= 0 && dist[next] <=
// remaining - 1).  A slot at temperature 0 (greedy ignores truncation, as it ignores top-k / top-p) or with neutral
// parameters (minp_ln = -inf, typical >= 1) returns after reading its parameters.  Otherwise, over the legal tokens
// with x_v = float(logit), raw logits before temperature:
//
//   typical_p (tp < 1):  m = max x, Z = sum exp(x - m), logp_v = x_v - m - log Z, H = -sum p_v logp_v,
//                        d_v = |-logp_v - H|; tokens are walked by ascending d accumulating p, d* is the d of the
//                        first token at which the accumulated mass exceeds tp, every token with d_v <= d* survives
//                        (ties kept: equal logits share their fate, at least one token survives).
//                        Since H = log Z - sum p_v (x_v - m), d_v = |(m - x_v) + sum p_u (x_u - m)|: the kernel needs
//                        sum e and sum e (x - m) with e = exp(x - m) and never log Z itself.
//   min_p (ln p > -inf), after typical_p:  m' = max x over the survivors, a token survives iff x_v >= m' + ln p
//                        (one fp32 add: bit-reproducible against the reference).
//
// and -inf is written, in the row's dtype, into the legal tokens that do not survive.  Nothing else is touched: not
// the illegal tokens, not the padding past the DFA vocabulary, not the rows of skipped slots.  With at most one legal
// token, or every legal logit already -inf, nothing is written: a grammar-forced token stays forced.
//
// The boundary d* is an exact radix select on the 31 value bits of fp32 d (d >= 0): three histogram passes over 11,
// 10 and 10 bits, each a 2048-bin LDS histogram of softmax mass, scanned by the whole workgroup.  (A 16-bit key as
// top-p uses would not do: d of bf16 logits merges far too many classes at the boundary.)  Mass is accumulated in
// 64-bit fixed point, floor(e * 2^40): integer adds commute, so the histograms, the boundary and hence the written
// row do not depend on the order in which the LDS atomics land; a token with e < 2^-40 carries no mass (it is below
// m by more than 27.7 and at most 2^-23 of the total together with all its like in a 128k vocabulary).
//
// Row passes: min_p only reads the row twice (max, write); typical_p six times (max, sums, three histograms, write),
// seven with min_p (the survivors' max).
//
// Decode gate (chronos_hip.h): like the sampler, the logprob and the penalty kernels, this one does not take the gate;
// the per-slot liveness test turns a closed gate into an immediate return.
#include "chronos_hip.h"

namespace chronos {

constexpr int kTrThreads = 1024;  // the scan below assigns two histogram bins to each thread
constexpr int kTrBins = 2048;

template <typename LT>
__device__ __forceinline__ float tr_load(const LT* p, int64_t i);
template <>
__device__ __forceinline__ float tr_load<uint16_t>(const uint16_t* p, int64_t i) { return bf2f(p[i]); }
template <>
__device__ __forceinline__ float tr_load<float>(const float* p, int64_t i) { return p[i]; }

template <typename LT>
__device__ __forceinline__ void tr_kill(LT* p, int64_t i);
template <>
__device__ __forceinline__ void tr_kill<uint16_t>(uint16_t* p, int64_t i) { p[i] = 0xFF80u; }  // bf16 -inf
template <>
__device__ __forceinline__ void tr_kill<float>(float* p, int64_t i) { p[i] = -INFINITY; }

__device__ __forceinline__ float tr_block_max(float v, float* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    v = wave_max(v);
    if (lane == 0) red[w] = v;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int k = 1; k < kTrThreads / 64; ++k) r = fmaxf(r, red[k]);
    __syncthreads();
    return r;
}

// softmax mass of a token in 2^-40 units (x <= m, so e <= 1 and the product is exact in fp32)
__device__ __forceinline__ unsigned long long tr_mass(float x, float m) {
    return (unsigned long long)(expf(x - m) * 1099511627776.f);
}

template <typename LT>
__global__ void __launch_bounds__(kTrThreads) truncate_logits_kernel(
    LT* __restrict__ logits, int64_t lstride, const int32_t* __restrict__ row_of_slot, int vocab,
    const int16_t* __restrict__ next, const int16_t* __restrict__ dist, int done_state,
    const int32_t* __restrict__ state, const int32_t* __restrict__ remaining, const float* __restrict__ temperature,
    const float* __restrict__ minp_ln, const float* __restrict__ typical) {
    __shared__ unsigned long long h[kTrBins];
    __shared__ unsigned long long wtot[kTrThreads / 64];
    __shared__ float red[16];
    __shared__ unsigned long long sh_below, sh_target;
    __shared__ uint32_t sh_bin;
    const int slot = blockIdx.x;
    const int s = state[slot];
    if (s < 0 || s == done_state) return;
    const int row = row_of_slot ? row_of_slot[slot] : slot;
    if (row < 0) return;
    if (!(temperature[slot] > 0.f)) return;
    const float lnp = minp_ln[slot], tp = typical[slot];
    const bool minp_on = lnp > -INFINITY, typ_on = tp < 1.f;
    if (!minp_on && !typ_on) return;
    LT* lg = logits + (int64_t)row * lstride;
    const int16_t* nx = next + (int64_t)s * vocab;
    const int budget = remaining[slot] - 1;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    // body(v, x) for every legal token v of the row, x = float(logit[v]); an illegal token's logit is never loaded.
    // (Eight tokens per iteration with all loads issued up front was measured and is slower, 1.3x at 1 row and 1.5x at
    // 1024: the plain loop already overlaps its iterations, and the verdict grammar's rows are nearly all illegal.)
    auto for_legal = [&](auto&& body) {
        for (int v = t; v < vocab; v += kTrThreads) {
            const int ns = nx[v];
            if (ns >= 0 && dist[ns] <= budget) body(v, tr_load<LT>(lg, v));
        }
    };

    // ---- pass 1: the legal maximum and the number of legal tokens -------------------------------------------------
    float m = -INFINITY;
    int cnt = 0;
    for_legal([&](int, float x) {
        m = fmaxf(m, x);
        ++cnt;
    });
    m = tr_block_max(m, red);
    const float nlegal = block_sum((float)cnt, red);  // exact: at most 2^24 tokens
    if (nlegal < 2.f || !(m > -INFINITY)) return;     // forced token, or nothing with mass: write nothing

    uint32_t dstar = 0x7FFFFFFFu;  // largest key: every token survives typical_p
    float c = 0.f;                 // sum p_u (x_u - m) = log Z - H, <= 0
    auto dkey = [&](float x) { return __float_as_uint(fabsf((m - x) + c)) & 0x7FFFFFFFu; };
    if (typ_on) {
        // ---- pass 2: Z and sum e (x - m), fixed reduction order ---------------------------------------------------
        float z = 0.f, sx = 0.f;
        for_legal([&](int, float x) {
            const float dx = x - m;
            const float e = expf(dx);
            if (e > 0.f) {  // p = 0 contributes 0 (dx may be -inf)
                z += e;
                sx += e * dx;
            }
        });
        z = block_sum(z, red);
        sx = block_sum(sx, red);
        c = sx / z;  // z >= 1: the maximum itself

        // ---- passes 3-5: radix select of d* on the 31 value bits of d, by mass ------------------------------------
        // Pass p histograms bits [shift, shift + bits) of the keys whose higher bits equal `prefix`; the workgroup
        // scans the bins (two per thread) and the one thread whose bin takes the accumulated mass across the target
        // publishes it.  below = mass of all keys smaller than the prefix's range.
        uint32_t prefix = 0;
        unsigned long long below = 0;
#pragma unroll 1
        for (int pass = 0; pass < 3; ++pass) {
            const int shift = pass == 0 ? 20 : pass == 1 ? 10 : 0;
            const int hishift = pass == 0 ? 31 : pass == 1 ? 20 : 10;  // key >> hishift must equal prefix
            const uint32_t mask = pass == 0 ? 2047u : 1023u;
            h[2 * t] = 0;
            h[2 * t + 1] = 0;
            if (t == 0) {  // if no bin is found (cannot happen: the target is below the total) keep the whole range
                sh_bin = mask;
                sh_below = below;
            }
            __syncthreads();
            for_legal([&](int, float x) {
                const uint32_t k = dkey(x);
                if ((k >> hishift) == prefix) {
                    const unsigned long long q = tr_mass(x, m);
                    if (q) atomicAdd(&h[(k >> shift) & mask], q);
                }
            });
            __syncthreads();
            const unsigned long long a = h[2 * t], b = h[2 * t + 1];
            unsigned long long inc = a + b;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned long long n = __shfl_up(inc, o, 64);
                if (lane >= o) inc += n;
            }
            if (lane == 63) wtot[w] = inc;
            __syncthreads();
            unsigned long long pre = 0, tot = 0;
#pragma unroll
            for (int k = 0; k < kTrThreads / 64; ++k) {
                if (k < w) pre += wtot[k];
                tot += wtot[k];
            }
            // the first pass sees the whole mass: target = floor(tp * total) < total, "exceeds" is a strict >
            const unsigned long long target =
                pass == 0 ? (unsigned long long)((double)fmaxf(tp, 0.f) * (double)tot) : sh_target;
            const unsigned long long e0 = below + pre + inc - (a + b), e1 = e0 + a, e2 = e1 + b;
            if (e0 <= target && target < e1) {
                sh_bin = 2 * t;
                sh_below = e0;
            } else if (e1 <= target && target < e2) {
                sh_bin = 2 * t + 1;
                sh_below = e1;
            }
            if (pass == 0 && t == 0) sh_target = target;
            __syncthreads();
            prefix = (prefix << (pass == 0 ? 11 : 10)) | sh_bin;
            below = sh_below;
            __syncthreads();  // sh_bin / sh_below are rewritten by the next pass
        }
        dstar = prefix;
    }

    // ---- min_p keys off the maximum of the typical_p survivors ------------------------------------------------------
    float cut = -INFINITY;
    if (minp_on) {
        float m2 = m;
        if (typ_on) {
            m2 = -INFINITY;
            for_legal([&](int, float x) {
                if (dkey(x) <= dstar) m2 = fmaxf(m2, x);
            });
            m2 = tr_block_max(m2, red);
        }
        cut = __fadd_rn(m2, lnp);
    }

    // ---- write pass -------------------------------------------------------------------------------------------------
    for_legal([&](int v, float x) {
        const bool keep = (!typ_on || dkey(x) <= dstar) && x >= cut;
        if (!keep && x > -INFINITY) tr_kill<LT>(lg, v);
    });
}

void launch_truncate_logits(void* logits, bool logits_f32, int64_t lstride, const int32_t* row_of_slot, int nslots,
                            int vocab, const int16_t* next, const int16_t* dist, int done_state, const int32_t* state,
                            const int32_t* remaining, const float* temperature, const float* minp_ln,
                            const float* typical, hipStream_t st) {
    if (nslots == 0) return;
    if (logits_f32)
        hipLaunchKernelGGL(truncate_logits_kernel<float>, dim3(nslots), dim3(kTrThreads), 0, st, (float*)logits,
                           lstride, row_of_slot, vocab, next, dist, done_state, state, remaining, temperature, minp_ln,
                           typical);
    else
        hipLaunchKernelGGL(truncate_logits_kernel<uint16_t>, dim3(nslots), dim3(kTrThreads), 0, st, (uint16_t*)logits,
                           lstride, row_of_slot, vocab, next, dist, done_state, state, remaining, temperature, minp_ln,
                           typical);
}

}  // namespace chronos
