// mirostat.hip — Mirostat 2.0 (llama.cpp's llama_sampler_mirostat_v2, which Ollama exposes as options.mirostat: 2 with
// mirostat_tau / mirostat_eta) on the device, inside the same (captured) decode step as the sampler.  Unlike the
// penalty and truncation kernels it carries state from one token to the next: the per-slot surprise target mu.
//
// Two kernels bracket the sampler launch (sampler.hip), like the logprob pair:
//
//   mirostat_truncate_kernel  AFTER the penalty kernel and the logprob pre-kernel, BEFORE the sampler.  One workgroup
//                             per slot with the sampler's row_of_slot / first-n-slots addressing, its liveness test
//                             (empty, parked and DONE slots, and slots with row_of_slot < 0, are skipped) and its
//                             legal set (next[s][v] >= 0 && dist[next] <= remaining - 1).  For a slot with mirostat on
//                             and temperature T > 0, over the legal tokens with x_v = float(logit):
//                               m = max x, Z = sum exp((x_u - m) / T),
//                               S_v = ((m - x_v) / T + ln Z) / ln 2          the surprise of v in bits
//                             a token survives iff S_v <= mu or x_v == m (the maxima have the least surprise, so this
//                             is "if nothing survives the maxima do"; equal logits share their fate), -inf is written
//                             in the row's dtype into the legal tokens that do not survive, and the slot keeps
//                               mi_m = m,  mi_lnz = ln Z' with Z' = sum over the survivors of exp((x_u - m) / T),
//                               mi_mark = nout[slot]: the output index the sampler is about to fill.
//                             Nothing else is touched: not the illegal tokens, not the padding past the DFA
//                             vocabulary, not the rows of skipped slots.  A forced step (fewer than two legal tokens,
//                             or every legal logit -inf) writes nothing to the row, and it — like every skipped slot,
//                             a slot at temperature 0 and a slot with mirostat off — gets mi_mark = -1.
//   mirostat_update_kernel    AFTER the sampler, one thread per slot.  Where the sampler did emit output index mi_mark
//                             (nout advanced by one), with t that token:
//                               S_obs = ((m - x_t) / T + ln Z') / ln 2       under the renormalised distribution
//                               mu <- mu - eta * (S_obs - tau)
//                             x_t is a survivor's logit, which the first kernel never rewrites.  A slot marked -1
//                             keeps its mu: forced tokens do not move it (a deviation from llama.cpp, which books
//                             surprise 0 for them; brain/api/protocol.py).
//
// Three row passes (max + legal count, Z, write + Z').  No atomics: the sums go through block_sum in a fixed order,
// so the same row gives the same bits on every launch and under graph replay.
//
// Decode gate (chronos_hip.h): like the sampler, the logprob, the penalty and the truncation kernels, these do not
// take the gate; the per-slot liveness test turns a closed gate into mi_mark = -1 and an immediate return, and the
// update kernel then finds no advanced slot.
#include "chronos_hip.h"

namespace chronos {

constexpr int kMiThreads = 1024;
constexpr float kMiInvLn2 = 1.4426950408889634f;

template <typename LT>
__device__ __forceinline__ float mi_load(const LT* p, int64_t i);
template <>
__device__ __forceinline__ float mi_load<uint16_t>(const uint16_t* p, int64_t i) { return bf2f(p[i]); }
template <>
__device__ __forceinline__ float mi_load<float>(const float* p, int64_t i) { return p[i]; }

template <typename LT>
__device__ __forceinline__ void mi_kill(LT* p, int64_t i);
template <>
__device__ __forceinline__ void mi_kill<uint16_t>(uint16_t* p, int64_t i) { p[i] = 0xFF80u; }  // bf16 -inf
template <>
__device__ __forceinline__ void mi_kill<float>(float* p, int64_t i) { p[i] = -INFINITY; }

__device__ __forceinline__ float mi_block_max(float v, float* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    v = wave_max(v);
    if (lane == 0) red[w] = v;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int k = 1; k < kMiThreads / 64; ++k) r = fmaxf(r, red[k]);
    __syncthreads();
    return r;
}

// the surprise in bits of a token at logit x, every fp32 step rounded on its own (ops/reference.py does the same)
__device__ __forceinline__ float mi_surprise(float x, float m, float T, float lnz) {
    return __fmul_rn(__fadd_rn(__fdiv_rn(__fsub_rn(m, x), T), lnz), kMiInvLn2);
}

template <typename LT>
__global__ void __launch_bounds__(kMiThreads) mirostat_truncate_kernel(
    LT* __restrict__ logits, int64_t lstride, const int32_t* __restrict__ row_of_slot, int vocab,
    const int16_t* __restrict__ next, const int16_t* __restrict__ dist, int done_state,
    const int32_t* __restrict__ state, const int32_t* __restrict__ remaining, const int32_t* __restrict__ nout,
    const float* __restrict__ temperature, const int32_t* __restrict__ mi_on, const float* __restrict__ mi_mu,
    float* __restrict__ mi_m, float* __restrict__ mi_lnz, int32_t* __restrict__ mi_mark) {
    __shared__ float red[16];
    const int slot = blockIdx.x;
    const int t = threadIdx.x;
    const int s = state[slot];
    const int row = row_of_slot ? row_of_slot[slot] : slot;
    const float T = temperature[slot];
    if (!mi_on[slot] || s < 0 || s == done_state || row < 0 || !(T > 0.f)) {
        if (t == 0) mi_mark[slot] = -1;
        return;
    }
    const float mu = mi_mu[slot];
    LT* lg = logits + (int64_t)row * lstride;
    const int16_t* nx = next + (int64_t)s * vocab;
    const int budget = remaining[slot] - 1;
    // body(v, x) for every legal token v of the row, x = float(logit[v]); an illegal token's logit is never loaded
    auto for_legal = [&](auto&& body) {
        for (int v = t; v < vocab; v += kMiThreads) {
            const int ns = nx[v];
            if (ns >= 0 && dist[ns] <= budget) body(v, mi_load<LT>(lg, v));
        }
    };

    // ---- pass 1: the legal maximum and the number of legal tokens -------------------------------------------------
    float m = -INFINITY;
    int cnt = 0;
    for_legal([&](int, float x) {
        m = fmaxf(m, x);
        ++cnt;
    });
    m = mi_block_max(m, red);
    const float nlegal = block_sum((float)cnt, red);  // exact: at most 2^24 tokens
    if (nlegal < 2.f || !(m > -INFINITY)) {           // forced token, or nothing with mass: write nothing, mu stays
        if (t == 0) mi_mark[slot] = -1;
        return;
    }

    // ---- pass 2: Z, fixed reduction order -------------------------------------------------------------------------
    float z = 0.f;
    for_legal([&](int, float x) { z += expf(__fdiv_rn(__fsub_rn(x, m), T)); });  // exp(-inf) = 0
    z = block_sum(z, red);  // >= 1: the maximum itself
    const float lnz = logf(z);

    // ---- pass 3: write, and Z' over the survivors -----------------------------------------------------------------
    float z2 = 0.f;
    for_legal([&](int v, float x) {
        if (x == m || mi_surprise(x, m, T, lnz) <= mu)
            z2 += expf(__fdiv_rn(__fsub_rn(x, m), T));
        else if (x > -INFINITY)
            mi_kill<LT>(lg, v);
    });
    z2 = block_sum(z2, red);
    if (t == 0) {
        mi_m[slot] = m;
        mi_lnz[slot] = logf(z2);
        mi_mark[slot] = nout[slot];
    }
}

template <typename LT>
__global__ void __launch_bounds__(64) mirostat_update_kernel(
    const LT* __restrict__ logits, int64_t lstride, int lcols, const int32_t* __restrict__ row_of_slot, int nslots,
    const int32_t* __restrict__ nout, const int32_t* __restrict__ out_tokens, int max_out,
    const float* __restrict__ temperature, const int32_t* __restrict__ mi_on, float* __restrict__ mi_mu,
    const float* __restrict__ mi_tau, const float* __restrict__ mi_eta, const float* __restrict__ mi_m,
    const float* __restrict__ mi_lnz, const int32_t* __restrict__ mi_mark) {
    const int slot = blockIdx.x * 64 + threadIdx.x;
    if (slot >= nslots) return;
    const int i = mi_mark[slot];
    if (i < 0 || i >= max_out || !mi_on[slot] || nout[slot] != i + 1) return;
    const int row = row_of_slot ? row_of_slot[slot] : slot;
    const float T = temperature[slot];
    if (row < 0 || !(T > 0.f)) return;  // (the first kernel marks such a slot -1; kept so a stale mark cannot index)
    const int tok = out_tokens[(int64_t)slot * max_out + i];
    if (tok < 0 || tok >= lcols) return;
    const float x = mi_load<LT>(logits + (int64_t)row * lstride, tok);
    const float sobs = mi_surprise(x, mi_m[slot], T, mi_lnz[slot]);
    if (!(fabsf(sobs) < INFINITY)) return;  // never a survivor's: keep mu finite whatever the sampler was given
    mi_mu[slot] = __fsub_rn(mi_mu[slot], __fmul_rn(mi_eta[slot], __fsub_rn(sobs, mi_tau[slot])));
}

void launch_mirostat_truncate(void* logits, bool logits_f32, int64_t lstride, const int32_t* row_of_slot, int nslots,
                              int vocab, const int16_t* next, const int16_t* dist, int done_state,
                              const int32_t* state, const int32_t* remaining, const int32_t* nout,
                              const float* temperature, const int32_t* mi_on, const float* mi_mu, float* mi_m,
                              float* mi_lnz, int32_t* mi_mark, hipStream_t st) {
    if (nslots == 0) return;
    if (logits_f32)
        hipLaunchKernelGGL(mirostat_truncate_kernel<float>, dim3(nslots), dim3(kMiThreads), 0, st, (float*)logits,
                           lstride, row_of_slot, vocab, next, dist, done_state, state, remaining, nout, temperature,
                           mi_on, mi_mu, mi_m, mi_lnz, mi_mark);
    else
        hipLaunchKernelGGL(mirostat_truncate_kernel<uint16_t>, dim3(nslots), dim3(kMiThreads), 0, st,
                           (uint16_t*)logits, lstride, row_of_slot, vocab, next, dist, done_state, state, remaining,
                           nout, temperature, mi_on, mi_mu, mi_m, mi_lnz, mi_mark);
}

void launch_mirostat_update(const void* logits, bool logits_f32, int64_t lstride, int lcols,
                            const int32_t* row_of_slot, int nslots, const int32_t* nout, const int32_t* out_tokens,
                            int max_out, const float* temperature, const int32_t* mi_on, float* mi_mu,
                            const float* mi_tau, const float* mi_eta, const float* mi_m, const float* mi_lnz,
                            const int32_t* mi_mark, hipStream_t st) {
    if (nslots == 0) return;
    const dim3 grid((nslots + 63) / 64);
    if (logits_f32)
        hipLaunchKernelGGL(mirostat_update_kernel<float>, grid, dim3(64), 0, st, (const float*)logits, lstride, lcols,
                           row_of_slot, nslots, nout, out_tokens, max_out, temperature, mi_on, mi_mu, mi_tau, mi_eta,
                           mi_m, mi_lnz, mi_mark);
    else
        hipLaunchKernelGGL(mirostat_update_kernel<uint16_t>, grid, dim3(64), 0, st, (const uint16_t*)logits, lstride,
                           lcols, row_of_slot, nslots, nout, out_tokens, max_out, temperature, mi_on, mi_mu, mi_tau,
                           mi_eta, mi_m, mi_lnz, mi_mark);
}

}  // namespace chronos
