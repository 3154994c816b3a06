// penalties.hip — repeat / frequency / presence penalties (llama.cpp's, which Ollama exposes as options.repeat_penalty,
// frequency_penalty, presence_penalty and repeat_last_n) applied to the logits on the device, inside the same
// (captured) decode step as the sampler, so a penalised request costs no host round trip per token.
//
// One kernel, launched BEFORE token_logprobs (logprobs.hip) and the sampler (sampler.hip), one workgroup per slot with
// their row_of_slot / first-n-slots addressing and their liveness test (empty, parked and DONE slots, and slots with
// row_of_slot < 0, are skipped).  For a live slot with non-neutral parameters and window L > 0:
//
//   history  H = the slot's prompt tail (pen_tail[slot, 0:pen_tlen[slot]], the last <= W prompt ids in order) followed
//                by the tokens generated so far (the sampler's own ring out_tokens[slot, 0:nout[slot]], which also
//                holds the grammar-forced runs Engine._jump appends), cut to its last L entries;
//   for every distinct token v of H with count c (ids outside [0, logits width) are skipped), in fp32:
//                x = logit[v];  x = x <= 0 ? x * rp : x / rp;  x -= c * fq + pr;  logit[v] = x (in the row's dtype).
//
// The window (at most kPenMaxWindow ids) is staged in LDS.  The thread that holds entry t counts the entries equal to
// its own and finds out whether it is the first occurrence; only first occurrences read, modify and write their logit,
// so each penalised logit is written by exactly one thread, with no atomics, and the result does not depend on
// scheduling.  Every other logit of the row, and every row of a skipped or neutral slot, is not touched at all: a slot
// with neutral parameters (rp = 1, fq = 0, pr = 0) or L = 0 returns after reading its four parameters.
//
// Decode gate (chronos_hip.h): like the sampler and the logprob kernels, this one does not take the gate.  A closed gate
// means no slot of the bucket is live, which the per-slot test below already turns into an immediate return.
#include "chronos_hip.h"

namespace chronos {

constexpr int kPenMaxWindow = 1024;  // compile-time cap of the history window (EngineConfig.penalty_window)

template <typename LT>
__device__ __forceinline__ float pen_load(const LT* p, int64_t i);
template <>
__device__ __forceinline__ float pen_load<uint16_t>(const uint16_t* p, int64_t i) { return bf2f(p[i]); }
template <>
__device__ __forceinline__ float pen_load<float>(const float* p, int64_t i) { return p[i]; }

template <typename LT>
__device__ __forceinline__ void pen_store(LT* p, int64_t i, float x);
template <>
__device__ __forceinline__ void pen_store<uint16_t>(uint16_t* p, int64_t i, float x) { p[i] = f2bf(x); }
template <>
__device__ __forceinline__ void pen_store<float>(float* p, int64_t i, float x) { p[i] = x; }

template <typename LT>
__global__ void __launch_bounds__(kPenMaxWindow) apply_penalties_kernel(
    LT* __restrict__ logits, int64_t lstride, int width, const int32_t* __restrict__ row_of_slot, int done_state,
    const int32_t* __restrict__ state, const int32_t* __restrict__ nout, const int32_t* __restrict__ out_tokens,
    int max_out, const float* __restrict__ pen_par, const int32_t* __restrict__ pen_last,
    const int32_t* __restrict__ pen_tail, const int32_t* __restrict__ pen_tlen, int W) {
    __shared__ __attribute__((aligned(16))) int32_t win[kPenMaxWindow];
    const int slot = blockIdx.x;
    const int s = state[slot];
    if (s < 0 || s == done_state) return;
    const int row = row_of_slot ? row_of_slot[slot] : slot;
    if (row < 0) return;
    const int L = min(pen_last[slot], W);  // W <= blockDim.x: one window entry per thread
    const float rp = pen_par[slot * 3 + 0], fq = pen_par[slot * 3 + 1], pr = pen_par[slot * 3 + 2];
    if (L <= 0 || (rp == 1.f && fq == 0.f && pr == 0.f)) return;
    const int tl = min(max(pen_tlen[slot], 0), W);
    const int no = min(max(nout[slot], 0), max_out);
    const int total = tl + no;
    const int m = min(L, total);  // window entries: history positions [total - m, total)
    if (m <= 0) return;
    const int t = threadIdx.x;
    int mine = -1;
    const int m4 = (m + 3) & ~3;  // <= blockDim.x (a multiple of 64 that is >= W >= m)
    if (t < m) {
        const int g = total - m + t;
        mine = g < tl ? pen_tail[(int64_t)slot * W + g] : out_tokens[(int64_t)slot * max_out + (g - tl)];
        win[t] = mine;
    } else if (t < m4) {
        win[t] = -1;  // pads the last group of four: never equal to a valid id
    }
    __syncthreads();
    if (t >= m || mine < 0 || mine >= width) return;
    // four ids per 16-byte LDS read; every lane reads the same address: a broadcast, no bank conflict
    int count = 0, before = 0;
    for (int j = 0; j < m4; j += 4) {
        const int4 w = *reinterpret_cast<const int4*>(&win[j]);
        const int e0 = w.x == mine, e1 = w.y == mine, e2 = w.z == mine, e3 = w.w == mine;
        count += e0 + e1 + e2 + e3;
        before += (e0 & (j < t)) + (e1 & (j + 1 < t)) + (e2 & (j + 2 < t)) + (e3 & (j + 3 < t));
    }
    if (before) return;  // an earlier entry holds the same id: that thread writes the logit
    LT* lg = logits + (int64_t)row * lstride;
    float x = pen_load<LT>(lg, mine);
    // every step rounded on its own (no FMA contraction, IEEE division): the result is the fp32 formula's, bit for bit
    x = x <= 0.f ? __fmul_rn(x, rp) : __fdiv_rn(x, rp);
    x = __fsub_rn(x, __fadd_rn(__fmul_rn((float)count, fq), pr));
    pen_store<LT>(lg, mine, x);
}

void launch_apply_penalties(void* logits, bool logits_f32, int64_t lstride, int width, const int32_t* row_of_slot,
                            int nslots, int done_state, const int32_t* state, const int32_t* nout,
                            const int32_t* out_tokens, int max_out, const float* pen_par, const int32_t* pen_last,
                            const int32_t* pen_tail, const int32_t* pen_tlen, int W, hipStream_t st) {
    if (nslots == 0 || W <= 0) return;
    // one thread per window entry, whole waves (the binding rejects W > kPenMaxWindow)
    const int threads = W >= kPenMaxWindow ? kPenMaxWindow : (W + 63) / 64 * 64;
    if (logits_f32)
        hipLaunchKernelGGL(apply_penalties_kernel<float>, dim3(nslots), dim3(threads), 0, st, (float*)logits, lstride,
                           width, row_of_slot, done_state, state, nout, out_tokens, max_out, pen_par, pen_last,
                           pen_tail, pen_tlen, W);
    else
        hipLaunchKernelGGL(apply_penalties_kernel<uint16_t>, dim3(nslots), dim3(threads), 0, st, (uint16_t*)logits,
                           lstride, width, row_of_slot, done_state, state, nout, out_tokens, max_out, pen_par,
                           pen_last, pen_tail, pen_tlen, W);
}

}  // namespace chronos
