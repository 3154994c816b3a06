// logprobs.hip — per-token log-probabilities of the grammar-constrained sampler (sampler.hip), produced on the device
// inside the same (captured) decode step, so asking "how sure was the model" costs no host round trip per token.
//
// Two kernels bracket the sampler launch, one workgroup per slot like the sampler itself:
//
//   token_logprobs_kernel         BEFORE the sampler.  For a live slot that wants logprobs it reads the slot's logits
//                                 row and DFA row exactly as the sampler is about to (same legality: next[s][v] >= 0 and
//                                 dist[next[s][v]] <= remaining - 1) and writes, into per-slot scratch,
//                                   lp_lse       logsumexp over the legal tokens' raw logits (fp32, max subtracted),
//                                   lp_top_*     the K legal tokens with the largest logits as (id, raw logit), ordered
//                                                by logit descending then id ascending, tail (id -1, -inf),
//                                   lp_mark      nout[slot]: the output index the sampler is about to fill.
//                                 Every other slot (empty, parked, DONE, not sampled in this launch, not wanted) gets
//                                 lp_mark = -1 and nothing else.
//   token_logprobs_commit_kernel  AFTER the sampler.  Where the sampler did emit output index lp_mark (nout advanced by
//                                 one) it writes ring entry [slot, lp_mark]: the chosen token's logprob and the top-K
//                                 (id, logprob) pairs.  It writes nothing else and never past max_out.
//
// Top-K of ~128k tokens: the sampler's exact radix select on the monotone 16-bit logit key (two 256-bin LDS histograms:
// high byte, then low byte inside the bin that crosses K) gives the key of the K-th largest legal logit.  Tokens
// strictly above it (< K of them) and the tokens of that boundary key are ranked in LDS by (exact fp32 logit
// descending, id ascending): the 16-bit key merges distinct fp32 logits, the ranking does not.
// Usually the row is streamed twice: pass 1 keeps a running (max, sum of exp) per thread for the logsumexp and builds
// the high-byte histogram; pass 2 gathers every token of the crossing bin and above into LDS (up to 4 096), where the
// low-byte select and the ranking run without touching memory again.  A crossing bin wider than the list costs a third
// pass (low-byte histogram over the row, then the gather), and a boundary KEY shared by more tokens than the list holds
// (a plateau of equal logits thousands wide) is resolved by one arg-max pass over the row per missing entry.
//
// Decode gate (chronos_hip.h): like the sampler, neither kernel takes the gate.  A closed gate means no slot of the
// bucket is live, which the per-slot test below already turns into lp_mark = -1 and an immediate return; and the commit
// kernel runs after the sampler may have closed the gate with the very token it has to record.
#include "chronos_hip.h"

namespace chronos {

constexpr int kLpMaxTop = 20;    // Ollama's top_logprobs cap
constexpr int kLpCand = 4096;    // LDS candidate list (the tokens of the K-th largest logit's key bin and above)
constexpr int kLpSmall = 256;    // compacted list of the candidates at or above the 16-bit threshold key

template <typename LT>
__device__ __forceinline__ float lp_logit_at(const LT* p, int64_t i);
template <>
__device__ __forceinline__ float lp_logit_at<uint16_t>(const uint16_t* p, int64_t i) { return bf2f(p[i]); }
template <>
__device__ __forceinline__ float lp_logit_at<float>(const float* p, int64_t i) { return p[i]; }

// Monotone 16-bit key of a logit's bf16 rounding (sampler.hip ord_key).  -0 is folded into +0 first: the two compare
// equal as logits, so they must share a key (ties are broken by token id, not by the sign of zero).
__device__ __forceinline__ uint32_t lp_key(float x) {
    if (x == 0.f) x = 0.f;
    const uint32_t b = f2bf(x);
    return (b & 0x8000u) ? (~b & 0xFFFFu) : (b | 0x8000u);
}

// (va, ia) ranks before (vb, ib): larger logit first, then smaller token id
__device__ __forceinline__ bool lp_before(float va, int ia, float vb, int ib) {
    return va > vb || (va == vb && ia < ib);
}

// One count into an LDS histogram per (wave, distinct bin) instead of one per lane: logits crowd into a handful of
// high-byte bins, and same-address LDS atomics serialise.  Called by every lane of the wave that is in the loop.
__device__ __forceinline__ void lp_hist_add(int* h, uint32_t bin, bool active) {
    uint64_t todo = __ballot(active);
    while (todo) {
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const uint32_t b = __shfl(bin, leader, 64);
        const uint64_t same = __ballot(active && bin == b);
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&h[b], __popcll(same));
        todo &= ~same;
    }
}

// f(v, logit, legal) for every token v of [begin, end) (begin a multiple of 8 * blockDim.x), each token exactly once
// (order unspecified across threads); called by all lanes that hold a token, so f may use wave-wide ballots.
// VEC: 8 consecutive tokens per thread per iteration (16-byte loads of the DFA row and the logits row).
template <typename LT, bool VEC, typename F>
__device__ __forceinline__ void lp_for_legal(const LT* lg, const int16_t* nx, const int16_t* dist, int budget,
                                             int begin, int end, F f) {
    if constexpr (VEC) {
        // two iterations' loads are issued before either is consumed: with one workgroup per row a lone row has nothing
        // else to hide the memory latency behind
        constexpr int U = 2;
        const int stride = blockDim.x * 8;
        for (int v0 = begin + threadIdx.x * 8; v0 < end; v0 += stride * U) {
            int4 nv[U];
            float x[U][8];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int vu = v0 + u * stride;
                if (vu >= end) continue;
                nv[u] = *reinterpret_cast<const int4*>(nx + vu);
                if constexpr (sizeof(LT) == 2) {
                    const u16x8 lv = *reinterpret_cast<const u16x8*>(reinterpret_cast<const uint16_t*>(lg) + vu);
#pragma unroll
                    for (int j = 0; j < 8; ++j) x[u][j] = bf2f(lv[j]);
                } else {
                    const float4 a = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(lg) + vu);
                    const float4 b = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(lg) + vu + 4);
                    x[u][0] = a.x; x[u][1] = a.y; x[u][2] = a.z; x[u][3] = a.w;
                    x[u][4] = b.x; x[u][5] = b.y; x[u][6] = b.z; x[u][7] = b.w;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int vu = v0 + u * stride;
                if (vu >= end) continue;
                const int nw32[4] = {nv[u].x, nv[u].y, nv[u].z, nv[u].w};
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int ns = (int)(int16_t)(nw32[j >> 1] >> (16 * (j & 1)));
                    f(vu + j, x[u][j], ns >= 0 && dist[ns] <= budget);
                }
            }
        }
    } else {
        for (int v = begin + threadIdx.x; v < end; v += blockDim.x) {
            const int ns = nx[v];
            f(v, lp_logit_at<LT>(lg, v), ns >= 0 && dist[ns] <= budget);
        }
    }
}

// Largest bin b (scanning down from 255) with start + count(bins > b) + h[b] >= k, with above = start + count(bins > b)
// and in_bin = h[b]; bin 0 if no bin crosses k.  Called by all 64 lanes of one wave (4 bins per lane, a suffix sum
// over the lanes): a single lane walking 256 dependent LDS reads costs more than a pass over the logits row.
__device__ __forceinline__ void lp_scan(const int* h, int k, int start, uint32_t& bin, int& above, int& in_bin) {
    const int lane = threadIdx.x & 63;
    const int c0 = h[4 * lane], c1 = h[4 * lane + 1], c2 = h[4 * lane + 2], c3 = h[4 * lane + 3];
    const int tot = c0 + c1 + c2 + c3;
    int suf = tot;  // this lane's bins and every bin above them
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_down(suf, o, 64);
        if (lane + o < 64) suf += t;
    }
    const uint64_t m = __ballot(start + suf >= k);
    const int L = m ? 63 - __clzll((unsigned long long)m) : 0;  // the lane whose bins cross k (none: lane 0, bin 0)
    int b = 0, ab = start + suf - c0, ib = c0;
    int cnt = start + suf - tot;
    if (m) {
        if (cnt + c3 >= k) {
            b = 3; ab = cnt; ib = c3;
        } else if (cnt + c3 + c2 >= k) {
            b = 2; ab = cnt + c3; ib = c2;
        } else if (cnt + c3 + c2 + c1 >= k) {
            b = 1; ab = cnt + c3 + c2; ib = c1;
        }
    }
    bin = (uint32_t)__shfl(4 * lane + b, L, 64);
    above = __shfl(ab, L, 64);
    in_bin = __shfl(ib, L, 64);
}

template <typename LT, bool VEC>
__global__ void __launch_bounds__(1024) token_logprobs_kernel(
    const LT* __restrict__ logits, int64_t lstride, const int32_t* __restrict__ row_of_slot, int vocab,
    const int16_t* __restrict__ next, const int16_t* __restrict__ dist, int done_state,
    const int32_t* __restrict__ state, const int32_t* __restrict__ remaining, const int32_t* __restrict__ nout,
    const int32_t* __restrict__ lp_want, int32_t* __restrict__ lp_mark, float* __restrict__ lp_lse,
    int32_t* __restrict__ lp_top_ids, float* __restrict__ lp_top_val, int K) {
    __shared__ float red[16];
    __shared__ int redi[16];
    __shared__ int hc[256];
    __shared__ float cand_v[kLpCand];
    __shared__ int cand_i[kLpCand];
    __shared__ float top_v[kLpSmall];
    __shared__ int top_i[kLpSmall];
    __shared__ int sh_n, sh_m, sh_above, sh_cb, sh_early;
    __shared__ uint32_t sh_bk, sh_thr, sh_floor;
    const int slot = blockIdx.x;
    const int s = state[slot];
    const int row = (s < 0 || s == done_state) ? -1 : (row_of_slot ? row_of_slot[slot] : slot);
    if (row < 0 || lp_want[slot] < 0) {  // the sampler skips this slot, or nobody asked
        if (threadIdx.x == 0) lp_mark[slot] = -1;
        return;
    }
    const LT* lg = logits + (int64_t)row * lstride;
    const int16_t* nx = next + (int64_t)s * vocab;
    const int budget = remaining[slot] - 1;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int32_t* tid_out = lp_top_ids + (int64_t)slot * K;
    float* tval_out = lp_top_val + (int64_t)slot * K;

    // ---- pass 1: running (max, sum of exp) per thread, legal count, histogram of the keys' high bytes -----------------
    // The histogram only has to be exact from the bin of the K-th largest logit upwards.  The first 8 * blockDim tokens
    // are counted in full; the bin in which THEIR K-th largest falls is a floor (the row's K-th largest cannot be
    // below it), and the rest of the row only counts tokens at or above that floor: a few per cent of them, so the LDS
    // atomics stay off the critical path of what is otherwise a streaming pass.
    for (int i = threadIdx.x; i < 256; i += blockDim.x) hc[i] = 0;
    if (threadIdx.x == 0) {
        sh_n = 0;
        sh_m = 0;
    }
    __syncthreads();
    float mx = -INFINITY, sum = 0.f;
    int nleg = 0;
    auto softmax_step = [&](float x) {
        if (x > mx) {
            sum = sum * __expf(mx - x) + 1.f;
            mx = x;
        } else if (x > -INFINITY) {
            sum += __expf(x - mx);
        }
    };
    const int head = min(vocab, (int)blockDim.x * 8);
    lp_for_legal<LT, VEC>(lg, nx, dist, budget, 0, head, [&](int, float x, bool ok) {
        if (ok) {
            softmax_step(x);
            ++nleg;
        }
        lp_hist_add(hc, lp_key(x) >> 8, ok);
    });
    __syncthreads();
    if (threadIdx.x < 64) {
        uint32_t fl;
        int ab, ib;
        lp_scan(hc, K, 0, fl, ab, ib);
        if (lane == 0) sh_floor = ab + ib >= K ? fl : 0u;  // fewer than K legal tokens so far: count everything
    }
    __syncthreads();
    const uint32_t floor_bin = sh_floor;
    lp_for_legal<LT, VEC>(lg, nx, dist, budget, head, vocab, [&](int, float x, bool ok) {
        if (ok) {
            softmax_step(x);
            ++nleg;
        }
        const uint32_t hb = lp_key(x) >> 8;
        lp_hist_add(hc, hb, ok && hb >= floor_bin);
    });
    // block-wide: max, then the sums rescaled to it, and the legal count
    const float wmx = wave_max(mx);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nleg += __shfl_xor(nleg, o, 64);
    if (lane == 0) {
        red[w] = wmx;
        redi[w] = nleg;
    }
    __syncthreads();
    float bmx = red[0];
    int nlegal = redi[0];
    for (int k = 1; k < nw; ++k) {
        bmx = fmaxf(bmx, red[k]);
        nlegal += redi[k];
    }
    if (nlegal == 0) {  // no legal token (malformed DFA): the sampler closes the row without emitting anything
        if (threadIdx.x == 0) lp_mark[slot] = -1;
        return;
    }
    const float mxs = bmx == -INFINITY ? 0.f : bmx;  // every legal logit -inf: the sum is 0 and the lse -inf, not NaN
    sum = wave_sum(sum * __expf(mx - mxs));  // (a thread without a legal token: 0 * exp(-inf) = 0)
    __syncthreads();  // red[] was read above
    if (lane == 0) red[w] = sum;
    __syncthreads();
    const int kp = nlegal < K ? nlegal : K;
    if (threadIdx.x < 64) {
        uint32_t bk;
        int ab, ib;
        lp_scan(hc, kp, 0, bk, ab, ib);  // (bk >= the floor: the histogram is exact from bk upwards)
        if (lane == 0) {
            float z = 0.f;
            for (int k = 0; k < nw; ++k) z += red[k];
            lp_lse[slot] = mxs + logf(z);
            sh_bk = bk;
            sh_above = ab;
            sh_early = ab + ib <= kLpCand;  // every token of bin bk and above fits the LDS list: one more pass, not two
        }
    }
    __syncthreads();
    const uint32_t bk = sh_bk;
    const bool early = sh_early != 0;
    uint32_t thr;
    int above;
    bool fits;
    int nc;
    if (early) {
        // ---- pass 2 (usual): gather every legal token of high-byte bin >= bk; the low-byte select runs on the list ----
        lp_for_legal<LT, VEC>(lg, nx, dist, budget, 0, vocab, [&](int v, float x, bool ok) {
            if (ok && (lp_key(x) >> 8) >= bk) {
                const int p = atomicAdd(&sh_n, 1);
                if (p < kLpCand) {
                    cand_v[p] = x;
                    cand_i[p] = v;
                }
            }
        });
        for (int i = threadIdx.x; i < 256; i += blockDim.x) hc[i] = 0;
        __syncthreads();
        nc = sh_n < kLpCand ? sh_n : kLpCand;
        for (int e = threadIdx.x; e < nc; e += blockDim.x) {
            const uint32_t kk = lp_key(cand_v[e]);
            if ((kk >> 8) == bk) atomicAdd(&hc[kk & 255], 1);
        }
        __syncthreads();
        if (threadIdx.x < 64) {
            uint32_t lo;
            int ab, ib;
            lp_scan(hc, kp, sh_above, lo, ab, ib);
            if (lane == 0) {
                sh_thr = (bk << 8) | lo;
                sh_above = ab;
                sh_cb = ib;
            }
        }
        __syncthreads();
        thr = sh_thr;
        above = sh_above;
        fits = true;
    } else {
        // ---- pass 2 + 3 (bin bk alone overflows the list): low-byte histogram over the row, then gather ---------------
        for (int i = threadIdx.x; i < 256; i += blockDim.x) hc[i] = 0;
        __syncthreads();
        lp_for_legal<LT, VEC>(lg, nx, dist, budget, 0, vocab, [&](int, float x, bool ok) {
            const uint32_t kk = lp_key(x);
            if (ok && (kk >> 8) == bk) atomicAdd(&hc[kk & 255], 1);
        });
        __syncthreads();
        if (threadIdx.x < 64) {
            uint32_t lo;
            int ab, ib;
            lp_scan(hc, kp, sh_above, lo, ab, ib);
            if (lane == 0) {
                sh_thr = (bk << 8) | lo;
                sh_above = ab;  // legal tokens with key > thr: fewer than kp
                sh_cb = ib;     // legal tokens with key == thr: above + cb >= kp
            }
        }
        __syncthreads();
        thr = sh_thr;
        above = sh_above;
        fits = above + sh_cb <= kLpCand;
        lp_for_legal<LT, VEC>(lg, nx, dist, budget, 0, vocab, [&](int v, float x, bool ok) {
            const uint32_t kk = lp_key(x);
            if (ok && (kk > thr || (fits && kk == thr))) {
                const int p = atomicAdd(&sh_n, 1);
                if (p < kLpCand) {
                    cand_v[p] = x;
                    cand_i[p] = v;
                }
            }
        });
        __syncthreads();
        nc = sh_n < kLpCand ? sh_n : kLpCand;
    }
    // ---- rank the candidates with key >= thr among themselves (LDS broadcast reads); ranks below kp are the answer ----
    // (a candidate below thr has at least kp tokens before it, and is before none of those at or above thr)
    const float* rv = cand_v;
    const int* ri = cand_i;
    int rn = nc;
    if (early && above + sh_cb <= kLpSmall) {  // usual: a few dozen survive; compact them so the ranking loop is short
        for (int e = threadIdx.x; e < nc; e += blockDim.x) {
            const float ve = cand_v[e];
            if (lp_key(ve) >= thr) {
                const int p = atomicAdd(&sh_m, 1);
                if (p < kLpSmall) {
                    top_v[p] = ve;
                    top_i[p] = cand_i[e];
                }
            }
        }
        __syncthreads();
        rv = top_v;
        ri = top_i;
        rn = sh_m < kLpSmall ? sh_m : kLpSmall;
    }
    for (int e = threadIdx.x; e < rn; e += blockDim.x) {
        const float ve = rv[e];
        const int ie = ri[e];
        if (lp_key(ve) < thr) continue;
        int rank = 0;
        for (int j = 0; j < rn; ++j) rank += lp_before(rv[j], ri[j], ve, ie) ? 1 : 0;
        if (rank < kp) {
            tid_out[rank] = ie;
            tval_out[rank] = ve;
        }
    }
    if (!fits) {
        // The boundary key is a plateau wider than the LDS list: take its kp - above best tokens one arg-max pass at a
        // time, each pass restricted to the tokens that rank after the previous pick.
        float pv = INFINITY;
        int pi = -1;
        for (int r = above; r < kp; ++r) {
            float bv = -INFINITY;
            int bi = 0x7fffffff;
            lp_for_legal<LT, VEC>(lg, nx, dist, budget, 0, vocab, [&](int v, float x, bool ok) {
                if (ok && lp_key(x) == thr && lp_before(pv, pi, x, v) && (bi == 0x7fffffff || lp_before(x, v, bv, bi))) {
                    bv = x;
                    bi = v;
                }
            });
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (oi != 0x7fffffff && (bi == 0x7fffffff || lp_before(ov, oi, bv, bi))) {
                    bv = ov;
                    bi = oi;
                }
            }
            __syncthreads();  // red/redi of the previous round (or of pass 1) were read
            if (lane == 0) {
                red[w] = bv;
                redi[w] = bi;
            }
            __syncthreads();
            bv = red[0];
            bi = redi[0];
            for (int k = 1; k < nw; ++k)
                if (redi[k] != 0x7fffffff && (bi == 0x7fffffff || lp_before(red[k], redi[k], bv, bi))) {
                    bv = red[k];
                    bi = redi[k];
                }
            if (bi == 0x7fffffff) break;  // (cannot happen: the histogram counted at least kp - above of them)
            if (threadIdx.x == 0) {
                tid_out[r] = bi;
                tval_out[r] = bv;
            }
            pv = bv;
            pi = bi;
        }
    }
    for (int j = kp + threadIdx.x; j < K; j += blockDim.x) {  // fewer legal tokens than K
        tid_out[j] = -1;
        tval_out[j] = -INFINITY;
    }
    if (threadIdx.x == 0) lp_mark[slot] = nout[slot];
}

template <typename LT>
__global__ void __launch_bounds__(64) token_logprobs_commit_kernel(
    const LT* __restrict__ logits, int64_t lstride, int lcols, const int32_t* __restrict__ row_of_slot,
    const int32_t* __restrict__ nout, const int32_t* __restrict__ out_tokens, int max_out,
    const int32_t* __restrict__ lp_want, const int32_t* __restrict__ lp_mark, const float* __restrict__ lp_lse,
    const int32_t* __restrict__ lp_top_ids, const float* __restrict__ lp_top_val, int K,
    float* __restrict__ out_lp, int32_t* __restrict__ out_lp_ids) {
    const int slot = blockIdx.x;
    const int i = lp_mark[slot];
    if (i < 0 || i >= max_out || lp_want[slot] < 0 || nout[slot] != i + 1) return;
    const int row = row_of_slot ? row_of_slot[slot] : slot;
    if (row < 0) return;  // (the pre-kernel marks such a slot -1; kept so a stale mark can never index the logits)
    const float lse = lp_lse[slot];
    float* lp = out_lp + ((int64_t)slot * max_out + i) * (1 + K);
    int32_t* li = out_lp_ids + ((int64_t)slot * max_out + i) * K;
    const int j = threadIdx.x;
    if (j == 0) {
        const int tok = out_tokens[(int64_t)slot * max_out + i];
        lp[0] = (tok >= 0 && tok < lcols) ? lp_logit_at<LT>(logits + (int64_t)row * lstride, tok) - lse : -INFINITY;
    }
    for (int t = j; t < K; t += blockDim.x) {
        lp[1 + t] = lp_top_val[(int64_t)slot * K + t] - lse;
        li[t] = lp_top_ids[(int64_t)slot * K + t];
    }
}

void launch_token_logprobs(const void* logits, bool logits_f32, int64_t lstride, const int32_t* row_of_slot,
                           int nslots, int vocab, const int16_t* next, const int16_t* dist, int done_state,
                           const int32_t* state, const int32_t* remaining, const int32_t* nout,
                           const int32_t* lp_want, int32_t* lp_mark, float* lp_lse, int32_t* lp_top_ids,
                           float* lp_top_val, int K, hipStream_t st) {
    if (nslots == 0 || K < 0 || K > kLpMaxTop) return;  // (K is validated by the binding)
    const size_t esz = logits_f32 ? 4 : 2;
    const bool vec = ((uintptr_t)logits % 16 == 0) && ((size_t)lstride * esz) % 16 == 0 &&
                     ((uintptr_t)next % 16 == 0) && (vocab & 7) == 0;
#define LP_LAUNCH(LT, V)                                                                                           \
    hipLaunchKernelGGL((token_logprobs_kernel<LT, V>), dim3(nslots), dim3(1024), 0, st, (const LT*)logits, lstride, \
                       row_of_slot, vocab, next, dist, done_state, state, remaining, nout, lp_want, lp_mark, lp_lse, \
                       lp_top_ids, lp_top_val, K)
    if (logits_f32) {
        if (vec) LP_LAUNCH(float, true); else LP_LAUNCH(float, false);
    } else {
        if (vec) LP_LAUNCH(uint16_t, true); else LP_LAUNCH(uint16_t, false);
    }
#undef LP_LAUNCH
}

void launch_token_logprobs_commit(const void* logits, bool logits_f32, int64_t lstride, int lcols,
                                  const int32_t* row_of_slot, int nslots, const int32_t* nout,
                                  const int32_t* out_tokens, int max_out, const int32_t* lp_want,
                                  const int32_t* lp_mark, const float* lp_lse, const int32_t* lp_top_ids,
                                  const float* lp_top_val, int K, float* out_lp, int32_t* out_lp_ids, hipStream_t st) {
    if (nslots == 0 || K < 0 || K > kLpMaxTop) return;
    if (logits_f32)
        hipLaunchKernelGGL(token_logprobs_commit_kernel<float>, dim3(nslots), dim3(64), 0, st, (const float*)logits,
                           lstride, lcols, row_of_slot, nout, out_tokens, max_out, lp_want, lp_mark, lp_lse,
                           lp_top_ids, lp_top_val, K, out_lp, out_lp_ids);
    else
        hipLaunchKernelGGL(token_logprobs_commit_kernel<uint16_t>, dim3(nslots), dim3(64), 0, st,
                           (const uint16_t*)logits, lstride, lcols, row_of_slot, nout, out_tokens, max_out, lp_want,
                           lp_mark, lp_lse, lp_top_ids, lp_top_val, K, out_lp, out_lp_ids);
}

}  // namespace chronos
