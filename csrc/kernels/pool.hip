// pool.hip — sequence embeddings from the prefill path: pooling of the final-RMSNorm hidden state on the device.
//
// An embedding request ends after its prompt.  What it returns is the direction of
//     g (.) sum_t  s_t * rsqrt(mean(s_t^2) + eps)
// over the pooled tokens t of the sequence, with s_t the un-normalised residual stream after the last layer and g the
// final norm weight.  g is constant over tokens, so it is applied once, to the sum (pool_finish), and the token count
// cancels in the L2 normalisation: "mean" pooling is the direction of the sum.
//
//   pool_accum   acc[sel[b], :] += sum over rows r in [q_rows[b][0], q_rows[b][1]) of s[r, :] * rsqrt(mean(s[r, :]^2) + eps)
//                for every sequence b with sel[b] >= 0, all in fp32.  The normalised row exists in registers only: never
//                rounded to bf16, never written; s is read once, 16 B per lane.  A prompt that prefills in several
//                chunks calls it once per chunk into the same accumulator row.  Three launches:
//                  plan     one workgroup: cuts every selected range into segments of kPoolSeg rows (the segment
//                           length doubles, for every sequence alike, until the items fit the scratch the host sized
//                           from T and B alone: never for ranges that do not overlap), prefix-sums the segment
//                           counts and lists the sequence of every work item;
//                  partial  one workgroup per item: the segment's rows, kPoolRows at a time in flight, each row's sum
//                           of squares through the block reduction, the column sums in row order.  A sequence of one
//                           segment adds straight into its accumulator row, any other writes a scratch row;
//                  reduce   per sequence of several segments: scratch rows summed in segment order, added to acc.
//                No floating-point atomics and no order that depends on scheduling: the same call gives the same bits
//                on every launch.  Rows outside every range are never read; a range is clipped to [0, T), a sel
//                outside [0, S) counts as -1.  Two sequences must not select the same accumulator row.
//   pool_finish  per listed accumulator row: v = g (.) acc[row], out[i] = v / ||v||_2 (zeros when the norm is 0), then
//                acc[row] <- 0 for the slot's next request.  One workgroup per row, the row held in registers.
//
// H is one of 256, 1024, 4096, 8192 (the presets' hidden sizes): a row is H / 8 pieces of 16 B.  At H = 256 that is
// 32 pieces, fewer than a wave has lanes: the workgroup is one wave whose halves take alternate rows, each half
// reduces its own row's squares, and the halves' column sums are added at the end.
#include "chronos_hip.h"

namespace chronos {

constexpr int kPoolSeg = 32;        // rows per segment (before any doubling)
constexpr int kPoolRows = 4;        // rows in flight per row group
constexpr int kPoolPlanThreads = 1024;
constexpr int kPoolMaxSeqs = 4 * kPoolPlanThreads;

__device__ __forceinline__ int pool_nseg(const int32_t* q_rows, const int32_t* sel, int b, int B, int T, int S,
                                         int seg) {
    if (b >= B) return 0;
    const int row = sel[b];
    if (row < 0 || row >= S) return 0;
    const int lo = max(q_rows[2 * b], 0), hi = min(q_rows[2 * b + 1], T);
    return hi > lo ? (hi - lo + seg - 1) / seg : 0;
}

// plan[0] = segment length, plan[1] = number of items, plan[2 + b] = first item of sequence b (b = 0..B),
// plan[2 + B + 1 + i] = sequence of item i
__global__ void __launch_bounds__(kPoolPlanThreads) pool_plan_kernel(
    const int32_t* __restrict__ q_rows, const int32_t* __restrict__ sel, int B, int T, int S, int max_items,
    int32_t* __restrict__ plan) {
    __shared__ int start[kPoolMaxSeqs + 1];
    __shared__ int scan[kPoolPlanThreads];
    const int t = threadIdx.x;
    int seg = kPoolSeg, total = 0;
    for (;;) {
        int n[4], mine = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            n[k] = pool_nseg(q_rows, sel, 4 * t + k, B, T, S, seg);
            mine += n[k];
        }
        scan[t] = mine;
        __syncthreads();
        for (int o = 1; o < kPoolPlanThreads; o <<= 1) {  // inclusive scan
            const int v = t >= o ? scan[t - o] : 0;
            __syncthreads();
            scan[t] += v;
            __syncthreads();
        }
        total = scan[kPoolPlanThreads - 1];
        int at = scan[t] - mine;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            start[4 * t + k] = at;
            at += n[k];
        }
        if (t == kPoolPlanThreads - 1) start[kPoolMaxSeqs] = total;
        __syncthreads();
        if (total <= max_items || seg >= (1 << 30)) break;
        seg <<= 1;  // (uniform: every thread read the same total)
    }
    if (t == 0) {
        plan[0] = seg;
        plan[1] = min(total, max_items);
    }
    for (int b = t; b <= B; b += kPoolPlanThreads) plan[2 + b] = b < B ? start[b] : total;
    int32_t* item_seq = plan + 2 + B + 1;
    for (int i = t; i < min(total, max_items); i += kPoolPlanThreads) {
        int lo = 0, hi = B - 1;  // the last b with start[b] <= i (empty sequences share a start: take the last)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (start[mid] <= i) lo = mid; else hi = mid - 1;
        }
        item_seq[i] = lo;
    }
}

// NT threads; a row group is GW = min(H / 8, NT) threads wide and there are RG = NT / GW of them (2 at H = 256, else
// 1); a thread owns PPT = H / 8 / GW pieces of 8 columns: piece p of its row at columns (p * GW + lane-in-group) * 8.
template <int H, int NT>
__global__ void __launch_bounds__(NT) pool_partial_kernel(
    const uint16_t* __restrict__ s, int T, float eps, const int32_t* __restrict__ q_rows,
    const int32_t* __restrict__ sel, int B, const int32_t* __restrict__ plan, float* __restrict__ scratch,
    float* __restrict__ acc) {
    constexpr int P = H / 8;
    constexpr int GW = P < NT ? P : NT;
    constexpr int RG = NT / GW;
    constexpr int PPT = P / GW;
    constexpr int NW = NT / 64;
    static_assert(GW * PPT == P && RG * GW == NT && (RG == 1 || NT == 64), "pool: shape");
    __shared__ float red[NW > 1 ? NW * kPoolRows : 1];

    const int item = blockIdx.x;
    if (item >= plan[1]) return;
    const int seg = plan[0];
    const int b = plan[2 + B + 1 + item];
    const int first = plan[2 + b], nseg = plan[2 + b + 1] - first;
    const int lo = max(q_rows[2 * b], 0), hi = min(q_rows[2 * b + 1], T);
    const int r0 = lo + (item - first) * seg;
    const int r1 = min(hi, r0 + seg);  // (seg <= 2^30 and r0 < T: no overflow)
    const int t = threadIdx.x, g = t / GW, c = t % GW;

    float sum[PPT][8];
#pragma unroll
    for (int p = 0; p < PPT; ++p)
#pragma unroll
        for (int e = 0; e < 8; ++e) sum[p][e] = 0.f;

    for (int base = r0; base < r1; base += kPoolRows * RG) {
        u16x8 x[kPoolRows][PPT];
        float ss[kPoolRows];
#pragma unroll
        for (int k = 0; k < kPoolRows; ++k) {  // row base + k * RG + g; every load of the iteration is issued first
            const int r = base + k * RG + g;
#pragma unroll
            for (int p = 0; p < PPT; ++p) {
                if (r < r1)
                    x[k][p] = *reinterpret_cast<const u16x8*>(s + (int64_t)r * H + (p * GW + c) * 8);
                else
                    x[k][p] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
            }
        }
#pragma unroll
        for (int k = 0; k < kPoolRows; ++k) {
            float q = 0.f;
#pragma unroll
            for (int p = 0; p < PPT; ++p)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float v = bf2f(x[k][p][e]);
                    q += v * v;
                }
#pragma unroll
            for (int o = (GW < 64 ? GW : 64) / 2; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);  // within the row group
            ss[k] = q;
        }
        if constexpr (NW > 1) {  // block_sum's order (wave sums, then the waves in order), kPoolRows rows at a time
            const int lane = t & 63, w = t >> 6;
            if (lane == 0)
#pragma unroll
                for (int k = 0; k < kPoolRows; ++k) red[w * kPoolRows + k] = ss[k];
            __syncthreads();
#pragma unroll
            for (int k = 0; k < kPoolRows; ++k) {
                float q = red[k];
#pragma unroll
                for (int ww = 1; ww < NW; ++ww) q += red[ww * kPoolRows + k];
                ss[k] = q;
            }
            __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < kPoolRows; ++k) {
            if (base + k * RG + g >= r1) continue;  // (a padded row would be 0 * rsqrt(0 + eps): NaN at eps = 0)
            // (once per row: the correctly rounded square root and quotient, exact where the mean square is a power of 4)
            const float rinv = 1.f / sqrtf(ss[k] * (1.f / (float)H) + eps);
#pragma unroll
            for (int p = 0; p < PPT; ++p)
#pragma unroll
                for (int e = 0; e < 8; ++e) sum[p][e] += bf2f(x[k][p][e]) * rinv;
        }
    }
    if constexpr (RG == 2) {  // one wave, two row groups: lower half + upper half
#pragma unroll
        for (int e = 0; e < 8; ++e) sum[0][e] += __shfl_xor(sum[0][e], 32, 64);
        if (g != 0) return;
    }
    const bool direct = nseg == 1;
    float* dst = direct ? acc + (int64_t)sel[b] * H : scratch + (int64_t)item * H;
#pragma unroll
    for (int p = 0; p < PPT; ++p) {
        f32x4* d = reinterpret_cast<f32x4*>(dst + (p * GW + c) * 8);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            f32x4 v{sum[p][4 * h], sum[p][4 * h + 1], sum[p][4 * h + 2], sum[p][4 * h + 3]};
            if (direct) {
                const f32x4 a = d[h];
                v = a + v;
            }
            d[h] = v;
        }
    }
}

// grid (B, H / 1024): thread = 4 columns; scratch rows of the sequence's items in order, then += into acc
__global__ void __launch_bounds__(256) pool_reduce_kernel(const int32_t* __restrict__ sel, int B, int H,
                                                          const int32_t* __restrict__ plan,
                                                          const float* __restrict__ scratch, float* __restrict__ acc) {
    const int b = blockIdx.x;
    const int col = (blockIdx.y * 256 + threadIdx.x) * 4;
    if (col >= H) return;
    const int nitems = plan[1];
    const int first = plan[2 + b];
    const int last = min(plan[2 + b + 1], nitems);
    if (last - first < 2) return;  // nothing selected, or added by the partial kernel itself
    f32x4 v = *reinterpret_cast<const f32x4*>(scratch + (int64_t)first * H + col);
    for (int i = first + 1; i < last; ++i) v += *reinterpret_cast<const f32x4*>(scratch + (int64_t)i * H + col);
    f32x4* d = reinterpret_cast<f32x4*>(acc + (int64_t)sel[b] * H + col);
    *d = *d + v;
}

// one workgroup of 256 per listed row; thread t holds columns (k * 256 + t) * 4, k < H / 1024
__global__ void __launch_bounds__(256) pool_finish_kernel(float* __restrict__ acc, int S, int H,
                                                          const int32_t* __restrict__ rows,
                                                          const uint16_t* __restrict__ g, float* __restrict__ out) {
    __shared__ float red[16];
    constexpr int kMaxK = 8;  // H <= 8192
    const int i = blockIdx.x, t = threadIdx.x;
    const int row = rows[i];
    const bool ok = row >= 0 && row < S;  // (uniform over the workgroup)
    f32x4 v[kMaxK];
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
        const int col = (k * 256 + t) * 4;
        v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (ok && col < H) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(acc + (int64_t)row * H + col);
            const u16x4 w = *reinterpret_cast<const u16x4*>(g + col);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[k][e] = a[e] * bf2f(w[e]);
                q += v[k][e] * v[k][e];
            }
        }
    }
    q = block_sum(q, red);
    const float inv = q > 0.f ? 1.f / sqrtf(q) : 0.f;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
        const int col = (k * 256 + t) * 4;
        if (col < H) {
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = q > 0.f ? v[k][e] * inv : 0.f;
            *reinterpret_cast<f32x4*>(out + (int64_t)i * H + col) = o;
            if (ok) *reinterpret_cast<f32x4*>(acc + (int64_t)row * H + col) = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
}

int pool_max_items(int T, int B) { return (T + kPoolSeg - 1) / kPoolSeg + B; }
int pool_max_seqs() { return kPoolMaxSeqs; }

// plan: int32 [2 + B + 1 + max_items]; scratch: f32 [max_items, H]
void launch_pool_accum(const uint16_t* s, int T, int H, float eps, const int32_t* q_rows, const int32_t* sel, int B,
                       float* acc, int S, int32_t* plan, float* scratch, hipStream_t st) {
    if (B == 0 || T == 0) return;
    const int items = pool_max_items(T, B);
    hipLaunchKernelGGL(pool_plan_kernel, dim3(1), dim3(kPoolPlanThreads), 0, st, q_rows, sel, B, T, S, items, plan);
#define CHRONOS_POOL(HH, NT)                                                                                       \
    hipLaunchKernelGGL((pool_partial_kernel<HH, NT>), dim3(items), dim3(NT), 0, st, s, T, eps, q_rows, sel, B, plan, \
                       scratch, acc)
    switch (H) {
        case 256: CHRONOS_POOL(256, 64); break;
        case 1024: CHRONOS_POOL(1024, 128); break;
        case 4096: CHRONOS_POOL(4096, 256); break;
        default: CHRONOS_POOL(8192, 256); break;  // (the binding admits no other H)
    }
#undef CHRONOS_POOL
    hipLaunchKernelGGL(pool_reduce_kernel, dim3(B, (H + 1023) / 1024), dim3(256), 0, st, sel, B, H, plan, scratch, acc);
}

void launch_pool_finish(float* acc, int S, int H, const int32_t* rows, int n, const uint16_t* g, float* out,
                        hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(pool_finish_kernel, dim3(n), dim3(256), 0, st, acc, S, H, rows, g, out);
}

}  // namespace chronos
