// gemm_w4m.hip — fused W4A16 MFMA GEMM for mid M (65-512 rows: the 65-512-stream decode buckets, mixed steps and
// prefill chunks of an mxfp4 model), the step after gemm_skinny.hip's W4A16 mode (M <= 64).
//
//   y[M, N] = x[M, K] · dequant(q, e)^T   x bf16, q uint8 [N, K / 2] packed e2m1 (element 2i in the low nibble),
//   e uint8 [N, K / 32] e8m0 (OCP MXFP4; PPArgs.w = q, PPArgs.wexp = e), fp32 accumulate, bf16 out, with the PPArgs
//   family's epilogues in gemm_skinny.hip's semantics: plain, SwiGLU (w = [gate; up]), residual add + RMSNorm partial
//   sums of the stored values (kResid, [M, N / (WN / 2)]: one partial per wave's W rows), folded-norm row scale (NORMP).
//
//   * workgroup = 4 waves, 2 (W) x 2 (x); tile = WN W rows x XM x rows; wave (ww, wx) owns WN / 2 W rows (AT = WN / 32
//     MFMA A tiles; SwiGLU: AT / 2 gate tiles and the up tiles of the same columns) and XM / 2 x rows (BT = XM / 32 B
//     tiles); any M: M tiles in the grid, rows >= M are clamped on the way in and never stored;
//   * stage = 128 k.  W goes straight from global memory into VGPRs in the MFMA A layout, exactly as gemm_skinny.hip's
//     w4_stream: lane l (r = l & 15, q = l >> 4) loads the 16-B piece that is MX block k / 32 + q of row r and its scale
//     byte; MFMA step i = 0..3 converts dword i with four v_cvt_scalef32_pk_bf16_fp4 (scale operand e << 23: exact,
//     bit-equal to ops.reference.dequantize_mxfp4 for 2 <= e <= 254) into the A operand of v_mfma_f32_16x16x32_bf16,
//     k = 32 q + 8 i .. + 8; the B operand of the lane with x row n and the same q is x[n][k0 + 32 q + 8 i .. + 8];
//   * x goes through an LDS ring of ST stages shared by the workgroup (XM rows x 256 B each), filled by LDS-DMA
//     (buffer_load_dwordx4 ... lds: lane l of piece p fills row 4 p + l / 16, slot l % 16).  The 16-B chunk swizzle is
//     applied on the source address and undone on the ds_read_b128: slot = chunk ^ g(row), g(t) = t ^ 4 [4 <= t <= 11].
//     ds_read_b128 is served in the lane groups {0-3, 12-15, 20-27}, ... (two q, every r once): chunk = 4 q + i differs
//     by 4 between a group's two q, which plain chunk ^ row folds back onto the same slots; g's extra 4 takes it out
//     again, so the 16 lanes of a group read 16 distinct slots;
//   * ring schedule, one barrier per stage: wait for this wave's DMA of stage t (stages t + 1 .. t + ST - 2 and their W
//     loads stay in flight: vmcnt is in order, so the W ring is as deep as the x ring), barrier (every wave's DMA of
//     stage t landed, every wave's reads of stage t - 1 done), issue stage t + ST - 1 into the buffer and registers of
//     stage t - 1, then 4 BT ds_read_b128 and 4 AT BT MFMAs; the last NS % ST stages run after one full wait;
//   * split-K: fp32 slabs in register order (write-through stores), one ticket per tile, the last arriver sums the
//     slabs in slice order and leaves its ticket at zero (gemm_skinny.hip's hand-off: no fences, bitwise repeatable,
//     graph-capturable).
//
// K % (128 splitk) == 0 is the only K rule (no per-wave split of K: K = 2816 is accepted); N % WN == 0 (SwiGLU:
// F % (WN / 2) == 0); M K < 2^30 (32-bit byte offsets of the x descriptor).
//
// hipcc -Rpass-analysis=kernel-resource-usage per W4M_CONFIGS id (all epilogues within 4 VGPRs of each other): no
// instantiation uses scratch.  VGPRs + AGPRs, waves per SIMD by registers, LDS per workgroup (workgroups per CU by LDS):
//   0 (64 x 64):   100-102 + 24, 4,  65,808 B (2);     1 (128 x 64):  152-156 + 44-48, 2,  65,808 B (2);
//   2 (64 x 128):  136-138 + 48, 2, 131,600 B (1);     3 (128 x 128): 200-202 + 96,    1, 131,600 B (1).
// Measured (scripts/bench_mid_w4.py, profiles/mxfp4/mid_table.jsonl; the figures are in the README): a stage takes
// 0.8-1.8 us where its MFMAs need 0.1-0.4, and the time follows the W rows per wave (AT) more than the x bytes — the
// kernel is bound by its load path, not by the matrix cores; walking each tile's K range from its own starting block
// (so that concurrent workgroups do not all ask for the same 256-B column block of every x row) changed nothing and
// was not kept.
#include <algorithm>

#include "chronos_gemm.h"
#include "chronos_hip.h"

namespace chronos {
namespace {

enum : int { kPlain = kPPPlain, kSwiglu = kPPSwiglu, kResid = kPPResid };

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

template <int N>
__device__ __forceinline__ void w4m_vmcnt() {
    static_assert(N >= 0 && N < 64, "vmcnt range");
    __builtin_amdgcn_s_waitcnt((N & 0xF) | (0x7 << 4) | (0xF << 8) | ((N >> 4) << 14));
}

// raw workgroup barrier nothing is scheduled across (never __syncthreads in the loop: its vmcnt(0) would drain the ring)
__device__ __forceinline__ void w4m_bar() {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// one 1 KiB LDS-DMA piece: lane l's 16 bytes from byte voff + soff of the buffer to LDS dst + 16 l (dst wave-uniform);
// bytes past `bytes` read as zeros
__device__ __forceinline__ void w4m_dma16(const void* base, int bytes, unsigned char* dst, uint32_t voff, int soff) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, bytes,
                                                                        0x00020000);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)dst, 16, voff, soff, 0, 0);
}

// slot = chunk ^ w4m_swz(row) inside a 256-B row (file header)
__device__ __forceinline__ int w4m_swz(int row) {
    const int t = row & 15;
    return t ^ (((t + 4) & 8) >> 1);
}

template <int WN, int XM, int ST, int MODE, bool NORMP>
__global__ void __launch_bounds__(256) w4m_kernel(PPArgs a) {
    constexpr int AT = WN / 32, BT = XM / 32;  // A (W) and B (x) tiles of 16 rows per wave
    constexpr int NX = XM / 16;                // LDS-DMA pieces (4 x rows) per wave and stage
    constexpr int NPER = NX + 2 * AT;          // vector-memory operations per wave and stage
    constexpr int STAGE = XM * 256;            // bytes of one x stage
    static_assert(WN % 32 == 0 && XM % 32 == 0 && ST >= 2 && (ST - 2) * NPER < 64, "tile / ring");
    static_assert(MODE != kSwiglu || AT % 2 == 0, "swiglu: AT / 2 gate tiles + AT / 2 up tiles per wave");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* inv = reinterpret_cast<float*>(smem + ST * STAGE);  // [XM]
    int* flag = reinterpret_cast<int*>(inv + XM);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ww = wave >> 1, wx = wave & 1;
    const int r = lane & 15, q = lane >> 4;
    const int M = a.M, K = a.K, S = a.splitk;
    const int TN = MODE == kSwiglu ? a.F / (WN / 2) : a.N / WN;
    const int TM = (M + XM - 1) / XM;
    const int task = xcd_remap(blockIdx.x, TN * TM * S);
    const int s = task % S, tile = task / S;  // the slices of a tile are consecutive tasks: one slab block per tile
    const int tm = tile % TM, tn = tile / TM;  // ... and the M tiles of a W panel follow each other
    const int m0 = tm * XM;
    const int KS = K / S, NS = KS / 128, k0 = s * KS;

    // ---- W: first output column (SwiGLU: gate column) and source rows of A tile i
    int col0[AT];
    const i32x4* wp[AT];
    const unsigned char* ep[AT];
#pragma unroll
    for (int i = 0; i < AT; ++i) {
        int row;
        if constexpr (MODE == kSwiglu) {
            col0[i] = tn * (WN / 2) + ww * (WN / 4) + 16 * (i % (AT / 2));
            row = (i < AT / 2 ? 0 : a.F) + col0[i];
        } else {
            col0[i] = tn * WN + ww * (WN / 2) + 16 * i;
            row = col0[i];
        }
        wp[i] = reinterpret_cast<const i32x4*>(reinterpret_cast<const unsigned char*>(a.w) +
                                               (int64_t)(row + r) * (K / 2) + k0 / 2 + 16 * q);
        ep[i] = a.wexp + (int64_t)(row + r) * (K / 32) + k0 / 32 + q;
    }
    // ---- x: LDS-DMA sources (piece p = wave NX + i: rows 4 p .. 4 p + 3 of the tile; rows >= M clamped to M - 1)
    const int xbytes = (int)((int64_t)M * K * 2);
    uint32_t voff[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) {
        const int row = 4 * (wave * NX + i) + q;
        const int lc = r ^ w4m_swz(row);
        voff[i] = (uint32_t)(((int64_t)min(m0 + row, M - 1) * K + k0) * 2 + lc * 16);
    }
    // ... and fragment reads: B tile j, step i at xb + j * 4096 + sw[i]
    const int rbase = (wx * (XM / 2) + r) * 256;
    int sw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) sw[i] = ((4 * q + i) ^ w4m_swz(r)) << 4;

    i32x4 wr[ST][AT];
    uint32_t er[ST][AT];
    // Stage j into ring slot d = j % ST: the W loads first, the DMA pieces last.  Issued unconditionally, so that every
    // ring stage is one basic block that leaves the same vmcnt count (hipcc's own wait bookkeeping then agrees with the
    // counted waits below): a stage past the end re-reads the last stage's 64 B of each W row into registers nobody
    // uses and sends its DMA pieces past the descriptor's range (zeros, no memory traffic) into a buffer no later
    // stage reads
    auto issue = [&](int j, int d) {
        const bool in = j < NS;
        const int jw = min(j, NS - 1);
#pragma unroll
        for (int i = 0; i < AT; ++i) {
            wr[d][i] = __builtin_nontemporal_load(wp[i] + 4 * jw);  // 128 k = 64 B
            er[d][i] = ep[i][4 * jw];
        }
        // the order is part of the protocol: the counted wait below relies on every operation of stage j lying in
        // front of every operation of stage j + 1 in the (in-order) vmcnt queue, and on the W loads of a stage lying
        // in front of its DMA pieces
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < NX; ++i)
            w4m_dma16(a.x, xbytes, smem + d * STAGE + (wave * NX + i) * 1024, in ? voff[i] : 0x80000000u,
                      in ? jw * 256 : 0);
        __builtin_amdgcn_sched_barrier(0);
    };
#pragma unroll
    for (int d = 0; d < ST - 1; ++d) issue(d, d);

    f32x4 acc[AT][BT];
#pragma unroll
    for (int i = 0; i < AT; ++i)
#pragma unroll
        for (int j = 0; j < BT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto compute = [&](int d) {  // the stage in ring slot d
        const unsigned char* xb = smem + d * STAGE + rbase;
#pragma unroll
        for (int i4 = 0; i4 < 4; ++i4) {
            bf16x8 xf[BT];
#pragma unroll
            for (int j = 0; j < BT; ++j) xf[j] = *reinterpret_cast<const bf16x8*>(xb + j * 4096 + sw[i4]);
#pragma unroll
            for (int i = 0; i < AT; ++i) {
                const float sc = __builtin_bit_cast(float, er[d][i] << 23);
                const int wi = wr[d][i][i4];
                const bf16x2 c0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(wi, sc, 0);
                const bf16x2 c1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(wi, sc, 1);
                const bf16x2 c2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(wi, sc, 2);
                const bf16x2 c3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(wi, sc, 3);
                const bf16x8 wa = bf16x8{c0[0], c0[1], c1[0], c1[1], c2[0], c2[1], c3[0], c3[1]};
#pragma unroll
                for (int j = 0; j < BT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa, xf[j], acc[i][j], 0, 0, 0);
            }
        }
    };
    // whole rings: stage t = t0 + d sits in slot d; stages t + 1 .. t + ST - 2 were issued after it
    int t0 = 0;
    for (; t0 + ST <= NS; t0 += ST) {
#pragma unroll
        for (int d = 0; d < ST; ++d) {
            __builtin_amdgcn_sched_barrier(0);  // (the wait stays behind the previous stage's last MFMA)
            w4m_vmcnt<(ST - 2) * NPER>();
            w4m_bar();
            issue(t0 + d + ST - 1, (d + ST - 1) % ST);
            compute(d);
        }
    }
    // the last NS % ST stages (slots 0 ..; every stage after them was past the end): everything has been issued, and
    // every DMA must have landed before the workgroup's LDS is released anyway
    const int rem = NS - t0;
    w4m_vmcnt<0>();
    w4m_bar();
#pragma unroll
    for (int d = 0; d < ST - 1; ++d)
        if (d < rem) compute(d);

    // NORMP: inv[m] of the tile's x rows from the producer's partials — fetched only now, so these loads never sit in
    // front of the rings in the in-order vmcnt queue.  inv and flag lie behind the ring: no aliasing with late readers
    if constexpr (NORMP) {
        constexpr int RPW = XM / 4;
        float pv[RPW];
#pragma unroll
        for (int j = 0; j < RPW; ++j) {
            const int m = min(m0 + wave + 4 * j, M - 1);
            pv[j] = lane < a.nparts_in ? a.part_in[(int64_t)m * a.nparts_in + lane] : 0.f;
        }
        if (a.nparts_in > 64) {
#pragma unroll
            for (int j = 0; j < RPW; ++j) {
                const int m = min(m0 + wave + 4 * j, M - 1);
                for (int i = lane + 64; i < a.nparts_in; i += 64) pv[j] += a.part_in[(int64_t)m * a.nparts_in + i];
            }
        }
#pragma unroll
        for (int j = 0; j < RPW; ++j) {
            const float ss = wave_sum(pv[j]);
            if (lane == 0) inv[wave + 4 * j] = rsqrtf(ss / (float)K + a.eps);
        }
        __syncthreads();
    }

    if (S > 1) {  // split-K: slab per task in register order, ticket per tile, the last arriver sums in slice order
        constexpr int SLAB = WN * XM / 4;  // f32x4 per task
        float* slab = a.ws + (int64_t)task * SLAB * 4;
#pragma unroll
        for (int i = 0; i < AT; ++i)
#pragma unroll
            for (int j = 0; j < BT; ++j) st_wt(slab + ((i * BT + j) * 256 + tid) * 4, acc[i][j]);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            const int old = __hip_atomic_fetch_add(a.cnt + tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int last = old == S - 1;
            if (last) __hip_atomic_store(a.cnt + tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *flag = last;
        }
        __syncthreads();
        if (!*flag) return;
        const float* base = a.ws + (int64_t)tile * S * SLAB * 4;
        for (int o = 0; o < S; ++o) {
#pragma unroll
            for (int i = 0; i < AT; ++i)
#pragma unroll
                for (int j = 0; j < BT; ++j) {
                    const f32x4 v = ld_wt(base + ((int64_t)o * SLAB + (i * BT + j) * 256 + tid) * 4);
                    acc[i][j] = o == 0 ? v : acc[i][j] + v;
                }
        }
    }

    // A lane's acc[i][j] is x row m0 + wx XM / 2 + 16 j + r, outputs col0[i] + 4 q .. + 3 (8-byte stores)
#pragma unroll
    for (int j = 0; j < BT; ++j) {
        const int lr = wx * (XM / 2) + 16 * j + r;
        const int m = m0 + lr;
        const bool live = m < M;
        float sc = 1.f;
        if constexpr (NORMP) sc = inv[lr];
        if constexpr (MODE == kSwiglu) {
            if (live) {
#pragma unroll
                for (int i = 0; i < AT / 2; ++i) {
                    u16x4 o;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float gv = bf2f(f2bf(acc[i][j][c] * sc));
                        const float sg = bf2f(f2bf(gv / (1.f + __expf(-gv))));
                        o[c] = f2bf(sg * bf2f(f2bf(acc[i + AT / 2][j][c] * sc)));
                    }
                    *reinterpret_cast<u16x4*>(a.y + (int64_t)m * a.F + col0[i] + 4 * q) = o;
                }
            }
        } else if constexpr (MODE == kResid) {
            float ss = 0.f;
            if (live) {
#pragma unroll
                for (int i = 0; i < AT; ++i) {
                    const int64_t at = (int64_t)m * a.N + col0[i] + 4 * q;
                    const u16x4 rv = *reinterpret_cast<const u16x4*>(a.resid + at);
                    u16x4 o;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float sv = bf2f(f2bf(bf2f(f2bf(acc[i][j][c])) + bf2f(rv[c])));
                        o[c] = f2bf(sv);
                        ss += sv * sv;
                    }
                    *reinterpret_cast<u16x4*>(a.y + at) = o;
                }
            }
            // the 4 lanes of a row (q = 0..3) hold the wave's WN / 2 outputs of it: butterfly in a fixed order
            ss += __shfl_xor(ss, 16, 64);
            ss += __shfl_xor(ss, 32, 64);
            if (q == 0 && live) a.part_out[(int64_t)m * (a.N / (WN / 2)) + 2 * tn + ww] = ss;
        } else {
            if (live) {
#pragma unroll
                for (int i = 0; i < AT; ++i) {
                    u16x4 o;
#pragma unroll
                    for (int c = 0; c < 4; ++c) o[c] = f2bf(acc[i][j][c] * sc);
                    *reinterpret_cast<u16x4*>(a.y + (int64_t)m * a.N + col0[i] + 4 * q) = o;
                }
            }
        }
    }
}

template <int WN, int XM, int ST, int MODE, bool NORMP>
void launch_cfg(const PPArgs& a, hipStream_t st) {
    const int lds = ST * XM * 256 + XM * 4 + 16;
    auto kern = w4m_kernel<WN, XM, ST, MODE, NORMP>;
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        attr = true;
    }
    const int TN = MODE == kSwiglu ? a.F / (WN / 2) : a.N / WN;
    const int TM = (a.M + XM - 1) / XM;
    hipLaunchKernelGGL(kern, dim3(TN * TM * a.splitk), dim3(256), lds, st, a);
}

// configs {WN (W rows per tile), XM (x rows per tile), ST (x ring stages of XM x 256 B; W register ring of the same
// depth)}.  LDS = ST XM 256 B + XM 4 + 16.
#define W4M_CONFIGS(X)  \
    X(0, 64, 64, 4)     \
    X(1, 128, 64, 4)    \
    X(2, 64, 128, 4)    \
    X(3, 128, 128, 4)

template <int MODE, bool NORMP>
bool launch_mode(int cfg, const PPArgs& a, hipStream_t st) {
    switch (cfg) {
#define W4M_CASE(ID, WN_, XM_, ST_)                        \
    case ID:                                               \
        launch_cfg<WN_, XM_, ST_, MODE, NORMP>(a, st);     \
        return true;
        W4M_CONFIGS(W4M_CASE)
#undef W4M_CASE
        default: return false;
    }
}

}  // namespace

int gemm_w4m_wn(int cfg) {
    switch (cfg) {
#define W4M_WN(ID, WN_, XM_, ST_) case ID: return WN_;
        W4M_CONFIGS(W4M_WN)
#undef W4M_WN
        default: return 0;
    }
}
int gemm_w4m_xm(int cfg) {
    switch (cfg) {
#define W4M_XM(ID, WN_, XM_, ST_) case ID: return XM_;
        W4M_CONFIGS(W4M_XM)
#undef W4M_XM
        default: return 0;
    }
}
int gemm_w4m_st(int cfg) {
    switch (cfg) {
#define W4M_ST(ID, WN_, XM_, ST_) case ID: return ST_;
        W4M_CONFIGS(W4M_ST)
#undef W4M_ST
        default: return 0;
    }
}

// a.w = q bytes [N, K / 2], a.wexp = e8m0 bytes [N, K / 32]; cfg indexes W4M_CONFIGS
bool launch_gemm_w4m(int cfg, int mode, bool normp, const PPArgs& a, hipStream_t st) {
    if (a.M == 0) return true;
    if (a.wexp == nullptr) return false;
    if (mode == kResid) return normp ? false : launch_mode<kResid, false>(cfg, a, st);
    if (mode == kSwiglu) return normp ? launch_mode<kSwiglu, true>(cfg, a, st) : launch_mode<kSwiglu, false>(cfg, a, st);
    return normp ? launch_mode<kPlain, true>(cfg, a, st) : launch_mode<kPlain, false>(cfg, a, st);
}

}  // namespace chronos
