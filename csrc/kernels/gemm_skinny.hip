// gemm_skinny.hip — skinny-M projection GEMM (M = 3..128 rows): jump-forward forwards, the tail decode buckets and
// 70B TP=8 per-GPU decode (SURVEY.md §2.3 K3/K7/K8/K10/K11, §7.3 hard part 1; VERDICT r2 "skinny-M GEMM").
//
//   y[M, N] = x[M, K] · W[N, K]^T   (bf16 in, fp32 accumulate) with the batched family's epilogues (chronos_gemm.h):
//   plain, SwiGLU (w = [gate; up]), residual add + RMSNorm partial sums (kResid producer), folded-norm row scale
//   (NORMP consumer of a kResid producer's partials).
//
// At these M the op is a weight stream (the whole W once per call) with at most 64 columns of arithmetic per weight
// element, so the design is the decode GEMV's (gemv.hip) with the dot products moved onto the matrix cores:
//   * a workgroup owns 16*RT output rows (RT MFMA A tiles) and a K range; its NW waves split that range in 64-k
//     units (wave w takes units w, w+NW, ...), so the main loop has no barrier and no LDS at all.  NW up to 16 waves
//     gives the latency hiding of 4 waves per SIMD without splitting K across workgroups: a cross-workgroup split
//     costs an agent-scope release per workgroup (an L2 write-back) plus the slab round trip — 15-25 us on the 8B
//     decode shapes, more than the whole weight stream (profiles/r3_gemm_table.md);
//   * W goes straight from HBM into VGPRs in the v_mfma_f32_16x16x32_bf16 A layout (lane l: row l&15, k 8(l>>4)..+8
//     of each 32-k block).  A unit is two such loads per A tile, i.e. one full 128-B line of each of 16 rows;
//     x (L2-resident: <= 128 x K bf16) comes the same way as the B operand (column = x row l&15), rows >= M clamped;
//   * a register ring D units deep keeps D * RT KiB of weights in flight per wave (in-order vmcnt: the compiler's
//     counted waits retire the oldest unit only);
//   * MT x tiles of 16 rows (M <= 16 MT), RT W tiles: x bytes / W bytes = MT / RT per wave, kept <= 2 so the TCP
//     carries the weight stream plus the x re-reads;
//   * the NW waves' accumulators meet in LDS (fixed order), optional split-K across workgroups through write-through
//     fp32 slabs and an agent-scope ticket whose last arriver sums the slabs in slice order (no fences; bitwise
//     reproducible, graph == eager);
//   * epilogue per (row m, 4 consecutive outputs): 8-byte stores, CPR consecutive lanes cover a row's 16 RT outputs.
//
// W4A16 weight mode (WM = kW4, M <= 64: jump-forward chunks and 2-64 stream decode of an mxfp4 model): the same
// kernel with the main loop replaced by w4_stream below — W arrives as OCP MXFP4 (PPArgs.w = packed e2m1 [N, K / 2],
// PPArgs.wexp = e8m0 [N, K / 32], 4.25 bits per weight), is converted in registers (exact) and feeds the same bf16
// MFMA, accumulators, cross-wave reduction, split-K hand-off and epilogues; own config table (SK4_CONFIGS).  The bf16
// instantiations compile to the instructions they had before the mode existed (NU = 0 makes the bf16 loop dead code
// in a W4 instantiation instead of moving it into a branch, which changed the bf16 register allocation).
// On cold 8B weights (scripts/bench_skinny_w4.py, profiles/mxfp4/skinny_table.jsonl; the figures are in the README)
// it beats the bf16 kernel that the dequantised copy is routed to at M = 2-32 on all four projections, by less at
// M = 48 / 64 on O and down, and not at QKV and gate_up there, which stay on the copy (ops/gemm_plan.json "w4plans").
//
// W8A16 weight mode (WM = kW8, M <= 64: jump-forward chunks and few-stream decode of an fp8 model on bf16 activations):
// the main loop replaced by w8_stream below — W arrives as e4m3fn bytes [N, K] (PPArgs.w) with per-row f32 scales
// (PPArgs.wsc), is converted in registers (exact) and feeds the same bf16 MFMA, accumulators, cross-wave reduction,
// split-K hand-off and epilogues, the row scale applied once to the summed f32 result; own config table (SK8_CONFIGS).
// The bf16 and W4 instantiations compile to the instructions they had before (profiles/fp8/skinny_isa_same.txt).  It is
// reached only by ``a16`` callers (ops/gemm.py w8_plan, ops/gemm_plan.json "w8plans"); the measurements are in the README.
#include <algorithm>

#include "chronos_gemm.h"
#include "chronos_hip.h"

namespace chronos {
namespace {

enum : int { kPlain = kPPPlain, kSwiglu = kPPSwiglu, kResid = kPPResid };
// weight mode: bf16 | packed e2m1 + e8m0 block scales (W4A16, OCP MXFP4: PPArgs w = q bytes, wexp = e bytes)
// | e4m3fn bytes + per-row f32 scales (W8A16: PPArgs w = the bytes, wsc = the scales)
enum : int { kW16 = 0, kW8 = 1, kW4 = 2 };
constexpr int XL_MIN_MT = 2;  // x staged through LDS from MT = 2 (x bytes >= the weight bytes per wave)

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// W4A16 main loop (WM = kW4): the same workgroup, accumulators, reduction and epilogues, with W streamed as OCP MXFP4
// (q [N, K / 2] packed e2m1, element 2i in the low nibble of byte i; e [N, K / 32] e8m0) — 0.27 of the bf16 bytes.
//   * unit = 128 k.  Lane l (r = l & 15, q = l >> 4) loads the 16-B piece that is MX block k0 / 32 + q of row r — 32
//     elements, one scale byte — and MFMA step i = 0..3 takes the four v_cvt_scalef32_pk_bf16_fp4 of dword i (the e8m0
//     byte as the f32 exponent: exact, as in gemv.hip q4bf) as its A operand: k0 + 32 q + 8 i .. + 8.  The B operand of
//     the lane with x row n and the same q is x[n][k0 + 32 q + 8 i .. + 8]: both sides put the same k into the same
//     MFMA slot, and after 4 MFMAs the unit's 128 k were each used once (a dot product does not care about k order);
//   * a wave's K range is contiguous (wave w: KS / NW from s KS + w KS / NW on), not interleaved in units like the bf16
//     loop: a unit touches half a 128-B line of each of its 16 rows and the same wave's next unit, which is in flight
//     with it in the ring (D >= 2), touches the other half.  It also keeps the divisibility at K % (128 NW splitk),
//     which 16 waves meet at K = 14336; a 256-k unit of two pieces would not;
//   * x per unit is 16 MT rows x 256 B, four times what the bf16 loop reads per weight byte.  Without XL a lane loads
//     its four B operands directly (64 contiguous bytes: per instruction 16 rows x 4 pieces of 16 B, 64 B apart);
//     with XL the unit's x tile comes in whole rows (lane l: row 4 j + l / 16, 16-B chunk l % 16 of the row's 256 B)
//     and goes through the wave's LDS tile (slot chunk ^ (row & 15): both sides conflict-free) into the B layout;
//   * ring stage = RT pieces (4 VGPRs) + RT scale bytes + 16 MT VGPRs of x.
// hipcc -Rpass-analysis=kernel-resource-usage, per SK4_CONFIGS id (plain epilogue; the others within 4 VGPRs): no
// config uses scratch.  VGPRs (+ AGPRs), waves per SIMD:  0: 178 + 16, 2;  1: 198 + 16, 2;  2: 160, 3;  3: 138, 3;
// 4: 146, 3;  5: 88, 5;  6: 88, 5;  7: 208 + 32, 2;  8: 186, 2;  9: 186, 2;  10: 254 + 92, 1 (up to + 104 with NORMP);
// 11: 242, 2;  12: 232 + 40, 1.
// Subnormals: with e = 1 the products 0.5 .. 6 * 2^-127 are bf16 subnormals or just above; measured on gfx950
// (tests/test_mxfp4_skinny_gpu.py prints it), a one-hot probe returns every one of the 16 codes exactly, 0.5 * 2^-126
// included: neither the conversion nor the bf16 MFMA nor the f32 -> bf16 store flushes them.  The tests assert e >= 2.
// The scale operand is the e8m0 byte moved into an f32 exponent field (e << 23, as gemv.hip q4bf), so the two end
// codes are not representable this way: e = 0 (2^-127, an f32 subnormal) becomes 0.0 and e = 255 (the MX NaN code)
// becomes inf.  ops.reference.quantize_mxfp4 emits neither.
// Measured: XL at MT = 1 (ids 1, 4 against 0, 3) is within 3 % either way, so x is not bound by the load shape
// there; plain instead of nontemporal weight loads gained 0-5 % on the 4-wave configs and nothing on the others and
// were not kept.
template <int RT, int MT, int D, int NW, int MODE, bool XL>
__device__ __forceinline__ void w4_stream(const PPArgs& a, int g, int s, int KS, int lane, int wave,
                                          unsigned char* smem, f32x4 (&acc)[RT][MT]) {
    const int M = a.M, K = a.K;
    const int KW = KS / NW;   // this wave's contiguous K range
    const int NU = KW / 128;  // 128-k units per wave
    const int kw = s * KS + wave * KW;
    const int r = lane & 15, q = lane >> 4;
    const unsigned char* wq = reinterpret_cast<const unsigned char*>(a.w);
    const i32x4* wp[RT];
    const unsigned char* ep[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        int row;
        if constexpr (MODE == kSwiglu)
            row = rt < RT / 2 ? g * 8 * RT + 16 * rt : a.F + g * 8 * RT + 16 * (rt - RT / 2);
        else
            row = g * 16 * RT + 16 * rt;
        wp[rt] = reinterpret_cast<const i32x4*>(wq + (int64_t)(row + r) * (K / 2) + kw / 2 + 16 * q);
        ep[rt] = a.wexp + (int64_t)(row + r) * (K / 32) + kw / 32 + q;
    }
    // x offsets in 16-B pieces from a.x (M K < 2^31 elements): XL 4 MT row pieces, else one per x tile
    const bf16x8* xb = reinterpret_cast<const bf16x8*>(a.x);
    constexpr int NX = XL ? 4 * MT : MT;
    uint32_t xo[NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) {
        if constexpr (XL)
            xo[j] = (uint32_t)(((int64_t)min(4 * j + q, M - 1) * K + kw) / 8 + r);
        else
            xo[j] = (uint32_t)(((int64_t)min(16 * j + r, M - 1) * K + kw) / 8 + 4 * q);
    }
    unsigned char* xs = smem + wave * (MT * 4096);  // XL: this wave's x tile, 16 MT rows x 256 B

    i32x4 wr[D][RT];
    uint32_t er[D][RT];
    bf16x8 xr[D][MT][4];
    auto load = [&](int u, int d) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            wr[d][rt] = __builtin_nontemporal_load(wp[rt] + 4 * u);  // 128 k = 64 B
            er[d][rt] = ep[rt][4 * u];
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i)  // 128 k = 16 pieces
                xr[d][mt][i] = XL ? xb[xo[4 * mt + i] + 16 * u] : xb[xo[mt] + 16 * u + i];
    };
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (d < NU) load(d, d);

    for (int u0 = 0; u0 < NU; u0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int u = u0 + d;
            if (u < NU) {
                if constexpr (XL) {
                    // row layout -> LDS -> MFMA layout (row 16 mt + r, chunk 4 q + i); LDS ops of a wave run in order
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int t = 4 * (4 * mt + i) + q;
                            *reinterpret_cast<bf16x8*>(xs + t * 256 + ((r ^ (t & 15)) << 4)) = xr[d][mt][i];
                        }
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int t = 16 * mt + r;
                            xr[d][mt][i] = *reinterpret_cast<const bf16x8*>(xs + t * 256 + (((4 * q + i) ^ r) << 4));
                        }
                }
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const float sc = __builtin_bit_cast(float, er[d][rt] << 23);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int wi = wr[d][rt][i];
                        const bf16x2 c0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(wi, sc, 0);
                        const bf16x2 c1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(wi, sc, 1);
                        const bf16x2 c2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(wi, sc, 2);
                        const bf16x2 c3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(wi, sc, 3);
                        const bf16x8 wa = bf16x8{c0[0], c0[1], c1[0], c1[1], c2[0], c2[1], c3[0], c3[1]};
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt)
                            acc[rt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa, xr[d][mt][i], acc[rt][mt], 0, 0, 0);
                    }
                }
                if (u + D < NU) load(u + D, d);
            }
        }
    }
}

// W8A16 main loop (WM = kW8, M <= 64: jump-forward chunks and 3-64 stream decode of an fp8 model on bf16 activations):
// W streamed as e4m3fn bytes [N, K] (PPArgs.w) with one f32 scale per output row (PPArgs.wsc) — half the bf16 bytes.
//   * unit = 64 k.  Lane l (r = l & 15, q = l >> 4) loads the 16-B piece of 16 consecutive k of W row r at k0 + 16 q;
//     its two halves are the A operands of two MFMA steps, each four v_cvt_scalef32_pk_bf16_fp8 with scale 1 (exact:
//     e4m3 fits bf16, subnormals included; as gemv.hip q2bf): step i covers k0 + 16 q + 8 i .. + 8.  The B operand of
//     the lane with x row n and the same q is x[n][k0 + 16 q + 8 i .. + 8]: the same k in the same slot, no shuffle;
//   * a wave's K range is contiguous, as in w4_stream: a unit touches half a 128-B line of each of its 16 rows and the
//     wave's next unit, in flight with it, the other half.  K % (64 NW splitk) == 0, the bf16 rule: K = 2816 (the
//     small preset's down projection) is taken by the 4-wave configs;
//   * x per unit is 16 MT rows x 128 B, the bf16 loop's tile: x bytes / W bytes = 2 MT / RT.  Without XL a lane loads
//     its two B operands directly (32 contiguous bytes); with XL the tile comes in whole 128-B lines and goes through
//     the wave's LDS tile exactly like the bf16 loop's, read back at chunk 2 q + i;
//   * ring stage = RT pieces (4 VGPRs) + 8 MT VGPRs of x: 1 KiB of weights per W tile, half a bf16 stage, so D is twice
//     the bf16 config's of the same (RT, NW) wherever the registers allow (SK8_CONFIGS below);
//   * the row scale is not in the loop: the epilogue multiplies the f32 sum by wsc[n] once, after the waves and the
//     split-K slices are summed and before the NORMP row scale, SwiGLU, the residual add and the store (gemv.hip WQ).
// hipcc -Rpass-analysis=kernel-resource-usage, per SK8_CONFIGS id (the five epilogue instantiations within 2 VGPRs of
// each other): no config uses scratch.  VGPRs (+ AGPRs), waves per SIMD:  0: 220 + 16, 2;  1: 190, 2;  2: 160, 3;
// 3: 96, 5;  4: 118, 4;  5: 220 + 32, 2;  6: 234, 2;  7: 190, 2;  8: 228 + 64, 1;  9: 222, 2;  10: 256 + 46, 1;
// 11: 120, 4.
template <int RT, int MT, int D, int NW, int MODE, bool XL>
__device__ __forceinline__ void w8_stream(const PPArgs& a, int g, int s, int KS, int lane, int wave,
                                          unsigned char* smem, f32x4 (&acc)[RT][MT]) {
    const int M = a.M, K = a.K;
    const int KW = KS / NW;  // this wave's contiguous K range
    const int NU = KW / 64;  // 64-k units per wave
    const int kw = s * KS + wave * KW;
    const int r = lane & 15, q = lane >> 4;
    const unsigned char* wq = reinterpret_cast<const unsigned char*>(a.w);
    const i32x4* wp[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        int row;
        if constexpr (MODE == kSwiglu)
            row = rt < RT / 2 ? g * 8 * RT + 16 * rt : a.F + g * 8 * RT + 16 * (rt - RT / 2);
        else
            row = g * 16 * RT + 16 * rt;
        wp[rt] = reinterpret_cast<const i32x4*>(wq + (int64_t)(row + r) * K + kw + 16 * q);
    }
    // x offsets in 16-B pieces from a.x (M K < 2^31 elements): XL 2 MT line pieces (rows 8 j .. 8 j + 7), else one per tile
    const bf16x8* xb = reinterpret_cast<const bf16x8*>(a.x);
    constexpr int NX = XL ? 2 * MT : MT;
    uint32_t xo[NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) {
        if constexpr (XL)
            xo[j] = (uint32_t)(((int64_t)min(8 * j + (lane >> 3), M - 1) * K + kw) / 8 + (lane & 7));
        else
            xo[j] = (uint32_t)(((int64_t)min(16 * j + r, M - 1) * K + kw) / 8 + 2 * q);
    }
    unsigned char* xs = smem + wave * (MT * 2048);  // XL: this wave's x tile, 16 MT rows x 128 B

    i32x4 wr[D][RT];
    bf16x8 xr[D][MT][2];
    auto load = [&](int u, int d) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) wr[d][rt] = __builtin_nontemporal_load(wp[rt] + 4 * u);  // 64 k = 64 B
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int i = 0; i < 2; ++i)  // 64 k = 8 pieces
                xr[d][mt][i] = XL ? xb[xo[2 * mt + i] + 8 * u] : xb[xo[mt] + 8 * u + i];
    };
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (d < NU) load(d, d);

    for (int u0 = 0; u0 < NU; u0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int u = u0 + d;
            if (u < NU) {
                if constexpr (XL) {
                    // line layout -> LDS (row t, chunk lane % 8 in slot chunk ^ (t & 7)) -> MFMA layout (row 16 mt + r,
                    // chunk 2 q + i); LDS ops of a wave run in order
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const int t = 8 * (2 * mt + h) + (lane >> 3);
                            *reinterpret_cast<bf16x8*>(xs + t * 128 + (((lane & 7) ^ (t & 7)) << 4)) = xr[d][mt][h];
                        }
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                        for (int i = 0; i < 2; ++i) {
                            const int t = 16 * mt + r;
                            xr[d][mt][i] = *reinterpret_cast<const bf16x8*>(xs + t * 128 + (((2 * q + i) ^ (t & 7)) << 4));
                        }
                }
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int w0 = wr[d][rt][2 * i], w1 = wr[d][rt][2 * i + 1];
                        const bf16x2 c0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.f, false);
                        const bf16x2 c1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.f, true);
                        const bf16x2 c2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.f, false);
                        const bf16x2 c3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.f, true);
                        const bf16x8 wa = bf16x8{c0[0], c0[1], c1[0], c1[1], c2[0], c2[1], c3[0], c3[1]};
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt)
                            acc[rt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa, xr[d][mt][i], acc[rt][mt], 0, 0, 0);
                    }
                if (u + D < NU) load(u + D, d);
            }
        }
    }
}
template <int RT, int MT, int D, int NW, int MODE, bool NORMP, int WM = kW16, bool XL4 = false>
__global__ void __launch_bounds__(64 * NW) skinny_kernel(PPArgs a) {
    static_assert(MODE != kSwiglu || RT % 2 == 0, "swiglu: RT/2 gate tiles + RT/2 up tiles");
    constexpr bool W4 = WM == kW4, W8 = WM == kW8;
    constexpr bool XL = WM != kW16 ? XL4 : MT >= XL_MIN_MT;  // x through the wave's LDS tile (below; W4 / W8: per config)
    constexpr int NT = 64 * NW;                        // threads
    constexpr int UNITS = RT * MT * 64;                // f32x4 accumulators per wave
    constexpr int CPR = MODE == kSwiglu ? 2 * RT : 4 * RT;  // output units (4 columns each) per row
    constexpr int NOUT = 16 * MT * CPR;                // output units per workgroup (a multiple of 64)
    constexpr int VP = NOUT >= NT ? NOUT / NT : 1;     // output units per thread
    constexpr int PAIR = MODE == kSwiglu ? 2 : 1;       // swiglu: a gate unit and its up unit
    constexpr int NP = NOUT + NOUT / 16;               // one padded half (pad: 1 slot per 16, see red_at)
    constexpr int SZ = PAIR * NP;                      // f32x4 slots per wave
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    f32x4* red = reinterpret_cast<f32x4*>(smem);       // [NW waves][SZ]
    float* inv = reinterpret_cast<float*>(smem + NW * SZ * 16);  // [16 MT]
    int* flag = reinterpret_cast<int*>(inv + 16 * MT);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = a.M, K = a.K, S = a.splitk;
    const int G = MODE == kSwiglu ? a.F / (8 * RT) : a.N / (16 * RT);
    const int task = xcd_remap(blockIdx.x, G * S);
    const int g = task / S, s = task - g * S;
    const int KS = K / S;
    // 64-k units per wave (W4 / W8: none, this loop is dead and w4_stream / w8_stream runs)
    const int NU = WM != kW16 ? 0 : KS / (64 * NW);
    const int kbase = s * KS + wave * 64 + 8 * (lane >> 4);

    const bf16x8* wp[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        int row;
        if constexpr (MODE == kSwiglu)
            row = rt < RT / 2 ? g * 8 * RT + 16 * rt : a.F + g * 8 * RT + 16 * (rt - RT / 2);
        else
            row = g * 16 * RT + 16 * rt;
        wp[rt] = reinterpret_cast<const bf16x8*>(a.w + (int64_t)(row + (lane & 15)) * K + kbase);
    }
    // XL (MT >= XL_MIN_MT, x bytes = MT / RT x the weight bytes): x is loaded in whole 128-B lines (lane l: row 8 i + l / 8,
    // 16-B chunk l % 8 of the unit's 64 k) and turned into the MFMA B layout through the wave's private LDS tile
    // (swizzled ds_write_b128, ds_read_b128).  Loads shaped like the MFMA operand (16 rows x 64 B per instruction)
    // reach only ~18 B/clk per CU from L2 against ~50 for whole lines (csrc/microbench/l2_feed.hip): at M = 128 the x
    // re-reads, not the weight stream, set the kernel time.
    const bf16x8* xp[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        if constexpr (XL)  // pieces of 8 rows: xp[i] for i < 2 MT covers rows 8 i .. 8 i + 7
            xp[mt] = nullptr;
        else
            xp[mt] = reinterpret_cast<const bf16x8*>(a.x + (int64_t)min(16 * mt + (lane & 15), M - 1) * K + kbase);
    }
    const bf16x8* xl[XL ? 2 * MT : 1];
    if constexpr (XL) {
#pragma unroll
        for (int i = 0; i < 2 * MT; ++i)
            xl[i] = reinterpret_cast<const bf16x8*>(a.x + (int64_t)min(8 * i + (lane >> 3), M - 1) * K + s * KS +
                                                    wave * 64 + 8 * (lane & 7));
    }
    unsigned char* xs = smem + wave * (MT * 2048);  // XL: this wave's x tile, 16 MT rows x 128 B

    // unit u of this wave covers k = kbase + 64 NW u + {0, 32} (+ 8 (lane >> 4) already in the pointers)
    bf16x8 wr[D][RT][2], xr[D][MT][2];
    auto load = [&](int u, int d) {
        const int off = u * 8 * NW;  // 64 NW bf16 = 8 NW bf16x8
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            wr[d][rt][0] = __builtin_nontemporal_load(wp[rt] + off);
            wr[d][rt][1] = __builtin_nontemporal_load(wp[rt] + off + 4);
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            if constexpr (XL) {  // the same registers, in the line layout: piece 2 mt + h
                xr[d][mt][0] = xl[2 * mt][off];
                xr[d][mt][1] = xl[2 * mt + 1][off];
            } else {
                xr[d][mt][0] = xp[mt][off];
                xr[d][mt][1] = xp[mt][off + 4];
            }
        }
    };
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (d < NU) load(d, d);

    f32x4 acc[RT][MT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[rt][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int u0 = 0; u0 < NU; u0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int u = u0 + d;
            if (u < NU) {
                if constexpr (XL) {
                    // line layout -> LDS (row t = 8 i + lane / 8, chunk lane % 8 in slot chunk ^ (t & 7)) -> MFMA layout
                    // (row 16 mt + lane % 16, chunk 4 h + lane / 16); LDS ops of a wave run in order, so the previous
                    // unit's reads are served before these writes
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const int t = 8 * (2 * mt + h) + (lane >> 3);
                            *reinterpret_cast<bf16x8*>(xs + t * 128 + (((lane & 7) ^ (t & 7)) << 4)) = xr[d][mt][h];
                        }
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const int t = 16 * mt + (lane & 15);
                            xr[d][mt][h] = *reinterpret_cast<const bf16x8*>(
                                xs + t * 128 + (((4 * h + (lane >> 4)) ^ (t & 7)) << 4));
                        }
                }
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt)
                            acc[rt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wr[d][rt][h], xr[d][mt][h],
                                                                                  acc[rt][mt], 0, 0, 0);
                if (u + D < NU) load(u + D, d);
            }
        }
    }

    if constexpr (W4) w4_stream<RT, MT, D, NW, MODE, XL>(a, g, s, KS, lane, wave, smem, acc);
    if constexpr (W8) w8_stream<RT, MT, D, NW, MODE, XL>(a, g, s, KS, lane, wave, smem, acc);

    // XL: the reduction slots, inv and the flag alias the other waves' x tiles — wait until every wave's loop is done
    if constexpr (XL) __syncthreads();
    // NORMP: inv[m] of the x rows from the producer's partials — fetched only now, so these loads never sit in front
    // of the weight ring in the in-order vmcnt queue
    if constexpr (NORMP) {
        // every load of the wave's rows issued before any is reduced: one memory latency, not one per row
        constexpr int RPW = (16 * MT + NW - 1) / NW;
        float pv[RPW];
#pragma unroll
        for (int j = 0; j < RPW; ++j) {
            const int m = min(wave + NW * j, M - 1);
            pv[j] = lane < a.nparts_in ? a.part_in[(int64_t)m * a.nparts_in + lane] : 0.f;
        }
        if (a.nparts_in > 64) {
#pragma unroll
            for (int j = 0; j < RPW; ++j) {
                const int m = min(wave + NW * j, M - 1);
                for (int i = lane + 64; i < a.nparts_in; i += 64) pv[j] += a.part_in[(int64_t)m * a.nparts_in + i];
            }
        }
#pragma unroll
        for (int j = 0; j < RPW; ++j) {
            const int r = wave + NW * j;
            const float ss = wave_sum(pv[j]);
            if (lane == 0 && r < 16 * MT) inv[r] = rsqrtf(ss / (float)K + a.eps);
        }
    }
    // Output unit v = r * CPR + c: row r, outputs 4c..4c+3 of the workgroup's (gate) rows.  A lane's accumulator
    // acc[rt][mt] is unit (16 mt + (lane & 15), 4 (rt mod RT/2) + (lane >> 4)) of half rt / (RT/2) (swiglu; else rt).
    // Slots are padded by one per 16 (v + v/16): the lane-consecutive writes (unit stride CPR) and the
    // thread-consecutive reads (unit stride 1) both hit distinct banks.
    auto red_at = [&](int w, int p, int v) { return w * SZ + p * NP + v + (v >> 4); };
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            constexpr int HALF = MODE == kSwiglu ? RT / 2 : RT;
            const int p = rt / HALF, c = 4 * (rt % HALF) + (lane >> 4);
            red[red_at(wave, p, (16 * mt + (lane & 15)) * CPR + c)] = acc[rt][mt];
        }
    __syncthreads();

    f32x4 val[VP][PAIR];
    const bool active = tid < NOUT;  // wave-uniform (NOUT % 64 == 0)
    // W8: the row scales of this thread's output units, fetched behind the weight ring and in front of the LDS sum
    f32x4 wv[W8 ? VP : 1][PAIR];
    if constexpr (W8) {
        if (active) {
#pragma unroll
            for (int j = 0; j < VP; ++j)
#pragma unroll
                for (int p = 0; p < PAIR; ++p) {
                    const int c = (tid + NT * j) % CPR;
                    const float* sp = a.wsc + (MODE == kSwiglu ? p * a.F + g * 8 * RT : g * 16 * RT) + 4 * c;
                    wv[j][p] = f32x4{sp[0], sp[1], sp[2], sp[3]};
                }
        }
    }
    if (active) {
#pragma unroll
        for (int j = 0; j < VP; ++j)
#pragma unroll
            for (int p = 0; p < PAIR; ++p) {
                const int v = tid + NT * j;
                f32x4 acc4 = red[red_at(0, p, v)];
#pragma unroll
                for (int w = 1; w < NW; ++w) acc4 += red[red_at(w, p, v)];
                val[j][p] = acc4;
            }
    }

    if (S > 1) {  // split-K: slab per task in output-unit order, ticket per row group, last arriver sums in order
        // fence-free hand-off (chronos_hip.h st_wt / ld_wt): write-through slab stores, one lane's ticket after every
        // wave drained its stores, sc1 slab loads by the last arriver — an agent release + acquire pair per workgroup
        // (an L2 write-back + an L1 invalidate) cost 15-25 us on the decode shapes, more than the split saved
        constexpr int SLAB = NOUT * PAIR;  // f32x4 per task
        float* slab = a.ws + (int64_t)task * SLAB * 4;
        if (active) {
#pragma unroll
            for (int j = 0; j < VP; ++j)
#pragma unroll
                for (int p = 0; p < PAIR; ++p) st_wt(slab + ((tid + NT * j) * PAIR + p) * 4, val[j][p]);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            const int old = __hip_atomic_fetch_add(a.cnt + g, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int last = old == S - 1;
            if (last) __hip_atomic_store(a.cnt + g, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *flag = last;
        }
        __syncthreads();
        if (!*flag) return;
        if (active) {
            const float* base = a.ws + (int64_t)g * S * SLAB * 4;
            for (int o = 0; o < S; ++o) {
#pragma unroll
                for (int j = 0; j < VP; ++j)
#pragma unroll
                    for (int p = 0; p < PAIR; ++p) {
                        const f32x4 v = ld_wt(base + ((int64_t)o * SLAB + (tid + NT * j) * PAIR + p) * 4);
                        val[j][p] = o == 0 ? v : val[j][p] + v;
                    }
            }
        }
    }
    if (!active) return;
    if constexpr (W8) {
#pragma unroll
        for (int j = 0; j < VP; ++j)
#pragma unroll
            for (int p = 0; p < PAIR; ++p) val[j][p] *= wv[j][p];
    }

#pragma unroll
    for (int j = 0; j < VP; ++j) {
        const int v = tid + NT * j;
        const int r = v / CPR, c = v % CPR;
        const bool live = r < M;
        float sc = 1.f;
        if constexpr (NORMP) sc = inv[r];
        if constexpr (MODE == kSwiglu) {
            if (live) {
                u16x4 o;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float gv = bf2f(f2bf(val[j][0][i] * sc));
                    const float sg = bf2f(f2bf(gv / (1.f + __expf(-gv))));
                    o[i] = f2bf(sg * bf2f(f2bf(val[j][1][i] * sc)));
                }
                *reinterpret_cast<u16x4*>(a.y + (int64_t)r * a.F + g * 8 * RT + 4 * c) = o;
            }
        } else if constexpr (MODE == kResid) {
            const int64_t at = (int64_t)r * a.N + g * 16 * RT + 4 * c;
            float ss = 0.f;
            if (live) {
                const u16x4 rv = *reinterpret_cast<const u16x4*>(a.resid + at);
                u16x4 o;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float sv = bf2f(f2bf(bf2f(f2bf(val[j][0][i])) + bf2f(rv[i])));
                    o[i] = f2bf(sv);
                    ss += sv * sv;
                }
                *reinterpret_cast<u16x4*>(a.y + at) = o;
            }
            // the CPR consecutive lanes of a row hold its 16 RT outputs: butterfly in a fixed order
#pragma unroll
            for (int off = 1; off < CPR; off <<= 1) ss += __shfl_xor(ss, off, 64);
            if (c == 0 && live) a.part_out[(int64_t)r * (a.N / (16 * RT)) + g] = ss;
        } else {
            if (live) {
                u16x4 o;
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = f2bf(val[j][0][i] * sc);
                *reinterpret_cast<u16x4*>(a.y + (int64_t)r * a.N + g * 16 * RT + 4 * c) = o;
            }
        }
    }
}

template <int RT, int MT, int D, int NW, int MODE, bool NORMP, int WM = kW16, bool XL4 = false>
void launch_cfg(const PPArgs& a, hipStream_t st) {
    constexpr int UNITS = RT * MT * 64;
    // the reduction slots (+ inv, flag) alias the XL x tiles, which are dead once the main loop ends
    constexpr int XT = WM == kW4   ? (XL4 ? NW * MT * 4096 : 0)
                       : WM == kW8 ? (XL4 ? NW * MT * 2048 : 0)
                                   : (MT >= XL_MIN_MT ? NW * MT * 2048 : 0);
    const int lds = std::max(NW * (UNITS + UNITS / 16) * 16 + 16 * MT * 4 + 16, XT);
    auto kern = skinny_kernel<RT, MT, D, NW, MODE, NORMP, WM, XL4>;
    static bool attr = false;
    if (!attr) {
        hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        attr = true;
    }
    const int G = MODE == kSwiglu ? a.F / (8 * RT) : a.N / (16 * RT);
    hipLaunchKernelGGL(kern, dim3(G * a.splitk), dim3(64 * NW), lds, st, a);
}

// configs {RT (W tiles of 16 rows per workgroup), MT (x tiles: M <= 16 MT), D (ring depth in 64-k units), NW (waves
// splitting K inside the workgroup; K % (64 NW splitk) == 0)}
#define SK_CONFIGS(X)  \
    X(0, 1, 1, 4, 16)  \
    X(1, 2, 1, 4, 8)   \
    X(2, 4, 1, 4, 4)   \
    X(3, 2, 2, 4, 8)   \
    X(4, 4, 2, 3, 4)   \
    X(5, 2, 4, 3, 4)   \
    X(6, 4, 4, 2, 4)   \
    X(7, 2, 8, 2, 4)   \
    X(8, 1, 2, 4, 16)  \
    X(9, 1, 4, 2, 16)  \
    X(10, 2, 4, 2, 8)  \
    X(11, 1, 1, 4, 8)

template <int MODE, bool NORMP>
bool launch_mode(int cfg, const PPArgs& a, hipStream_t st) {
    switch (cfg) {
#define SK_CASE(ID, RT_, MT_, D_, NW_)                                     \
    case ID:                                                               \
        if constexpr (MODE == kSwiglu && RT_ % 2) return false;            \
        else {                                                             \
            launch_cfg<RT_, MT_, D_, NW_, MODE, NORMP>(a, st);             \
            return true;                                                   \
        }
        SK_CONFIGS(SK_CASE)
#undef SK_CASE
        default: return false;
    }
}

// W4A16 configs {RT, MT, D (ring depth in 128-k units), NW (K % (128 NW splitk) == 0), XL (x through LDS)}.  A ring
// stage is 5 RT + 16 MT VGPRs; the budget is 512 registers at NW = 4, 256 at 8, 128 at 16 (one workgroup per CU).
// Both 8B K (4096 = 128 * 32, 14336 = 128 * 112) divide by 128 * 16, so every config reaches both at splitk 1.
#define SK4_CONFIGS(X)    \
    X(0, 4, 1, 4, 4, 0)   \
    X(1, 4, 1, 4, 4, 1)   \
    X(2, 4, 1, 3, 8, 0)   \
    X(3, 2, 1, 4, 8, 0)   \
    X(4, 2, 1, 4, 8, 1)   \
    X(5, 2, 1, 2, 16, 0)  \
    X(6, 1, 1, 3, 16, 0)  \
    X(7, 4, 2, 3, 4, 1)   \
    X(8, 2, 2, 3, 8, 1)   \
    X(9, 4, 2, 2, 8, 1)   \
    X(10, 4, 4, 2, 4, 1)  \
    X(11, 2, 4, 2, 8, 1)  \
    X(12, 2, 4, 2, 4, 1)

template <int MODE, bool NORMP>
bool launch_mode_w4(int cfg, const PPArgs& a, hipStream_t st) {
    switch (cfg) {
#define SK4_CASE(ID, RT_, MT_, D_, NW_, XL_)                                     \
    case ID:                                                                     \
        if constexpr (MODE == kSwiglu && RT_ % 2) return false;                  \
        else {                                                                   \
            launch_cfg<RT_, MT_, D_, NW_, MODE, NORMP, kW4, XL_ != 0>(a, st);    \
            return true;                                                         \
        }
        SK4_CONFIGS(SK4_CASE)
#undef SK4_CASE
        default: return false;
    }
}

// W8A16 configs {RT, MT, D (ring depth in 64-k units), NW (K % (64 NW splitk) == 0), XL (x through LDS)}.  A ring
// stage is 4 RT + 8 MT VGPRs and 1 KiB of weights per W tile — half a bf16 stage — so D is twice the D of the bf16
// config with the same (RT, NW) where there is one.  The 4-wave configs (0, 5, 8, 10: every MT) take K = 2816.
#define SK8_CONFIGS(X)    \
    X(0, 4, 1, 8, 4, 0)   \
    X(1, 4, 1, 6, 8, 0)   \
    X(2, 2, 1, 8, 8, 0)   \
    X(3, 2, 1, 4, 16, 0)  \
    X(4, 1, 1, 8, 16, 0)  \
    X(5, 4, 2, 6, 4, 1)   \
    X(6, 2, 2, 8, 8, 1)   \
    X(7, 4, 2, 4, 8, 1)   \
    X(8, 4, 4, 4, 4, 1)   \
    X(9, 2, 4, 4, 8, 1)   \
    X(10, 2, 4, 6, 4, 1)  \
    X(11, 1, 1, 8, 8, 0)

template <int MODE, bool NORMP>
bool launch_mode_w8(int cfg, const PPArgs& a, hipStream_t st) {
    switch (cfg) {
#define SK8_CASE(ID, RT_, MT_, D_, NW_, XL_)                                     \
    case ID:                                                                     \
        if constexpr (MODE == kSwiglu && RT_ % 2) return false;                  \
        else {                                                                   \
            launch_cfg<RT_, MT_, D_, NW_, MODE, NORMP, kW8, XL_ != 0>(a, st);    \
            return true;                                                         \
        }
        SK8_CONFIGS(SK8_CASE)
#undef SK8_CASE
        default: return false;
    }
}

}  // namespace

int gemm_skinny_w8_rt(int cfg) {
    switch (cfg) {
#define SK8_RT(ID, RT_, MT_, D_, NW_, XL_) case ID: return RT_;
        SK8_CONFIGS(SK8_RT)
#undef SK8_RT
        default: return 0;
    }
}
int gemm_skinny_w8_nw(int cfg) {
    switch (cfg) {
#define SK8_NW(ID, RT_, MT_, D_, NW_, XL_) case ID: return NW_;
        SK8_CONFIGS(SK8_NW)
#undef SK8_NW
        default: return 0;
    }
}
int gemm_skinny_w8_mt(int cfg) {
    switch (cfg) {
#define SK8_MT(ID, RT_, MT_, D_, NW_, XL_) case ID: return MT_;
        SK8_CONFIGS(SK8_MT)
#undef SK8_MT
        default: return 0;
    }
}

// W8A16: a.w = e4m3fn bytes [N, K], a.wsc = f32 row scales [N]; cfg indexes SK8_CONFIGS
bool launch_gemm_skinny_w8(int cfg, int mode, bool normp, const PPArgs& a, hipStream_t st) {
    if (a.M == 0) return true;
    if (a.wsc == nullptr) return false;
    if (mode == kResid) return normp ? false : launch_mode_w8<kResid, false>(cfg, a, st);
    if (mode == kSwiglu)
        return normp ? launch_mode_w8<kSwiglu, true>(cfg, a, st) : launch_mode_w8<kSwiglu, false>(cfg, a, st);
    return normp ? launch_mode_w8<kPlain, true>(cfg, a, st) : launch_mode_w8<kPlain, false>(cfg, a, st);
}

int gemm_skinny_w4_rt(int cfg) {
    switch (cfg) {
#define SK4_RT(ID, RT_, MT_, D_, NW_, XL_) case ID: return RT_;
        SK4_CONFIGS(SK4_RT)
#undef SK4_RT
        default: return 0;
    }
}
int gemm_skinny_w4_nw(int cfg) {
    switch (cfg) {
#define SK4_NW(ID, RT_, MT_, D_, NW_, XL_) case ID: return NW_;
        SK4_CONFIGS(SK4_NW)
#undef SK4_NW
        default: return 0;
    }
}
int gemm_skinny_w4_mt(int cfg) {
    switch (cfg) {
#define SK4_MT(ID, RT_, MT_, D_, NW_, XL_) case ID: return MT_;
        SK4_CONFIGS(SK4_MT)
#undef SK4_MT
        default: return 0;
    }
}

// W4A16: a.w = q bytes [N, K / 2], a.wexp = e8m0 bytes [N, K / 32]; cfg indexes SK4_CONFIGS
bool launch_gemm_skinny_w4(int cfg, int mode, bool normp, const PPArgs& a, hipStream_t st) {
    if (a.M == 0) return true;
    if (a.wexp == nullptr) return false;
    if (mode == kResid) return normp ? false : launch_mode_w4<kResid, false>(cfg, a, st);
    if (mode == kSwiglu)
        return normp ? launch_mode_w4<kSwiglu, true>(cfg, a, st) : launch_mode_w4<kSwiglu, false>(cfg, a, st);
    return normp ? launch_mode_w4<kPlain, true>(cfg, a, st) : launch_mode_w4<kPlain, false>(cfg, a, st);
}

int gemm_skinny_rt(int cfg) {
    switch (cfg) {
#define SK_RT(ID, RT_, MT_, D_, NW_) case ID: return RT_;
        SK_CONFIGS(SK_RT)
#undef SK_RT
        default: return 0;
    }
}
int gemm_skinny_nw(int cfg) {
    switch (cfg) {
#define SK_NW(ID, RT_, MT_, D_, NW_) case ID: return NW_;
        SK_CONFIGS(SK_NW)
#undef SK_NW
        default: return 0;
    }
}
int gemm_skinny_mt(int cfg) {
    switch (cfg) {
#define SK_MT(ID, RT_, MT_, D_, NW_) case ID: return MT_;
        SK_CONFIGS(SK_MT)
#undef SK_MT
        default: return 0;
    }
}

bool launch_gemm_skinny(int cfg, int mode, bool normp, const PPArgs& a, hipStream_t st) {
    if (a.M == 0) return true;
    if (mode == kResid) return normp ? false : launch_mode<kResid, false>(cfg, a, st);
    if (mode == kSwiglu) return normp ? launch_mode<kSwiglu, true>(cfg, a, st) : launch_mode<kSwiglu, false>(cfg, a, st);
    return normp ? launch_mode<kPlain, true>(cfg, a, st) : launch_mode<kPlain, false>(cfg, a, st);
}

}  // namespace chronos
