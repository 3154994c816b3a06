// w4_expand.hip — MXFP4 (OCP e2m1 + e8m0 block scales) -> bf16 expansion of a whole projection weight.
//
// The packed-only weight mode ("mxfp4-packed", models/llama.py) keeps no bf16 copy of a Q4Tensor.  Where a projection
// has no W4A16 kernel (prefill, M > 64, shapes off the skinny plan) the existing bf16 GEMMs run on a per-model scratch
// that this kernel fills right before them: out[n, k] = e2m1(q[n, k / 2] nibble k % 2) * 2^(e[n, k / 32] - 127), the
// bytes Q4Tensor.w holds in copy mode, bit for bit.  The conversion is v_cvt_scalef32_pk_bf16_fp4 with the block's
// e8m0 byte moved into an f32 exponent field, exactly as gemv.hip (q4bf) and gemm_skinny.hip use it: a 1-bit mantissa
// times a power of two is exact in bf16.
//
// Layout.  With K % 32 == 0 and q / e / out contiguous the row structure drops out: "piece" p is dword p of q
// (8 elements), its scale is byte p / 4 of e, its output the 16 B at element 8 p of out.  One lane takes one piece:
// a wave's load instruction reads 256 B of q (and 16 scale bytes, four lanes sharing one), its four conversions make
// 8 bf16 and its one 16-B store writes 1 KB contiguous per wave.  A workgroup of 256 lanes takes tiles of kPieces
// pieces per lane (all loads of a tile issued before its first conversion) and strides over the tiles with a grid
// of at most `w4_expand_grid` workgroups (knob, default 1024: four per CU); offsets are 64-bit.  The last tile checks
// every piece against the total, so neither K / 8 nor N K / 8 has to be a multiple of anything.
//
// Decode gate (chronos_hip.h): taken, early.  A gated step of a small decode bucket must not rewrite a weight matrix.
#include "chronos_hip.h"

namespace chronos {

typedef __bf16 bf16x2_e __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_e __attribute__((ext_vector_type(4)));

constexpr int kExpThreads = 256;
constexpr int kPieces = 4;  // pieces in flight per lane

__device__ __forceinline__ u32x4_e w4_piece(uint32_t q, uint32_t e) {
    const float sc = __builtin_bit_cast(float, e << 23);
    u32x4_e o;
    o[0] = __builtin_bit_cast(uint32_t, (bf16x2_e)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 0));
    o[1] = __builtin_bit_cast(uint32_t, (bf16x2_e)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 1));
    o[2] = __builtin_bit_cast(uint32_t, (bf16x2_e)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 2));
    o[3] = __builtin_bit_cast(uint32_t, (bf16x2_e)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 3));
    return o;
}

__global__ void __launch_bounds__(kExpThreads) w4_expand_kernel(const uint32_t* __restrict__ q,
                                                                const uint8_t* __restrict__ e,
                                                                u32x4_e* __restrict__ out, int64_t pieces,
                                                                int64_t tiles, const int32_t* __restrict__ gst,
                                                                int gn) {
    if (gate_closed(gst, gn)) return;
    constexpr int64_t kTile = (int64_t)kExpThreads * kPieces;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t p0 = t * kTile + threadIdx.x;
        uint32_t qv[kPieces], ev[kPieces];
        if (p0 + (kPieces - 1) * kExpThreads < pieces) {  // whole tile in range for this lane
#pragma unroll
            for (int u = 0; u < kPieces; ++u) {
                const int64_t p = p0 + u * kExpThreads;
                qv[u] = q[p];
                ev[u] = e[p >> 2];
            }
#pragma unroll
            for (int u = 0; u < kPieces; ++u) out[p0 + u * kExpThreads] = w4_piece(qv[u], ev[u]);
        } else {
#pragma unroll
            for (int u = 0; u < kPieces; ++u) {
                const int64_t p = p0 + u * kExpThreads;
                if (p < pieces) out[p] = w4_piece(q[p], e[p >> 2]);
            }
        }
    }
}

// q: N K / 2 bytes, e: N K / 32 bytes, out: N K bf16 (16-B aligned); elems = N K, a multiple of 32 (the binding's checks)
void launch_w4_expand(const uint8_t* q, const uint8_t* e, uint16_t* out, int64_t elems, hipStream_t st) {
    if (elems <= 0) return;
    const int64_t pieces = elems / 8;
    const int64_t tile = (int64_t)kExpThreads * kPieces;
    const int64_t tiles = (pieces + tile - 1) / tile;
    int cap = knob("w4_expand_grid", 1024);
    if (cap < 1) cap = 1;
    const int grid = (int)(tiles < cap ? tiles : cap);
    hipLaunchKernelGGL(w4_expand_kernel, dim3(grid), dim3(kExpThreads), 0, st, reinterpret_cast<const uint32_t*>(q), e,
                       reinterpret_cast<u32x4_e*>(out), pieces, tiles, CHRONOS_GATE);
}

}  // namespace chronos
