// bindings.cpp — registers the gfx950 HIP kernels as torch operators (torch.ops.chronos.*).
//
// Every op checks dtype/shape/contiguity on the host BEFORE launching (a bad launch geometry on a hand-written kernel
// can fault the whole GPU box), launches on the current HIP stream (so ops are hipGraph-capturable), and never
// allocates inside a captured region except through torch's caching allocator.
#include <ATen/ATen.h>
// ROCm torch presents HIP devices as DeviceType::CUDA ("masquerading"): guards/streams must use these forms.
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/library.h>

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <tuple>
#include <string>
#include <unordered_map>
#include <vector>
#include <cstring>

#include "chronos_gemv.h"
#include "chronos_gemm.h"

namespace chronos {
void launch_embedding(const int32_t*, const uint16_t*, uint16_t*, int, int, int64_t, int64_t, hipStream_t);
void launch_rmsnorm(const uint16_t*, uint16_t*, const uint16_t*, uint16_t*, int, int, float, hipStream_t);
void launch_rope_kv_write(const uint16_t*, const int32_t*, const int32_t*, const int32_t*, int, const float*,
                          uint16_t*, void*, void*, int, int, int, int, int, bool, float, float, hipStream_t);
void launch_silu_mul(const uint16_t*, uint16_t*, int64_t, int, hipStream_t);
size_t paged_attn_smem(int nqt);
bool launch_decode_attn_rope(const uint16_t*, const int32_t*, const float*, void*, void*, const int32_t*, int,
                             const int32_t*, uint16_t*, int, int, int, int, float, hipStream_t, const int32_t*,
                             uint16_t*, float*);
void launch_paged_attn(const uint16_t*, const void*, const void*, const int32_t*, int, const int32_t*,
                       const int32_t*, const int32_t*, int, int, int, uint16_t*, float*, float*, int, int, int, float,
                       bool, float, float, hipStream_t, int);
void launch_constrained_sample(const void*, bool, int64_t, const int32_t*, int, int, const int16_t*, const int16_t*,
                               const int16_t*, int, int32_t*, int32_t*, const float*, const int32_t*, const int32_t*, const float*,
                               int32_t*, int32_t*, int32_t*, int32_t*, int32_t*, int, hipStream_t);
void launch_token_logprobs(const void*, bool, int64_t, const int32_t*, int, int, const int16_t*, const int16_t*, int,
                           const int32_t*, const int32_t*, const int32_t*, const int32_t*, int32_t*, float*, int32_t*,
                           float*, int, hipStream_t);
void launch_token_logprobs_commit(const void*, bool, int64_t, int, const int32_t*, int, const int32_t*,
                                  const int32_t*, int, const int32_t*, const int32_t*, const float*, const int32_t*,
                                  const float*, int, float*, int32_t*, hipStream_t);
void launch_apply_penalties(void*, bool, int64_t, int, const int32_t*, int, int, const int32_t*, const int32_t*,
                            const int32_t*, int, const float*, const int32_t*, const int32_t*, const int32_t*, int,
                            hipStream_t);
void launch_truncate_logits(void*, bool, int64_t, const int32_t*, int, int, const int16_t*, const int16_t*, int,
                            const int32_t*, const int32_t*, const float*, const float*, const float*, hipStream_t);
void launch_mirostat_truncate(void*, bool, int64_t, const int32_t*, int, int, const int16_t*, const int16_t*, int,
                              const int32_t*, const int32_t*, const int32_t*, const float*, const int32_t*, const float*,
                              float*, float*, int32_t*, hipStream_t);
void launch_mirostat_update(const void*, bool, int64_t, int, const int32_t*, int, const int32_t*, const int32_t*, int,
                            const float*, const int32_t*, float*, const float*, const float*, const float*,
                            const float*, const int32_t*, hipStream_t);
int pool_max_items(int, int);
int pool_max_seqs();
void launch_pool_accum(const uint16_t*, int, int, float, const int32_t*, const int32_t*, int, float*, int, int32_t*,
                       float*, hipStream_t);
void launch_pool_finish(float*, int, int, const int32_t*, int, const uint16_t*, float*, hipStream_t);
void launch_gemv(const uint16_t*, int, int, const uint16_t*, int, uint16_t*, bool, hipStream_t);
void launch_w4_expand(const uint8_t*, const uint8_t*, uint16_t*, int64_t, hipStream_t);
void attn_init();
void launch_gemm(const uint16_t*, const uint16_t*, uint16_t*, int, int, int, bool, int, hipStream_t);
void* ar_create(int, int, int64_t);
std::vector<uint8_t> ar_handles(void*);
void ar_open(void*, const std::vector<std::vector<uint8_t>>&);
void ar_run(void*, const uint16_t*, uint16_t*, int64_t, int64_t, int, hipStream_t);
void ar_run_norm(void*, const uint16_t*, uint16_t*, const uint16_t*, uint16_t*, int64_t, int, float, int64_t,
                 hipStream_t);
uint32_t ar_error(void*);
int64_t ar_capacity(void*);
void ar_destroy(void*);
void launch_attn_prefill(const uint16_t*, const void*, const void*, const int32_t*, int, const int32_t*,
                         const int32_t*, const int32_t*, int, uint16_t*, int, int, int, float, bool, float, float,
                         hipStream_t);
void launch_quant_rows(const uint16_t*, uint16_t*, const uint16_t*, uint8_t*, float*, int, int, float, int,
                       hipStream_t);
void launch_qlinear(const uint8_t*, const float*, const uint8_t*, const float*, uint16_t*, int, int, int, bool,
                    hipStream_t);
}  // namespace chronos

namespace chronos {
// decode early-exit gate (chronos_hip.h): read by the launchers, baked into captured graphs as kernel arguments
const int32_t* g_gate_state = nullptr;
int g_gate_n = 0;

namespace {
std::mutex g_knob_mu;
std::unordered_map<std::string, int> g_knobs;
}  // namespace

int resident_workgroups_of(const void* kernel, int threads) {
    static std::mutex mu;
    static std::unordered_map<const void*, int> cache;
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(kernel);
    if (it != cache.end()) return it->second;
    int per_cu = 0, dev = 0, cus = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0);
    const int v = per_cu > 0 && cus > 0 ? per_cu * cus : 256;
    cache[kernel] = v;
    return v;
}

int knob(const char* name, int dflt) {
    std::lock_guard<std::mutex> lk(g_knob_mu);
    auto it = g_knobs.find(name);
    if (it != g_knobs.end()) return it->second;
    std::string env = "CHRONOS_";
    for (const char* c = name; *c; ++c) env += (char)toupper(*c);
    const char* e = getenv(env.c_str());
    const int v = e ? atoi(e) : dflt;
    g_knobs[name] = v;
    return v;
}
}  // namespace chronos

namespace {

using at::Tensor;

inline hipStream_t cur_stream() { return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream(); }
inline const uint16_t* bf(const Tensor& t) { return reinterpret_cast<const uint16_t*>(t.data_ptr()); }
inline uint16_t* bfm(const Tensor& t) { return reinterpret_cast<uint16_t*>(t.data_ptr()); }
inline const int32_t* i32(const Tensor& t) { return t.data_ptr<int32_t>(); }
inline int32_t* i32m(const Tensor& t) { return t.data_ptr<int32_t>(); }

#define CHK(c, msg) TORCH_CHECK((c), "chronos: ", msg)
inline void chk_gpu(const Tensor& t, const char* n) {
    CHK(t.is_cuda(), std::string(n) + " must be a GPU tensor");
    CHK(t.is_contiguous(), std::string(n) + " must be contiguous");
}
inline void chk_bf16(const Tensor& t, const char* n) {
    chk_gpu(t, n);
    CHK(t.scalar_type() == at::kBFloat16, std::string(n) + " must be bfloat16");
}
inline void chk_i32(const Tensor& t, const char* n) {
    chk_gpu(t, n);
    CHK(t.scalar_type() == at::kInt, std::string(n) + " must be int32");
}

// Decode GEMV weights: bf16 [N, K], or (ws given) fp8-e4m3 bytes [N, K] with per-row f32 scales [N] (W8A16: the
// fp8-weight model's decode step keeps bf16 activations; csrc/kernels/gemv.hip WQ).  Returns the scale pointer.
inline const float* chk_gemv_w(const Tensor& w, const c10::optional<Tensor>& ws, int64_t K, int64_t M) {
    chk_gpu(w, "w");
    if (!ws.has_value()) {
        CHK(w.scalar_type() == at::kBFloat16, "w must be bfloat16 (or uint8 e4m3 with ws)");
        return nullptr;
    }
    chk_gpu(*ws, "ws");
    CHK(w.scalar_type() == at::kByte, "w must be uint8 (e4m3 bytes) when ws is given");
    CHK(ws->scalar_type() == at::kFloat && ws->numel() == w.size(0), "ws must be [N] f32");
    CHK(K % 1024 == 0 && M <= 4, "fp8-weight GEMV: K % 1024 == 0, M <= 4 (the fused epilogues: M <= 2)");
    return ws->data_ptr<float>();
}

// W4A16 decode GEMV weights (we given): packed e2m1 bytes [N, K / 2] with e8m0 block scales [N, K / 32] (OCP MXFP4;
// csrc/kernels/gemv.hip W4).  Returns the scale-byte pointer, or nullptr when we is absent.
inline const uint8_t* chk_gemv_w4(const Tensor& w, const c10::optional<Tensor>& ws, const c10::optional<Tensor>& we,
                                  int64_t K, int64_t M) {
    if (!we.has_value()) return nullptr;
    CHK(!ws.has_value(), "ws (fp8 row scales) and we (mxfp4 block scales) are exclusive");
    chk_gpu(w, "w");
    chk_gpu(*we, "we");
    CHK(w.scalar_type() == at::kByte && we->scalar_type() == at::kByte, "mxfp4 GEMV: w and we must be uint8");
    CHK(K % 1024 == 0 && M >= 1 && M <= 4, "mxfp4 GEMV: K % 1024 == 0, M <= 4 (the fused epilogues: M <= 2)");
    CHK(w.dim() == 2 && w.size(1) == K / 2, "mxfp4 GEMV: w must be [N, K / 2] (two e2m1 per byte)");
    CHK(w.size(0) % 16 == 0, "mxfp4 GEMV: N % 16 == 0");
    CHK(we->dim() == 2 && we->size(0) == w.size(0) && we->size(1) == K / 32, "mxfp4 GEMV: we must be [N, K / 32]");
    return we->data_ptr<uint8_t>();
}

// KV caches are bf16 or fp8-e4m3 stored as uint8 (OCP e4m3fn bytes; dequantised with a per-layer scale)
inline bool chk_kv(const Tensor& k, const Tensor& v) {
    chk_gpu(k, "k_cache");
    chk_gpu(v, "v_cache");
    CHK(k.scalar_type() == v.scalar_type(), "k/v cache dtypes differ");
    CHK(k.scalar_type() == at::kBFloat16 || k.scalar_type() == at::kByte, "kv cache must be bf16 or uint8 (fp8 e4m3)");
    return k.scalar_type() == at::kByte;
}

Tensor embedding(const Tensor& ids, const Tensor& table, int64_t vstart) {
    chk_i32(ids, "ids");
    chk_bf16(table, "table");
    CHK(table.dim() == 2 && table.size(1) % 8 == 0, "table must be [V, d] with d % 8 == 0");
    c10::hip::HIPGuardMasqueradingAsCUDA g(ids.device());
    auto out = at::empty({ids.numel(), table.size(1)}, table.options());
    chronos::launch_embedding(i32(ids), bf(table), bfm(out), (int)ids.numel(), (int)table.size(1), vstart,
                              table.size(0), cur_stream());
    return out;
}

Tensor rmsnorm(const Tensor& x, const Tensor& w, double eps) {
    chk_bf16(x, "x");
    chk_bf16(w, "w");
    const int64_t d = x.size(-1);
    CHK(w.numel() == d && d % 8 == 0 && d <= 16384, "rmsnorm: d must match w, be % 8 and <= 16384");
    c10::hip::HIPGuardMasqueradingAsCUDA g(x.device());
    auto y = at::empty_like(x);
    chronos::launch_rmsnorm(bf(x), nullptr, bf(w), bfm(y), (int)(x.numel() / d), (int)d, (float)eps, cur_stream());
    return y;
}

// resid <- bf16(x + resid); returns rmsnorm(resid) * w
Tensor add_rmsnorm(const Tensor& x, const Tensor& resid, const Tensor& w, double eps) {
    chk_bf16(x, "x");
    chk_bf16(resid, "resid");
    chk_bf16(w, "w");
    const int64_t d = x.size(-1);
    CHK(resid.sizes() == x.sizes(), "add_rmsnorm: shape mismatch");
    CHK(w.numel() == d && d % 8 == 0 && d <= 16384, "add_rmsnorm: d must match w, be % 8 and <= 16384");
    c10::hip::HIPGuardMasqueradingAsCUDA g(x.device());
    auto y = at::empty_like(x);
    chronos::launch_rmsnorm(bf(x), bfm(resid), bf(w), bfm(y), (int)(x.numel() / d), (int)d, (float)eps, cur_stream());
    return y;
}

void rope_kv_write(const Tensor& qkv, const Tensor& pos, const Tensor& tok_seq, const Tensor& block_table,
                   const Tensor& cos_sin, const Tensor& q_out, const Tensor& k_cache, const Tensor& v_cache, int64_t hq,
                   int64_t hkv, bool write_q, double k_scale, double v_scale) {
    chk_bf16(qkv, "qkv");
    chk_i32(pos, "pos");
    chk_i32(tok_seq, "tok_seq");
    chk_i32(block_table, "block_table");
    chk_gpu(cos_sin, "cos_sin");
    CHK(cos_sin.scalar_type() == at::kFloat && cos_sin.dim() == 2 && cos_sin.size(1) == 128, "cos_sin [P,128] f32");
    chk_bf16(q_out, "q_out");
    const bool fp8 = chk_kv(k_cache, v_cache);
    const int64_t t = qkv.size(0);
    CHK(qkv.dim() == 2 && qkv.size(1) == (hq + 2 * hkv) * 128, "qkv must be [T, (hq+2hkv)*128]");
    CHK(pos.numel() == t && tok_seq.numel() == t, "pos/tok_seq must have T entries");
    CHK(!write_q || q_out.numel() >= t * hq * 128, "q_out too small");
    CHK(k_cache.dim() == 4 && k_cache.size(1) == hkv && k_cache.size(3) == 128, "k_cache [NB, hkv, BS, 128]");
    CHK(v_cache.dim() == 4 && v_cache.size(1) == hkv && v_cache.size(2) == 128 && v_cache.size(3) == k_cache.size(2),
        "v_cache [NB, hkv, 128, BS]");
    CHK(block_table.dim() == 2, "block_table [B, max_blocks]");
    c10::hip::HIPGuardMasqueradingAsCUDA g(qkv.device());
    chronos::launch_rope_kv_write(bf(qkv), i32(pos), i32(tok_seq), i32(block_table), (int)block_table.size(1),
                                  cos_sin.data_ptr<float>(), bfm(q_out), k_cache.data_ptr(), v_cache.data_ptr(), (int)t,
                                  (int)hq, (int)hkv, (int)k_cache.size(2), write_q ? 1 : 0, fp8, (float)k_scale,
                                  (float)v_scale, cur_stream());
}

// Decode step attention with RoPE + paged-KV write fused in (attention.hip paged_decode_kernel<..., RP = true>).
// Returns the [n, hq, 128] attention output, or an empty tensor when the fused kernel does not serve this shape (the
// caller then runs rope_kv_write + paged_attention).  Decode rows only: row i is sequence i, its one token at pos[i]
// is the last of its context (ctx_len[i] == pos[i] + 1).
// casc (optional, int32 [1 + P_max] on the device: P, then the shared prefix's block ids) with casc_o (bf16 [>= n, hq,
// 128]) and casc_l (f32 [>= n, hq]) scratch: cascade attention over the shared prefix (attention.hip
// casc_prefix_kernel) merged into the decode kernel.  casc[0] = 0 turns it off without re-capturing a graph.
Tensor decode_attention_rope(const Tensor& qkv, const Tensor& pos, const Tensor& cos_sin, const Tensor& k_cache,
                             const Tensor& v_cache, const Tensor& block_table, const Tensor& ctx_len, int64_t n,
                             int64_t hq, double scale, const c10::optional<Tensor>& casc,
                             const c10::optional<Tensor>& casc_o, const c10::optional<Tensor>& casc_l) {
    chk_bf16(qkv, "qkv");
    chk_i32(pos, "pos");
    chk_i32(block_table, "block_table");
    chk_i32(ctx_len, "ctx_len");
    chk_gpu(cos_sin, "cos_sin");
    CHK(cos_sin.scalar_type() == at::kFloat && cos_sin.dim() == 2 && cos_sin.size(1) == 128, "cos_sin [P,128] f32");
    const bool fp8 = chk_kv(k_cache, v_cache);
    const int64_t hkv = k_cache.size(1), bs = k_cache.size(2);
    CHK(qkv.dim() == 2 && qkv.size(0) >= n && qkv.size(1) == (hq + 2 * hkv) * 128, "qkv must be [>=n, (hq+2hkv)*128]");
    CHK(pos.numel() >= n && ctx_len.numel() >= n && block_table.dim() == 2 && block_table.size(0) >= n,
        "pos / ctx_len / block_table need n rows");
    CHK(hq % hkv == 0 && 16 % (hq / hkv) == 0, "GQA group Hq/Hkv must divide 16");
    CHK(k_cache.dim() == 4 && k_cache.size(3) == 128 && v_cache.size(2) == 128 && v_cache.size(3) == bs,
        "k_cache [NB, hkv, BS, 128], v_cache [NB, hkv, 128, BS]");
    c10::hip::HIPGuardMasqueradingAsCUDA g(qkv.device());
    if (fp8) return at::empty({0}, qkv.options());
    const int32_t* cp = nullptr;
    uint16_t* co = nullptr;
    float* cl = nullptr;
    if (casc.has_value()) {
        chk_i32(*casc, "casc");
        CHK(casc_o.has_value() && casc_l.has_value(), "casc needs casc_o and casc_l");
        chk_bf16(*casc_o, "casc_o");
        chk_gpu(*casc_l, "casc_l");
        CHK(casc->numel() >= 2 && casc->numel() <= 65, "casc: [1 + P_max], P_max <= 64");
        CHK(casc_o->numel() >= n * hq * 128 && casc_l->scalar_type() == at::kFloat && casc_l->numel() >= n * hq,
            "casc_o [>= n, hq, 128] bf16, casc_l [>= n, hq] f32");
        cp = i32(*casc);
        co = bfm(*casc_o);
        cl = casc_l->data_ptr<float>();
    }
    auto out = at::empty({n, hq, 128}, qkv.options());
    if (!chronos::launch_decode_attn_rope(bf(qkv), i32(pos), cos_sin.data_ptr<float>(), k_cache.data_ptr(),
                                          v_cache.data_ptr(), i32(block_table), (int)block_table.size(1), i32(ctx_len),
                                          bfm(out), (int)n, (int)hq, (int)hkv, (int)bs, (float)scale, cur_stream(),
                                          cp, co, cl))
        return at::empty({0}, qkv.options());
    return out;
}

Tensor silu_mul(const Tensor& gu) {
    chk_bf16(gu, "gate_up");
    const int64_t f2 = gu.size(-1);
    CHK(f2 % 16 == 0, "gate_up last dim must be 2F with F % 8 == 0");
    c10::hip::HIPGuardMasqueradingAsCUDA g(gu.device());
    auto sizes = gu.sizes().vec();
    sizes.back() = f2 / 2;
    auto out = at::empty(sizes, gu.options());
    chronos::launch_silu_mul(bf(gu), bfm(out), gu.numel() / f2, (int)(f2 / 2), cur_stream());
    return out;
}

Tensor paged_attention(const Tensor& q, const Tensor& k_cache, const Tensor& v_cache, const Tensor& block_table,
                       const Tensor& q_start, const Tensor& ctx_len, const c10::optional<Tensor>& tiles,
                       int64_t ntiles, int64_t nqt, int64_t nsplit, double scale, double k_scale, double v_scale,
                       int64_t max_q) {
    chk_bf16(q, "q");
    const bool fp8 = chk_kv(k_cache, v_cache);
    chk_i32(block_table, "block_table");
    chk_i32(q_start, "q_start");
    chk_i32(ctx_len, "ctx_len");
    CHK(q.dim() == 3 && q.size(2) == 128, "q must be [T, Hq, 128]");
    const int64_t hq = q.size(1), hkv = k_cache.size(1), bs = k_cache.size(2);
    CHK(hq % hkv == 0 && 16 % (hq / hkv) == 0, "GQA group Hq/Hkv must divide 16");
    CHK(bs % 16 == 0, "block size must be a multiple of 16");
    CHK(v_cache.size(2) == 128 && v_cache.size(3) == bs, "v_cache [NB, hkv, 128, BS]");
    CHK(nqt == 1 || nqt == 2 || nqt == 8, "nqt must be 1, 2 (split-K paged kernel) or 8 (flash prefill)");
    CHK(nsplit >= 1 && nsplit <= 256, "nsplit in [1, 256]");
    const int32_t* tp = nullptr;
    if (tiles.has_value()) {
        chk_i32(*tiles, "tiles");
        CHK(tiles->numel() >= 2 * ntiles, "tiles must be [ntiles, 2]");
        tp = i32(*tiles);
    } else if (max_q > 1) {
        CHK(nqt == 1 && max_q * (hq / hkv) <= 16 && bs == 16, "multi-token decode: nqt 1, max_q x GQA group <= 16");
        CHK(q_start.numel() >= ntiles + 1 && ctx_len.numel() >= ntiles, "multi-token decode: q_start [B + 1], ctx [B]");
    } else {
        CHK(ctx_len.numel() >= ntiles && q.size(0) >= ntiles, "decode mode: one query token per tile");
    }
    c10::hip::HIPGuardMasqueradingAsCUDA g(q.device());
    auto out = at::empty_like(q);
    Tensor po, pl;
    if (nsplit > 1 && nqt != 8) {
        const int64_t rows = nsplit * ntiles * hkv * nqt * 16;
        po = at::empty({rows, 128}, q.options().dtype(at::kFloat));
        pl = at::empty({rows}, q.options().dtype(at::kFloat));
    }
    if (nqt == 8) {  // flash prefill kernel: 128 query rows per workgroup, K/V tiles shared through LDS
        CHK(tp != nullptr, "nqt=8 (flash prefill) needs a tile list");
        chronos::launch_attn_prefill(bf(q), k_cache.data_ptr(), v_cache.data_ptr(), i32(block_table),
                                     (int)block_table.size(1), i32(q_start), i32(ctx_len), tp, (int)ntiles, bfm(out),
                                     (int)hq, (int)hkv, (int)bs, (float)scale, fp8, (float)k_scale, (float)v_scale,
                                     cur_stream());
        return out;
    }
    chronos::launch_paged_attn(bf(q), k_cache.data_ptr(), v_cache.data_ptr(), i32(block_table),
                               (int)block_table.size(1), i32(q_start), i32(ctx_len), tp, (int)ntiles, (int)nqt,
                               (int)nsplit, bfm(out), nsplit > 1 ? po.data_ptr<float>() : nullptr,
                               nsplit > 1 ? pl.data_ptr<float>() : nullptr, (int)hq, (int)hkv, (int)bs, (float)scale,
                               fp8, (float)k_scale, (float)v_scale, cur_stream(), (int)max_q);
    return out;
}

void constrained_sample(const Tensor& logits, const c10::optional<Tensor>& row_of_slot, const Tensor& next,
                        const Tensor& dist, int64_t done_state, const Tensor& state, const Tensor& remaining,
                        const c10::optional<Tensor>& temperature, const c10::optional<Tensor>& seed, const Tensor& ids,
                        const Tensor& pos, const Tensor& ctx, const Tensor& nout, const Tensor& out_tokens,
                        const c10::optional<Tensor>& topk, const c10::optional<Tensor>& topp,
                        const c10::optional<Tensor>& jump) {
    CHK(logits.is_cuda() && logits.dim() == 2 && logits.stride(1) == 1, "logits [rows, V] row-contiguous");
    CHK(logits.scalar_type() == at::kBFloat16 || logits.scalar_type() == at::kFloat, "logits bf16 or f32");
    chk_gpu(next, "next");
    CHK(next.scalar_type() == at::kShort && next.dim() == 2, "next must be int16 [S, V]");
    CHK(dist.scalar_type() == at::kShort && dist.numel() == next.size(0), "dist must be int16 [S]");
    const int64_t vocab = next.size(1);
    CHK(logits.size(1) >= vocab, "logits narrower than the DFA vocabulary");
    chk_i32(state, "state");
    const int64_t n = state.numel();
    for (const Tensor* t : {&remaining, &ids, &pos, &ctx, &nout}) {
        chk_i32(*t, "slot tensor");
        CHK(t->numel() >= n, "slot tensors must have one entry per slot");
    }
    chk_i32(out_tokens, "out_tokens");
    CHK(out_tokens.dim() == 2 && out_tokens.size(0) >= n, "out_tokens [slots, max_out]");
    const int32_t* rp = nullptr;
    if (row_of_slot.has_value()) {
        chk_i32(*row_of_slot, "row_of_slot");
        rp = i32(*row_of_slot);
    } else {
        CHK(logits.size(0) >= n, "one logits row per slot");
    }
    const float* tp = nullptr;
    if (temperature.has_value()) {
        chk_gpu(*temperature, "temperature");
        CHK(temperature->scalar_type() == at::kFloat, "temperature f32");
        tp = temperature->data_ptr<float>();
    }
    const int32_t* sp = nullptr;
    if (seed.has_value()) {
        chk_i32(*seed, "seed");
        sp = i32(*seed);
    }
    const int32_t* kp = nullptr;
    if (topk.has_value()) {
        chk_i32(*topk, "topk");
        CHK(topk->numel() >= n, "topk: one entry per slot");
        kp = i32(*topk);
    }
    const float* pp = nullptr;
    if (topp.has_value()) {
        chk_gpu(*topp, "topp");
        CHK(topp->scalar_type() == at::kFloat && topp->numel() >= n, "topp: f32, one entry per slot");
        pp = topp->data_ptr<float>();
    }
    const int16_t* jp = nullptr;
    if (jump.has_value()) {
        chk_gpu(*jump, "jump");
        CHK(jump->scalar_type() == at::kShort && jump->numel() == next.size(0), "jump must be int16 [S]");
        jp = jump->data_ptr<int16_t>();
    }
    c10::hip::HIPGuardMasqueradingAsCUDA g(logits.device());
    chronos::launch_constrained_sample(logits.data_ptr(), logits.scalar_type() == at::kFloat, logits.stride(0), rp,
                                       (int)n, (int)vocab, next.data_ptr<int16_t>(), dist.data_ptr<int16_t>(), jp,
                                       (int)done_state, i32m(state), i32m(remaining), tp, sp, kp, pp, i32m(ids),
                                       i32m(pos), i32m(ctx), i32m(nout), i32m(out_tokens), (int)out_tokens.size(1),
                                       cur_stream());
}

// Per-token logprobs (csrc/kernels/logprobs.hip).  Shared checks of the per-slot scratch: lp_want / lp_mark / lp_lse
// one entry per slot, lp_top_ids / lp_top_val [slots, K] with K <= 20.  Returns K.
int64_t chk_lp_scratch(int64_t n, const Tensor& lp_want, const Tensor& lp_mark, const Tensor& lp_lse,
                       const Tensor& lp_top_ids, const Tensor& lp_top_val) {
    chk_i32(lp_want, "lp_want");
    chk_i32(lp_mark, "lp_mark");
    chk_gpu(lp_lse, "lp_lse");
    chk_i32(lp_top_ids, "lp_top_ids");
    chk_gpu(lp_top_val, "lp_top_val");
    CHK(lp_lse.scalar_type() == at::kFloat && lp_top_val.scalar_type() == at::kFloat, "lp_lse / lp_top_val f32");
    CHK(lp_want.numel() >= n && lp_mark.numel() >= n && lp_lse.numel() >= n, "lp_*: one entry per slot");
    CHK(lp_top_ids.dim() == 2 && lp_top_val.dim() == 2 && lp_top_ids.size(0) >= n && lp_top_val.size(0) >= n &&
            lp_top_ids.size(1) == lp_top_val.size(1),
        "lp_top_ids / lp_top_val [slots, K]");
    CHK(lp_top_ids.size(1) <= 20, "at most 20 top logprobs (MAX_TOP)");
    return lp_top_ids.size(1);
}

const int32_t* chk_lp_rows(const Tensor& logits, const c10::optional<Tensor>& row_of_slot, int64_t n) {
    CHK(logits.is_cuda() && logits.dim() == 2 && logits.stride(1) == 1, "logits [rows, V] row-contiguous");
    CHK(logits.scalar_type() == at::kBFloat16 || logits.scalar_type() == at::kFloat, "logits bf16 or f32");
    if (row_of_slot.has_value()) {
        chk_i32(*row_of_slot, "row_of_slot");
        CHK(row_of_slot->numel() >= n, "row_of_slot: one entry per slot");
        return i32(*row_of_slot);
    }
    CHK(logits.size(0) >= n, "one logits row per slot");
    return nullptr;
}

void token_logprobs(const Tensor& logits, const c10::optional<Tensor>& row_of_slot, const Tensor& next,
                    const Tensor& dist, int64_t done_state, const Tensor& state, const Tensor& remaining,
                    const Tensor& nout, const Tensor& lp_want, const Tensor& lp_mark, const Tensor& lp_lse,
                    const Tensor& lp_top_ids, const Tensor& lp_top_val) {
    chk_gpu(next, "next");
    CHK(next.scalar_type() == at::kShort && next.dim() == 2, "next must be int16 [S, V]");
    chk_gpu(dist, "dist");
    CHK(dist.scalar_type() == at::kShort && dist.numel() == next.size(0), "dist must be int16 [S]");
    const int64_t vocab = next.size(1);
    chk_i32(state, "state");
    const int64_t n = state.numel();
    const int32_t* rp = chk_lp_rows(logits, row_of_slot, n);
    CHK(logits.size(1) >= vocab, "logits narrower than the DFA vocabulary");
    chk_i32(remaining, "remaining");
    chk_i32(nout, "nout");
    CHK(remaining.numel() >= n && nout.numel() >= n, "slot tensors must have one entry per slot");
    const int64_t K = chk_lp_scratch(n, lp_want, lp_mark, lp_lse, lp_top_ids, lp_top_val);
    c10::hip::HIPGuardMasqueradingAsCUDA g(logits.device());
    chronos::launch_token_logprobs(logits.data_ptr(), logits.scalar_type() == at::kFloat, logits.stride(0), rp, (int)n,
                                   (int)vocab, next.data_ptr<int16_t>(), dist.data_ptr<int16_t>(), (int)done_state,
                                   i32(state), i32(remaining), i32(nout), i32(lp_want), i32m(lp_mark),
                                   lp_lse.data_ptr<float>(), i32m(lp_top_ids), lp_top_val.data_ptr<float>(), (int)K,
                                   cur_stream());
}

void token_logprobs_commit(const Tensor& logits, const c10::optional<Tensor>& row_of_slot, const Tensor& nout,
                           const Tensor& out_tokens, const Tensor& lp_want, const Tensor& lp_mark,
                           const Tensor& lp_lse, const Tensor& lp_top_ids, const Tensor& lp_top_val,
                           const Tensor& out_lp, const Tensor& out_lp_ids) {
    chk_i32(nout, "nout");
    const int64_t n = nout.numel();
    const int32_t* rp = chk_lp_rows(logits, row_of_slot, n);
    const int64_t K = chk_lp_scratch(n, lp_want, lp_mark, lp_lse, lp_top_ids, lp_top_val);
    chk_i32(out_tokens, "out_tokens");
    CHK(out_tokens.dim() == 2 && out_tokens.size(0) >= n, "out_tokens [slots, max_out]");
    const int64_t max_out = out_tokens.size(1);
    chk_gpu(out_lp, "out_lp");
    chk_i32(out_lp_ids, "out_lp_ids");
    CHK(out_lp.scalar_type() == at::kFloat && out_lp.dim() == 3 && out_lp.size(0) >= n && out_lp.size(1) == max_out &&
            out_lp.size(2) == 1 + K,
        "out_lp f32 [slots, max_out, 1 + K]");
    CHK(out_lp_ids.dim() == 3 && out_lp_ids.size(0) >= n && out_lp_ids.size(1) == max_out && out_lp_ids.size(2) == K,
        "out_lp_ids int32 [slots, max_out, K]");
    c10::hip::HIPGuardMasqueradingAsCUDA g(logits.device());
    chronos::launch_token_logprobs_commit(logits.data_ptr(), logits.scalar_type() == at::kFloat, logits.stride(0),
                                          (int)logits.size(1), rp, (int)n, i32(nout), i32(out_tokens), (int)max_out,
                                          i32(lp_want), i32(lp_mark), lp_lse.data_ptr<float>(), i32(lp_top_ids),
                                          lp_top_val.data_ptr<float>(), (int)K, out_lp.data_ptr<float>(),
                                          i32m(out_lp_ids), cur_stream());
}

// Repeat / frequency / presence penalties (csrc/kernels/penalties.hip): rewrites, in place and before the sampler, the
// logits of the tokens in each live slot's history window.  pen_par f32 [slots, 3] = (repeat, frequency, presence),
// pen_last int32 [slots] = window length L, pen_tail int32 [slots, W] / pen_tlen int32 [slots] = the prompt tail.
void apply_penalties(const Tensor& logits, const c10::optional<Tensor>& row_of_slot, int64_t done_state,
                     const Tensor& state, const Tensor& nout, const Tensor& out_tokens, const Tensor& pen_par,
                     const Tensor& pen_last, const Tensor& pen_tail, const Tensor& pen_tlen) {
    chk_i32(state, "state");
    const int64_t n = state.numel();
    const int32_t* rp = chk_lp_rows(logits, row_of_slot, n);
    CHK(logits.size(1) < (int64_t(1) << 31), "logits too wide");
    chk_i32(nout, "nout");
    CHK(nout.numel() >= n, "nout: one entry per slot");
    chk_i32(out_tokens, "out_tokens");
    CHK(out_tokens.dim() == 2 && out_tokens.size(0) >= n, "out_tokens [slots, max_out]");
    chk_gpu(pen_par, "pen_par");
    CHK(pen_par.scalar_type() == at::kFloat && pen_par.dim() == 2 && pen_par.size(0) >= n && pen_par.size(1) == 3,
        "pen_par f32 [slots, 3]");
    chk_i32(pen_last, "pen_last");
    chk_i32(pen_tlen, "pen_tlen");
    CHK(pen_last.numel() >= n && pen_tlen.numel() >= n, "pen_last / pen_tlen: one entry per slot");
    chk_i32(pen_tail, "pen_tail");
    CHK(pen_tail.dim() == 2 && pen_tail.size(0) >= n, "pen_tail int32 [slots, W]");
    const int64_t W = pen_tail.size(1);
    CHK(W >= 1 && W <= 1024, "penalty window W must be in 1..1024 (MAX_PENALTY_WINDOW)");
    c10::hip::HIPGuardMasqueradingAsCUDA g(logits.device());
    chronos::launch_apply_penalties(logits.data_ptr(), logits.scalar_type() == at::kFloat, logits.stride(0),
                                    (int)logits.size(1), rp, (int)n, (int)done_state, i32(state), i32(nout),
                                    i32(out_tokens), (int)out_tokens.size(1), pen_par.data_ptr<float>(), i32(pen_last),
                                    i32(pen_tail), i32(pen_tlen), (int)W, cur_stream());
}

// min_p / typical_p (csrc/kernels/truncate.hip): writes -inf, in place and before the sampler, into the legal tokens of
// each live sampling slot that do not survive.  minp_ln f32 [slots] = ln(min_p) (-inf = off), typical f32 [slots] =
// typical_p (>= 1 = off).
void truncate_logits(const Tensor& logits, const c10::optional<Tensor>& row_of_slot, const Tensor& next,
                     const Tensor& dist, int64_t done_state, const Tensor& state, const Tensor& remaining,
                     const Tensor& temperature, const Tensor& minp_ln, const Tensor& typical) {
    chk_gpu(next, "next");
    CHK(next.scalar_type() == at::kShort && next.dim() == 2, "next must be int16 [S, V]");
    chk_gpu(dist, "dist");
    CHK(dist.scalar_type() == at::kShort && dist.numel() == next.size(0), "dist must be int16 [S]");
    const int64_t vocab = next.size(1);
    chk_i32(state, "state");
    const int64_t n = state.numel();
    const int32_t* rp = chk_lp_rows(logits, row_of_slot, n);
    CHK(logits.size(1) >= vocab, "logits narrower than the DFA vocabulary");
    CHK(vocab < (int64_t(1) << 31) - 1024, "vocabulary too wide");  // the kernel strides 1024 tokens in int
    chk_i32(remaining, "remaining");
    CHK(remaining.numel() >= n, "remaining: one entry per slot");
    for (const Tensor* t : {&temperature, &minp_ln, &typical}) {
        chk_gpu(*t, "temperature / minp_ln / typical");
        CHK(t->scalar_type() == at::kFloat && t->numel() >= n, "temperature / minp_ln / typical: f32, one per slot");
    }
    c10::hip::HIPGuardMasqueradingAsCUDA g(logits.device());
    chronos::launch_truncate_logits(logits.data_ptr(), logits.scalar_type() == at::kFloat, logits.stride(0), rp, (int)n,
                                    (int)vocab, next.data_ptr<int16_t>(), dist.data_ptr<int16_t>(), (int)done_state,
                                    i32(state), i32(remaining), temperature.data_ptr<float>(),
                                    minp_ln.data_ptr<float>(), typical.data_ptr<float>(), cur_stream());
}

// Mirostat 2.0 (csrc/kernels/mirostat.hip).  Per slot: mi_on int32 (0 = off), mi_mu / mi_tau / mi_eta f32 (the surprise
// target and its controller), and the scratch the two kernels hand over: mi_m (legal maximum), mi_lnz (ln Z' of the
// survivors) f32, mi_mark int32 (the output index the sampler was about to fill, -1 = leave mu alone).
static void chk_mi(int64_t n, std::initializer_list<const Tensor*> f32s, std::initializer_list<const Tensor*> i32s) {
    for (const Tensor* t : f32s) {
        chk_gpu(*t, "mirostat f32 state");
        CHK(t->scalar_type() == at::kFloat && t->numel() >= n, "mirostat state: f32, one per slot");
    }
    for (const Tensor* t : i32s) {
        chk_i32(*t, "mirostat int32 state");
        CHK(t->numel() >= n, "mirostat state: int32, one per slot");
    }
}

// mirostat_truncate: before the sampler, -inf into the legal tokens of each live sampling slot with mirostat on whose
// surprise exceeds mu; records m, ln Z' and the mark.
void mirostat_truncate(const Tensor& logits, const c10::optional<Tensor>& row_of_slot, const Tensor& next,
                       const Tensor& dist, int64_t done_state, const Tensor& state, const Tensor& remaining,
                       const Tensor& nout, const Tensor& temperature, const Tensor& mi_on, const Tensor& mi_mu,
                       const Tensor& mi_m, const Tensor& mi_lnz, const Tensor& mi_mark) {
    chk_gpu(next, "next");
    CHK(next.scalar_type() == at::kShort && next.dim() == 2, "next must be int16 [S, V]");
    chk_gpu(dist, "dist");
    CHK(dist.scalar_type() == at::kShort && dist.numel() == next.size(0), "dist must be int16 [S]");
    const int64_t vocab = next.size(1);
    chk_i32(state, "state");
    const int64_t n = state.numel();
    const int32_t* rp = chk_lp_rows(logits, row_of_slot, n);
    CHK(logits.size(1) >= vocab, "logits narrower than the DFA vocabulary");
    CHK(vocab < (int64_t(1) << 31) - 1024, "vocabulary too wide");  // the kernel strides 1024 tokens in int
    chk_mi(n, {&temperature, &mi_mu, &mi_m, &mi_lnz}, {&remaining, &nout, &mi_on, &mi_mark});
    c10::hip::HIPGuardMasqueradingAsCUDA g(logits.device());
    chronos::launch_mirostat_truncate(logits.data_ptr(), logits.scalar_type() == at::kFloat, logits.stride(0), rp, (int)n,
                                      (int)vocab, next.data_ptr<int16_t>(), dist.data_ptr<int16_t>(), (int)done_state,
                                      i32(state), i32(remaining), i32(nout), temperature.data_ptr<float>(), i32(mi_on),
                                      mi_mu.data_ptr<float>(), mi_m.data_ptr<float>(), mi_lnz.data_ptr<float>(),
                                      i32m(mi_mark), cur_stream());
}

// mirostat_update: after the sampler, mu <- mu - eta * (S_obs - tau) for the slots whose nout advanced past the mark.
void mirostat_update(const Tensor& logits, const c10::optional<Tensor>& row_of_slot, const Tensor& nout,
                     const Tensor& out_tokens, const Tensor& temperature, const Tensor& mi_on, const Tensor& mi_mu,
                     const Tensor& mi_tau, const Tensor& mi_eta, const Tensor& mi_m, const Tensor& mi_lnz,
                     const Tensor& mi_mark) {
    chk_i32(nout, "nout");
    const int64_t n = nout.numel();
    const int32_t* rp = chk_lp_rows(logits, row_of_slot, n);
    CHK(logits.size(1) < (int64_t(1) << 31), "logits too wide");
    chk_i32(out_tokens, "out_tokens");
    CHK(out_tokens.dim() == 2 && out_tokens.size(0) >= n, "out_tokens [slots, max_out]");
    chk_mi(n, {&temperature, &mi_mu, &mi_tau, &mi_eta, &mi_m, &mi_lnz}, {&mi_on, &mi_mark});
    c10::hip::HIPGuardMasqueradingAsCUDA g(logits.device());
    chronos::launch_mirostat_update(logits.data_ptr(), logits.scalar_type() == at::kFloat, logits.stride(0),
                                    (int)logits.size(1), rp, (int)n, i32(nout), i32(out_tokens),
                                    (int)out_tokens.size(1), temperature.data_ptr<float>(), i32(mi_on),
                                    mi_mu.data_ptr<float>(), mi_tau.data_ptr<float>(), mi_eta.data_ptr<float>(),
                                    mi_m.data_ptr<float>(), mi_lnz.data_ptr<float>(), i32(mi_mark), cur_stream());
}

// Embedding pooling (csrc/kernels/pool.hip).  H is one of the presets' hidden sizes: the kernels are compiled per H.
static void chk_pool_acc(const Tensor& acc, int64_t H) {
    chk_gpu(acc, "acc");
    CHK(acc.scalar_type() == at::kFloat && acc.dim() == 2 && acc.size(1) == H, "pool: acc must be f32 [S, H]");
    CHK(H == 256 || H == 1024 || H == 4096 || H == 8192, "pool: hidden size must be 256, 1024, 4096 or 8192");
    CHK(acc.size(0) < (int64_t(1) << 31) / H, "pool: acc too large");
}

// pool_accum: acc[sel[b]] += sum over rows [q_rows[b][0], q_rows[b][1]) of s[r] * rsqrt(mean(s[r]^2) + eps), fp32.
void pool_accum(const Tensor& s, double eps, const Tensor& q_rows, const Tensor& sel, const Tensor& acc) {
    chk_bf16(s, "s");
    CHK(s.dim() == 2, "pool_accum: s must be [T, H]");
    const int64_t T = s.size(0), H = s.size(1);
    chk_pool_acc(acc, H);
    chk_i32(q_rows, "q_rows");
    chk_i32(sel, "sel");
    const int64_t B = sel.numel();
    CHK(q_rows.dim() == 2 && q_rows.size(0) == B && q_rows.size(1) == 2, "pool_accum: q_rows must be [B, 2]");
    CHK(B <= chronos::pool_max_seqs(), "pool_accum: too many sequences in one call");
    CHK(T < (int64_t(1) << 30), "pool_accum: too many rows");
    if (B == 0 || T == 0) return;
    c10::hip::HIPGuardMasqueradingAsCUDA g(s.device());
    const int64_t items = chronos::pool_max_items((int)T, (int)B);
    auto plan = at::empty({2 + B + 1 + items}, sel.options());
    auto scratch = at::empty({items, H}, acc.options());
    chronos::launch_pool_accum(bf(s), (int)T, (int)H, (float)eps, i32(q_rows), i32(sel), (int)B,
                               acc.data_ptr<float>(), (int)acc.size(0), i32m(plan), scratch.data_ptr<float>(),
                               cur_stream());
}

// pool_finish: out[i] = normalise(g (.) acc[rows[i]]) (zeros at norm 0), then acc[rows[i]] <- 0.
void pool_finish(const Tensor& acc, const Tensor& rows, const Tensor& g, const Tensor& out) {
    chk_bf16(g, "g");
    const int64_t H = g.numel();
    chk_pool_acc(acc, H);
    chk_i32(rows, "rows");
    chk_gpu(out, "out");
    const int64_t n = rows.numel();
    CHK(out.scalar_type() == at::kFloat && out.dim() == 2 && out.size(0) == n && out.size(1) == H,
        "pool_finish: out must be f32 [n, H]");
    CHK(n < (int64_t(1) << 31) / H, "pool_finish: too many rows");
    c10::hip::HIPGuardMasqueradingAsCUDA gd(acc.device());
    chronos::launch_pool_finish(acc.data_ptr<float>(), (int)acc.size(0), (int)H, i32(rows), (int)n, bf(g),
                                out.data_ptr<float>(), cur_stream());
}

// y = x @ w.T for M <= 8 rows (decode); swiglu: w = [gate; up] -> y = silu(x@gate.T) * (x@up.T)
Tensor gemv(const Tensor& x, const Tensor& w, bool swiglu, const c10::optional<Tensor>& ws,
            const c10::optional<Tensor>& we) {
    chk_bf16(x, "x");
    const int64_t K = x.size(-1), M = x.numel() / K, N = w.size(0);
    if (const uint8_t* wex = chk_gemv_w4(w, ws, we, K, M)) {
        c10::hip::HIPGuardMasqueradingAsCUDA g(x.device());
        auto y = at::empty({M, swiglu ? N / 2 : N}, x.options());
        chronos::launch_gemv_w4(bf(x), (int)M, (int)K, w.data_ptr<uint8_t>(), wex, (int)N, bfm(y), swiglu,
                                cur_stream());
        return y;
    }
    const float* wsc = chk_gemv_w(w, ws, K, M);
    CHK(w.dim() == 2 && w.size(1) == K, "gemv: w must be [N, K]");
    CHK(M >= 1 && M <= 8, "gemv: 1 <= M <= 8");
    CHK(K % 512 == 0, "gemv: K % 512 == 0");
    CHK(N % 16 == 0, "gemv: N % 16 == 0");
    c10::hip::HIPGuardMasqueradingAsCUDA g(x.device());
    auto y = at::empty({M, swiglu ? N / 2 : N}, x.options());
    if (wsc)
        chronos::launch_gemv_q(bf(x), (int)M, (int)K, reinterpret_cast<const uint8_t*>(w.data_ptr()), wsc, (int)N,
                               bfm(y), swiglu, cur_stream());
    else
        chronos::launch_gemv(bf(x), (int)M, (int)K, bf(w), (int)N, bfm(y), swiglu, cur_stream());
    return y;
}

// MXFP4 -> bf16 expansion of a projection weight (csrc/kernels/w4_expand.hip): q uint8 [N, K / 2] packed e2m1, e uint8
// [N, K / 32] e8m0 block scales, out a bf16 buffer of at least N K elements whose first N K become the contiguous
// [N, K] dequantisation (the packed-only weight mode's scratch).  Honours the decode gate.
void w4_expand(const Tensor& q, const Tensor& e, const Tensor& out) {
    chk_gpu(q, "q");
    chk_gpu(e, "e");
    chk_bf16(out, "out");
    CHK(q.scalar_type() == at::kByte && e.scalar_type() == at::kByte, "w4_expand: q and e must be uint8");
    CHK(q.device() == e.device() && q.device() == out.device(), "w4_expand: q, e and out must be on one device");
    CHK(q.dim() == 2 && e.dim() == 2 && q.size(0) >= 1 && q.size(1) >= 16, "w4_expand: q [N, K / 2], e [N, K / 32]");
    const int64_t N = q.size(0), K = q.size(1) * 2;
    CHK(K % 32 == 0, "w4_expand: K % 32 == 0 (whole MX blocks)");
    CHK(e.size(0) == N && e.size(1) == K / 32, "w4_expand: e must be [N, K / 32] for q [N, K / 2]");
    CHK(N <= (int64_t(1) << 40) / K, "w4_expand: N K too large");
    CHK(out.numel() >= N * K, "w4_expand: out holds fewer than N K elements");
    CHK(reinterpret_cast<uintptr_t>(out.data_ptr()) % 16 == 0, "w4_expand: out must be 16-byte aligned");
    CHK(reinterpret_cast<uintptr_t>(q.data_ptr()) % 4 == 0, "w4_expand: q must be 4-byte aligned");
    c10::hip::HIPGuardMasqueradingAsCUDA g(q.device());
    chronos::launch_w4_expand(q.data_ptr<uint8_t>(), e.data_ptr<uint8_t>(), bfm(out), N * K, cur_stream());
}

// Decode gate: state = the engine's slot-state vector (int32, >= n rows); n in [1, 8] arms it for the launches that
// follow, n = 0 disarms.  Only decode steps of a small bucket arm it (a prefill or a large bucket never does).
void set_decode_gate(const c10::optional<Tensor>& state, int64_t n) {
    if (!state.has_value() || n <= 0) {
        chronos::g_gate_state = nullptr;
        chronos::g_gate_n = 0;
        return;
    }
    chk_i32(*state, "gate state");
    CHK(n <= 8 && state->numel() >= n, "decode gate: 1 <= n <= 8 and n <= numel(state)");
    chronos::g_gate_state = i32(*state);
    chronos::g_gate_n = (int)n;
}

// Decode producer (O / down projection at TP=1, M <= 2): resid_out = bf16(bf16(x @ w.T) + resid_in); returns the
// per-workgroup sums of resid_out^2 [M, P] f32 that the consuming GEMV's norm prologue reduces (chronos_gemv.h).
Tensor gemv_resid(const Tensor& x, const Tensor& w, const Tensor& resid_in, const Tensor& resid_out,
                  const c10::optional<Tensor>& ws, const c10::optional<Tensor>& we) {
    chk_bf16(x, "x");
    chk_bf16(resid_in, "resid_in");
    chk_bf16(resid_out, "resid_out");
    const int64_t K = x.size(-1), M = x.numel() / K, N = w.size(0);
    const uint8_t* wex = chk_gemv_w4(w, ws, we, K, M);
    const float* wsc = wex ? nullptr : chk_gemv_w(w, ws, K, M);
    CHK(w.dim() == 2 && (wex || w.size(1) == K), "gemv_resid: w must be [N, K]");
    CHK(M >= 1 && M <= 2 && K % 512 == 0 && N % 16 == 0, "gemv_resid: M <= 2, K % 512, N % 16");
    CHK(resid_in.numel() == M * N && resid_out.numel() == M * N, "gemv_resid: residuals must be [M, N]");
    CHK(resid_in.data_ptr() != resid_out.data_ptr(), "gemv_resid: out of place only");
    c10::hip::HIPGuardMasqueradingAsCUDA g(x.device());
    CHK(wsc == nullptr || M <= 2, "gemv_resid: M <= 2");
    auto part = at::empty({M, chronos::gemv_resid_parts((int)M, (int)N, wex ? 2 : wsc ? 1 : 0)},
                          x.options().dtype(at::kFloat));
    chronos::launch_gemv_resid(bf(x), (int)M, (int)K, bf(w), (int)N, bf(resid_in), bfm(resid_out),
                               part.data_ptr<float>(), cur_stream(), wsc, wex);
    return part;
}

inline chronos::GemvNorm normp_args(const Tensor& s, const Tensor& part, double eps, int64_t M) {
    chk_gpu(part, "part");
    CHK(part.scalar_type() == at::kFloat && part.dim() == 2 && part.size(0) == M, "part must be [M, P] f32");
    CHK(part.size(1) % 4 == 0 && part.size(1) <= (M == 1 ? 2048 : 1024),
        "part: P % 4 == 0, P <= 2048 (one row) / 1024 (two rows)");
    (void)s;
    chronos::GemvNorm n{};
    n.part = part.data_ptr<float>();
    n.nparts = (int)part.size(1);
    n.eps = (float)eps;
    return n;
}

// Decode consumer: y = rmsnorm(s) @ w.T for a projection w whose norm weight is folded in (models/llama.py
// fold_norm), the norm's sum of squares taken from a gemv_resid producer's partials (swiglu: gate/up pair ->
// silu(g) * u).  s: [M, K], M <= 2.
Tensor gemv_normp(const Tensor& s, const Tensor& part, double eps, const Tensor& w, bool swiglu,
                  const c10::optional<Tensor>& ws, const c10::optional<Tensor>& we) {
    chk_bf16(s, "s");
    const int64_t K = s.size(-1), M = s.numel() / K, N = w.size(0);
    const uint8_t* wex = chk_gemv_w4(w, ws, we, K, M);
    const float* wsc = wex ? nullptr : chk_gemv_w(w, ws, K, M);
    CHK(w.dim() == 2 && (wex || w.size(1) == K), "gemv_normp: w must be [N, K]");
    CHK(M >= 1 && M <= 2 && K % 512 == 0 && N % 16 == 0, "gemv_normp: M <= 2, K % 512, N % 16");
    const chronos::GemvNorm n = normp_args(s, part, eps, M);
    c10::hip::HIPGuardMasqueradingAsCUDA g(s.device());
    auto y = at::empty({M, swiglu ? N / 2 : N}, s.options());
    chronos::launch_gemv_ex(bf(s), (int)M, (int)K, bf(w), (int)N, bfm(y), swiglu, &n, nullptr, false, cur_stream(),
                            wsc, wex);
    return y;
}

// Decode QKV projection with the RoPE + paged-KV epilogue (rope_kv_write's semantics): q -> q_out, k/v -> the caches.
// part given: x is the residual stream s and the (folded) input RMSNorm is fused as in gemv_normp; else x is the
// normalised input.  M <= 2 tokens, token m belongs to block-table row tok_seq[m].
void qkv_rope(const Tensor& x, const c10::optional<Tensor>& part, double eps,
              const Tensor& w, const Tensor& pos, const Tensor& tok_seq, const Tensor& block_table,
              const Tensor& cos_sin, const Tensor& q_out, const Tensor& k_cache, const Tensor& v_cache, int64_t hq,
              int64_t hkv, double k_scale, double v_scale, const c10::optional<Tensor>& ws,
              const c10::optional<Tensor>& we) {
    chk_bf16(x, "x");
    chk_i32(pos, "pos");
    chk_i32(tok_seq, "tok_seq");
    chk_i32(block_table, "block_table");
    chk_gpu(cos_sin, "cos_sin");
    CHK(cos_sin.scalar_type() == at::kFloat && cos_sin.dim() == 2 && cos_sin.size(1) == 128, "cos_sin [P,128] f32");
    chk_bf16(q_out, "q_out");
    const bool fp8 = chk_kv(k_cache, v_cache);
    const int64_t K = x.size(-1), M = x.numel() / K, N = w.size(0);
    const uint8_t* wex = chk_gemv_w4(w, ws, we, K, M);
    const float* wsc = wex ? nullptr : chk_gemv_w(w, ws, K, M);
    CHK(M >= 1 && M <= 2 && K % 512 == 0, "qkv_rope: M <= 2, K % 512 == 0");
    CHK(w.dim() == 2 && (wex || w.size(1) == K) && N == (hq + 2 * hkv) * 128, "w must be [(hq+2hkv)*128, K]");
    CHK(pos.numel() >= M && tok_seq.numel() >= M && q_out.numel() >= M * hq * 128, "pos/tok_seq/q_out too small");
    CHK(k_cache.dim() == 4 && k_cache.size(1) == hkv && k_cache.size(3) == 128, "k_cache [NB, hkv, BS, 128]");
    CHK(v_cache.dim() == 4 && v_cache.size(1) == hkv && v_cache.size(2) == 128 && v_cache.size(3) == k_cache.size(2),
        "v_cache [NB, hkv, 128, BS]");
    CHK(block_table.dim() == 2, "block_table [B, max_blocks]");
    chronos::GemvNorm n{};
    if (part.has_value()) n = normp_args(x, *part, eps, M);
    c10::hip::HIPGuardMasqueradingAsCUDA g(x.device());
    chronos::GemvRope rp{i32(pos), i32(tok_seq), i32(block_table), (int)block_table.size(1), cos_sin.data_ptr<float>(),
                         bfm(q_out), k_cache.data_ptr(), v_cache.data_ptr(), (int)hq, (int)hkv, (int)k_cache.size(2),
                         (float)(1.0 / k_scale), (float)(1.0 / v_scale)};
    chronos::launch_gemv_ex(bf(x), (int)M, (int)K, bf(w), (int)N, nullptr, false, part.has_value() ? &n : nullptr,
                            &rp, fp8, cur_stream(), wsc, wex);
}

// y = x @ w.T on MFMA (gemm.hip); swiglu as gemv.  stages = depth of the LDS-DMA ring (2..4)
Tensor gemm(const Tensor& x, const Tensor& w, bool swiglu, int64_t stages) {
    chk_bf16(x, "x");
    chk_bf16(w, "w");
    const int64_t K = x.size(-1), M = x.numel() / K, N = w.size(0);
    CHK(w.dim() == 2 && w.size(1) == K, "gemm: w must be [N, K]");
    CHK(K % 64 == 0, "gemm: K % 64 == 0");
    CHK(N % 128 == 0, "gemm: N % 128 == 0");
    CHK(M < (1LL << 31) / 128 && N * K < (1LL << 40), "gemm: size");
    CHK(stages >= 2 && stages <= 4, "gemm: stages in [2, 4]");
    c10::hip::HIPGuardMasqueradingAsCUDA g(x.device());
    auto y = at::empty({M, swiglu ? N / 2 : N}, x.options());
    chronos::launch_gemm(bf(x), bf(w), bfm(y), (int)M, (int)N, (int)K, swiglu, (int)stages, cur_stream());
    return y;
}


// Split-K tickets: one zeroed int buffer per (device, stream), at least n long; every call leaves it zeroed (each
// group's last arriver resets its own counter), so calls on one stream — and graph replays — share it.
static int32_t* split_tickets(const Tensor& x, int64_t n) {
    static std::mutex mu;
    static std::unordered_map<int64_t, Tensor> cnts;
    std::lock_guard<std::mutex> lk(mu);
    const int64_t key = ((int64_t)x.get_device() << 48) ^ (int64_t)(intptr_t)cur_stream();
    auto it = cnts.find(key);
    if (it == cnts.end() || it->second.numel() < n)
        it = cnts.insert_or_assign(key, at::zeros({std::max<int64_t>(n, 1 << 16)}, x.options().dtype(at::kInt))).first;
    return it->second.data_ptr<int32_t>();
}

// ---- what the three projection GEMM ops (gemm_pp, gemm_skinny, gemm_w4m) share -----------------------------------
// x bf16 [M, K] (any leading dims), one fused epilogue by mode: 0 plain (y [M, N]); 1 swiglu (w = [gate; up] [2F, K],
// y [M, F] = silu(x Wg^T) * (x Wu^T)); 2 resid (y = the new residual stream bf16(bf16(x @ w.T) + resid), second output =
// per-row partial sums of y^2, one per ``pcols`` output columns of the family).  part_in given (modes 0 / 1): x is the
// raw residual stream s and the folded input RMSNorm is applied as the per-row scale rsqrt(sum(part_in[m]) / K + eps).
struct GemmIO {
    Tensor y, part_out, ws;  // ws: the split-K workspace, alive until the launch is enqueued
};

inline void chk_gemm_x(const std::string& op, const Tensor& x, int64_t mode, const c10::optional<Tensor>& part_in) {
    chk_bf16(x, "x");
    CHK(x.dim() >= 1 && x.size(-1) > 0, op + ": x must be [M, K]");
    CHK(mode >= 0 && mode <= 2, op + ": mode");
    CHK(mode != 2 || !part_in.has_value(), op + ": resid mode has no norm prologue");
}

// mxfp4 weights (OCP MXFP4): q = packed e2m1 bytes [N, K / 2], e = e8m0 block scales [N, K / 32], on x's device
inline void chk_mxfp4(const std::string& op, const Tensor& x, const Tensor& q, const char* qn, const Tensor& e,
                      const char* en) {
    chk_gpu(q, qn);
    chk_gpu(e, en);
    const int64_t K = x.size(-1), N = q.size(0);
    CHK(q.scalar_type() == at::kByte && q.dim() == 2 && K % 32 == 0 && q.size(1) == K / 2,
        op + ": " + qn + " must be uint8 [N, K / 2]");
    CHK(e.scalar_type() == at::kByte && e.dim() == 2 && e.size(0) == N && e.size(1) == K / 32,
        op + ": " + en + " must be uint8 [N, K / 32]");
    CHK(q.device() == x.device() && e.device() == x.device(), op + ": " + qn + " / " + en + " on x's device");
}

// Fills the operand-independent part of the launch arguments: sizes, the output by mode, resid with the kResid
// partials [M, N / pcols], the norm prologue's partials.  Call with x's device current, after the shape checks.
static GemmIO gemm_io(const std::string& op, chronos::PPArgs& a, const Tensor& x, int64_t N, int64_t mode,
                      int64_t splitk, double eps, const c10::optional<Tensor>& resid,
                      const c10::optional<Tensor>& part_in, int64_t pcols) {
    const int64_t K = x.size(-1), M = x.numel() / K;
    GemmIO io;
    a.x = bf(x);
    a.M = (int)M;
    a.N = (int)N;
    a.K = (int)K;
    a.F = (int)(N / 2);
    a.splitk = (int)splitk;
    a.eps = (float)eps;
    io.y = at::empty({M, mode == 1 ? N / 2 : N}, x.options());
    a.y = bfm(io.y);
    if (mode == 2) {
        CHK(resid.has_value(), op + ": resid mode needs resid");
        chk_bf16(*resid, "resid");
        CHK(resid->numel() == M * N && resid->device() == x.device(), op + ": resid must be [M, N] on x's device");
        a.resid = bf(*resid);
        io.part_out = at::empty({M, N / pcols}, x.options().dtype(at::kFloat));
        a.part_out = io.part_out.data_ptr<float>();
    }
    if (part_in.has_value()) {
        chk_gpu(*part_in, "part_in");
        CHK(part_in->scalar_type() == at::kFloat && part_in->dim() == 2 && part_in->size(0) == M &&
                part_in->size(1) >= 1 && part_in->device() == x.device(),
            op + ": part_in must be f32 [M, P] on x's device");
        a.part_in = part_in->data_ptr<float>();
        a.nparts_in = (int)part_in->size(1);
    }
    return io;
}

// Split-K: ``floats`` f32 of workspace per (workgroup group, slice) and one ticket per group
static void gemm_splitk(chronos::PPArgs& a, GemmIO& io, const Tensor& x, int64_t groups, int64_t floats) {
    if (a.splitk > 1) {
        io.ws = at::empty({groups * a.splitk * floats}, x.options().dtype(at::kFloat));
        a.ws = io.ws.data_ptr<float>();
        a.cnt = split_tickets(x, groups);
    }
}

// Batched projection GEMM family (gemm_pp.hip, gemm_lg.hip), M >= 3: w bf16 [N, K]; the kResid partials are
// [M, N / (BN / 4)] (gemm_lg: BN / 2).  cfg = tile config (gemm_pp_bm / gemm_pp_bn), splitk divides K / 64.
std::tuple<Tensor, Tensor> gemm_pp(const Tensor& x, const Tensor& w, int64_t mode, int64_t cfg, int64_t splitk,
                                   const c10::optional<Tensor>& resid, const c10::optional<Tensor>& part_in,
                                   double eps, bool prio) {
    chk_gemm_x("gemm_pp", x, mode, part_in);
    chk_bf16(w, "w");
    const int64_t K = x.size(-1), M = x.numel() / K, N = w.size(0);
    CHK(w.dim() == 2 && w.size(1) == K, "gemm_pp: w must be [N, K]");
    const bool lg = cfg >= chronos::kPPConfigs;  // gemm_lg.hip configs continue the id space
    // 40-71: gemm_lg's timing-only ablations (wrong results by design), rejected unless built in
    CHK((cfg >= 0 && cfg < chronos::kPPConfigs + chronos::kLGConfigs) ||
            (chronos::gemm_lg_ablations_built() && cfg >= 40 && cfg < 72) ||
            (cfg >= chronos::kLGTinyFirst && cfg < chronos::kLGTinyFirst + chronos::kLGTinyConfigs), "gemm_pp: cfg");
    const int BM = lg ? chronos::gemm_lg_xm((int)cfg) : chronos::gemm_pp_bm((int)cfg);
    const int BN = lg ? chronos::gemm_lg_wn((int)cfg) : chronos::gemm_pp_bn((int)cfg);
    // gemm_lg addresses both operands through buffer descriptors: 32-bit byte offsets, with one tile of slack
    CHK(!lg || ((N + BN) * K * 2 < (1LL << 31) && (M + BM) * K * 2 < (1LL << 31)), "gemm_lg: operand > 2 GiB");
    CHK(M >= 1 && M < (1LL << 31) / BM && K % 64 == 0 && K <= (1 << 20) && N * K < (1LL << 40), "gemm_pp: size");
    CHK(splitk >= 1 && (K / 64) % splitk == 0, "gemm_pp: splitk must divide K / 64");
    CHK(!lg || splitk == 1 || chronos::gemm_lg_splitk_ok((int)cfg), "gemm_lg: this config has no split-K");
    CHK(mode == 0 ? N % 4 == 0 : N % BN == 0, "gemm_pp: N % 4 (plain) / N % BN (swiglu, resid)");
    CHK(mode != 1 || (lg ? (BN / 4) % 16 == 0 : (BN / 8) % 16 == 0), "gemm_pp: swiglu needs BN >= 128 (gemm_lg: 64)");
    c10::hip::HIPGuardMasqueradingAsCUDA g(x.device());
    chronos::PPArgs a{};
    GemmIO io = gemm_io("gemm_pp", a, x, N, mode, splitk, eps, resid, part_in, lg ? BN / 2 : BN / 4);
    a.w = bf(w);
    a.kts = (int)(K / 64 / splitk);
    // timing-only diagnostics (wrong results by design): honoured only in a CHRONOS_GEMM_ABLATIONS build
    a.ablate = chronos::gemm_lg_ablations_built() ? chronos::knob("pp_ablate", 0) : 0;
    a.gm = chronos::knob("pp_gm", 8);  // +7-9 % at M = 16384 (profiles/r3_gemm_tile_order_m16384.jsonl)
    a.handoff = chronos::knob("lg_handoff", -1);
    const int64_t tiles = ((M + BM - 1) / BM) * (mode == 1 ? (N / 2) / (BN / 2) : (N + BN - 1) / BN);
    gemm_splitk(a, io, x, tiles, (int64_t)BM * BN);
    if (lg) {
        CHK(!prio && chronos::launch_gemm_lg((int)cfg, (int)mode, part_in.has_value(), a, cur_stream()), "gemm_lg: launch");
    } else {
        CHK(chronos::launch_gemm_pp((int)cfg, (int)mode, part_in.has_value(), prio, a, cur_stream()), "gemm_pp: launch");
    }
    return {io.y, io.part_out};
}

// Skinny-M GEMM (gemm_skinny.hip), M <= 16 * MT of the config: the kResid partials are [M, N / (16 * RT)].  With ``we``
// the W4A16 weight mode: w / we = mxfp4 q / e, cfg an id of the W4 config table, K % (128 * NW * splitk) == 0.  With
// ``wscale`` (and no ``we``) the W8A16 weight mode: w = e4m3fn bytes [N, K], wscale = f32 per-row scales [N], cfg an id
// of the W8 config table, K % (64 * NW * splitk) == 0.
std::tuple<Tensor, Tensor> gemm_skinny(const Tensor& x, const Tensor& w, int64_t mode, int64_t cfg, int64_t splitk,
                                       const c10::optional<Tensor>& resid, const c10::optional<Tensor>& part_in,
                                       double eps, const c10::optional<Tensor>& we,
                                       const c10::optional<Tensor>& wscale) {
    chk_gemm_x("gemm_skinny", x, mode, part_in);
    const bool w4 = we.has_value(), w8 = wscale.has_value();
    CHK(!(w4 && w8), "gemm_skinny: wscale (W8A16) and we (W4A16) exclude each other");
    const int64_t K = x.size(-1), M = x.numel() / K, N = w.size(0);
    if (w8) {
        chk_gpu(w, "w");
        chk_gpu(*wscale, "wscale");
        CHK(w.scalar_type() == at::kByte && w.dim() == 2 && w.size(1) == K && w.is_contiguous() &&
                reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0,
            "gemm_skinny: W8 w must be contiguous uint8 [N, K], 16-B aligned");
        CHK(wscale->scalar_type() == at::kFloat && wscale->dim() == 1 && wscale->size(0) == N && wscale->is_contiguous(),
            "gemm_skinny: wscale must be contiguous f32 [N]");
        CHK(w.device() == x.device() && wscale->device() == x.device(), "gemm_skinny: w / wscale on x's device");
        CHK(cfg >= 0 && cfg < chronos::kSkinnyW8Configs, "gemm_skinny: W8 cfg");
    } else if (w4) {
        chk_mxfp4("gemm_skinny", x, w, "w", *we, "we");
        CHK(cfg >= 0 && cfg < chronos::kSkinnyW4Configs, "gemm_skinny: W4 cfg");
    } else {
        chk_bf16(w, "w");
        CHK(w.dim() == 2 && w.size(1) == K, "gemm_skinny: w must be [N, K]");
        CHK(cfg >= 0 && cfg < chronos::kSkinnyConfigs, "gemm_skinny: cfg");
    }
    const int c = (int)cfg;
    const int RT = w8 ? chronos::gemm_skinny_w8_rt(c) : w4 ? chronos::gemm_skinny_w4_rt(c) : chronos::gemm_skinny_rt(c);
    const int MT = w8 ? chronos::gemm_skinny_w8_mt(c) : w4 ? chronos::gemm_skinny_w4_mt(c) : chronos::gemm_skinny_mt(c);
    const int NW = w8 ? chronos::gemm_skinny_w8_nw(c) : w4 ? chronos::gemm_skinny_w4_nw(c) : chronos::gemm_skinny_nw(c);
    CHK(M >= 1 && M <= 16 * MT, "gemm_skinny: M must be in [1, 16 * MT] of the config");
    CHK(splitk >= 1 && K % ((w4 ? 128 : 64) * NW * splitk) == 0 && K <= (1 << 20) && N * K < (1LL << 40),
        w4 ? "gemm_skinny: W4 K % (128 * NW * splitk) == 0" : "gemm_skinny: K % (64 * NW * splitk) == 0");
    CHK(mode == 1 ? RT % 2 == 0 && (N / 2) % (8 * RT) == 0 && N % 2 == 0 : N % (16 * RT) == 0,
        "gemm_skinny: N % (16 RT) (swiglu: F % (8 RT), RT even)");
    c10::hip::HIPGuardMasqueradingAsCUDA g(x.device());
    chronos::PPArgs a{};
    GemmIO io = gemm_io("gemm_skinny", a, x, N, mode, splitk, eps, resid, part_in, 16 * RT);
    if (w8) {
        a.w = reinterpret_cast<const uint16_t*>(w.data_ptr<uint8_t>());
        a.wsc = wscale->data_ptr<float>();
    } else if (w4) {
        a.w = reinterpret_cast<const uint16_t*>(w.data_ptr<uint8_t>());
        a.wexp = we->data_ptr<uint8_t>();
    } else {
        a.w = bf(w);
    }
    gemm_splitk(a, io, x, mode == 1 ? (N / 2) / (8 * RT) : N / (16 * RT), (int64_t)64 * RT * MT * 4);
    if (w8) {
        CHK(chronos::launch_gemm_skinny_w8((int)cfg, (int)mode, part_in.has_value(), a, cur_stream()),
            "gemm_skinny: W8 launch");
    } else if (w4) {
        CHK(chronos::launch_gemm_skinny_w4((int)cfg, (int)mode, part_in.has_value(), a, cur_stream()),
            "gemm_skinny: W4 launch");
    } else {
        CHK(chronos::launch_gemm_skinny((int)cfg, (int)mode, part_in.has_value(), a, cur_stream()), "gemm_skinny: launch");
    }
    return {io.y, io.part_out};
}

// Mid-M W4A16 GEMM (gemm_w4m.hip): q / e = mxfp4 weights.  cfg indexes W4M_CONFIGS (tile = WN W rows x XM x rows, any
// M >= 1), K % (128 * splitk) == 0, N % WN == 0 (swiglu: F % (WN / 2) == 0); the kResid partials are [M, N / (WN / 2)].
std::tuple<Tensor, Tensor> gemm_w4m(const Tensor& x, const Tensor& q, const Tensor& e, int64_t mode, int64_t cfg,
                                    int64_t splitk, const c10::optional<Tensor>& resid,
                                    const c10::optional<Tensor>& part_in, double eps) {
    chk_gemm_x("gemm_w4m", x, mode, part_in);
    chk_mxfp4("gemm_w4m", x, q, "q", e, "e");
    const int64_t K = x.size(-1), M = x.numel() / K, N = q.size(0);
    CHK(cfg >= 0 && cfg < chronos::kW4MConfigs, "gemm_w4m: cfg");
    const int WN = chronos::gemm_w4m_wn((int)cfg), XM = chronos::gemm_w4m_xm((int)cfg);
    // x is addressed through a buffer descriptor: 32-bit byte offsets
    CHK(M >= 1 && K <= (1 << 20) && M * K < (1LL << 30) && N * K < (1LL << 40), "gemm_w4m: size (M K < 2^30)");
    CHK(splitk >= 1 && K % (128 * splitk) == 0, "gemm_w4m: K % (128 * splitk) == 0");
    CHK(mode == 1 ? N % 2 == 0 && (N / 2) % (WN / 2) == 0 : N % WN == 0,
        "gemm_w4m: N % WN (swiglu: F % (WN / 2)) == 0");
    c10::hip::HIPGuardMasqueradingAsCUDA g(x.device());
    chronos::PPArgs a{};
    GemmIO io = gemm_io("gemm_w4m", a, x, N, mode, splitk, eps, resid, part_in, WN / 2);
    a.w = reinterpret_cast<const uint16_t*>(q.data_ptr<uint8_t>());
    a.wexp = e.data_ptr<uint8_t>();
    const int64_t tiles = ((M + XM - 1) / XM) * (mode == 1 ? (N / 2) / (WN / 2) : N / WN);
    CHK(tiles * splitk < (1LL << 31), "gemm_w4m: grid");
    gemm_splitk(a, io, x, tiles, (int64_t)WN * XM);
    CHK(chronos::launch_gemm_w4m((int)cfg, (int)mode, part_in.has_value(), a, cur_stream()), "gemm_w4m: launch");
    return {io.y, io.part_out};
}

// [kW4MConfigs, 3] int64 on the CPU: (WN, XM, ST) per config id, so that ops/gemm.py's table can be pinned to the kernel's
Tensor gemm_w4m_configs() {
    Tensor t = at::empty({chronos::kW4MConfigs, 3}, at::TensorOptions().dtype(at::kLong));
    auto acc = t.accessor<int64_t, 2>();
    for (int c = 0; c < chronos::kW4MConfigs; ++c) {
        acc[c][0] = chronos::gemm_w4m_wn(c);
        acc[c][1] = chronos::gemm_w4m_xm(c);
        acc[c][2] = chronos::gemm_w4m_st(c);
    }
    return t;
}

// The split-K tickets of like's device and the current stream (what the GEMM families' launches use): every launch
// must leave them at zero.  An empty tensor before the first split-K launch.
Tensor split_ticket_state(const Tensor& like) {
    chk_gpu(like, "like");
    c10::hip::HIPGuardMasqueradingAsCUDA g(like.device());
    return at::from_blob(split_tickets(like, 1), {1 << 16}, like.options().dtype(at::kInt)).clone();
}

// ---- W8A8 fp8-e4m3 path (fp8.hip).  Quantised tensors travel as uint8 (OCP e4m3fn bytes) + fp32 scales.
// mode 0: quant(x); 1: quant(rmsnorm(x) * w); 2: resid <- bf16(x + resid), quant(rmsnorm(resid) * w);
// 3: x = [gate | up] rows of 2F, quant(silu(gate) * up)
std::tuple<Tensor, Tensor> quant_rows(const Tensor& x, const c10::optional<Tensor>& resid,
                                      const c10::optional<Tensor>& w, double eps, int64_t mode) {
    chk_bf16(x, "x");
    CHK(mode >= 0 && mode <= 3, "quant_rows: mode in {0, 1, 2, 3}");
    const int64_t d = mode == 3 ? x.size(-1) / 2 : x.size(-1), rows = x.numel() / x.size(-1);
    CHK(d % 8 == 0 && d <= 16384, "quant_rows: d must be % 8 and <= 16384");
    CHK(mode != 3 || x.size(-1) == 2 * d, "quant_rows: mode 3 needs [rows, 2F]");
    const bool norm = mode == 1 || mode == 2;
    if (norm) {
        CHK(w.has_value(), "quant_rows: rmsnorm modes need w");
        chk_bf16(*w, "w");
        CHK(w->numel() == d, "quant_rows: w must have d entries");
    }
    if (mode == 2) {
        CHK(resid.has_value(), "quant_rows: mode 2 needs resid");
        chk_bf16(*resid, "resid");
        CHK(resid->sizes() == x.sizes(), "quant_rows: resid shape mismatch");
    }
    c10::hip::HIPGuardMasqueradingAsCUDA g(x.device());
    auto q = at::empty({rows, d}, x.options().dtype(at::kByte));
    auto s = at::empty({rows}, x.options().dtype(at::kFloat));
    chronos::launch_quant_rows(bf(x), mode == 2 ? bfm(*resid) : nullptr, norm ? bf(*w) : nullptr,
                               q.data_ptr<uint8_t>(), s.data_ptr<float>(), (int)rows, (int)d, (float)eps, (int)mode,
                               cur_stream());
    return {q, s};
}

// y = (xq @ wq.T) * xs[:, None] * ws[None, :] (bf16); swiglu: wq = [gate; up] -> silu(gate) * up
Tensor qlinear(const Tensor& xq, const Tensor& xs, const Tensor& wq, const Tensor& ws, bool swiglu) {
    chk_gpu(xq, "xq");
    chk_gpu(wq, "wq");
    chk_gpu(xs, "xs");
    chk_gpu(ws, "ws");
    CHK(xq.scalar_type() == at::kByte && wq.scalar_type() == at::kByte, "qlinear: xq / wq must be uint8 (e4m3fn)");
    CHK(xs.scalar_type() == at::kFloat && ws.scalar_type() == at::kFloat, "qlinear: scales must be f32");
    const int64_t K = xq.size(-1), M = xq.numel() / K, N = wq.size(0);
    CHK(wq.dim() == 2 && wq.size(1) == K, "qlinear: wq must be [N, K]");
    CHK(xs.numel() == M && ws.numel() == N, "qlinear: one scale per token row / weight row");
    CHK(K % 128 == 0, "qlinear: K % 128 == 0");
    CHK(N % 128 == 0 && (!swiglu || (N / 2) % 64 == 0), "qlinear: N % 128 == 0 (SwiGLU: F % 64 == 0)");
    CHK(M < (1LL << 31) / 128 && N * K < (1LL << 40), "qlinear: size");
    c10::hip::HIPGuardMasqueradingAsCUDA g(xq.device());
    auto y = at::empty({M, swiglu ? N / 2 : N}, xq.options().dtype(at::kBFloat16));
    chronos::launch_qlinear(xq.data_ptr<uint8_t>(), xs.data_ptr<float>(), wq.data_ptr<uint8_t>(), ws.data_ptr<float>(),
                            bfm(y), (int)M, (int)N, (int)K, swiglu, cur_stream());
    return y;
}

// W8A8 on gemm_lg.hip's ring schedule (fp8 configs, gemm_lg_f8_*): the same result as qlinear for M >= 256 shapes.
// splitk divides K / 128.
Tensor qgemm_lg(const Tensor& xq, const Tensor& xs, const Tensor& wq, const Tensor& ws, bool swiglu, int64_t cfg,
                int64_t splitk) {
    chk_gpu(xq, "xq");
    chk_gpu(wq, "wq");
    chk_gpu(xs, "xs");
    chk_gpu(ws, "ws");
    CHK(xq.scalar_type() == at::kByte && wq.scalar_type() == at::kByte, "qgemm_lg: xq / wq must be uint8 (e4m3fn)");
    CHK(xs.scalar_type() == at::kFloat && ws.scalar_type() == at::kFloat, "qgemm_lg: scales must be f32");
    CHK(cfg >= 0 && cfg < chronos::kLGF8Configs, "qgemm_lg: cfg");
    const int64_t K = xq.size(-1), M = xq.numel() / K, N = wq.size(0);
    const int BM = chronos::gemm_lg_f8_xm((int)cfg), BN = chronos::gemm_lg_f8_wn((int)cfg);
    CHK(wq.dim() == 2 && wq.size(1) == K, "qgemm_lg: wq must be [N, K]");
    CHK(xs.numel() == M && ws.numel() == N, "qgemm_lg: one scale per token row / weight row");
    CHK(K % 128 == 0 && K <= (1 << 20) && splitk >= 1 && (K / 128) % splitk == 0, "qgemm_lg: splitk must divide K / 128");
    CHK(swiglu ? N % BN == 0 : N % 4 == 0, "qgemm_lg: N % 4 (plain) / N % BN (swiglu)");
    CHK(M >= 1 && (N + BN) * K < (1LL << 31) && (M + BM) * K < (1LL << 31), "qgemm_lg: operand > 2 GiB");
    c10::hip::HIPGuardMasqueradingAsCUDA g(xq.device());
    chronos::PPArgs a{};
    a.x = reinterpret_cast<const uint16_t*>(xq.data_ptr<uint8_t>());
    a.w = reinterpret_cast<const uint16_t*>(wq.data_ptr<uint8_t>());
    a.xsc = xs.data_ptr<float>();
    a.wsc = ws.data_ptr<float>();
    a.M = (int)M;
    a.N = (int)N;
    a.K = (int)K;
    a.F = (int)(N / 2);
    a.splitk = (int)splitk;
    a.kts = (int)(K / 128 / splitk);
    a.gm = chronos::knob("pp_gm", 8);
    a.handoff = chronos::knob("lg_handoff", -1);
    Tensor y = at::empty({M, swiglu ? N / 2 : N}, xq.options().dtype(at::kBFloat16));
    a.y = bfm(y);
    const int64_t tiles = ((M + BM - 1) / BM) * (swiglu ? (N / 2) / (BN / 2) : (N + BN - 1) / BN);
    Tensor wsl;
    if (splitk > 1) {
        wsl = at::empty({tiles * splitk * BM * BN}, xs.options());
        a.ws = wsl.data_ptr<float>();
        a.cnt = split_tickets(xq, tiles);
    }
    CHK(chronos::launch_gemm_lg_f8((int)cfg, swiglu, a, cur_stream()), "qgemm_lg: launch");
    return y;
}

// value < 0: forget the setting (the next read takes CHRONOS_<NAME> or the built-in default again)
void set_knob(const std::string& name, int64_t value) {
    std::lock_guard<std::mutex> lk(chronos::g_knob_mu);
    if (value < 0) chronos::g_knobs.erase(name);
    else chronos::g_knobs[name] = (int)value;
}

// ---- K14 IPC one-shot all-reduce (allreduce.hip); the handle is the C++ object's address as an int
int64_t ar_create(int64_t rank, int64_t world, int64_t max_bytes) {
    return reinterpret_cast<int64_t>(chronos::ar_create((int)rank, (int)world, max_bytes));
}
Tensor ar_handles(int64_t h) {
    auto v = chronos::ar_handles(reinterpret_cast<void*>(h));
    auto t = at::empty({(int64_t)v.size()}, at::TensorOptions().dtype(at::kByte));
    memcpy(t.data_ptr(), v.data(), v.size());
    return t;
}
void ar_open(int64_t h, const Tensor& all) {
    CHK(!all.is_cuda() && all.scalar_type() == at::kByte && all.dim() == 2, "ar_open: uint8 [world, bytes] CPU");
    auto c = all.contiguous();
    std::vector<std::vector<uint8_t>> v;
    for (int64_t i = 0; i < c.size(0); ++i) {
        const uint8_t* p = c.data_ptr<uint8_t>() + i * c.size(1);
        v.emplace_back(p, p + c.size(1));
    }
    chronos::ar_open(reinterpret_cast<void*>(h), v);
}
void ar_all_reduce(int64_t h, const Tensor& inp, const Tensor& out, int64_t spin_limit, int64_t algo) {
    chk_bf16(inp, "inp");
    chk_bf16(out, "out");
    CHK(inp.numel() == out.numel(), "ar_all_reduce: size mismatch");
    CHK(inp.numel() % 8 == 0 && inp.numel() <= chronos::ar_capacity(reinterpret_cast<void*>(h)),
        "ar_all_reduce: numel must be % 8 and fit the IPC buffer");
    c10::hip::HIPGuardMasqueradingAsCUDA g(inp.device());
    CHK(algo == 1 || algo == 2, "ar_all_reduce: algo must be 1 (one-shot) or 2 (two-shot)");
    chronos::ar_run(reinterpret_cast<void*>(h), bf(inp), bfm(out), inp.numel(), spin_limit, (int)algo, cur_stream());
}
// fused one-shot all-reduce + residual add + RMSNorm: resid <- bf16(sum(inp) + resid), y <- rmsnorm(resid) * w
void ar_all_reduce_norm(int64_t h, const Tensor& inp, const Tensor& resid, const Tensor& w, const Tensor& y, double eps,
                        int64_t spin_limit) {
    chk_bf16(inp, "inp");
    chk_bf16(resid, "resid");
    chk_bf16(w, "w");
    chk_bf16(y, "y");
    CHK(inp.dim() == 2 && resid.sizes() == inp.sizes() && y.sizes() == inp.sizes(), "ar_all_reduce_norm: [T, d] rows");
    CHK(w.numel() == inp.size(1) && inp.size(1) % 8 == 0 && inp.size(1) <= 8 * 256 * 8, "ar_all_reduce_norm: d");
    CHK(inp.numel() <= chronos::ar_capacity(reinterpret_cast<void*>(h)), "ar_all_reduce_norm: exceeds the IPC buffer");
    c10::hip::HIPGuardMasqueradingAsCUDA g(inp.device());
    chronos::ar_run_norm(reinterpret_cast<void*>(h), bf(inp), bfm(resid), bf(w), bfm(y), inp.size(0),
                         (int)inp.size(1), (float)eps, spin_limit, cur_stream());
}
int64_t ar_error(int64_t h) { return chronos::ar_error(reinterpret_cast<void*>(h)); }
int64_t ar_capacity(int64_t h) { return chronos::ar_capacity(reinterpret_cast<void*>(h)); }
void ar_destroy(int64_t h) { chronos::ar_destroy(reinterpret_cast<void*>(h)); }

}  // namespace

TORCH_LIBRARY(chronos, m) {
    m.def("embedding(Tensor ids, Tensor table, int vstart) -> Tensor");
    m.def("rmsnorm(Tensor x, Tensor w, float eps) -> Tensor");
    m.def("add_rmsnorm(Tensor x, Tensor(a!) resid, Tensor w, float eps) -> Tensor");
    m.def("rope_kv_write(Tensor qkv, Tensor pos, Tensor tok_seq, Tensor block_table, Tensor cos_sin, "
          "Tensor(a!) q_out, Tensor(b!) k_cache, Tensor(c!) v_cache, int hq, int hkv, bool write_q, "
          "float k_scale=1.0, float v_scale=1.0) -> ()");
    m.def("silu_mul(Tensor gate_up) -> Tensor");
    m.def("gemv(Tensor x, Tensor w, bool swiglu, Tensor? ws=None, Tensor? we=None) -> Tensor");
    m.def("gemm(Tensor x, Tensor w, bool swiglu, int stages=3) -> Tensor");
    m.def("gemm_pp(Tensor x, Tensor w, int mode, int cfg, int splitk, Tensor? resid, Tensor? part_in, float eps, bool prio) -> (Tensor, Tensor)");
    m.def("gemm_skinny(Tensor x, Tensor w, int mode, int cfg, int splitk, Tensor? resid, Tensor? part_in, float eps, Tensor? we=None, Tensor? wscale=None) "
          "-> (Tensor, Tensor)");
    m.def("gemm_w4m(Tensor x, Tensor q, Tensor e, int mode, int cfg, int splitk, Tensor? resid, Tensor? part_in, float eps) "
          "-> (Tensor, Tensor)");
    m.def("gemm_w4m_configs() -> Tensor", &gemm_w4m_configs);
    m.def("split_ticket_state(Tensor like) -> Tensor");
    m.def("gemv_resid(Tensor x, Tensor w, Tensor resid_in, Tensor(a!) resid_out, Tensor? ws=None, Tensor? we=None) -> Tensor");
    m.def("gemv_normp(Tensor s, Tensor part, float eps, Tensor w, bool swiglu, Tensor? ws=None, Tensor? we=None) -> Tensor");
    m.def("qkv_rope(Tensor x, Tensor? part, float eps, Tensor w, Tensor pos, Tensor tok_seq, "
          "Tensor block_table, Tensor cos_sin, Tensor(a!) q_out, Tensor(b!) k_cache, Tensor(c!) v_cache, int hq, "
          "int hkv, float k_scale=1.0, float v_scale=1.0, Tensor? ws=None, Tensor? we=None) -> ()");
    m.def("w4_expand(Tensor q, Tensor e, Tensor(a!) out) -> ()");
    m.def("set_decode_gate(Tensor? state, int n) -> ()", &set_decode_gate);
    m.def("attn_init() -> ()", [] { chronos::attn_init(); });
    m.def("quant_rows(Tensor x, Tensor(a!)? resid, Tensor? w, float eps, int mode) -> (Tensor, Tensor)");
    m.def("qlinear(Tensor xq, Tensor xs, Tensor wq, Tensor ws, bool swiglu) -> Tensor");
    m.def("qgemm_lg(Tensor xq, Tensor xs, Tensor wq, Tensor ws, bool swiglu, int cfg, int splitk) -> Tensor");
    m.def("set_knob(str name, int value) -> ()", &set_knob);
    m.def("ar_create(int rank, int world, int max_bytes) -> int", &ar_create);
    m.def("ar_handles(int h) -> Tensor", &ar_handles);
    m.def("ar_open(int h, Tensor all) -> ()", &ar_open);
    m.def("ar_all_reduce(int h, Tensor inp, Tensor(a!) out, int spin_limit, int algo=1) -> ()");
    m.def("ar_all_reduce_norm(int h, Tensor inp, Tensor(a!) resid, Tensor w, Tensor(b!) y, float eps, int spin_limit) -> ()");
    m.def("ar_error(int h) -> int", &ar_error);
    m.def("ar_capacity(int h) -> int", &ar_capacity);
    m.def("ar_destroy(int h) -> ()", &ar_destroy);
    m.def("decode_attention_rope(Tensor qkv, Tensor pos, Tensor cos_sin, Tensor(a!) k_cache, Tensor(b!) v_cache, "
          "Tensor block_table, Tensor ctx_len, int n, int hq, float scale, Tensor? casc=None, Tensor(c!)? casc_o=None, "
          "Tensor(d!)? casc_l=None) -> Tensor");
    m.def("paged_attention(Tensor q, Tensor k_cache, Tensor v_cache, Tensor block_table, Tensor q_start, "
          "Tensor ctx_len, Tensor? tiles, int ntiles, int nqt, int nsplit, float scale, float k_scale=1.0, "
          "float v_scale=1.0, int max_q=1) -> Tensor");
    m.def("constrained_sample(Tensor logits, Tensor? row_of_slot, Tensor next, Tensor dist, int done_state, "
          "Tensor(a!) state, Tensor(b!) remaining, Tensor? temperature, Tensor? seed, Tensor(c!) ids, Tensor(d!) pos, "
          "Tensor(e!) ctx, Tensor(f!) nout, Tensor(g!) out_tokens, Tensor? topk=None, Tensor? topp=None, "
          "Tensor? jump=None) -> ()");
    m.def("token_logprobs(Tensor logits, Tensor? row_of_slot, Tensor next, Tensor dist, int done_state, Tensor state, "
          "Tensor remaining, Tensor nout, Tensor lp_want, Tensor(a!) lp_mark, Tensor(b!) lp_lse, Tensor(c!) lp_top_ids, "
          "Tensor(d!) lp_top_val) -> ()");
    m.def("token_logprobs_commit(Tensor logits, Tensor? row_of_slot, Tensor nout, Tensor out_tokens, Tensor lp_want, "
          "Tensor lp_mark, Tensor lp_lse, Tensor lp_top_ids, Tensor lp_top_val, Tensor(a!) out_lp, "
          "Tensor(b!) out_lp_ids) -> ()");
    m.def("apply_penalties(Tensor(a!) logits, Tensor? row_of_slot, int done_state, Tensor state, Tensor nout, "
          "Tensor out_tokens, Tensor pen_par, Tensor pen_last, Tensor pen_tail, Tensor pen_tlen) -> ()");
    m.def("truncate_logits(Tensor(a!) logits, Tensor? row_of_slot, Tensor next, Tensor dist, int done_state, "
          "Tensor state, Tensor remaining, Tensor temperature, Tensor minp_ln, Tensor typical) -> ()");
    m.def("mirostat_truncate(Tensor(a!) logits, Tensor? row_of_slot, Tensor next, Tensor dist, int done_state, "
          "Tensor state, Tensor remaining, Tensor nout, Tensor temperature, Tensor mi_on, Tensor mi_mu, "
          "Tensor(b!) mi_m, Tensor(c!) mi_lnz, Tensor(d!) mi_mark) -> ()");
    m.def("mirostat_update(Tensor logits, Tensor? row_of_slot, Tensor nout, Tensor out_tokens, Tensor temperature, "
          "Tensor mi_on, Tensor(a!) mi_mu, Tensor mi_tau, Tensor mi_eta, Tensor mi_m, Tensor mi_lnz, Tensor mi_mark) "
          "-> ()");
    m.def("pool_accum(Tensor s, float eps, Tensor q_rows, Tensor sel, Tensor(a!) acc) -> ()");
    m.def("pool_finish(Tensor(a!) acc, Tensor rows, Tensor g, Tensor(b!) out) -> ()");
}

TORCH_LIBRARY_IMPL(chronos, CUDA, m) {
    m.impl("embedding", &embedding);
    m.impl("rmsnorm", &rmsnorm);
    m.impl("add_rmsnorm", &add_rmsnorm);
    m.impl("rope_kv_write", &rope_kv_write);
    m.impl("silu_mul", &silu_mul);
    m.impl("gemv", &gemv);
    m.impl("gemm", &gemm);
    m.impl("gemm_pp", &gemm_pp);
    m.impl("gemm_skinny", &gemm_skinny);
    m.impl("gemm_w4m", &gemm_w4m);
    m.impl("split_ticket_state", &split_ticket_state);
    m.impl("w4_expand", &w4_expand);
    m.impl("gemv_resid", &gemv_resid);
    m.impl("gemv_normp", &gemv_normp);
    m.impl("qkv_rope", &qkv_rope);
    m.impl("quant_rows", &quant_rows);
    m.impl("qlinear", &qlinear);
    m.impl("qgemm_lg", &qgemm_lg);
    m.impl("paged_attention", &paged_attention);
    m.impl("decode_attention_rope", &decode_attention_rope);
    m.impl("constrained_sample", &constrained_sample);
    m.impl("token_logprobs", &token_logprobs);
    m.impl("token_logprobs_commit", &token_logprobs_commit);
    m.impl("apply_penalties", &apply_penalties);
    m.impl("truncate_logits", &truncate_logits);
    m.impl("mirostat_truncate", &mirostat_truncate);
    m.impl("mirostat_update", &mirostat_update);
    m.impl("pool_accum", &pool_accum);
    m.impl("pool_finish", &pool_finish);
    m.impl("ar_all_reduce", &ar_all_reduce);
    m.impl("ar_all_reduce_norm", &ar_all_reduce_norm);
}
