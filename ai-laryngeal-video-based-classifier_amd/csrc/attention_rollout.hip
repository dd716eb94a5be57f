// One step of attention rollout (Abnar & Zuidema 2020) for the CLS row, flash-style: the
// probabilities are recomputed from q', k and the forward's base-2 log-sum-exp and never stored.
//
// Rollout multiplies the layers' head-averaged attention matrices, each mixed with the identity for
// the residual branch; the classifier reads the CLS token alone, so only the CLS row of that product
// is wanted and the L matrix products become L vector-times-matrix products, last layer first:
//     u[b][j]     = (1/H) sum_h sum_i r_in[b][i] * P_h[i][j],   P_h[i][j] = exp2(q'_i . k_j - lse2[i])
//     r_out[b][j] = alpha * u[b][j] + (1 - alpha) * r_in[b][j]
// This is the shape of the first two steps of the dK/dV kernel (attention_bwd.hip): one wave per 32
// keys with K in registers, looping over 64-query tiles of Q' staged in LDS; S = Q'.K^T comes out of
// the MFMA with the query on the accumulator's register index, so -lse initialises it per register
// and the weighted sum over queries is a per-lane fp32 FMA chain on the accumulator (P is never
// rounded and there is no second MFMA).
// Two launches, deterministic (no atomics), batch-invariant:
//   partial : work[(b*H + h)*S + j] = sum_i r_in[b][i] P_h[i][j], queries summed in index order per
//             lane half, then the two halves;
//   combine : the heads summed in head order, the mean and the residual mix.
//
// The gradient-weighted step (Chefer, Gur & Wolf 2021, the self-attention rule) is the same kernel
// with a second factor per score, the gradient of the target logit with respect to the probability,
// dP_h[i][j] = dO_h[i] . v_j, and the positive part of the product:
//     u[b][j]     = (1/H) sum_h sum_i r_in[b][i] * max(P_h[i][j] * dP_h[i][j], 0)
//     r_out[b][j] = alpha * u[b][j] + beta * r_in[b][j]
// The wave keeps its 32 V rows in registers beside K, a dO image is staged beside the Q' image, and a
// second MFMA chain yields dP in the accumulator layout of S, so the product is per register.
#include "common.hpp"

namespace vc {
namespace roll {

constexpr int TILE_BYTES = 64 * 64 * 2;  // one [64 queries][64 bf16] image, 128-B rows

// 16-B chunk swizzle of a 128-B-row image, conflict-free for ds_read_b128 row reads (as attention_bwd.hip)
__device__ __forceinline__ int bswz(int r, int c) {
    const int m = (r >> 1) & 7;
    return c ^ (((m & 1) << 2) | (m & 2) | ((m >> 2) & 1));
}

// bijective XCD-aware remap of the linear workgroup id (as the forward kernel)
__device__ __forceinline__ int xcd_remap(int L, int nwg) {
    const int xq = nwg >> 3, xr = nwg & 7, xcd = L & 7;
    return (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (L >> 3);
}

// ---------------------------------------------------------------------------------
// workgroup = 128 keys of one (clip, head), wave w owns keys 32w..32w+31.
// Per 64-query tile (double-buffered LDS: Q' image, -lse[64], r_in[64]), per 32-query block:
//   S [q][key] = Q'.K^T - lse     A = Q' rows (LDS b128), B = K (registers), C = -lse per register
//   acc[key]  += sum_q r_in[q] * exp2(S[q][key])
// Register 4g+e of lane (r, h) holds query 8g + 4h + e of the block and key r.
// No row outside the clip is read: the row index of a partial tile's overhang is clamped to the
// clip's last token, and those queries are then masked by index (S = -inf, P = 0 exactly), as are
// the keys past S (never stored).
// GRAD (the gradient-weighted step): V in registers beside K, a dO image after the Q' image in the
// slot (same swizzle, rows clamped as Q''s) and a second chain of four MFMAs,
//   dP[q][key] = dO.V^T           A = dO rows (LDS b128), B = V (registers), C = 0
//   acc[key]  += sum_q r_in[q] * max(exp2(S[q][key]) * dP[q][key], 0)
// The masked queries also get dP = 0, so nothing is left to a 0 * NaN.
// ---------------------------------------------------------------------------------
template <bool GRAD>
__global__ void __launch_bounds__(256, 2)
rollout_partial_kernel(const uint16_t* __restrict__ qkv, int64_t ld, const uint16_t* __restrict__ dout, int64_t lddo,
                       const float* __restrict__ lse, const float* __restrict__ rin, int S, int H,
                       float* __restrict__ work) {
    constexpr int IMG = (GRAD ? 2 : 1) * TILE_BYTES;  // the slot's images: Q', then dO
    constexpr int SLOT = IMG + 2 * 64 * 4;            // + -lse[64] + r_in[64]
    __shared__ __attribute__((aligned(16))) char smem[2 * SLOT];
    const int nk = gridDim.x;
    const int wg = xcd_remap(blockIdx.y * nk + blockIdx.x, nk * gridDim.y);
    const int kblk = wg % nk, bh = wg / nk;
    const int b = bh / H, hh = bh % H;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;

    const int64_t tok0 = (int64_t)b * S;
    const uint16_t* qbase = qkv + tok0 * ld + hh * 64;
    const uint16_t* kbase = qkv + tok0 * ld + (int64_t)H * 64 + hh * 64;
    const float* lseb = lse + (int64_t)bh * S;
    const float* rb = rin + tok0;

    const int key = kblk * 128 + wave * 32 + r;
    const int kc = key < S ? key : S - 1;
    v8bf kf[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
        kf[kk] = __builtin_bit_cast(v8bf, *reinterpret_cast<const v8s*>(kbase + (int64_t)kc * ld + 16 * kk + 8 * h));
    [[maybe_unused]] v8bf vf[4];
    [[maybe_unused]] const uint16_t* dbase = nullptr;
    if constexpr (GRAD) {
        const uint16_t* vbase = kbase + (int64_t)H * 64;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
            vf[kk] = __builtin_bit_cast(v8bf, *reinterpret_cast<const v8s*>(vbase + (int64_t)kc * ld + 16 * kk + 8 * h));
        dbase = dout + tok0 * lddo + hh * 64;
    }
    int roff[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) roff[kk] = r * 128 + bswz(r, 2 * kk + h) * 16;

    const int nt = (S + 63) / 64;
    uint4 pq0, pq1;
    [[maybe_unused]] uint4 pd0, pd1;
    float tf = 0.f;  // the raw lse (threads 0-63) / r_in (64-127) of the prefetched tile
    const int sr0 = tid >> 3, sc = tid & 7;
    const int so0 = sr0 * 128 + bswz(sr0, sc) * 16, so1 = (sr0 + 32) * 128 + bswz(sr0 + 32, sc) * 16;
#define ROLL_LOAD(t)                                                                                    \
    {                                                                                                   \
        const int q0 = (t) * 64 + sr0, q1 = q0 + 32;                                                    \
        pq0 = *reinterpret_cast<const uint4*>(qbase + (int64_t)(q0 < S ? q0 : S - 1) * ld + sc * 8);    \
        pq1 = *reinterpret_cast<const uint4*>(qbase + (int64_t)(q1 < S ? q1 : S - 1) * ld + sc * 8);    \
        if constexpr (GRAD) {                                                                           \
            pd0 = *reinterpret_cast<const uint4*>(dbase + (int64_t)(q0 < S ? q0 : S - 1) * lddo + sc * 8); \
            pd1 = *reinterpret_cast<const uint4*>(dbase + (int64_t)(q1 < S ? q1 : S - 1) * lddo + sc * 8); \
        }                                                                                               \
        const int q = (t) * 64 + (tid & 63);                                                            \
        const int qc = q < S ? q : S - 1;                                                               \
        tf = ((tid >> 6) & 1) ? rb[qc] : lseb[qc];                                                      \
    }
    // LDS holds -lse (the S accumulator's initial value) and r_in; 0 for the queries past S, which
    // the last tile masks by index below
#define ROLL_STORE(slot, t)                                                                             \
    {                                                                                                   \
        *reinterpret_cast<uint4*>((slot) + so0) = pq0;                                                  \
        *reinterpret_cast<uint4*>((slot) + so1) = pq1;                                                  \
        if constexpr (GRAD) {                                                                           \
            *reinterpret_cast<uint4*>((slot) + TILE_BYTES + so0) = pd0;                                 \
            *reinterpret_cast<uint4*>((slot) + TILE_BYTES + so1) = pd1;                                 \
        }                                                                                               \
        if (tid < 128)                                                                                  \
            reinterpret_cast<float*>((slot) + IMG)[tid] =                                               \
                ((t) * 64 + (tid & 63) >= S) ? 0.f : (tid < 64 ? -tf : tf);                             \
    }
    ROLL_LOAD(0);
    ROLL_STORE(smem, 0);
    __syncthreads();

    float acc = 0.f;
    for (int t = 0; t < nt; ++t) {
        const char* qi = smem + (t & 1) * SLOT;
        const float* fl = reinterpret_cast<const float*>(qi + IMG);  // [0,64) -lse, [64,128) r_in
        if (t + 1 < nt) ROLL_LOAD(t + 1);
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            v16f s, w;
            [[maybe_unused]] v16f dp;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 L0 = *reinterpret_cast<const float4*>(fl + 32 * qb + 8 * g + 4 * h);
                const float4 W0 = *reinterpret_cast<const float4*>(fl + 64 + 32 * qb + 8 * g + 4 * h);
                s[4 * g + 0] = L0.x; s[4 * g + 1] = L0.y; s[4 * g + 2] = L0.z; s[4 * g + 3] = L0.w;
                w[4 * g + 0] = W0.x; w[4 * g + 1] = W0.y; w[4 * g + 2] = W0.z; w[4 * g + 3] = W0.w;
            }
            if constexpr (GRAD) {
#pragma unroll
                for (int e = 0; e < 16; ++e) dp[e] = 0.f;
            }
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const v8bf qf = __builtin_bit_cast(v8bf, *reinterpret_cast<const v8s*>(qi + qb * 4096 + roff[kk]));
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf, kf[kk], s, 0, 0, 0);
                if constexpr (GRAD) {
                    const v8bf df = __builtin_bit_cast(
                        v8bf, *reinterpret_cast<const v8s*>(qi + TILE_BYTES + qb * 4096 + roff[kk]));
                    dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(df, vf[kk], dp, 0, 0, 0);
                }
            }
            if (t == nt - 1) {
                const int q0 = t * 64 + 32 * qb + 4 * h;
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    if (q0 + 8 * (e >> 2) + (e & 3) >= S) {
                        s[e] = -INFINITY;
                        if constexpr (GRAD) dp[e] = 0.f;
                    }
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                if constexpr (GRAD)
                    acc = __builtin_fmaf(w[e], fmaxf(__builtin_amdgcn_exp2f(s[e]) * dp[e], 0.f), acc);
                else
                    acc = __builtin_fmaf(w[e], __builtin_amdgcn_exp2f(s[e]), acc);
            }
        }
        if (t + 1 < nt) ROLL_STORE(smem + ((t + 1) & 1) * SLOT, t + 1);
        __syncthreads();
    }
#undef ROLL_LOAD
#undef ROLL_STORE
    // the two lane halves hold the queries 8g + e and 8g + 4 + e of every block: lower half first
    const float other = __shfl_xor(acc, 32, 64);
    if (h == 0 && key < S) work[(int64_t)bh * S + key] = acc + other;
}

// r_out[b][j] = alpha * (1/H) sum_h work[b][h][j] + beta * r_in[b][j], heads in order.  The plain step passes
// beta = 1 - alpha, formed on the host in fp32: the same subtraction, so its bits stay as they are.
__global__ void __launch_bounds__(256) rollout_combine_kernel(const float* __restrict__ work, const float* __restrict__ rin,
                                                             int64_t n, int S, int H, float alpha, float beta,
                                                             float* __restrict__ rout) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t b = i / S, j = i - b * S;
    const float* p = work + b * H * S + j;
    float u = 0.f;
    for (int hh = 0; hh < H; ++hh) u += p[(int64_t)hh * S];
    rout[i] = alpha * (u / (float)H) + beta * rin[i];
}

// both entries: validation and the two launches; `me` names the entry in the messages, `grad`: dout / lddo are used
static int rollout_step(const char* me, bool grad, const uint16_t* qkv, int64_t ld, const uint16_t* dout, int64_t lddo,
                        const float* lse, const float* r_in, int64_t B, int64_t S, int64_t H, int64_t head_dim, float alpha,
                        float beta, float* work, int64_t work_elems, float* r_out, hipStream_t stream) {
    auto bad = [&](int code, const char* what) { return fail(code, std::string(me) + ": " + what); };
    if (!qkv || (grad && !dout) || !lse || !r_in || !work || !r_out) return bad(VC_ERR_INVALID_ARG, "null pointer");
    if (head_dim != 64) return bad(VC_ERR_UNSUPPORTED, "head_dim must be 64");
    if (B <= 0 || S <= 0 || H <= 0 || ld < 3 * H * 64 || ld % 8)
        return bad(VC_ERR_INVALID_ARG, "bad shape / leading dimension");
    if (grad && (lddo < H * 64 || lddo % 8)) return bad(VC_ERR_INVALID_ARG, "bad dO leading dimension");
    if ((((uintptr_t)qkv) | ((uintptr_t)dout)) & 15)
        return bad(VC_ERR_INVALID_ARG, grad ? "qkv and dO must be 16-byte aligned" : "qkv must be 16-byte aligned");
    if ((((uintptr_t)lse) | ((uintptr_t)r_in) | ((uintptr_t)work) | ((uintptr_t)r_out)) & 3)
        return bad(VC_ERR_INVALID_ARG, "f32 pointers must be 4-byte aligned");
    if (B * H > 65535 || S > (1 << 24)) return bad(VC_ERR_INVALID_ARG, "grid too large");
    if (work_elems < B * H * S) return bad(VC_ERR_INVALID_ARG, "work buffer too small");
    if (work == r_in || work == r_out) return bad(VC_ERR_INVALID_ARG, "work must not alias r_in / r_out");
    const dim3 grid((unsigned)((S + 127) / 128), (unsigned)(B * H));
    if (grad)
        rollout_partial_kernel<true><<<grid, 256, 0, stream>>>(qkv, ld, dout, lddo, lse, r_in, (int)S, (int)H, work);
    else
        rollout_partial_kernel<false><<<grid, 256, 0, stream>>>(qkv, ld, nullptr, 0, lse, r_in, (int)S, (int)H, work);
    const int64_t n = B * S;
    rollout_combine_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(work, r_in, n, (int)S, (int)H, alpha, beta,
                                                                            r_out);
    return check_launch(me);
}

}  // namespace roll
}  // namespace vc

using namespace vc;
using namespace vc::roll;

extern "C" int vc_attention_rollout_step(const uint16_t* qkv, int64_t ld, const float* lse, const float* r_in, int64_t B,
                                         int64_t S, int64_t H, int64_t head_dim, float alpha, float* work,
                                         int64_t work_elems, float* r_out, hipStream_t stream) {
    return rollout_step("vc_attention_rollout_step", false, qkv, ld, nullptr, 0, lse, r_in, B, S, H, head_dim, alpha,
                        1.0f - alpha, work, work_elems, r_out, stream);
}

extern "C" int vc_attention_grad_rollout_step(const uint16_t* qkv, int64_t ld, const uint16_t* dout, int64_t lddo,
                                              const float* lse, const float* r_in, int64_t B, int64_t S, int64_t H,
                                              int64_t head_dim, float alpha, float beta, float* work,
                                              int64_t work_elems, float* r_out, hipStream_t stream) {
    return rollout_step("vc_attention_grad_rollout_step", true, qkv, ld, dout, lddo, lse, r_in, B, S, H, head_dim, alpha,
                        beta, work, work_elems, r_out, stream);
}
