// The temporal half of one attention-rollout step through a TimeSformer layer (divided space-time
// attention), flash-style: the T x T probabilities of every (patch, head) are recomputed from the kept
// temporal q'|k rows and never stored.
//
// A divided layer mixes tokens as x <- A_s A_t x, so the CLS row of the rollout takes per layer, last
// layer first, the spatial step and then the temporal one: r <- (r A_s) A_t.  The spatial step is
// vc_attention_rollout_step on the frame layout (B*T sequences of 1 + P tokens, every frame's slot 0
// holding r_CLS / T).  This file is the temporal step and the hop between the two layouts:
//     patch (p, t'):  y[t'] = alpha * (1/H) sum_h sum_t x[t] * P_h[t][t'] + (1 - alpha) * x[t'],
//                     x[t] = r_frame_in[b][t][1 + p],  P_h[t][.] = softmax2(q'_t . k_.) over the T frames
//     CLS:            c = sum_t r_frame_in[b][t][0]  (the temporal branch never updates CLS: identity row)
// y goes to the clip layout (r_clip_out[b][1 + p*T + t']) and, with the same bits, back to the frame
// layout for the next layer's spatial step (r_frame_out[b][t'][1 + p], slot 0 = c / T).
//
// The shape of temporal_attn_lds_kernel (divided.hip): one workgroup per (clip, patch), the patch's T
// rows of q'|k (not v) staged in LDS with 16-byte loads, one lane pair per (query frame, head) with 32 of
// the 64 dims each.  Exact maximum and exact sum over the T keys, so no lse is needed.  Deterministic
// (no atomics: heads summed in head order, then frames in frame order) and batch-invariant.
#include "common.hpp"

namespace vc {
namespace droll {

constexpr int64_t LDS_MAX = 160 * 1024;

// LDS: [T rows][2*H*8 uint4] q'|k image, then pw f32 [T query frames][H][T keys] (the probabilities),
// then xs f32 [T] (the patch's relevances).
__host__ __device__ inline int64_t lds_bytes(int64_t T, int64_t H) {
    return T * 2 * H * 64 * 2 + T * H * T * 4 + T * 4;
}

template <int TMAX>
__global__ void __launch_bounds__(256) temporal_rollout_kernel(const uint16_t* __restrict__ qkv, int64_t ld,
                                                               const float* __restrict__ rin, int P, int T, int H,
                                                               float alpha, float* __restrict__ rclip,
                                                               float* __restrict__ rframe) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t bp = blockIdx.x;  // b*P + p
    const int64_t b = bp / P, p = bp % P;
    const int64_t S = 1 + (int64_t)P * T;
    const int64_t row0 = b * S + 1 + p * T;  // the patch's first frame: the clip's CLS row is never read
    const int rw = 2 * H * 8;                // 16-byte pieces of q'|k per staged row
    uint4* lds = reinterpret_cast<uint4*>(smem);
    float* pw = reinterpret_cast<float*>(smem + (int64_t)T * rw * 16);
    float* xs = pw + T * H * T;
    for (int i = threadIdx.x; i < T * rw; i += blockDim.x) {
        const int t = i / rw, j = i - t * rw;
        lds[i] = reinterpret_cast<const uint4*>(qkv + (row0 + t) * ld)[j];
    }
    const float* rb = rin + b * T * (1 + (int64_t)P);  // the clip's T frame sequences
    if ((int)threadIdx.x < T) xs[threadIdx.x] = rb[(int64_t)threadIdx.x * (1 + P) + 1 + p];
    __syncthreads();
    const int hf = threadIdx.x & 1;
    for (int pair = threadIdx.x >> 1; pair < T * H; pair += blockDim.x >> 1) {  // uniform trip count per lane pair
        const int t = pair / H, hh = pair - t * H;
        const uint4* qp = lds + t * rw + hh * 8 + hf * 4;
        unsigned qw[16];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint4 u = qp[j];
            qw[4 * j] = u.x; qw[4 * j + 1] = u.y; qw[4 * j + 2] = u.z; qw[4 * j + 3] = u.w;
        }
        float s[TMAX];
        float m = -INFINITY;
#pragma unroll
        for (int k = 0; k < TMAX; ++k) {
            if (k < T) {
                const uint4* kp = lds + k * rw + (H + hh) * 8 + hf * 4;
                float a = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint4 u = kp[j];
                    a = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(v2bf, qw[4 * j]), __builtin_bit_cast(v2bf, u.x), a, false);
                    a = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(v2bf, qw[4 * j + 1]), __builtin_bit_cast(v2bf, u.y), a, false);
                    a = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(v2bf, qw[4 * j + 2]), __builtin_bit_cast(v2bf, u.z), a, false);
                    a = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(v2bf, qw[4 * j + 3]), __builtin_bit_cast(v2bf, u.w), a, false);
                }
                a += __shfl_xor(a, 1, 64);  // both lanes of the pair hold the same sum (a + b == b + a)
                s[k] = a;
                m = fmaxf(m, a);
            }
        }
        float l = 0.f;
#pragma unroll
        for (int k = 0; k < TMAX; ++k) {
            if (k < T) {
                s[k] = exp2f(s[k] - m);
                l += s[k];
            }
        }
        const float inv = 1.0f / l;
        float* dst = pw + (int64_t)pair * T;
        // the pair's two lanes split the keys: even / odd
#pragma unroll
        for (int k = 0; k < TMAX; ++k)
            if (k < T && (k & 1) == hf) dst[k] = s[k] * inv;
    }
    __syncthreads();
    const int tq = threadIdx.x;  // the key frame t' this thread finishes
    if (tq < T) {
        float u = 0.f;
        for (int t = 0; t < T; ++t) {  // frames in frame order, each one's heads in head order
            const float* pt = pw + (int64_t)t * H * T + tq;
            float a = 0.f;
            for (int hh = 0; hh < H; ++hh) a += pt[hh * T];
            u = __builtin_fmaf(xs[t], a, u);
        }
        const float y = alpha * (u / (float)H) + (1.0f - alpha) * xs[tq];
        rclip[b * S + 1 + p * T + tq] = y;
        if (rframe) rframe[(b * T + tq) * (1 + (int64_t)P) + 1 + p] = y;
        if (p == 0) {  // the clip's CLS entry, by its first patch's workgroup: every thread sums in t order
            float c = 0.f;
            for (int t = 0; t < T; ++t) c += rb[(int64_t)t * (1 + P)];
            if (tq == 0) rclip[b * S] = c;
            if (rframe) rframe[(b * T + tq) * (1 + (int64_t)P)] = __fdiv_rn(c, (float)T);
        }
    }
}

static bool overlap(const float* a, int64_t na, const float* b, int64_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)nb * 4 && b0 < a0 + (uintptr_t)na * 4;
}

template <int TMAX>
static int launch(const uint16_t* qkv, int64_t ld, const float* rin, int64_t B, int64_t P, int64_t T, int64_t H,
                  float alpha, float* rclip, float* rframe, hipStream_t stream) {
    const int64_t lds = lds_bytes(T, H);
    static bool attr_set = false;  // per instantiation; benign race (idempotent)
    if (lds > 64 * 1024 && !attr_set) {
        hipError_t e = hipFuncSetAttribute((const void*)temporal_rollout_kernel<TMAX>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX);
        if (e != hipSuccess)
            return fail((int)e, std::string("vc_temporal_rollout_step: hipFuncSetAttribute: ") + hipGetErrorString(e));
        attr_set = true;
    }
    // one lane pair per (frame, head), whole waves, at most 256 threads (TimeSformer-B: 192)
    const int64_t want = (2 * T * H + 63) / 64 * 64;
    const unsigned nt = (unsigned)(want < 256 ? want : 256);
    temporal_rollout_kernel<TMAX><<<(unsigned)(B * P), nt, (size_t)lds, stream>>>(qkv, ld, rin, (int)P, (int)T, (int)H,
                                                                                 alpha, rclip, rframe);
    return check_launch("vc_temporal_rollout_step");
}

}  // namespace droll
}  // namespace vc

using namespace vc;
using namespace vc::droll;

extern "C" int vc_temporal_rollout_step(const uint16_t* qkv, int64_t ld, const float* r_frame_in, int64_t B, int64_t P,
                                        int64_t T, int64_t H, int64_t head_dim, float alpha, float* r_clip_out,
                                        float* r_frame_out, hipStream_t stream) {
    if (!qkv || !r_frame_in || !r_clip_out) return fail(VC_ERR_INVALID_ARG, "vc_temporal_rollout_step: null pointer");
    if (head_dim != 64) return fail(VC_ERR_UNSUPPORTED, "vc_temporal_rollout_step: head_dim must be 64");
    if (T > 32) return fail(VC_ERR_UNSUPPORTED, "vc_temporal_rollout_step: T > 32");
    if (B <= 0 || P <= 0 || T <= 0 || H <= 0 || ld < 3 * H * 64 || ld % 8)
        return fail(VC_ERR_INVALID_ARG, "vc_temporal_rollout_step: bad shape / leading dimension");
    if (((uintptr_t)qkv) & 15) return fail(VC_ERR_INVALID_ARG, "vc_temporal_rollout_step: qkv must be 16-byte aligned");
    if ((((uintptr_t)r_frame_in) | ((uintptr_t)r_clip_out) | ((uintptr_t)r_frame_out)) & 3)
        return fail(VC_ERR_INVALID_ARG, "vc_temporal_rollout_step: f32 pointers must be 4-byte aligned");
    if (B * P >= (1LL << 31) || P * T >= (1LL << 30))
        return fail(VC_ERR_INVALID_ARG, "vc_temporal_rollout_step: grid too large");
    if (lds_bytes(T, H) > LDS_MAX)
        return fail(VC_ERR_UNSUPPORTED, "vc_temporal_rollout_step: a patch's T rows of q|k and its T*H*T probabilities exceed the LDS");
    const int64_t nf = B * T * (1 + P), nc = B * (1 + P * T);
    if (overlap(r_clip_out, nc, r_frame_in, nf) || (r_frame_out && (overlap(r_frame_out, nf, r_frame_in, nf) ||
                                                                     overlap(r_frame_out, nf, r_clip_out, nc))))
        return fail(VC_ERR_INVALID_ARG, "vc_temporal_rollout_step: the outputs must not alias r_frame_in or each other");
    if (T <= 8) return launch<8>(qkv, ld, r_frame_in, B, P, T, H, alpha, r_clip_out, r_frame_out, stream);
    if (T <= 16) return launch<16>(qkv, ld, r_frame_in, B, P, T, H, alpha, r_clip_out, r_frame_out, stream);
    return launch<32>(qkv, ld, r_frame_in, B, P, T, H, alpha, r_clip_out, r_frame_out, stream);
}
