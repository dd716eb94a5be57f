// ResNet50-LSTM saliency (VideoResNet50LSTM.explain): the two links between the recurrence's data gradient and the
// class-activation maps of cam.hip.  The backbone is a 2D network applied per frame and ends in a per-frame
// AdaptiveAvgPool2d(1) (vc_frame_avgpool) over P positions, so with g[n] = d logit / d pooled features of frame n
// (fp32, as it leaves the lstm_dx GEMM) the gradient at res5 is g[n][c] / P at every position:
//  * frame_cam_kernel          map[n*P + p] = (1/P) sum_c g[n][c] x[n*P + p][c] (Grad-CAM and HiResCAM coincide
//                              there) and frame_rel[n] = sum_p map[n*P + p]: one workgroup per frame, the frame's g row
//                              held in registers (lane l the 8-channel chunks l, l + 64, ..., as cam_map_kernel), waves
//                              striding over the positions with a wave64 butterfly each, the frame sum in position
//                              order after a barrier.  With P = 1 and x the pooled features it is gradient x input;
//  * frame_avgpool_bwd_kernel  out[n*P + p][c] = bf16(g[n][c] / P): the adjoint of vc_frame_avgpool, the seed of the
//                              res4 chain.  One thread per (row, 8-channel chunk).
// cam.hip's conventions: channels-last bf16 rows, C % 8 == 0, 16-B loads, only rows < N*P and columns < C are read or
// written, no atomics and a fixed summation order (bit-reproducible; frame n's outputs do not depend on N).
#include "common.hpp"

namespace vc {
namespace frame_cam {

constexpr int MAX_CHUNKS = 8;  // 8-channel chunks a lane holds of the frame's g row: C <= 8 * 64 * 8 = 4096

__device__ __forceinline__ void unpack8(const uint4 u, float* v) {
    const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[2 * e] = bf2f((unsigned short)(w[e] & 0xffff));
        v[2 * e + 1] = bf2f((unsigned short)(w[e] >> 16));
    }
}

__device__ __forceinline__ void load8f(const float* p, float* v) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    const float4 b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// grid N, 4 waves; wave w the positions w, w + 4, ...
__global__ void __launch_bounds__(256) frame_cam_kernel(const uint16_t* __restrict__ x, int64_t ldx, const float* __restrict__ g,
                                                        int64_t ldg, int P, int C8, float* __restrict__ map,
                                                        float* __restrict__ frame_rel) {
    const int64_t n = blockIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float gr[MAX_CHUNKS][8];
#pragma unroll
    for (int k = 0; k < MAX_CHUNKS; ++k) {
        const int c8 = lane + 64 * k;
        if (c8 < C8) {
            load8f(g + n * ldg + c8 * 8, gr[k]);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) gr[k][e] = 0.f;
        }
    }
    const float fp = (float)P;
    float* out = map + n * P;
    for (int p = w; p < P; p += 4) {  // wave-uniform
        const uint16_t* row = x + (n * P + p) * ldx;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < MAX_CHUNKS; ++k) {
            const int c8 = lane + 64 * k;
            if (c8 < C8) {
                float a[8];
                unpack8(*reinterpret_cast<const uint4*>(row + c8 * 8), a);
#pragma unroll
                for (int e = 0; e < 8; ++e) s = __builtin_fmaf(gr[k][e], a[e], s);
            }
        }
        s = wave_sum(s);
        if (lane == 0) out[p] = s / fp;
    }
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int p = 0; p < P; ++p) s += out[p];
        frame_rel[n] = s;
    }
}

// one thread per (row, 8-channel chunk)
__global__ void __launch_bounds__(256) frame_avgpool_bwd_kernel(const float* __restrict__ g, int64_t ldg, int64_t total, int P,
                                                                int C8, uint16_t* __restrict__ out, int64_t ldo) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C8) * 8;
    const int64_t row = i / C8;
    const float fp = (float)P;
    float v[8];
    load8f(g + (row / P) * ldg + c, v);
    uint4 o;
    o.x = pack2bf(v[0] / fp, v[1] / fp);
    o.y = pack2bf(v[2] / fp, v[3] / fp);
    o.z = pack2bf(v[4] / fp, v[5] / fp);
    o.w = pack2bf(v[6] / fp, v[7] / fp);
    *reinterpret_cast<uint4*>(out + row * ldo + c) = o;
}

static bool rows16(const void* p, int64_t ld, int64_t per16) { return p && ld % per16 == 0 && ((uintptr_t)p & 15) == 0; }

}  // namespace frame_cam
}  // namespace vc

using namespace vc;
using namespace vc::frame_cam;

extern "C" {

int vc_frame_cam(const uint16_t* x, int64_t ldx, const float* g, int64_t ldg, int64_t N, int64_t P, int64_t C, float* map,
                 float* frame_rel, hipStream_t stream) {
    if (!x || !g || !map || !frame_rel) return fail(VC_ERR_INVALID_ARG, "vc_frame_cam: null pointer");
    if (N <= 0 || N > 0x7fffffff || P <= 0 || P > 0x7fffffff || C <= 0 || C % 8 || C > 8 * 64 * MAX_CHUNKS || ldx < C ||
        ldg < C || !rows16(x, ldx, 8) || !rows16(g, ldg, 4))
        return fail(VC_ERR_INVALID_ARG, "vc_frame_cam: need C % 8 == 0, C <= 4096, ldx >= C, ldg >= C, 16-B rows");
    frame_cam_kernel<<<(unsigned)N, 256, 0, stream>>>(x, ldx, g, ldg, (int)P, (int)(C / 8), map, frame_rel);
    return check_launch("vc_frame_cam");
}

int vc_frame_avgpool_bwd(const float* g, int64_t ldg, int64_t N, int64_t P, int64_t C, uint16_t* out, int64_t ldo,
                         hipStream_t stream) {
    if (!g || !out) return fail(VC_ERR_INVALID_ARG, "vc_frame_avgpool_bwd: null pointer");
    if (N <= 0 || P <= 0 || P > 0x7fffffff || C <= 0 || C % 8 || ldg < C || ldo < C || !rows16(g, ldg, 4) ||
        !rows16(out, ldo, 8))
        return fail(VC_ERR_INVALID_ARG, "vc_frame_avgpool_bwd: need C % 8 == 0, ldg >= C, ldo >= C, 16-B rows");
    const int64_t total = N * P * (C / 8);
    if (total > (int64_t)0x7fffffff * 256) return fail(VC_ERR_INVALID_ARG, "vc_frame_avgpool_bwd: grid too large");
    frame_avgpool_bwd_kernel<<<(unsigned)((total + 255) / 256), 256, 0, stream>>>(g, ldg, total, (int)P, (int)(C / 8), out, ldo);
    return check_launch("vc_frame_avgpool_bwd");
}

}  // extern "C"
