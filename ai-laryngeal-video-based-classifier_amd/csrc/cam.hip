// ResNet3D-50 saliency (ResNet3d.explain): Grad-CAM (Selvaraju et al. 2017) and HiResCAM (Draelos & Carin
// 2020) on channels-last bf16 rows ((b*T + t)*H + h)*W + w with row stride ld >= C.  Four bandwidth-bound
// row kernels around the data-gradient GEMMs and vc_col2im_cl of the eval-mode chain:
//  * cam_seed_kernel     d logit[target_b] / d x of the head AvgPool3d(pool, stride 1) -> Linear -> global
//                        mean in closed form: cnt(t, h, w) / (npos * pt*ph*pw) * Wc[target_b][c];
//  * relu_bwd_kernel     out = (y == NULL or y > 0) ? d1 + d2 : 0 as bf16: the ReLU masks, the join of a block's
//                        skip and branch gradients (d2) and the cast for the next GEMM (d1 / d2 f32 or bf16);
//  * cam_weights         alpha[b][c] = mean over clip b's rows of g: fixed-order partial sums in a caller
//                        buffer, then summed in order (no atomics: bit-reproducible, clip b independent of B);
//  * cam_map_kernel      out[row] = sum_c w[c] x[row][c], w = alpha[b] ("gradcam") or g[row] ("hirescam"): one
//                        wave per row, 16-B loads, a wave64 butterfly sum; signed, no ReLU.
// Every kernel reads rows < B*T*H*W and columns < C only (C % 8 == 0): the forward's padded rows hold
// relu(bias) and a caller's padding columns anything.
#include "common.hpp"

namespace vc {
namespace cam {

__device__ __forceinline__ void unpack8(const uint4 u, float* v) {
    const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[2 * e] = bf2f((unsigned short)(w[e] & 0xffff));
        v[2 * e + 1] = bf2f((unsigned short)(w[e] >> 16));
    }
}

__device__ __forceinline__ uint4 pack8(const float* v) {
    uint4 o;
    o.x = pack2bf(v[0], v[1]);
    o.y = pack2bf(v[2], v[3]);
    o.z = pack2bf(v[4], v[5]);
    o.w = pack2bf(v[6], v[7]);
    return o;
}

// 8 consecutive values of a gradient operand, f32 (two 16-B loads) or bf16 (one)
__device__ __forceinline__ void load8(const void* p, int is_f32, int64_t off, float* v) {
    if (is_f32) {
        const float4 a = *reinterpret_cast<const float4*>((const float*)p + off);
        const float4 b = *reinterpret_cast<const float4*>((const float*)p + off + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
        unpack8(*reinterpret_cast<const uint4*>((const uint16_t*)p + off), v);
    }
}

// number of pool windows (size k, stride 1) along an axis of length L that cover index i
__device__ __forceinline__ int pool_cnt(int i, int L, int k) {
    const int hi = i < L - k ? i : L - k;
    const int lo = i - k + 1 > 0 ? i - k + 1 : 0;
    return hi - lo + 1;
}

// one thread per (row, 8-channel chunk)
__global__ void __launch_bounds__(256) cam_seed_kernel(const float* __restrict__ Wc, const int* __restrict__ target,
                                                       int nl, int64_t total, int T, int H, int W, int C8, int kt,
                                                       int kh, int kw, float inv, uint16_t* __restrict__ g, int64_t ldg) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c8 = (int)(i % C8);
    const int64_t row = i / C8;
    const int w = (int)(row % W);
    const int h = (int)((row / W) % H);
    const int t = (int)((row / ((int64_t)W * H)) % T);
    const int64_t b = row / ((int64_t)W * H * T);
    const int tg = target[b];
    float v[8];
    if (tg >= 0 && tg < nl) {  // a class outside the head's rows reads nothing (the wrapper's callers check it)
        const float s = (float)(pool_cnt(t, T, kt) * pool_cnt(h, H, kh) * pool_cnt(w, W, kw)) * inv;
        const float* wr = Wc + (int64_t)tg * (C8 * 8) + c8 * 8;
        const float4 a = *reinterpret_cast<const float4*>(wr);
        const float4 c = *reinterpret_cast<const float4*>(wr + 4);
        v[0] = s * a.x; v[1] = s * a.y; v[2] = s * a.z; v[3] = s * a.w;
        v[4] = s * c.x; v[5] = s * c.y; v[6] = s * c.z; v[7] = s * c.w;
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = 0.f;
    }
    *reinterpret_cast<uint4*>(g + row * ldg + c8 * 8) = pack8(v);
}

// one thread per (row, 8-channel chunk)
__global__ void __launch_bounds__(256) relu_bwd_kernel(const uint16_t* __restrict__ y, int64_t ldy, const void* __restrict__ d1,
                                                       int d1_f32, int64_t ldd1, const void* __restrict__ d2, int d2_f32,
                                                       int64_t ldd2, int64_t total, int C8, uint16_t* __restrict__ out,
                                                       int64_t ldo) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C8) * 8;
    const int64_t row = i / C8;
    float v[8];
    load8(d1, d1_f32, row * ldd1 + c, v);
    if (d2) {
        float u[8];
        load8(d2, d2_f32, row * ldd2 + c, u);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += u[e];
    }
    if (y) {
        float a[8];
        unpack8(*reinterpret_cast<const uint4*>(y + row * ldy + c), a);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = a[e] > 0.f ? v[e] : 0.f;
    }
    *reinterpret_cast<uint4*>(out + row * ldo + c) = pack8(v);
}

constexpr int CAM_CHUNKS = 32;

// stage 1: grid (B, C8 / 64, CAM_CHUNKS); a lane owns an 8-channel chunk (a wave reads 1 KB of one row), wave w of
// chunk z the rows z*4 + w, + 4*CAM_CHUNKS, ...; the four waves' sums are added in wave order through LDS
__global__ void __launch_bounds__(256) cam_weights_partial_kernel(const uint16_t* __restrict__ g, int64_t ldg, int N, int C8,
                                                                  float* __restrict__ part) {
    __shared__ float sm[4][64][9];  // (+1: the 8 floats of neighbouring lanes on different banks)
    const int b = blockIdx.x, z = blockIdx.z;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c8 = blockIdx.y * 64 + lane;
    float s[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = 0.f;
    if (c8 < C8) {
        for (int n = z * 4 + w; n < N; n += 4 * CAM_CHUNKS) {
            float v[8];
            unpack8(*reinterpret_cast<const uint4*>(g + ((int64_t)b * N + n) * ldg + c8 * 8), v);
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] += v[e];
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) sm[w][lane][e] = s[e];
    __syncthreads();
    if (w == 0 && c8 < C8) {
        float* dst = part + ((int64_t)b * CAM_CHUNKS + z) * (C8 * 8) + c8 * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) dst[e] = ((sm[0][lane][e] + sm[1][lane][e]) + sm[2][lane][e]) + sm[3][lane][e];
    }
}

// stage 2: the chunks in order, then the mean
__global__ void __launch_bounds__(256) cam_weights_reduce_kernel(const float* __restrict__ part, int C, float inv_n,
                                                                 float* __restrict__ alpha) {
    const int b = blockIdx.x;
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= C) return;
    float s = 0.f;
    for (int z = 0; z < CAM_CHUNKS; ++z) s += part[((int64_t)b * CAM_CHUNKS + z) * C + c];
    alpha[(int64_t)b * C + c] = s * inv_n;
}

// one wave per row (4 rows per workgroup): lane l the chunks l, l + 64, ...; HIRES: weights g[row], else alpha[b]
template <bool HIRES>
__global__ void __launch_bounds__(256) cam_map_kernel(const uint16_t* __restrict__ x, int64_t ldx, const uint16_t* __restrict__ g,
                                                      int64_t ldg, const float* __restrict__ alpha, int64_t rows, int N,
                                                      int C8, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;  // wave-uniform
    const float* al = alpha + (HIRES ? 0 : (row / N) * (int64_t)(C8 * 8));
    float s = 0.f;
    for (int c8 = lane; c8 < C8; c8 += 64) {
        float a[8], wv[8];
        unpack8(*reinterpret_cast<const uint4*>(x + row * ldx + c8 * 8), a);
        if (HIRES) unpack8(*reinterpret_cast<const uint4*>(g + row * ldg + c8 * 8), wv);
        else load8(al, 1, c8 * 8, wv);
#pragma unroll
        for (int e = 0; e < 8; ++e) s = __builtin_fmaf(wv[e], a[e], s);
    }
    s = wave_sum(s);
    if (lane == 0) out[row] = s;
}

static bool rows16(const void* p, int64_t ld) { return p && ld % 8 == 0 && ((uintptr_t)p & 15) == 0; }

}  // namespace cam
}  // namespace vc

using namespace vc;
using namespace vc::cam;

extern "C" {

int vc_cam_seed(const float* Wc, int64_t num_labels, const int* target, int64_t B, int64_t T, int64_t H, int64_t W,
                int64_t C, const int* pool_kernel, uint16_t* g, int64_t ldg, hipStream_t stream) {
    if (!Wc || !target || !pool_kernel || !g) return fail(VC_ERR_INVALID_ARG, "vc_cam_seed: null pointer");
    if (B <= 0 || T <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 || num_labels <= 0 || ldg < C || !rows16(g, ldg) ||
        ((uintptr_t)Wc & 15))
        return fail(VC_ERR_INVALID_ARG, "vc_cam_seed: need C % 8 == 0, ldg >= C, 16-B rows");
    const int kt = pool_kernel[0], kh = pool_kernel[1], kw = pool_kernel[2];
    if (kt <= 0 || kh <= 0 || kw <= 0 || kt > T || kh > H || kw > W)
        return fail(VC_ERR_INVALID_ARG, "vc_cam_seed: pool kernel larger than the feature map");
    const double npos = (double)(T - kt + 1) * (double)(H - kh + 1) * (double)(W - kw + 1);
    const float inv = (float)(1.0 / (npos * kt * kh * kw));
    const int64_t total = B * T * H * W * (C / 8);
    if (total > (int64_t)0x7fffffff * 256) return fail(VC_ERR_INVALID_ARG, "vc_cam_seed: grid too large");
    cam_seed_kernel<<<(unsigned)((total + 255) / 256), 256, 0, stream>>>(Wc, target, (int)num_labels, total, (int)T, (int)H,
                                                                         (int)W, (int)(C / 8), kt, kh, kw, inv, g, ldg);
    return check_launch("vc_cam_seed");
}

int vc_relu_bwd(const uint16_t* y, int64_t ldy, const void* d1, int d1_f32, int64_t ldd1, const void* d2, int d2_f32,
                int64_t ldd2, int64_t M, int64_t C, uint16_t* out, int64_t ldo, hipStream_t stream) {
    if (!d1 || !out) return fail(VC_ERR_INVALID_ARG, "vc_relu_bwd: null pointer");
    if (M <= 0 || C <= 0 || C % 8 || ldd1 < C || ldo < C || !rows16(d1, ldd1) || !rows16(out, ldo) ||
        (y && (ldy < C || !rows16(y, ldy))) || (d2 && (ldd2 < C || !rows16(d2, ldd2))))
        return fail(VC_ERR_INVALID_ARG, "vc_relu_bwd: need C % 8 == 0, row strides >= C and % 8 == 0, 16-B aligned rows");
    const int64_t total = M * (C / 8);
    if (total > (int64_t)0x7fffffff * 256) return fail(VC_ERR_INVALID_ARG, "vc_relu_bwd: grid too large");
    relu_bwd_kernel<<<(unsigned)((total + 255) / 256), 256, 0, stream>>>(y, ldy, d1, d1_f32 != 0, ldd1, d2, d2_f32 != 0, ldd2,
                                                                         total, (int)(C / 8), out, ldo);
    return check_launch("vc_relu_bwd");
}

int vc_cam_weights(const uint16_t* g, int64_t ldg, int64_t B, int64_t N, int64_t C, float* work, int64_t work_elems,
                   float* alpha, hipStream_t stream) {
    if (!g || !work || !alpha) return fail(VC_ERR_INVALID_ARG, "vc_cam_weights: null pointer");
    if (B <= 0 || B > 65535 || N <= 0 || N > 0x7fffffff || C <= 0 || C % 8 || ldg < C || !rows16(g, ldg))
        return fail(VC_ERR_INVALID_ARG, "vc_cam_weights: need C % 8 == 0, ldg >= C, 16-B rows, B <= 65535");
    if (work_elems < B * CAM_CHUNKS * C) return fail(VC_ERR_INVALID_ARG, "vc_cam_weights: work needs B * 32 * C floats");
    const int C8 = (int)(C / 8);
    cam_weights_partial_kernel<<<dim3((unsigned)B, (unsigned)((C8 + 63) / 64), CAM_CHUNKS), 256, 0, stream>>>(g, ldg, (int)N,
                                                                                                             C8, work);
    cam_weights_reduce_kernel<<<dim3((unsigned)B, (unsigned)((C + 255) / 256)), 256, 0, stream>>>(work, (int)C,
                                                                                                  (float)(1.0 / (double)N), alpha);
    return check_launch("vc_cam_weights");
}

int vc_cam_map(int mode, const uint16_t* x, int64_t ldx, const uint16_t* g, int64_t ldg, const float* alpha, int64_t B,
               int64_t N, int64_t C, float* out, hipStream_t stream) {
    if (!x || !out) return fail(VC_ERR_INVALID_ARG, "vc_cam_map: null pointer");
    if (mode != VC_CAM_GRADCAM && mode != VC_CAM_HIRESCAM) return fail(VC_ERR_INVALID_ARG, "vc_cam_map: bad mode");
    if (B <= 0 || N <= 0 || N > 0x7fffffff || C <= 0 || C % 8 || ldx < C || !rows16(x, ldx))
        return fail(VC_ERR_INVALID_ARG, "vc_cam_map: need C % 8 == 0, ldx >= C, 16-B rows");
    const int64_t rows = B * N;
    if (rows > (int64_t)0x7fffffff * 4) return fail(VC_ERR_INVALID_ARG, "vc_cam_map: grid too large");
    const unsigned nb = (unsigned)((rows + 3) / 4);
    if (mode == VC_CAM_HIRESCAM) {
        if (ldg < C || !rows16(g, ldg)) return fail(VC_ERR_INVALID_ARG, "vc_cam_map: hirescam needs g with ldg >= C, 16-B rows");
        cam_map_kernel<true><<<nb, 256, 0, stream>>>(x, ldx, g, ldg, nullptr, rows, (int)N, (int)(C / 8), out);
    } else {
        if (!alpha || ((uintptr_t)alpha & 15)) return fail(VC_ERR_INVALID_ARG, "vc_cam_map: gradcam needs alpha f32 [B][C]");
        cam_map_kernel<false><<<nb, 256, 0, stream>>>(x, ldx, nullptr, 0, alpha, rows, (int)N, (int)(C / 8), out);
    }
    return check_launch("vc_cam_map");
}

}  // extern "C"
