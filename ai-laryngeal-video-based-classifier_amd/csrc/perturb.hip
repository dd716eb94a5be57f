// The device work of the saliency faithfulness test (vclip_amd/faithfulness.py): the deletion / insertion games of
// Petsiuk et al. 2018 (RISE) on a clip batch, for any family's saliency grid.
//
// vc_perturb_clips: all F perturbed copies of a clip batch in one pass over the input.  The clip is a flat run of
// n = B*T*C*H*W floats (either layout has H, W innermost); a lane takes four consecutive floats, finds each one's
// (clip, frame, row, column) and from them its cell
//     c = ((t*Tg/T)*Hg + y*Hg/H)*Wg + x*Wg/W        (integer division throughout)
// reads the four ranks rank[b][c] ONCE, and then writes the F copies: copy f keeps the clip where rank >= k[f] and
// takes the base (deletion), or the reverse (insertion).  A pure select: the output bits are the input's.  16-byte
// loads and stores when n % 4 == 0 and every pointer is 16-byte aligned (every slice f*n then is), one float per
// lane otherwise (W % 4 != 0 alone does not leave the vector path: a quad may straddle rows, every float finds its
// own cell).
//
// vc_gaussian_blur_planes: the insertion game's canvas, a separable Gaussian over H x W planes with replicated
// edges.  Two launches: rows (in -> work) and columns (work -> out), each staging its tile plus the halo in LDS with
// the edge clamp applied at the load, then y = x_c + sum_j w_j (x_j - x_c) around the centre pixel x_c, one fmaf per
// tap in tap order from 0: fp32, deterministic, and plane p's result does not depend on the number of planes.  The
// difference form equals sum_j w_j x_j up to (1 - sum w) x_c (the f32 taps sum to 1 within 4e-8) and keeps a constant
// plane exact, where the plain chain drifts by up to 3 ulp at 11 taps.  The taps exp(-d^2 / 2 sigma^2) / sum are
// computed on the host in double, rounded to f32 and passed by value.
#include <cmath>

#include "common.hpp"

namespace vc {
namespace perturb {

constexpr int KMAX = 31;  // taps
constexpr int RMAX = KMAX / 2;

struct Geom {
    unsigned T, C, H, W, Tg, Hg, Wg, N;  // N = Tg*Hg*Wg
    int layout;                          // 0: [B,T,C,H,W]  1: [B,C,T,H,W]
};

// offset of row r's (r = flat index / W) rank cells: b*N + ((t*Tg/T)*Hg + y*Hg/H)*Wg
__device__ __forceinline__ unsigned rank_row(const Geom& g, unsigned r) {
    const unsigned y = r % g.H;
    unsigned q = r / g.H, t, b;
    if (g.layout == 0) {
        q /= g.C;
        t = q % g.T;
        b = q / g.T;
    } else {
        t = q % g.T;
        b = q / g.T / g.C;
    }
    return b * g.N + ((t * g.Tg / g.T) * g.Hg + y * g.Hg / g.H) * g.Wg;
}

template <int V>
__global__ void __launch_bounds__(256) perturb_kernel(const float* __restrict__ clip, const float* __restrict__ base,
                                                      const int* __restrict__ rank, const int* __restrict__ k, Geom g,
                                                      unsigned n, int F, int insertion, float* __restrict__ out) {
    const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (i >= n) return;  // n % V == 0: a lane is all inside or all outside
    float x[V], z[V];
    int rk[V];
    if constexpr (V == 4) {
        const v4f a = *reinterpret_cast<const v4f*>(clip + i);
        x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
        if (base) {
            const v4f c = *reinterpret_cast<const v4f*>(base + i);
            z[0] = c.x; z[1] = c.y; z[2] = c.z; z[3] = c.w;
        } else {
            z[0] = z[1] = z[2] = z[3] = 0.0f;
        }
    } else {
        x[0] = clip[i];
        z[0] = base ? base[i] : 0.0f;
    }
    unsigned r = (unsigned)i / g.W, col = (unsigned)i - r * g.W;
    unsigned row = rank_row(g, r);
#pragma unroll
    for (int e = 0; e < V; ++e) {
        rk[e] = rank[row + col * g.Wg / g.W];
        if (++col == g.W && e + 1 < V) {  // the quad runs into the next row
            col = 0;
            row = rank_row(g, ++r);
        }
    }
    for (int f = 0; f < F; ++f) {
        const int kf = k[f];
        float* dst = out + (uint64_t)f * n + i;
        float y[V];
#pragma unroll
        for (int e = 0; e < V; ++e) y[e] = ((rk[e] < kf) != (insertion != 0)) ? z[e] : x[e];
        if constexpr (V == 4) {
            const v4f o = {y[0], y[1], y[2], y[3]};
            *reinterpret_cast<v4f*>(dst) = o;
        } else {
            dst[0] = y[0];
        }
    }
}

struct Taps {
    float w[KMAX];
};

// rows: one workgroup per (plane row, 256-column tile); LDS holds the tile and RMAX columns on either side
__global__ void __launch_bounds__(256) blur_rows_kernel(const float* __restrict__ in, int H, int W, int ksize, Taps taps,
                                                        float* __restrict__ out) {
    __shared__ float tile[256 + 2 * RMAX];
    const int R = ksize / 2;
    const int64_t row = blockIdx.x;  // plane*H + y
    const int x0 = blockIdx.y * 256;
    const float* src = in + row * W;
    for (int i = threadIdx.x; i < 256 + 2 * R; i += 256) {
        int x = x0 + i - R;
        x = x < 0 ? 0 : (x > W - 1 ? W - 1 : x);
        tile[i] = src[x];
    }
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= W) return;
    const float c = tile[threadIdx.x + R];
    float acc = 0.0f;
    for (int j = 0; j < ksize; ++j) acc = __builtin_fmaf(taps.w[j], tile[threadIdx.x + j] - c, acc);
    out[row * W + x] = c + acc;
}

// columns: one workgroup per (plane, 32-row tile, 64-column tile); LDS holds the tile and RMAX rows above and below;
// a lane owns one column and eight of the rows
__global__ void __launch_bounds__(256) blur_cols_kernel(const float* __restrict__ in, int H, int W, int ksize, Taps taps,
                                                        int tiles_y, float* __restrict__ out) {
    __shared__ float tile[(32 + 2 * RMAX) * 64];
    const int R = ksize / 2;
    const int64_t plane = blockIdx.x / tiles_y;
    const int y0 = (int)(blockIdx.x % tiles_y) * 32, x0 = blockIdx.y * 64;
    const float* src = in + plane * H * W;
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    const int x = x0 + lx < W ? x0 + lx : W - 1;  // lanes past the edge stage a copy of the last column, and store nothing
    for (int i = ly; i < 32 + 2 * R; i += 4) {
        int y = y0 + i - R;
        y = y < 0 ? 0 : (y > H - 1 ? H - 1 : y);
        tile[i * 64 + lx] = src[(int64_t)y * W + x];
    }
    __syncthreads();
    if (x0 + lx >= W) return;
    for (int i = ly * 8; i < ly * 8 + 8 && y0 + i < H; ++i) {
        const float c = tile[(i + R) * 64 + lx];
        float acc = 0.0f;
        for (int j = 0; j < ksize; ++j) acc = __builtin_fmaf(taps.w[j], tile[(i + j) * 64 + lx] - c, acc);
        out[plane * H * W + (int64_t)(y0 + i) * W + x] = c + acc;
    }
}

static bool overlap(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

}  // namespace perturb
}  // namespace vc

using namespace vc;
using namespace vc::perturb;

extern "C" int vc_perturb_clips(const float* clip, const float* base, const int32_t* rank, const int32_t* k, int64_t B,
                                int64_t C, int64_t T, int64_t H, int64_t W, int layout, int64_t Tg, int64_t Hg,
                                int64_t Wg, int64_t F, int mode, float* out, hipStream_t stream) {
    if (!clip || !rank || !k || !out) return fail(VC_ERR_INVALID_ARG, "vc_perturb_clips: null pointer");
    if (layout != 0 && layout != 1) return fail(VC_ERR_INVALID_ARG, "vc_perturb_clips: unknown layout (0: BTCHW, 1: BCTHW)");
    if (mode != 0 && mode != 1) return fail(VC_ERR_INVALID_ARG, "vc_perturb_clips: unknown mode (0: deletion, 1: insertion)");
    if (B <= 0 || C <= 0 || T <= 0 || H <= 0 || W <= 0 || F <= 0)
        return fail(VC_ERR_INVALID_ARG, "vc_perturb_clips: bad shape (B, C, T, H, W and F must be positive)");
    if (Tg <= 0 || Hg <= 0 || Wg <= 0 || Tg > T || Hg > H || Wg > W)
        return fail(VC_ERR_INVALID_ARG, "vc_perturb_clips: the saliency grid must be positive and no larger than the clip");
    const int64_t lim = 1LL << 31;
    if (B >= lim || C >= lim || T >= lim || H >= lim || W >= lim || F >= lim || B * C >= lim || B * C * T >= lim ||
        B * C * T * H >= lim || B * C * T * H * W >= lim)
        return fail(VC_ERR_INVALID_ARG, "vc_perturb_clips: a clip batch of 2^31 or more elements is not supported");
    if (T * Tg >= lim || H * Hg >= lim || W * Wg >= lim)  // the cell index is 32-bit arithmetic
        return fail(VC_ERR_INVALID_ARG, "vc_perturb_clips: clip extent times grid extent must stay below 2^31");
    const int64_t n = B * C * T * H * W, N = Tg * Hg * Wg;  // N <= T*H*W
    if ((((uintptr_t)clip) | ((uintptr_t)base) | ((uintptr_t)rank) | ((uintptr_t)k) | ((uintptr_t)out)) & 3)
        return fail(VC_ERR_INVALID_ARG, "vc_perturb_clips: pointers must be 4-byte aligned");
    if (overlap(out, F * n * 4, clip, n * 4) || (base && overlap(out, F * n * 4, base, n * 4)) ||
        overlap(out, F * n * 4, rank, B * N * 4) || overlap(out, F * n * 4, k, F * 4))
        return fail(VC_ERR_INVALID_ARG, "vc_perturb_clips: out must not alias clip, base, rank or k");
    const Geom g = {(unsigned)T, (unsigned)C, (unsigned)H, (unsigned)W, (unsigned)Tg, (unsigned)Hg, (unsigned)Wg,
                    (unsigned)N, layout};
    const bool vec = n % 4 == 0 && !((((uintptr_t)clip) | ((uintptr_t)base) | ((uintptr_t)out)) & 15);
    const int64_t lanes = vec ? n / 4 : n;
    const unsigned blocks = (unsigned)((lanes + 255) / 256);
    if (vec)
        perturb_kernel<4><<<blocks, 256, 0, stream>>>(clip, base, rank, k, g, (unsigned)n, (int)F, mode, out);
    else
        perturb_kernel<1><<<blocks, 256, 0, stream>>>(clip, base, rank, k, g, (unsigned)n, (int)F, mode, out);
    return check_launch("vc_perturb_clips");
}

extern "C" int vc_gaussian_blur_planes(const float* in, int64_t planes, int64_t H, int64_t W, int64_t ksize, float sigma,
                                       float* out, float* work, hipStream_t stream) {
    if (!in || !out || !work) return fail(VC_ERR_INVALID_ARG, "vc_gaussian_blur_planes: null pointer");
    if (planes <= 0 || H <= 0 || W <= 0) return fail(VC_ERR_INVALID_ARG, "vc_gaussian_blur_planes: bad shape");
    if (ksize < 1 || ksize > KMAX || ksize % 2 == 0)
        return fail(VC_ERR_INVALID_ARG, "vc_gaussian_blur_planes: ksize must be odd and at most 31");
    if (!(sigma > 0.0f) || !std::isfinite(sigma))
        return fail(VC_ERR_INVALID_ARG, "vc_gaussian_blur_planes: sigma must be positive and finite");
    const int64_t lim = 1LL << 31;
    const int64_t tiles_y = (H + 31) / 32;
    if (H >= lim || W >= lim || planes >= lim || planes * H >= (1LL << 23) || (W + 63) / 64 > 65535)
        return fail(VC_ERR_INVALID_ARG, "vc_gaussian_blur_planes: grid too large");
    if ((((uintptr_t)in) | ((uintptr_t)out) | ((uintptr_t)work)) & 3)
        return fail(VC_ERR_INVALID_ARG, "vc_gaussian_blur_planes: pointers must be 4-byte aligned");
    const int64_t bytes = planes * H * W * 4;
    if (overlap(out, bytes, in, bytes) || overlap(work, bytes, in, bytes) || overlap(work, bytes, out, bytes))
        return fail(VC_ERR_INVALID_ARG, "vc_gaussian_blur_planes: in, out and work must not alias one another");
    Taps taps;
    double w[KMAX], sum = 0.0;
    const double s = (double)sigma;
    const int R = (int)ksize / 2;
    for (int j = 0; j < ksize; ++j) {
        const double d = (double)(j - R);
        w[j] = std::exp(-(d * d) / (2.0 * s * s));
        sum += w[j];
    }
    for (int j = 0; j < KMAX; ++j) taps.w[j] = j < ksize ? (float)(w[j] / sum) : 0.0f;
    blur_rows_kernel<<<dim3((unsigned)(planes * H), (unsigned)((W + 255) / 256)), 256, 0, stream>>>(in, (int)H, (int)W,
                                                                                                     (int)ksize, taps, work);
    int rc = check_launch("vc_gaussian_blur_planes (rows)");
    if (rc) return rc;
    blur_cols_kernel<<<dim3((unsigned)(planes * tiles_y), (unsigned)((W + 63) / 64)), 256, 0, stream>>>(
        work, (int)H, (int)W, (int)ksize, taps, (int)tiles_y, out);
    return check_launch("vc_gaussian_blur_planes (columns)");
}
