// Low-rank adaptation (LoRA, Hu et al. 2021) of the ViViT train step: W_eff = W + s B A with
// A [r][K], B [N][r] fp32 masters, 1 <= r <= 64.
//   vc_lora_merge : v = W + s B A in fp32 -> bf16 forward operand, bf16 transposed dgrad operand, fp32 copy
//   vc_lora_down  : U = X S^T, the r-wide product both adapter gradients start from (S = A or B^T), on MFMAs
//   vc_lora_wgrad : out = c G^T U over M rows, split over M, partials reduced in a fixed order
// What bounds them is the one read of X / G (M (K + N) 2 B per adapted weight); the arithmetic is M K r
// FMAs, a few hundred MFLOP at ViViT-B.  No atomics: every sum has one fixed order.
#include "common.hpp"

namespace vc {
namespace lora {

constexpr int MAX_RANK = 64;

// ---------------------------------------------------------------------------------
// merge: 64 x 64 tiles of rows [row0, row0 + rows) of W [.., K]; the A columns and B rows of the
// tile in LDS; the bf16 stores and the transposed write exactly as pack_weight_kernel's
// (rows < nscaled times `scale` in the bf16 outputs only), so B = 0 gives its bits.
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) merge_kernel(const float* __restrict__ W, int64_t ldw, int64_t row0, int64_t rows,
                                                    int64_t K, const float* __restrict__ A, const float* __restrict__ Bm,
                                                    int r, float s, int64_t nscaled, float scale,
                                                    uint16_t* __restrict__ dst, int64_t ldd, uint16_t* __restrict__ dstT,
                                                    int64_t ldt, float* __restrict__ out, int64_t ldo) {
    __shared__ __align__(16) float As[MAX_RANK][64];
    __shared__ float Bs[64][MAX_RANK + 1];
    __shared__ float tile[64][65];
    const int64_t n0 = (int64_t)blockIdx.y * 64, k0 = (int64_t)blockIdx.x * 64;  // n0: row within the range
    const int t = threadIdx.x, rr0 = t >> 4, c4 = (t & 15) * 4;
    for (int idx = t; idx < r * 64; idx += 256) {
        const int j = idx >> 6, kk = idx & 63;
        As[j][kk] = (k0 + kk < K) ? A[(int64_t)j * K + k0 + kk] : 0.f;
    }
    for (int idx = t; idx < r * 64; idx += 256) {
        const int rr = idx / r, j = idx - rr * r;
        Bs[rr][j] = (n0 + rr < rows) ? Bm[(n0 + rr) * r + j] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int rr = rr0 + p * 16;
        const int64_t nl = n0 + rr, n = row0 + nl, k = k0 + c4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (nl < rows && k < K) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int j = 0; j < r; ++j) {  // j ascending: the one order every output shares
                const float b = Bs[rr][j];
                const float4 a = *reinterpret_cast<const float4*>(&As[j][c4]);
                acc.x = __builtin_fmaf(b, a.x, acc.x);
                acc.y = __builtin_fmaf(b, a.y, acc.y);
                acc.z = __builtin_fmaf(b, a.z, acc.z);
                acc.w = __builtin_fmaf(b, a.w, acc.w);
            }
            const float4 w = *reinterpret_cast<const float4*>(W + n * ldw + k);
            v = make_float4(__builtin_fmaf(s, acc.x, w.x), __builtin_fmaf(s, acc.y, w.y), __builtin_fmaf(s, acc.z, w.z),
                            __builtin_fmaf(s, acc.w, w.w));
            if (out) *reinterpret_cast<float4*>(out + n * ldo + k) = v;
            if (n < nscaled) { v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale; }
            if (dst) *reinterpret_cast<uint2*>(dst + n * ldd + k) = make_uint2(pack2bf(v.x, v.y), pack2bf(v.z, v.w));
        }
        tile[rr][c4 + 0] = v.x;
        tile[rr][c4 + 1] = v.y;
        tile[rr][c4 + 2] = v.z;
        tile[rr][c4 + 3] = v.w;
    }
    if (!dstT) return;
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int kr = rr0 + p * 16;  // k within the tile; c4: 4 consecutive n (host: row0, rows % 4 == 0)
        const int64_t k = k0 + kr, nl = n0 + c4;
        if (nl < rows && k < K)
            *reinterpret_cast<uint2*>(dstT + k * ldt + row0 + nl) =
                make_uint2(pack2bf(tile[c4][kr], tile[c4 + 1][kr]), pack2bf(tile[c4 + 2][kr], tile[c4 + 3][kr]));
    }
}

// ---------------------------------------------------------------------------------
// down: U[m][j] = bf16(sum_k X[m][k] bf16(S[j][k])) on the 16x16x32 bf16 MFMA.  S is f32 with element (j, k) at
// S[j sj + k sk]: A [r][K] with sj = K, sk = 1, or B [K][r] read transposed with sj = 1, sk = r; rows j >= r of
// the 16-row tiles are zero.  A workgroup owns 16 rows of X; its four waves take the 32-wide k steps round
// robin, each lane loading its MFMA fragments straight from global memory (X: row l & 15, 8 bf16 at
// 8 (l >> 4); S: 8 floats of row j, rounded to bf16 in registers; S is a few tens of KB and stays in cache): no
// LDS staging, and the four partial tiles are summed in wave order through LDS.
// ---------------------------------------------------------------------------------
template <int NT>  // NT = (r rounded up to 16) / 16 column tiles of U
__global__ void __launch_bounds__(256) down_kernel(const uint16_t* __restrict__ X, int64_t ldx, int64_t M, int64_t K,
                                                   const float* __restrict__ S, int64_t sj, int64_t sk, int r,
                                                   uint16_t* __restrict__ U) {
    __shared__ float red[4][NT][4][64];
    const int t = threadIdx.x, l = t & 63, w = t >> 6, row = l & 15, kq = l >> 4;
    const int64_t m0 = (int64_t)blockIdx.x * 16, m = m0 + row;
    const bool valid = m < M;
    const uint16_t* xp = X + (valid ? m : 0) * ldx + 8 * kq;
    v4f acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i] = v4f{0.f, 0.f, 0.f, 0.f};
    for (int64_t k0 = (int64_t)w * 32; k0 < K; k0 += 128) {  // host: K % 32 == 0
        uint4 a = make_uint4(0u, 0u, 0u, 0u);
        if (valid) a = *reinterpret_cast<const uint4*>(xp + k0);
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int j = 16 * i + row;
            uint4 b = make_uint4(0u, 0u, 0u, 0u);
            if (j < r) {
                const float* p = S + (int64_t)j * sj + (k0 + 8 * kq) * sk;
                if (sk == 1) {  // host: 16-byte aligned
                    const float4 lo = *reinterpret_cast<const float4*>(p), hi = *reinterpret_cast<const float4*>(p + 4);
                    b = make_uint4(pack2bf(lo.x, lo.y), pack2bf(lo.z, lo.w), pack2bf(hi.x, hi.y), pack2bf(hi.z, hi.w));
                } else {
                    b = make_uint4(pack2bf(p[0], p[sk]), pack2bf(p[2 * sk], p[3 * sk]), pack2bf(p[4 * sk], p[5 * sk]),
                                   pack2bf(p[6 * sk], p[7 * sk]));
                }
            }
            acc[i] = mfma16x32<VC_ELEM_BF16>(__builtin_bit_cast(v8s, a), __builtin_bit_cast(v8s, b), acc[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) red[w][i][e][l] = acc[i][e];
    __syncthreads();
    // thread t: tile i = t >> 6 (when < NT), lane l: D[4 (l >> 4) + e][l & 15], the waves' partials in wave order
    for (int i = w; i < NT; i += 4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float v = ((red[0][i][e][l] + red[1][i][e][l]) + red[2][i][e][l]) + red[3][i][e][l];
            const int64_t mr = m0 + 4 * kq + e;
            const int j = 16 * i + row;
            if (mr < M && j < r) U[mr * r + j] = f2bf(v);
        }
    }
}

// ---------------------------------------------------------------------------------
// wgrad: P[z][j][n] = sum over the rows m of split z of G[m][n] U[m][j].  G bf16 [M][ldg] (N columns), U bf16
// [M][r].  A workgroup owns 128 columns (two per lane) and one split of the rows, 64 rows at a time: their U
// rows in LDS as f32 (every lane reads the same value: a broadcast), wave w the rows 16 w .. 16 w + 15 of the
// 64 with all RP accumulators per column, its 16 loads of G in flight together.  The four waves' sums are
// added in wave order through LDS.  Plain fp32 FMAs: the product is M N r FMAs, far below the VALU rate.
// ---------------------------------------------------------------------------------
constexpr int WG_TN = 128, WG_ROWS = 64;

template <int RP>  // r rounded up to 8, 16, 32 or 64
__global__ void __launch_bounds__(256) wgrad_kernel(const uint16_t* __restrict__ G, int64_t ldg,
                                                    const uint16_t* __restrict__ U, int64_t M, int64_t N, int r,
                                                    int64_t chunk, float* __restrict__ P) {
    __shared__ __align__(16) float Us[WG_ROWS][RP];
    __shared__ float red[2 * RP][64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t n = (int64_t)blockIdx.x * WG_TN + 2 * lane;
    const int64_t z = blockIdx.y, mbeg = z * chunk, mend = (mbeg + chunk < M) ? mbeg + chunk : M;
    const bool col = n < N;  // host: N % 2 == 0, so the pair is whole or absent
    float a0[RP], a1[RP];
#pragma unroll
    for (int j = 0; j < RP; ++j) a0[j] = a1[j] = 0.f;
    for (int64_t m0 = mbeg; m0 < mend; m0 += WG_ROWS) {
        __syncthreads();
        for (int idx = t; idx < WG_ROWS * RP; idx += 256) {
            const int mm = idx / RP, j = idx - mm * RP;
            Us[mm][j] = (j < r && m0 + mm < mend) ? bf2f(U[(m0 + mm) * r + j]) : 0.f;
        }
        __syncthreads();
        unsigned int g[16];
#pragma unroll
        for (int mm = 0; mm < 16; ++mm) {
            const int64_t m = m0 + w * 16 + mm;
            g[mm] = (col && m < mend) ? *reinterpret_cast<const unsigned int*>(G + m * ldg + n) : 0u;
        }
#pragma unroll
        for (int mm = 0; mm < 16; ++mm) {
            const float g0 = bf2f((unsigned short)(g[mm] & 0xffffu)), g1 = bf2f((unsigned short)(g[mm] >> 16));
#pragma unroll
            for (int j = 0; j < RP; j += 4) {
                const float4 u = *reinterpret_cast<const float4*>(&Us[w * 16 + mm][j]);
                a0[j] = __builtin_fmaf(g0, u.x, a0[j]);         a1[j] = __builtin_fmaf(g1, u.x, a1[j]);
                a0[j + 1] = __builtin_fmaf(g0, u.y, a0[j + 1]); a1[j + 1] = __builtin_fmaf(g1, u.y, a1[j + 1]);
                a0[j + 2] = __builtin_fmaf(g0, u.z, a0[j + 2]); a1[j + 2] = __builtin_fmaf(g1, u.z, a1[j + 2]);
                a0[j + 3] = __builtin_fmaf(g0, u.w, a0[j + 3]); a1[j + 3] = __builtin_fmaf(g1, u.w, a1[j + 3]);
            }
        }
    }
    // ((wave 0 + wave 1) + wave 2) + wave 3, one wave at a time through LDS
    for (int ww = 0; ww < 4; ++ww) {
        if (w == ww) {
#pragma unroll
            for (int j = 0; j < RP; ++j) {
                if (ww == 0) {
                    red[2 * j][lane] = a0[j];
                    red[2 * j + 1][lane] = a1[j];
                } else if (ww < 3) {
                    red[2 * j][lane] += a0[j];
                    red[2 * j + 1][lane] += a1[j];
                } else if (col && j < r) {
                    *reinterpret_cast<float2*>(P + (z * r + j) * N + n) =
                        make_float2(red[2 * j][lane] + a0[j], red[2 * j + 1][lane] + a1[j]);
                }
            }
        }
        __syncthreads();
    }
}

// out = c * sum_z P[z] over P [splits][r][N]; out [r][N] when transposed, else [N][r].  A workgroup owns 64
// outputs; its four waves sum the splits z = w, w + 4, .. in order and the four sums are added in wave order.
__global__ void __launch_bounds__(256) wgrad_reduce_kernel(const float* __restrict__ P, int64_t N, int r, int splits,
                                                           float c, int transposed, float* __restrict__ out) {
    __shared__ float red[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * 64 + lane, total = N * r;
    float s = 0.f;
    if (i < total) {
#pragma unroll 4
        for (int z = w; z < splits; z += 4) s += P[(int64_t)z * total + i];
    }
    red[w][lane] = s;
    __syncthreads();
    if (w != 0 || i >= total) return;
    const float v = c * (((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]);
    const int64_t j = i / N, nn = i - j * N;
    out[transposed ? i : nn * r + j] = v;
}

// rows per split and the split count: ~512 workgroups, at least 64 rows each, within the scratch
static void plan_splits(int64_t M, int64_t N, int r, int64_t work_elems, int64_t* chunk, int64_t* splits) {
    const int64_t tiles = (N + WG_TN - 1) / WG_TN;
    int64_t sp = (512 + tiles - 1) / tiles;
    const int64_t cap_rows = (M + 63) / 64, cap_work = work_elems / (N * r);
    if (sp > cap_rows) sp = cap_rows;
    if (sp > cap_work) sp = cap_work;
    if (sp < 1) sp = 1;
    int64_t ch = (M + sp - 1) / sp;
    ch = (ch + WG_ROWS - 1) / WG_ROWS * WG_ROWS;
    *chunk = ch;
    *splits = (M + ch - 1) / ch;
}

}  // namespace lora
}  // namespace vc

using namespace vc;
using namespace vc::lora;

extern "C" {

int vc_lora_merge(const float* W, int64_t ldw, int64_t row0, int64_t rows, int64_t K, const float* A, const float* B,
                  int64_t r, float s, int64_t nscaled, float scale, uint16_t* dst, int64_t ldd, uint16_t* dstT,
                  int64_t ldt, float* out, int64_t ldo, hipStream_t stream) {
    if (!W || !A || !B || (!dst && !dstT && !out)) return fail(VC_ERR_INVALID_ARG, "vc_lora_merge: null pointer");
    if (r < 1 || r > MAX_RANK) return fail(VC_ERR_INVALID_ARG, "vc_lora_merge: rank must be 1..64");
    if (rows <= 0 || K <= 0 || row0 < 0 || rows % 4 || row0 % 4 || K % 4 || ldw < K || ldw % 4)
        return fail(VC_ERR_INVALID_ARG, "vc_lora_merge: need row0, rows, K, ldw % 4 == 0 and ldw >= K");
    if ((dst && (ldd < K || ldd % 4)) || (dstT && (ldt < row0 + rows || ldt % 4)) || (out && (ldo < K || ldo % 4)))
        return fail(VC_ERR_INVALID_ARG, "vc_lora_merge: output leading dimension");
    if ((((uintptr_t)W) & 15) || (((uintptr_t)out) & 15) || (((uintptr_t)dst) & 7) || (((uintptr_t)dstT) & 7))
        return fail(VC_ERR_INVALID_ARG, "vc_lora_merge: W / out 16-B, dst / dstT 8-B alignment");
    dim3 grid((unsigned)((K + 63) / 64), (unsigned)((rows + 63) / 64));
    merge_kernel<<<grid, 256, 0, stream>>>(W, ldw, row0, rows, K, A, B, (int)r, s, nscaled, scale, dst, ldd, dstT, ldt,
                                           out, ldo);
    return check_launch("vc_lora_merge");
}

int vc_lora_down(const uint16_t* X, int64_t ldx, int64_t M, int64_t K, const float* S, int64_t sj, int64_t sk,
                 int64_t r, uint16_t* U, hipStream_t stream) {
    if (!X || !S || !U) return fail(VC_ERR_INVALID_ARG, "vc_lora_down: null pointer");
    if (r < 1 || r > MAX_RANK) return fail(VC_ERR_INVALID_ARG, "vc_lora_down: rank must be 1..64");
    if (M <= 0 || K <= 0 || K % 32 || ldx < K || ldx % 8 || (((uintptr_t)X) & 15))
        return fail(VC_ERR_INVALID_ARG, "vc_lora_down: need K % 32 == 0, ldx % 8 == 0, ldx >= K, X 16-B aligned");
    if (!((sj == K && sk == 1) || (sj == 1 && sk == r)))
        return fail(VC_ERR_INVALID_ARG, "vc_lora_down: S is [r][K] (sj = K, sk = 1) or [K][r] read transposed (sj = 1, sk = r)");
    if (sk == 1 && (((uintptr_t)S) & 15)) return fail(VC_ERR_INVALID_ARG, "vc_lora_down: S [r][K] must be 16-B aligned");
    const unsigned grid = (unsigned)((M + 15) / 16);
    if (r <= 16) down_kernel<1><<<grid, 256, 0, stream>>>(X, ldx, M, K, S, sj, sk, (int)r, U);
    else if (r <= 32) down_kernel<2><<<grid, 256, 0, stream>>>(X, ldx, M, K, S, sj, sk, (int)r, U);
    else if (r <= 48) down_kernel<3><<<grid, 256, 0, stream>>>(X, ldx, M, K, S, sj, sk, (int)r, U);
    else down_kernel<4><<<grid, 256, 0, stream>>>(X, ldx, M, K, S, sj, sk, (int)r, U);
    return check_launch("vc_lora_down");
}

int vc_lora_wgrad(const uint16_t* G, int64_t ldg, const uint16_t* U, int64_t M, int64_t N, int64_t r, float c,
                  int transposed, float* out, float* work, int64_t work_elems, hipStream_t stream) {
    if (!G || !U || !out || !work) return fail(VC_ERR_INVALID_ARG, "vc_lora_wgrad: null pointer");
    if (r < 1 || r > MAX_RANK) return fail(VC_ERR_INVALID_ARG, "vc_lora_wgrad: rank must be 1..64");
    if (M <= 0 || N <= 0 || N % 2 || ldg < N || ldg % 2 || (((uintptr_t)G) & 3))
        return fail(VC_ERR_INVALID_ARG, "vc_lora_wgrad: need N, ldg % 2 == 0, ldg >= N, G 4-B aligned");
    if (work_elems < N * r) return fail(VC_ERR_INVALID_ARG, "vc_lora_wgrad: work holds less than one [N][r] partial");
    int64_t chunk, splits;
    plan_splits(M, N, (int)r, work_elems, &chunk, &splits);
    dim3 grid((unsigned)((N + WG_TN - 1) / WG_TN), (unsigned)splits);
    if (r <= 8) wgrad_kernel<8><<<grid, 256, 0, stream>>>(G, ldg, U, M, N, (int)r, chunk, work);
    else if (r <= 16) wgrad_kernel<16><<<grid, 256, 0, stream>>>(G, ldg, U, M, N, (int)r, chunk, work);
    else if (r <= 32) wgrad_kernel<32><<<grid, 256, 0, stream>>>(G, ldg, U, M, N, (int)r, chunk, work);
    else wgrad_kernel<64><<<grid, 256, 0, stream>>>(G, ldg, U, M, N, (int)r, chunk, work);
    int rc = check_launch("vc_lora_wgrad");
    if (rc) return rc;
    const int64_t total = N * r;
    wgrad_reduce_kernel<<<(unsigned)((total + 63) / 64), 256, 0, stream>>>(work, N, (int)r, (int)splits, c, transposed,
                                                                          out);
    return check_launch("vc_lora_wgrad (reduce)");
}

}  // extern "C"
