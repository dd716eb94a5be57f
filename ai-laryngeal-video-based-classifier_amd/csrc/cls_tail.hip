// The last ViViT layer for the CLS rows only (VivitForVideoClassification.cls_only_last_layer):
// the logits read one row per clip, so in the last layer the patch tokens are needed as keys and
// values alone.  Two kernels replace the full-size attention / o_proj / LN2 / fc1 / fc2 launches:
//   cls_attn_kernel + cls_attn_combine_kernel   one query per (clip, head) over all S keys
//   skinny_gemm_kernel                          a handful of gathered rows against a packed weight
// Both are bandwidth-bound (K/V rows, weights), deterministic (fixed reduction orders, no atomics)
// and row / batch invariant: a row's result depends neither on M or B nor on its position.
#include "common.hpp"

namespace vc {

// ---------------------------------------------------------------------------------
// CLS-query attention, head_dim 64.  One workgroup per (key split, head, clip): VC_CLS_ATTN_SPLIT
// keys, 8 lanes per key row (16 B = 8 dims each, a 128-B row segment per lane group), so a
// workgroup pass covers 32 keys and a thread holds 8 keys' K and V segments in registers -- all
// 16 loads are issued before the first use.  q arrives scaled by scale*log2(e) (the q_prescaled
// convention of attn_fwd_d64_kernel).  The split knows all of its scores before the first
// exponential, so its max is exact; P, the row sum and o[64] stay fp32.  Keys past S are masked
// by index and their rows never read.  Partials (m, l, o[64]) go to part[(pair*nsplit + split)*66].
// ---------------------------------------------------------------------------------
constexpr int kClsSplit = VC_CLS_ATTN_SPLIT;  // keys per workgroup
constexpr int kClsPart = 66;                  // floats per partial: m, l, o[64]

template <int ET>
__global__ void __launch_bounds__(256) cls_attn_kernel(const uint16_t* __restrict__ qkv, int64_t ld, int S, int H,
                                                       int nsplit, float* __restrict__ part) {
    __shared__ float red[4];
    __shared__ float redl[4];
    __shared__ float redo[4][64];
    const int split = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = tid & 7;   // which 8 of the 64 dims
    const int kslot = tid >> 3;  // key within a 32-key pass
    const int64_t row0 = (int64_t)b * S;
    const int HD = H * 64;
    const uint16_t* qp = qkv + row0 * ld + h * 64 + sub * 8;
    const uint16_t* kbase = qkv + HD + h * 64 + sub * 8;
    const uint16_t* vbase = qkv + 2 * HD + h * 64 + sub * 8;
    const v8s q8 = *reinterpret_cast<const v8s*>(qp);
    constexpr int NP = kClsSplit / 32;
    v8s k8[NP], v8[NP];
    const int key0 = split * kClsSplit + kslot;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int key = key0 + i * 32;
        const int64_t r = row0 + (key < S ? key : S - 1);  // masked below; never a row outside the clip
        k8[i] = *reinterpret_cast<const v8s*>(kbase + r * ld);
        v8[i] = *reinterpret_cast<const v8s*>(vbase + r * ld);
    }
    float q[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) q[e] = from16<ET>((unsigned short)q8[e]);
    float s[NP];
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        float d = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) d = __builtin_fmaf(q[e], from16<ET>((unsigned short)k8[i][e]), d);
        d = group_sum<8>(d);
        s[i] = key0 + i * 32 < S ? d : -INFINITY;
        m = fmaxf(m, s[i]);
    }
    // the split's exact max: over the wave, then over the four waves
#pragma unroll
    for (int o = 32; o >= 8; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));  // finite: every split holds a key < S
    float l = 0.f;
    float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const float p = key0 + i * 32 < S ? __builtin_amdgcn_exp2f(s[i] - m) : 0.f;
        l += p;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = __builtin_fmaf(p, from16<ET>((unsigned short)v8[i][e]), o[e]);
    }
    // over the 8 key slots of a wave (lanes with equal `sub`), then over the waves in order
#pragma unroll
    for (int sh = 8; sh <= 32; sh <<= 1) {
        l += __shfl_xor(l, sh, 64);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] += __shfl_xor(o[e], sh, 64);
    }
    if (lane < 8) {
#pragma unroll
        for (int e = 0; e < 8; ++e) redo[wave][lane * 8 + e] = o[e];
        if (lane == 0) redl[wave] = l;
    }
    __syncthreads();
    if (tid < 64) {
        float* dst = part + ((int64_t)(b * H + h) * nsplit + split) * kClsPart;
        dst[2 + tid] = ((redo[0][tid] + redo[1][tid]) + redo[2][tid]) + redo[3][tid];
        if (tid == 0) {
            dst[0] = m;
            dst[1] = ((redl[0] + redl[1]) + redl[2]) + redl[3];
        }
    }
}

// One wave per (clip, head): the splits' partials rescaled to the common max and summed, divided by
// the row sum, rounded to the 16-bit type into row b*S of out.  Lane i takes the splits i, i + 64, ...
// for the max and the row sum (a butterfly over the wave: an order that depends on S alone), lane d
// sums o[d] over the splits in order, four loads in flight at a time.
template <int ET>
__global__ void __launch_bounds__(64) cls_attn_combine_kernel(const float* __restrict__ part, int S, int H, int nsplit,
                                                              uint16_t* __restrict__ out, int64_t ldo) {
    const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
    const float* p = part + (int64_t)(b * H + h) * nsplit * kClsPart;
    float m = -INFINITY;
    for (int i = d; i < nsplit; i += 64) m = fmaxf(m, p[i * kClsPart]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float l = 0.f;
    for (int i = d; i < nsplit; i += 64) l = __builtin_fmaf(__builtin_amdgcn_exp2f(p[i * kClsPart] - m), p[i * kClsPart + 1], l);
    l = wave_sum(l);
    float o = 0.f;
    for (int i0 = 0; i0 < nsplit; i0 += 4) {
        float mv[4], ov[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u < nsplit ? i0 + u : nsplit - 1;
            mv[u] = p[i * kClsPart];
            ov[u] = p[i * kClsPart + 2 + d];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i0 + u < nsplit) o = __builtin_fmaf(__builtin_amdgcn_exp2f(mv[u] - m), ov[u], o);
    }
    out[(int64_t)b * S * ldo + h * 64 + d] = to16<ET>(o / l);
}

// ---------------------------------------------------------------------------------
// Skinny GEMM: out[r] = epi(A[r] . W^T + bias) for a handful of rows at arbitrary row strides.
// grid (ceil(N / 4), ceil(M / 8)): each of a workgroup's four waves owns one output column and
// first issues every 16-B load of that weight row (K <= 4096: at most 8 per lane, all in flight
// together); meanwhile the workgroup stages its <= 8 input rows in LDS as 16-bit lanes --
// copied, or LayerNorm'ed from fp32 rows (the arithmetic, reduction order and rounding of
// layernorm_kernel; a wave takes rows w and w + 4 together, from registers up to K = 1024).
// Then fp32 FMA chains per lane against all 8 rows and a wave sum.  Weight-bandwidth-bound; a
// row's chain depends on K alone, not on M or on the row's slot.
// ---------------------------------------------------------------------------------
constexpr int kSkinnyRows = 8;
constexpr int kSkinnyFrags = VC_SKINNY_MAX_K / 512;  // 16-B weight loads per lane
constexpr int kLnRegV = 4;                           // float4 per lane and row the LN prologue keeps in registers

template <int ET, bool LN>
__global__ void __launch_bounds__(256) skinny_gemm_kernel(const void* __restrict__ a_, int64_t lda, const float* __restrict__ ln_g,
                                                          const float* __restrict__ ln_b, float eps,
                                                          const uint16_t* __restrict__ w, int64_t ldw, int M, int N, int K,
                                                          const float* __restrict__ bias, int epilogue, void* out_,
                                                          int64_t ldo) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint16_t* As = reinterpret_cast<uint16_t*>(smem);  // [8][K]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = blockIdx.y * kSkinnyRows;
    const int mc = M - r0 < kSkinnyRows ? M - r0 : kSkinnyRows;
    const int n = blockIdx.x * 4 + wave;
    v8s wreg[kSkinnyFrags];
    {
        const uint16_t* wr = w + (int64_t)(n < N ? n : N - 1) * ldw;
#pragma unroll
        for (int j = 0; j < kSkinnyFrags; ++j) {
            const int k = (j * 64 + lane) * 8;
            if (j * 512 < K) wreg[j] = *reinterpret_cast<const v8s*>(wr + (k < K ? k : 0));  // wave-uniform test
        }
    }
    if constexpr (LN) {
#pragma clang fp contract(off)
        const float* a = reinterpret_cast<const float*>(a_);
        const int K4 = K >> 2;
        const float4* g4 = reinterpret_cast<const float4*>(ln_g);
        const float4* b4 = reinterpret_cast<const float4*>(ln_b);
        if (K4 <= 64 * kLnRegV) {
            float4 v[2][kLnRegV], gg[kLnRegV], bb[kLnRegV];
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
                const int r = wave + 4 * rr;
                const float4* xr = reinterpret_cast<const float4*>(a + (int64_t)(r0 + (r < mc ? r : 0)) * lda);
#pragma unroll
                for (int i = 0; i < kLnRegV; ++i) v[rr][i] = xr[i * 64 + lane < K4 ? i * 64 + lane : 0];
            }
#pragma unroll
            for (int i = 0; i < kLnRegV; ++i) {
                gg[i] = g4[i * 64 + lane < K4 ? i * 64 + lane : 0];
                bb[i] = b4[i * 64 + lane < K4 ? i * 64 + lane : 0];
            }
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
                const int r = wave + 4 * rr;
                float s = 0.f;
#pragma unroll
                for (int i = 0; i < kLnRegV; ++i)
                    if (i * 64 + lane < K4) s += (v[rr][i].x + v[rr][i].y) + (v[rr][i].z + v[rr][i].w);
                const float mean = wave_sum(s) * (1.0f / K);
                float q = 0.f;
#pragma unroll
                for (int i = 0; i < kLnRegV; ++i)
                    if (i * 64 + lane < K4) {
                        const float x0 = v[rr][i].x - mean, x1 = v[rr][i].y - mean, x2 = v[rr][i].z - mean, x3 = v[rr][i].w - mean;
                        q += (x0 * x0 + x1 * x1) + (x2 * x2 + x3 * x3);
                    }
                const float rstd = rsqrtf(wave_sum(q) * (1.0f / K) + eps);
#pragma unroll
                for (int i = 0; i < kLnRegV; ++i)
                    if (i * 64 + lane < K4) {
                        uint2 o = make_uint2(0u, 0u);  // rows past M: zeros
                        if (r < mc) {
                            o.x = pack2<ET>((v[rr][i].x - mean) * rstd * gg[i].x + bb[i].x, (v[rr][i].y - mean) * rstd * gg[i].y + bb[i].y);
                            o.y = pack2<ET>((v[rr][i].z - mean) * rstd * gg[i].z + bb[i].z, (v[rr][i].w - mean) * rstd * gg[i].w + bb[i].w);
                        }
                        *reinterpret_cast<uint2*>(As + r * K + (i * 64 + lane) * 4) = o;
                    }
            }
        } else {
            for (int r = wave; r < kSkinnyRows; r += 4) {
                if (r >= mc) {
                    for (int i = lane; i < K4; i += 64) *reinterpret_cast<uint2*>(As + r * K + i * 4) = make_uint2(0u, 0u);
                    continue;
                }
                const float4* xr = reinterpret_cast<const float4*>(a + (int64_t)(r0 + r) * lda);
                float s = 0.f;
                for (int i = lane; i < K4; i += 64) {
                    const float4 x = xr[i];
                    s += (x.x + x.y) + (x.z + x.w);
                }
                const float mean = wave_sum(s) * (1.0f / K);
                float q = 0.f;
                for (int i = lane; i < K4; i += 64) {
                    const float4 x = xr[i];
                    const float x0 = x.x - mean, x1 = x.y - mean, x2 = x.z - mean, x3 = x.w - mean;
                    q += (x0 * x0 + x1 * x1) + (x2 * x2 + x3 * x3);
                }
                const float rstd = rsqrtf(wave_sum(q) * (1.0f / K) + eps);
                for (int i = lane; i < K4; i += 64) {
                    const float4 x = xr[i], gg = g4[i], bb = b4[i];
                    uint2 o;
                    o.x = pack2<ET>((x.x - mean) * rstd * gg.x + bb.x, (x.y - mean) * rstd * gg.y + bb.y);
                    o.y = pack2<ET>((x.z - mean) * rstd * gg.z + bb.z, (x.w - mean) * rstd * gg.w + bb.w);
                    *reinterpret_cast<uint2*>(As + r * K + i * 4) = o;
                }
            }
        }
    } else {
        const uint16_t* a = reinterpret_cast<const uint16_t*>(a_);
        const int K8 = K >> 3;
        for (int i = tid; i < kSkinnyRows * K8; i += 256) {
            const int r = i / K8, c = i - r * K8;
            v4u v = {0u, 0u, 0u, 0u};
            if (r < mc) v = *reinterpret_cast<const v4u*>(a + (int64_t)(r0 + r) * lda + c * 8);
            *reinterpret_cast<v4u*>(As + r * K + c * 8) = v;
        }
    }
    __syncthreads();
    if (n >= N) return;
    float acc[kSkinnyRows];
#pragma unroll
    for (int r = 0; r < kSkinnyRows; ++r) acc[r] = 0.f;
#pragma unroll
    for (int j = 0; j < kSkinnyFrags; ++j) {
        const int k = (j * 64 + lane) * 8;
        if (k < K) {
            float wf[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) wf[e] = from16<ET>((unsigned short)wreg[j][e]);
#pragma unroll
            for (int r = 0; r < kSkinnyRows; ++r) {
                const v8s a8 = *reinterpret_cast<const v8s*>(As + r * K + k);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[r] = __builtin_fmaf(from16<ET>((unsigned short)a8[e]), wf[e], acc[r]);
            }
        }
    }
    float mine = 0.f;  // lane r keeps row r's sum
#pragma unroll
    for (int r = 0; r < kSkinnyRows; ++r) {
        const float t = wave_sum(acc[r]);
        if (lane == r) mine = t;
    }
    if (lane < mc) {
        const float v = mine + bias[n];
        const int64_t o = (int64_t)(r0 + lane) * ldo + n;
        if (epilogue == VC_EPI_BIAS_RESID_F32) {
            float* out = reinterpret_cast<float*>(out_);
            out[o] += v;
        } else {
            uint16_t* out = reinterpret_cast<uint16_t*>(out_);
            out[o] = to16<ET>(epilogue == VC_EPI_BIAS_GELU_TANH ? gelu_tanh(v) : epilogue == VC_EPI_BIAS_GELU_ERF ? gelu_erf(v) : v);
        }
    }
}

template <int ET>
static int cls_attention(const uint16_t* qkv, int64_t ld, int64_t B, int64_t S, int64_t H, float* work, uint16_t* out,
                         int64_t ldo, hipStream_t stream) {
    const int nsplit = (int)((S + kClsSplit - 1) / kClsSplit);
    cls_attn_kernel<ET><<<dim3((unsigned)nsplit, (unsigned)H, (unsigned)B), 256, 0, stream>>>(qkv, ld, (int)S, (int)H, nsplit, work);
    int rc = check_launch("vc_cls_attention");
    if (rc) return rc;
    cls_attn_combine_kernel<ET><<<dim3((unsigned)H, (unsigned)B), 64, 0, stream>>>(work, (int)S, (int)H, nsplit, out, ldo);
    return check_launch("vc_cls_attention (combine)");
}

template <int ET>
static int skinny_gemm(const void* a, int64_t lda, const float* g, const float* b, float eps, const uint16_t* w, int64_t ldw,
                       int64_t M, int64_t N, int64_t K, const float* bias, int epilogue, void* out, int64_t ldo,
                       hipStream_t stream) {
    const dim3 grid((unsigned)((N + 3) / 4), (unsigned)((M + kSkinnyRows - 1) / kSkinnyRows));
    const size_t lds = (size_t)kSkinnyRows * K * 2;
    if (g)
        skinny_gemm_kernel<ET, true><<<grid, 256, lds, stream>>>(a, lda, g, b, eps, w, ldw, (int)M, (int)N, (int)K, bias, epilogue, out, ldo);
    else
        skinny_gemm_kernel<ET, false><<<grid, 256, lds, stream>>>(a, lda, g, b, eps, w, ldw, (int)M, (int)N, (int)K, bias, epilogue, out, ldo);
    return check_launch("vc_skinny_gemm");
}

}  // namespace vc

using namespace vc;

extern "C" {

int vc_cls_attention(const uint16_t* qkv, int64_t ld, int64_t B, int64_t S, int64_t H, int64_t head_dim, int elem,
                     float* work, int64_t work_elems, uint16_t* out, int64_t ldo, hipStream_t stream) {
    if (!qkv || !work || !out) return fail(VC_ERR_INVALID_ARG, "vc_cls_attention: null pointer");
    if (head_dim != 64) return fail(VC_ERR_UNSUPPORTED, "vc_cls_attention: head_dim must be 64");
    if (elem != VC_ELEM_BF16 && elem != VC_ELEM_F16) return fail(VC_ERR_INVALID_ARG, "vc_cls_attention: bad elem");
    if (B <= 0 || S <= 0 || H <= 0 || B > 65535 || H > 65535 || B * S >= (int64_t)1 << 31)
        return fail(VC_ERR_INVALID_ARG, "vc_cls_attention: bad B / S / H");
    if (ld < 3 * H * 64 || ld % 8 || ((uintptr_t)qkv & 15)) return fail(VC_ERR_INVALID_ARG, "vc_cls_attention: qkv needs ld >= 3*H*64, ld % 8 == 0 and 16-byte alignment");
    if (ldo < H * 64) return fail(VC_ERR_INVALID_ARG, "vc_cls_attention: ldo < H*64");
    const int64_t nsplit = (S + kClsSplit - 1) / kClsSplit;
    if (work_elems < B * H * nsplit * kClsPart) return fail(VC_ERR_INVALID_ARG, "vc_cls_attention: work buffer too small");
    if (elem == VC_ELEM_F16) return cls_attention<VC_ELEM_F16>(qkv, ld, B, S, H, work, out, ldo, stream);
    return cls_attention<VC_ELEM_BF16>(qkv, ld, B, S, H, work, out, ldo, stream);
}

int vc_skinny_gemm(const void* A, int64_t lda, const float* ln_gamma, const float* ln_beta, float ln_eps,
                   const uint16_t* W, int64_t ldw, int64_t M, int64_t N, int64_t K, const float* bias, int epilogue,
                   int elem, void* out, int64_t ldo, hipStream_t stream) {
    if (!A || !W || !bias || !out) return fail(VC_ERR_INVALID_ARG, "vc_skinny_gemm: null pointer");
    if ((ln_gamma == nullptr) != (ln_beta == nullptr)) return fail(VC_ERR_INVALID_ARG, "vc_skinny_gemm: gamma and beta go together");
    if (elem != VC_ELEM_BF16 && elem != VC_ELEM_F16) return fail(VC_ERR_INVALID_ARG, "vc_skinny_gemm: bad elem");
    if (epilogue != VC_EPI_BIAS_BF16 && epilogue != VC_EPI_BIAS_GELU_TANH && epilogue != VC_EPI_BIAS_GELU_ERF &&
        epilogue != VC_EPI_BIAS_RESID_F32)
        return fail(VC_ERR_UNSUPPORTED, "vc_skinny_gemm: epilogue must be bias, bias + gelu or bias + f32 residual");
    if (M <= 0 || N <= 0 || K <= 0 || M > 8 * 65535 || N >= (int64_t)1 << 31) return fail(VC_ERR_INVALID_ARG, "vc_skinny_gemm: bad M / N / K");
    if (K % 8 || K > VC_SKINNY_MAX_K) return fail(VC_ERR_UNSUPPORTED, "vc_skinny_gemm: K must be a multiple of 8, at most VC_SKINNY_MAX_K");
    if (ldw < K || ldw % 8 || ((uintptr_t)W & 15)) return fail(VC_ERR_INVALID_ARG, "vc_skinny_gemm: W needs ldw >= K, ldw % 8 == 0 and 16-byte alignment");
    if (ln_gamma) {
        if (lda % 4 || (((uintptr_t)A | (uintptr_t)ln_gamma | (uintptr_t)ln_beta) & 15))
            return fail(VC_ERR_INVALID_ARG, "vc_skinny_gemm: f32 A, gamma and beta need 16-byte alignment and lda % 4 == 0");
    } else if (lda % 8 || ((uintptr_t)A & 15))
        return fail(VC_ERR_INVALID_ARG, "vc_skinny_gemm: 16-bit A needs 16-byte alignment and lda % 8 == 0");
    if (elem == VC_ELEM_F16)
        return skinny_gemm<VC_ELEM_F16>(A, lda, ln_gamma, ln_beta, ln_eps, W, ldw, M, N, K, bias, epilogue, out, ldo, stream);
    return skinny_gemm<VC_ELEM_BF16>(A, lda, ln_gamma, ln_beta, ln_eps, W, ldw, M, N, K, bias, epilogue, out, ldo, stream);
}

}  // extern "C"
