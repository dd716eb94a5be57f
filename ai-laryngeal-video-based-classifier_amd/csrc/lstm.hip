// ResNet50-LSTM (resnet50-2d-lstm/src/models/model.py:5-60, trainer.py:156-170), the part behind the
// ResNet-50 backbone: the per-frame global average pool, the LSTM recurrence forward and backward
// (the input projections of all T steps run outside as MFMA GEMMs, the weight gradients as the
// split-K wgrad GEMMs) and the Linear -> ReLU -> Dropout -> Linear head, forward and backward.
//
// There are two recurrence kernels, one forward and one backward.  The forward one is a template over
// <G, RAGGED, STATE, TRAIN>: dense inference, dense train (gates != nullptr), the ragged inference over
// sequences of different lengths, the stateful inference ((h0, c0) in, (h_n, c_n) out) and the stateful
// train variant are instantiations of one step loop, so a sequence comes out bit-identical whichever
// entry ran it.  The backward one is a template over <G, STATE>: BPTT from the zero state over dense rows,
// and BPTT over dense or ragged rows with c0 in and (dh0, dc0) out, again one step loop.  Both kernels
// share one schedule, whose launch geometry the host keeps in SeqLaunch.  A workgroup owns G whole sequences
// (G = 4 for hidden <= 512, else 2) from the first step to the last, so there is no cross-workgroup barrier.
// HP = hidden rounded up to 64; the block has S * HP threads, S = 1024 / HP.  Thread (s, j) owns
// hidden unit j and slice s of the reduction (forward: the k range of h_{t-1}; backward: the row
// range of the 4H gate gradients).  Lanes run over j, so every W_hh read is a contiguous row piece:
// forward reads the transposed image [H][4H], backward the natural [4H][H].  Slices s > 0 hand their
// partial sums to slice 0 through LDS, which adds them in slice order (fixed order: deterministic)
// and does the pointwise cell arithmetic with c / dc / dh in registers.  All arithmetic is fp32;
// the two sequences of a pair share one packed FMA.
#include "common.hpp"

namespace vc {
namespace lstm {

constexpr int kMaxThreads = 1024;

__host__ __device__ inline int group_of(int64_t hidden) { return hidden <= 512 ? 4 : 2; }

__device__ __forceinline__ float sigmoidf_(float v) { return 1.0f / (1.0f + __expf(-v)); }
// tanh(v) = 1 - 2 / (exp(2v) + 1): ABSOLUTE error ~1e-7 (exp -> inf / 0 gives the +-1 limits exactly), a
// fraction of libm tanhf's registers in the unrolled cell arithmetic.  The difference cancels for small |v|
// (relative error ~1e-3 at |v| ~ 1e-4): fine for the cell, whose bounds are absolute; do not reuse it
// where relative accuracy near zero matters.
__device__ __forceinline__ float tanhf_(float v) { return 1.0f - 2.0f / (__expf(2.0f * v) + 1.0f); }

// features[n][c] = mean_p x[n*P + p][c] (channels-last bf16 or fp16 in, fp32 sum, bf16 out for the next GEMM)
template <int ET>
__global__ void __launch_bounds__(256) frame_avgpool_kernel(const uint16_t* __restrict__ x, int64_t ldx, int P, int C,
                                                            uint16_t* __restrict__ out, int64_t ldo) {
    const int64_t n = blockIdx.x;
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= C) return;
    const uint16_t* xp = x + n * P * ldx + c;
    float s = 0.f;
    for (int p = 0; p < P; ++p) s += from16<ET>(xp[(int64_t)p * ldx]);
    out[n * ldo + c] = f2bf(s / (float)P);
}

// ---- the frozen backbone's train-mode forward with fp16 activations (resnet50_lstm.py) ----
// z = gamma (y - mean) rstd + beta (+ res), ReLU optional: vc_batchnorm_train_fwd's apply pass with fp16
// rows out (and an fp16 residual in); stat = [mean | rstd] as that entry leaves it.  C % 4 == 0.
__global__ void __launch_bounds__(256) bn_apply_h16_kernel(const float* __restrict__ y, int64_t ldy, int64_t M, int C,
                                                           const float* __restrict__ stat, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const uint16_t* __restrict__ res,
                                                           int64_t ldr, int relu, uint16_t* __restrict__ z, int64_t ldz) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int C4 = C >> 2;
    if (i >= M * C4) return;
    const int64_t r = i / C4;
    const int c = (int)(i - r * C4) * 4;
    const float4 v = *reinterpret_cast<const float4*>(y + r * ldy + c);
    float o[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        o[e] = gamma[c + e] * (o[e] - stat[c + e]) * stat[C + c + e] + beta[c + e];
        if (res) o[e] += from16<VC_ELEM_F16>(res[r * ldr + c + e]);
        if (relu) o[e] = fmaxf(o[e], 0.f);
    }
    uint2 p;
    p.x = pack2<VC_ELEM_F16>(o[0], o[1]);
    p.y = pack2<VC_ELEM_F16>(o[2], o[3]);
    *reinterpret_cast<uint2*>(z + r * ldz + c) = p;
}

// f32 clip [B][C][P] (P = T*H*W) -> channels-last fp16 rows [B*P][8], channels >= C zero (C <= 8)
__global__ void __launch_bounds__(256) video_to_cl_h16_kernel(const float* __restrict__ x, int64_t B, int C, int64_t P,
                                                              uint16_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B * P) return;
    const int64_t b = i / P, p = i - b * P;
    float v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = c < C ? x[(b * C + c) * P + p] : 0.f;
    uint4 o;
    o.x = pack2<VC_ELEM_F16>(v[0], v[1]);
    o.y = pack2<VC_ELEM_F16>(v[2], v[3]);
    o.z = pack2<VC_ELEM_F16>(v[4], v[5]);
    o.w = pack2<VC_ELEM_F16>(v[6], v[7]);
    *reinterpret_cast<uint4*>(out + i * 8) = o;
}

// One launch = all T steps of one layer.  pre[b*T + t][4H] = x_t W_ih^T + b_ih + b_hh (gate order
// i, f, g, o); WT = W_hh^T [H][4H].  Sequence b0 + g of the group owns rows r0[g] .. r0[g] + ln[g] - 1
// of pre and hseq; hlast[b] = h of its last step.
// Dense (RAGGED = false): r0 = b * T and ln = T in registers, row0 / len are not read.  Train outputs
// (gates != nullptr): post-activation gates, c, and bf16 h_{t-1} (zero at t = 0).  keep (optional,
// [B*T][H]) scales the stored h_seq only.
// Ragged (RAGGED = true, inference only): r0 = row0[b], ln = len[b] clamped to [0, T = max_len]; keep,
// gates, cseq and hprev are not touched.  The workgroup loops to the largest length of its group
// (uniform: the barriers stay legal); a sequence past its end keeps its h in LDS untouched, reads no
// row of pre and writes nothing; hlast[b] = 0 for len[b] = 0.  The step loop is the dense one and
// the lanes of a packed FMA are independent, so every sequence comes out bit-identical to a dense
// launch on it alone.
// Stateful (STATE = true, with RAGGED = true; inference only): row0 == nullptr selects the dense rows.
// h_{-1} = h0[b], c_{-1} = c0[b] (both nullptr: zero, and step 0 skips the W_hh product as above);
// hfin[b] / cfin[b] = h / c after the last step, the incoming state for len[b] = 0; hall (optional) = the
// unrounded h of every step.  hfin may alias h0 and cfin c0: the workgroup owns its sequences and has h0
// in LDS and c0 in registers before its first store, so these four carry no __restrict__.  hlast is
// not touched.  STATE = false compiles all of it out.
// Stateful train (TRAIN = true, with STATE = true): gates, cseq and hprev are written as in the dense train
// variant and keep scales the stored h_seq, all indexed by the sequence's own rows; hprev of a first step
// is bf16(h0[b]) (zero without a state), the operand of the W_hh gradient.  hall is not used.
template <int G, bool RAGGED, bool STATE = false, bool TRAIN = false>
__global__ void __launch_bounds__(kMaxThreads)
lstm_seq_fwd_kernel(const float* __restrict__ pre, int64_t ldpre, int B, int T, int H, const float* __restrict__ WT,
                    const int32_t* __restrict__ row0, const int32_t* __restrict__ len, const float* __restrict__ keep,
                    uint16_t* __restrict__ hseq, int64_t ldh, float* __restrict__ hlast, float* __restrict__ gates,
                    float* __restrict__ cseq, uint16_t* __restrict__ hprev, int64_t ldhp, const float* h0, const float* c0,
                    float* hfin, float* cfin, float* __restrict__ hall, int64_t ldha) {
    static_assert(RAGGED || !STATE, "the stateful instantiations are the ragged ones");
    static_assert(STATE || !TRAIN, "TRAIN marks the stateful train variant; the dense one is RAGGED = false with gates");
    extern __shared__ __align__(16) float smem[];
    const int HP = (H + 63) & ~63;
    const int S = kMaxThreads / HP;
    const int j = threadIdx.x % HP, s = threadIdx.x / HP;
    float* hl = smem;                      // [H][G]   h_{t-1} of the group
    float* part = smem + (size_t)H * G;    // [S - 1][4 * G][HP] partial gate sums of slices 1 .. S-1
    const int b0 = blockIdx.x * G;
    const int nb = min(G, B - b0);
    const int KC = (H + S - 1) / S;
    const int k0 = s * KC, k1 = min(H, k0 + KC);
    const bool unit = j < H;
    const int64_t H4 = 4 * (int64_t)H;

    int64_t r0[G];  // uniform over the workgroup, like ln and steps
    int ln[G];      // 0 for the absent sequences of a partial group
    int steps = 0;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (RAGGED && !(STATE && !row0)) {
            r0[g] = g < nb ? row0[b0 + g] : 0;
            ln[g] = g < nb ? min(max(len[b0 + g], 0), T) : 0;
        } else {
            r0[g] = (int64_t)(b0 + g) * T;
            ln[g] = g < nb ? T : 0;
        }
        steps = max(steps, ln[g]);
    }

    float c[G];
#pragma unroll
    for (int g = 0; g < G; ++g) c[g] = 0.f;
    const bool carried = STATE && h0;  // uniform: a state came in, so step 0 has a W_hh product
    if (carried) {
        for (int i = threadIdx.x; i < H * G; i += blockDim.x) {
            const int k = i / G, g = i % G;
            hl[i] = g < nb ? h0[(int64_t)(b0 + g) * H + k] : 0.f;
        }
        if (s == 0 && unit) {
#pragma unroll
            for (int g = 0; g < G; ++g)
                if (g < nb) c[g] = c0[(int64_t)(b0 + g) * H + j];
        }
    } else {
        for (int i = threadIdx.x; i < H * G; i += blockDim.x) hl[i] = 0.f;
    }
    if constexpr (RAGGED && !STATE) {
        if (s == 0 && unit) {
#pragma unroll
            for (int g = 0; g < G; ++g)
                if (g < nb && ln[g] == 0) hlast[(int64_t)(b0 + g) * H + j] = 0.f;
        }
    }
    __syncthreads();
    if constexpr (STATE) {  // after the barrier: every read of h0 / c0 is done, hfin / cfin may alias them
        if (s == 0 && unit) {
#pragma unroll
            for (int g = 0; g < G; ++g)
                if (g < nb && ln[g] == 0) {  // the state passes through, also when the step loop never runs
                    hfin[(int64_t)(b0 + g) * H + j] = hl[(size_t)j * G + g];
                    cfin[(int64_t)(b0 + g) * H + j] = c[g];
                }
        }
    }

    for (int t = 0; t < steps; ++t) {
        // acc[gate][pair] = sum over this slice's k of W_hh[gate*H + j][k] * h_{t-1}[k]
        v2f acc[4][G / 2];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int p = 0; p < G / 2; ++p) acc[q][p] = v2f{0.f, 0.f};
        if ((t > 0 || carried) && unit) {  // h_{-1} = 0 without a carried state
            const float* w = WT + (int64_t)k0 * H4 + j;
#pragma unroll 2
            for (int k = k0; k < k1; ++k, w += H4) {
                const float w0 = w[0], w1 = w[H], w2 = w[2 * (int64_t)H], w3 = w[3 * (int64_t)H];
                const v2f* hv = reinterpret_cast<const v2f*>(hl + (size_t)k * G);
#pragma unroll
                for (int p = 0; p < G / 2; ++p) {
                    const v2f h2 = hv[p];
                    acc[0][p] += h2 * w0;
                    acc[1][p] += h2 * w1;
                    acc[2][p] += h2 * w2;
                    acc[3][p] += h2 * w3;
                }
            }
        }
        if (s > 0) {
            float* pp = part + (size_t)(s - 1) * 4 * G * HP + j;
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int p = 0; p < G / 2; ++p) {
                    pp[(size_t)(q * G + 2 * p) * HP] = acc[q][p].x;
                    pp[(size_t)(q * G + 2 * p + 1) * HP] = acc[q][p].y;
                }
        }
        __syncthreads();  // partials written; every read of h_{t-1} done
        if (s == 0 && unit) {
#pragma unroll 1
            for (int r = 1; r < S; ++r) {
                const float* pp = part + (size_t)(r - 1) * 4 * G * HP + j;
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int p = 0; p < G / 2; ++p) {
                        acc[q][p].x += pp[(size_t)(q * G + 2 * p) * HP];
                        acc[q][p].y += pp[(size_t)(q * G + 2 * p + 1) * HP];
                    }
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (t >= ln[g]) {  // past this sequence's end, or an absent sequence
                    continue;
                }
                const int64_t row = r0[g] + t;
                const float* pr = pre + row * ldpre + j;
                const float a_i = pr[0] + ((g & 1) ? acc[0][g / 2].y : acc[0][g / 2].x);
                const float a_f = pr[H] + ((g & 1) ? acc[1][g / 2].y : acc[1][g / 2].x);
                const float a_g = pr[2 * (int64_t)H] + ((g & 1) ? acc[2][g / 2].y : acc[2][g / 2].x);
                const float a_o = pr[3 * (int64_t)H] + ((g & 1) ? acc[3][g / 2].y : acc[3][g / 2].x);
                const float ig = sigmoidf_(a_i), fg = sigmoidf_(a_f), gg = tanhf_(a_g), og = sigmoidf_(a_o);
                const float hold = hl[(size_t)j * G + g];
                // explicit fmaf: the compiler's own contraction differed by a last bit between instantiations
                c[g] = __builtin_fmaf(fg, c[g], ig * gg);
                const float hn = og * tanhf_(c[g]);
                hl[(size_t)j * G + g] = hn;
                float hs = hn;  // what h_seq keeps: times keep in the train steps
                if constexpr (!RAGGED || TRAIN) hs *= keep ? keep[row * H + j] : 1.0f;
                hseq[row * ldh + j] = f2bf(hs);
                if constexpr (STATE) {
                    if (hall) hall[row * ldha + j] = hn;
                    if (t == ln[g] - 1) {
                        hfin[(int64_t)(b0 + g) * H + j] = hn;
                        cfin[(int64_t)(b0 + g) * H + j] = c[g];
                    }
                } else {
                    if (t == ln[g] - 1) hlast[(int64_t)(b0 + g) * H + j] = hn;
                }
                if constexpr (!RAGGED || TRAIN) {
                    if (gates) {
                        float* gp = gates + row * H4 + j;
                        gp[0] = ig;
                        gp[H] = fg;
                        gp[2 * (int64_t)H] = gg;
                        gp[3 * (int64_t)H] = og;
                        cseq[row * H + j] = c[g];
                        hprev[row * ldhp + j] = f2bf(hold);
                    }
                }
            }
        }
        __syncthreads();  // h_t visible; partials consumed
    }
}

// BPTT, t = T-1 .. 0, from the saved gates and c.  dh: last_only = 0: [B*T][H] rows b*T + t;
// last_only = 1: [B][H], the gradient of the last step's h only.  keep (optional) scales the incoming
// dh rows like the forward scaled the stored h_seq.  W = W_hh [4H][H].  Writes dpre fp32 and bf16.
// Stateful (STATE = true): the backward of the stateful train forward.  Rows as there (row0 == nullptr: the
// dense rows b * T + t; else q0 = row0[b], ln = len[b] clamped to [0, T = max_len]).  The workgroup loops
// from the largest length of its group down to 0 (uniform: the barriers stay legal), so every sequence
// reaches its step 0 in the last pass; one that has not started yet (t >= ln) leaves its zero rows in the
// LDS dpre tile and touches no memory.  dh = dL/dh_seq rows (optional, times keep), last_only is not read;
// dhn / dcn (optional, [B][H], never masked) enter at a sequence's last valid step in place of the
// recurrent dh / the carried dc, which are zero there; c0 (optional) is the c_{-1} of step 0.  With dh0 /
// dc0 the W_hh^T product runs once more after step 0 on the same tile: dh0 = W_hh^T dpre_0, dc0 = dc_0 f_0,
// and a sequence of length 0 passes dhn / dcn (or zeros) through.  dh0 may alias dhn and dc0 dcn: the
// one thread that writes an element is the one that read it, so these four carry no __restrict__.
// STATE = false compiles all of it out.
template <int G, bool STATE = false>
__global__ void __launch_bounds__(kMaxThreads)
lstm_seq_bwd_kernel(const float* __restrict__ gates, const float* __restrict__ cseq, int B, int T, int H,
                    const float* __restrict__ W, const float* __restrict__ dh, int64_t lddh, int last_only,
                    const float* __restrict__ keep, float* __restrict__ dpre, uint16_t* __restrict__ dpreb, int64_t lddb,
                    const int32_t* __restrict__ row0, const int32_t* __restrict__ len, const float* __restrict__ c0,
                    const float* dhn, const float* dcn, float* dh0, float* dc0) {
    extern __shared__ __align__(16) float smem[];
    const int HP = (H + 63) & ~63;
    const int S = kMaxThreads / HP;
    const int j = threadIdx.x % HP, s = threadIdx.x / HP;
    const int R = 4 * H;
    float* dl = smem;                     // [4H][G]  dpre_t of the group
    float* part = smem + (size_t)R * G;   // [S - 1][G][HP]
    const int b0 = blockIdx.x * G;
    const int nb = min(G, B - b0);
    const int RC = (R + S - 1) / S;
    const int r0 = s * RC, r1 = min(R, r0 + RC);
    const bool unit = j < H;
    const int64_t H4 = R;

    float dc[G], dhr[G];  // carried dL/dc_t and the recurrent part of dL/dh_t (slice 0 threads)
#pragma unroll
    for (int g = 0; g < G; ++g) dc[g] = dhr[g] = 0.f;
    for (int i = threadIdx.x; i < R * G; i += blockDim.x) dl[i] = 0.f;  // rows of absent sequences stay 0
    __syncthreads();

    int64_t q0[G];  // STATE: the first row and the length of each sequence, uniform over the workgroup
    int ln[G];
    int steps = T;
    if constexpr (STATE) {
        steps = 0;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            q0[g] = row0 ? (g < nb ? row0[b0 + g] : 0) : (int64_t)(b0 + g) * T;
            ln[g] = g < nb ? (row0 ? min(max(len[b0 + g], 0), T) : T) : 0;
            steps = max(steps, ln[g]);
        }
    }

    for (int t = steps - 1; t >= 0; --t) {
        if (s == 0 && unit) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (STATE ? t >= ln[g] : g >= nb) {  // an absent sequence, or one that has not started yet
                    continue;
                }
                const int64_t row = STATE ? q0[g] + t : (int64_t)(b0 + g) * T + t;
                float dht = dhr[g];
                if constexpr (STATE) {
                    if (t == ln[g] - 1) {  // the last valid step: the gradients of the outgoing state come in
                        dht = dhn ? dhn[(int64_t)(b0 + g) * H + j] : 0.f;
                        dc[g] = dcn ? dcn[(int64_t)(b0 + g) * H + j] : 0.f;
                    }
                    if (dh) dht += dh[row * lddh + j] * (keep ? keep[row * H + j] : 1.0f);
                } else if (!last_only) {
                    dht += dh[row * lddh + j] * (keep ? keep[row * H + j] : 1.0f);
                } else if (t == T - 1) {
                    dht += dh[(int64_t)(b0 + g) * lddh + j] * (keep ? keep[row * H + j] : 1.0f);
                }
                const float* gp = gates + row * H4 + j;
                const float ig = gp[0], fg = gp[H], gg = gp[2 * (int64_t)H], og = gp[3 * (int64_t)H];
                const float ct = cseq[row * H + j];
                float cp = t > 0 ? cseq[(row - 1) * H + j] : 0.f;
                if constexpr (STATE) {
                    if (t == 0 && c0) cp = c0[(int64_t)(b0 + g) * H + j];
                }
                const float tc = tanhf_(ct);
                const float dct = dht * og * (1.0f - tc * tc) + dc[g];
                const float d_i = dct * gg * ig * (1.0f - ig);
                const float d_f = dct * cp * fg * (1.0f - fg);
                const float d_g = dct * ig * (1.0f - gg * gg);
                const float d_o = dht * tc * og * (1.0f - og);
                dc[g] = dct * fg;
                dl[(size_t)j * G + g] = d_i;
                dl[(size_t)(H + j) * G + g] = d_f;
                dl[(size_t)(2 * H + j) * G + g] = d_g;
                dl[(size_t)(3 * H + j) * G + g] = d_o;
                float* dp = dpre + row * H4 + j;
                dp[0] = d_i;
                dp[H] = d_f;
                dp[2 * (int64_t)H] = d_g;
                dp[3 * (int64_t)H] = d_o;
                uint16_t* db = dpreb + row * lddb + j;
                db[0] = f2bf(d_i);
                db[H] = f2bf(d_f);
                db[2 * (int64_t)H] = f2bf(d_g);
                db[3 * (int64_t)H] = f2bf(d_o);
            }
        }
        if (t == 0 && !(STATE && dh0)) break;  // uniform: nothing consumes dh_{-1} unless dh0 is asked for
        __syncthreads();                       // dpre_t of the group in LDS
        // dh_{t-1}[j] (recurrent part) = sum_r dpre_t[r] * W_hh[r][j]
        v2f acc[G / 2];
#pragma unroll
        for (int p = 0; p < G / 2; ++p) acc[p] = v2f{0.f, 0.f};
        if (unit) {
            const float* w = W + (int64_t)r0 * H + j;
#pragma unroll 8
            for (int r = r0; r < r1; ++r, w += H) {
                const float wv = w[0];
                const v2f* dv = reinterpret_cast<const v2f*>(dl + (size_t)r * G);
#pragma unroll
                for (int p = 0; p < G / 2; ++p) acc[p] += dv[p] * wv;
            }
        }
        if (s > 0) {
            float* pp = part + (size_t)(s - 1) * G * HP + j;
#pragma unroll
            for (int p = 0; p < G / 2; ++p) {
                pp[(size_t)(2 * p) * HP] = acc[p].x;
                pp[(size_t)(2 * p + 1) * HP] = acc[p].y;
            }
        }
        __syncthreads();  // partials written; every read of dpre_t done
        if (s == 0) {
            for (int r = 1; r < S; ++r) {
                const float* pp = part + (size_t)(r - 1) * G * HP + j;
#pragma unroll
                for (int p = 0; p < G / 2; ++p) {
                    acc[p].x += pp[(size_t)(2 * p) * HP];
                    acc[p].y += pp[(size_t)(2 * p + 1) * HP];
                }
            }
#pragma unroll
            for (int g = 0; g < G; ++g) dhr[g] = (g & 1) ? acc[g / 2].y : acc[g / 2].x;
        }
        // the next step's partial writes come after its first barrier, so these reads are ordered
    }
    if constexpr (STATE) {
        if (dh0 && s == 0 && unit) {  // dhr = W_hh^T dpre_0 and dc = dc_0 f_0 now; length 0: dhn / dcn pass through
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (g >= nb) {
                    continue;
                }
                const int64_t at = (int64_t)(b0 + g) * H + j;
                dh0[at] = ln[g] ? dhr[g] : (dhn ? dhn[at] : 0.f);
                dc0[at] = ln[g] ? dc[g] : (dcn ? dcn[at] : 0.f);
            }
        }
    }
}

// logits[b] = W2 . (relu(W1 . h[b] + b1) * keep[b]) + b2; hid (optional) keeps the masked hidden row
__global__ void __launch_bounds__(256) mlp_head_fwd_kernel(const float* __restrict__ h, int Hs, const float* __restrict__ W1,
                                                           const float* __restrict__ b1, int H1,
                                                           const float* __restrict__ keep, const float* __restrict__ W2,
                                                           const float* __restrict__ b2, int nl, float* __restrict__ hid,
                                                           float* __restrict__ logits) {
    __shared__ float hs[1024];
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int r = w; r < H1; r += 4) {
        float a = 0.f;
        for (int k = lane; k < Hs; k += 64) a += W1[(int64_t)r * Hs + k] * h[(int64_t)b * Hs + k];
        a = wave_sum(a);
        if (lane == 0) {
            float v = fmaxf(a + b1[r], 0.f);
            if (keep) v *= keep[(int64_t)b * H1 + r];
            hs[r] = v;
            if (hid) hid[(int64_t)b * H1 + r] = v;
        }
    }
    __syncthreads();
    for (int c = w; c < nl; c += 4) {
        float a = 0.f;
        for (int k = lane; k < H1; k += 64) a += W2[(int64_t)c * H1 + k] * hs[k];
        a = wave_sum(a);
        if (lane == 0) logits[(int64_t)b * nl + c] = a + b2[c];
    }
}

// da[b][r] = dL/d(W1 h + b1)[b][r] = keep * [hid > 0] * sum_c dlogits[b][c] W2[c][r]
__device__ __forceinline__ float head_da(const float* __restrict__ dl, const float* __restrict__ W2,
                                         const float* __restrict__ hid, const float* __restrict__ keep, int64_t b, int r,
                                         int H1, int nl) {
    if (!(hid[b * H1 + r] > 0.f)) return 0.f;
    float a = 0.f;
    for (int c = 0; c < nl; ++c) a += dl[b * nl + c] * W2[(int64_t)c * H1 + r];
    return keep ? a * keep[b * H1 + r] : a;
}

// blocks [0, H1): dW1 row r and db1[r]; blocks [H1, H1 + B): dh row b; block H1 + B: dW2, db2.
// Every sum runs over b (or r) in index order in one thread: deterministic, no atomics.
__global__ void __launch_bounds__(256) mlp_head_bwd_kernel(const float* __restrict__ h, const float* __restrict__ W1,
                                                           const float* __restrict__ W2, const float* __restrict__ hid,
                                                           const float* __restrict__ keep, const float* __restrict__ dl,
                                                           int B, int Hs, int H1, int nl, float* __restrict__ dh,
                                                           float* __restrict__ dW1, float* __restrict__ db1,
                                                           float* __restrict__ dW2, float* __restrict__ db2) {
    __shared__ float da_s[1024];
    const int blk = blockIdx.x;
    if (blk < H1) {
        const int r = blk;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};  // Hs <= 1024 = 4 * 256
        float sb = 0.f;
        for (int b = 0; b < B; ++b) {
            const float da = head_da(dl, W2, hid, keep, b, r, H1, nl);
            sb += da;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = q * 256 + threadIdx.x;
                if (k < Hs) acc[q] += da * h[(int64_t)b * Hs + k];
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = q * 256 + threadIdx.x;
            if (k < Hs) dW1[(int64_t)r * Hs + k] = acc[q];
        }
        if (threadIdx.x == 0) db1[r] = sb;
    } else if (blk < H1 + B) {
        const int64_t b = blk - H1;
        for (int r = threadIdx.x; r < H1; r += 256) da_s[r] = head_da(dl, W2, hid, keep, b, r, H1, nl);
        __syncthreads();
        for (int k = threadIdx.x; k < Hs; k += 256) {
            float a = 0.f;
            for (int r = 0; r < H1; ++r) a += da_s[r] * W1[(int64_t)r * Hs + k];
            dh[b * Hs + k] = a;
        }
    } else {
        for (int i = threadIdx.x; i < nl * H1; i += 256) {
            const int c = i / H1, r = i % H1;
            float a = 0.f;
            for (int b = 0; b < B; ++b) a += dl[(int64_t)b * nl + c] * hid[(int64_t)b * H1 + r];
            dW2[i] = a;
        }
        for (int c = threadIdx.x; c < nl; c += 256) {
            float a = 0.f;
            for (int b = 0; b < B; ++b) a += dl[(int64_t)b * nl + c];
            db2[c] = a;
        }
    }
}

static const char* check_hidden(int64_t B, int64_t T, int64_t hidden) {
    if (B <= 0 || T <= 0 || B > INT32_MAX / 4 || T > INT32_MAX / 4) return "B and T must be >= 1";
    if (hidden <= 0 || hidden > 1024 || hidden % 4) return "unsupported hidden size (hidden % 4 == 0 and hidden <= 1024)";
    return nullptr;
}

// The launch geometry of the recurrence kernels (the schedule in the header comment), in one place.
struct SeqLaunch {
    int H, G, HP, S;
    unsigned grid, block;
    SeqLaunch(int64_t B, int64_t hidden)
        : H((int)hidden), G(group_of(hidden)), HP((H + 63) & ~63), S(kMaxThreads / HP), grid((unsigned)((B + G - 1) / G)),
          block((unsigned)(S * HP)) {}
    size_t lds_fwd() const { return ((size_t)H * G + (size_t)(S - 1) * 4 * G * HP) * sizeof(float); }  // hl + part
    size_t lds_bwd() const { return ((size_t)4 * H * G + (size_t)(S - 1) * G * HP) * sizeof(float); }  // dl + part
    // k4 / k2: the G = 4 and G = 2 instantiations of one kernel
    template <typename K, typename... Args>
    void run(K k4, K k2, size_t lds, hipStream_t stream, Args... args) const {
        const K k = G == 4 ? k4 : k2;
        k<<<grid, block, lds, stream>>>(args...);
    }
};

}  // namespace lstm
}  // namespace vc

using namespace vc;
using namespace vc::lstm;

extern "C" {

int vc_frame_avgpool(const uint16_t* x, int elem_type, int64_t ldx, int64_t N, int64_t P, int64_t C, uint16_t* out,
                     int64_t ldo, hipStream_t stream) {
    if (!x || !out) return fail(VC_ERR_INVALID_ARG, "vc_frame_avgpool: null pointer");
    if (N <= 0 || P <= 0 || C <= 0 || ldx < C || ldo < C || N > INT32_MAX || P > INT32_MAX || C > 65535 * 256)
        return fail(VC_ERR_INVALID_ARG, "vc_frame_avgpool: bad shape");
    if (elem_type != VC_ELEM_BF16 && elem_type != VC_ELEM_F16) return fail(VC_ERR_INVALID_ARG, "vc_frame_avgpool: elem_type");
    const dim3 grid((unsigned)N, (unsigned)((C + 255) / 256));
    if (elem_type == VC_ELEM_F16)
        frame_avgpool_kernel<VC_ELEM_F16><<<grid, 256, 0, stream>>>(x, ldx, (int)P, (int)C, out, ldo);
    else
        frame_avgpool_kernel<VC_ELEM_BF16><<<grid, 256, 0, stream>>>(x, ldx, (int)P, (int)C, out, ldo);
    return check_launch("vc_frame_avgpool");
}

int vc_bn_apply_h16(const float* y, int64_t ldy, int64_t M, int64_t C, const float* stat, const float* gamma,
                    const float* beta, const uint16_t* res, int64_t ldr, int relu, uint16_t* z, int64_t ldz,
                    hipStream_t stream) {
    if (!y || !stat || !gamma || !beta || !z) return fail(VC_ERR_INVALID_ARG, "vc_bn_apply_h16: null pointer");
    if (M <= 0 || C <= 0 || C > INT32_MAX || C % 4 || ldy % 4 || ldy < C || ldz < C || ldz % 4 || (res && ldr < C) ||
        ((uintptr_t)y & 15) || ((uintptr_t)z & 7))
        return fail(VC_ERR_INVALID_ARG, "vc_bn_apply_h16: bad shape (C % 4, 16-B y rows, 8-B z rows)");
    bn_apply_h16_kernel<<<(unsigned)((M * (C / 4) + 255) / 256), 256, 0, stream>>>(y, ldy, M, (int)C, stat, gamma, beta, res,
                                                                                   ldr, relu, z, ldz);
    return check_launch("vc_bn_apply_h16");
}

int vc_video_to_cl_h16(const float* x, int64_t B, int64_t C, int64_t P, uint16_t* out, hipStream_t stream) {
    if (!x || !out) return fail(VC_ERR_INVALID_ARG, "vc_video_to_cl_h16: null pointer");
    if (B <= 0 || P <= 0 || C <= 0 || C > 8 || B * P > ((int64_t)1 << 38) || ((uintptr_t)out & 15))
        return fail(VC_ERR_INVALID_ARG, "vc_video_to_cl_h16: bad shape (1 <= C <= 8, 16-B aligned out)");
    video_to_cl_h16_kernel<<<(unsigned)((B * P + 255) / 256), 256, 0, stream>>>(x, B, (int)C, P, out);
    return check_launch("vc_video_to_cl_h16");
}

int vc_lstm_seq_fwd(const float* pre, int64_t ldpre, int64_t B, int64_t T, int64_t hidden, const float* W_hh_t,
                    const float* keep, uint16_t* h_seq, int64_t ldh, float* h_last, float* gates, float* c_seq,
                    uint16_t* h_prev, int64_t ldhp, hipStream_t stream) {
    if (!pre || !W_hh_t || !h_seq || !h_last) return fail(VC_ERR_INVALID_ARG, "vc_lstm_seq_fwd: null pointer");
    if (const char* m = check_hidden(B, T, hidden)) return fail(VC_ERR_INVALID_ARG, std::string("vc_lstm_seq_fwd: ") + m);
    if (ldpre < 4 * hidden || ldh < hidden) return fail(VC_ERR_INVALID_ARG, "vc_lstm_seq_fwd: row stride below the row length");
    if (gates && (!c_seq || !h_prev || ldhp < hidden))
        return fail(VC_ERR_INVALID_ARG, "vc_lstm_seq_fwd: the train variant needs gates, c_seq and h_prev (ldhp >= hidden)");
    const SeqLaunch L(B, hidden);
    L.run(lstm_seq_fwd_kernel<4, false>, lstm_seq_fwd_kernel<2, false>, L.lds_fwd(), stream, pre, ldpre, (int)B, (int)T, L.H,
          W_hh_t, nullptr, nullptr, keep, h_seq, ldh, h_last, gates, c_seq, h_prev, ldhp, nullptr, nullptr, nullptr, nullptr,
          nullptr, 0);
    return check_launch("vc_lstm_seq_fwd");
}

int vc_lstm_seq_fwd_ragged(const float* pre, int64_t ldpre, int64_t B, const int32_t* row0, const int32_t* len,
                           int64_t max_len, int64_t hidden, const float* W_hh_t, uint16_t* h_seq, int64_t ldh,
                           float* h_last, hipStream_t stream) {
    if (!pre || !row0 || !len || !W_hh_t || !h_seq || !h_last)
        return fail(VC_ERR_INVALID_ARG, "vc_lstm_seq_fwd_ragged: null pointer");
    if (const char* m = check_hidden(B, max_len, hidden))
        return fail(VC_ERR_INVALID_ARG, std::string("vc_lstm_seq_fwd_ragged (T = max_len): ") + m);
    if (ldpre < 4 * hidden || ldh < hidden)
        return fail(VC_ERR_INVALID_ARG, "vc_lstm_seq_fwd_ragged: row stride below the row length");
    const SeqLaunch L(B, hidden);
    L.run(lstm_seq_fwd_kernel<4, true>, lstm_seq_fwd_kernel<2, true>, L.lds_fwd(), stream, pre, ldpre, (int)B, (int)max_len,
          L.H, W_hh_t, row0, len, nullptr, h_seq, ldh, h_last, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
          nullptr, nullptr, 0);
    return check_launch("vc_lstm_seq_fwd_ragged");
}

int vc_lstm_seq_fwd_state(const float* pre, int64_t ldpre, int64_t B, const int32_t* row0, const int32_t* len,
                          int64_t max_len, int64_t hidden, const float* W_hh_t, const float* h0, const float* c0,
                          uint16_t* h_seq, int64_t ldh, float* h_all, int64_t ldha, float* h_n, float* c_n,
                          hipStream_t stream) {
    if (!pre || !W_hh_t || !h_seq || !h_n || !c_n) return fail(VC_ERR_INVALID_ARG, "vc_lstm_seq_fwd_state: null pointer");
    if (!row0 != !len)
        return fail(VC_ERR_INVALID_ARG, "vc_lstm_seq_fwd_state: row0 and len come together (both null: the dense layout)");
    if (!h0 != !c0)
        return fail(VC_ERR_INVALID_ARG, "vc_lstm_seq_fwd_state: h0 and c0 come together (both null: the zero state)");
    if (const char* m = check_hidden(B, max_len, hidden))
        return fail(VC_ERR_INVALID_ARG, std::string("vc_lstm_seq_fwd_state (T = max_len): ") + m);
    if (ldpre < 4 * hidden || ldh < hidden || (h_all && ldha < hidden))
        return fail(VC_ERR_INVALID_ARG, "vc_lstm_seq_fwd_state: row stride below the row length");
    const SeqLaunch L(B, hidden);
    L.run(lstm_seq_fwd_kernel<4, true, true>, lstm_seq_fwd_kernel<2, true, true>, L.lds_fwd(), stream, pre, ldpre, (int)B,
          (int)max_len, L.H, W_hh_t, row0, len, nullptr, h_seq, ldh, nullptr, nullptr, nullptr, nullptr, 0, h0, c0, h_n, c_n,
          h_all, ldha);
    return check_launch("vc_lstm_seq_fwd_state");
}

int vc_lstm_seq_fwd_train_state(const float* pre, int64_t ldpre, int64_t B, const int32_t* row0, const int32_t* len,
                                int64_t max_len, int64_t hidden, const float* W_hh_t, const float* h0, const float* c0,
                                const float* keep, uint16_t* h_seq, int64_t ldh, float* h_n, float* c_n, float* gates,
                                float* c_seq, uint16_t* h_prev, int64_t ldhp, hipStream_t stream) {
    if (!pre || !W_hh_t || !h_seq || !h_n || !c_n || !gates || !c_seq || !h_prev)
        return fail(VC_ERR_INVALID_ARG, "vc_lstm_seq_fwd_train_state: null pointer");
    if (!row0 != !len)
        return fail(VC_ERR_INVALID_ARG, "vc_lstm_seq_fwd_train_state: row0 and len come together (both null: the dense layout)");
    if (!h0 != !c0)
        return fail(VC_ERR_INVALID_ARG, "vc_lstm_seq_fwd_train_state: h0 and c0 come together (both null: the zero state)");
    if (const char* m = check_hidden(B, max_len, hidden))
        return fail(VC_ERR_INVALID_ARG, std::string("vc_lstm_seq_fwd_train_state (T = max_len): ") + m);
    if (ldpre < 4 * hidden || ldh < hidden || ldhp < hidden)
        return fail(VC_ERR_INVALID_ARG, "vc_lstm_seq_fwd_train_state: row stride below the row length");
    const SeqLaunch L(B, hidden);
    L.run(lstm_seq_fwd_kernel<4, true, true, true>, lstm_seq_fwd_kernel<2, true, true, true>, L.lds_fwd(), stream, pre, ldpre,
          (int)B, (int)max_len, L.H, W_hh_t, row0, len, keep, h_seq, ldh, nullptr, gates, c_seq, h_prev, ldhp, h0, c0, h_n,
          c_n, nullptr, 0);
    return check_launch("vc_lstm_seq_fwd_train_state");
}

int vc_lstm_seq_bwd(const float* gates, const float* c_seq, int64_t B, int64_t T, int64_t hidden, const float* W_hh,
                    const float* dh, int64_t lddh, int last_only, const float* keep, float* dpre, uint16_t* dpre_bf16,
                    int64_t lddb, hipStream_t stream) {
    if (!gates || !c_seq || !W_hh || !dh || !dpre || !dpre_bf16) return fail(VC_ERR_INVALID_ARG, "vc_lstm_seq_bwd: null pointer");
    if (const char* m = check_hidden(B, T, hidden)) return fail(VC_ERR_INVALID_ARG, std::string("vc_lstm_seq_bwd: ") + m);
    if (lddh < hidden || lddb < 4 * hidden) return fail(VC_ERR_INVALID_ARG, "vc_lstm_seq_bwd: row stride below the row length");
    const SeqLaunch L(B, hidden);
    L.run(lstm_seq_bwd_kernel<4>, lstm_seq_bwd_kernel<2>, L.lds_bwd(), stream, gates, c_seq, (int)B, (int)T, L.H, W_hh, dh,
          lddh, last_only, keep, dpre, dpre_bf16, lddb, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    return check_launch("vc_lstm_seq_bwd");
}

int vc_lstm_seq_bwd_state(const float* gates, const float* c_seq, const float* c0, int64_t B, const int32_t* row0,
                          const int32_t* len, int64_t max_len, int64_t hidden, const float* W_hh, const float* dh_seq,
                          int64_t lddh, const float* keep, const float* dh_n, const float* dc_n, float* dpre,
                          uint16_t* dpre_bf16, int64_t lddb, float* dh0, float* dc0, hipStream_t stream) {
    if (!gates || !c_seq || !W_hh || !dpre || !dpre_bf16) return fail(VC_ERR_INVALID_ARG, "vc_lstm_seq_bwd_state: null pointer");
    if (!row0 != !len)
        return fail(VC_ERR_INVALID_ARG, "vc_lstm_seq_bwd_state: row0 and len come together (both null: the dense layout)");
    if (!dh0 != !dc0) return fail(VC_ERR_INVALID_ARG, "vc_lstm_seq_bwd_state: dh0 and dc0 come together (both null: not wanted)");
    if (const char* m = check_hidden(B, max_len, hidden))
        return fail(VC_ERR_INVALID_ARG, std::string("vc_lstm_seq_bwd_state (T = max_len): ") + m);
    if ((dh_seq && lddh < hidden) || lddb < 4 * hidden)
        return fail(VC_ERR_INVALID_ARG, "vc_lstm_seq_bwd_state: row stride below the row length");
    const SeqLaunch L(B, hidden);
    L.run(lstm_seq_bwd_kernel<4, true>, lstm_seq_bwd_kernel<2, true>, L.lds_bwd(), stream, gates, c_seq, (int)B, (int)max_len,
          L.H, W_hh, dh_seq, lddh, 0, keep, dpre, dpre_bf16, lddb, row0, len, c0, dh_n, dc_n, dh0, dc0);
    return check_launch("vc_lstm_seq_bwd_state");
}

int vc_mlp_head_fwd(const float* h, int64_t B, int64_t hidden, const float* W1, const float* b1, int64_t H1,
                    const float* keep, const float* W2, const float* b2, int64_t num_labels, float* hid, float* logits,
                    hipStream_t stream) {
    if (!h || !W1 || !b1 || !W2 || !b2 || !logits) return fail(VC_ERR_INVALID_ARG, "vc_mlp_head_fwd: null pointer");
    if (B <= 0 || B > INT32_MAX || hidden <= 0 || hidden > 1024 || H1 <= 0 || H1 > 1024 || num_labels <= 0 || num_labels > 1024)
        return fail(VC_ERR_INVALID_ARG, "vc_mlp_head_fwd: B >= 1; hidden, H1, num_labels in (0, 1024]");
    mlp_head_fwd_kernel<<<(unsigned)B, 256, 0, stream>>>(h, (int)hidden, W1, b1, (int)H1, keep, W2, b2, (int)num_labels, hid,
                                                         logits);
    return check_launch("vc_mlp_head_fwd");
}

int vc_mlp_head_bwd(const float* h, const float* W1, const float* W2, const float* hid, const float* keep,
                    const float* dlogits, int64_t B, int64_t hidden, int64_t H1, int64_t num_labels, float* dh, float* dW1,
                    float* db1, float* dW2, float* db2, hipStream_t stream) {
    if (!h || !W1 || !W2 || !hid || !dlogits || !dh || !dW1 || !db1 || !dW2 || !db2)
        return fail(VC_ERR_INVALID_ARG, "vc_mlp_head_bwd: null pointer");
    if (B <= 0 || B > (1 << 30) || hidden <= 0 || hidden > 1024 || H1 <= 0 || H1 > 1024 || num_labels <= 0 || num_labels > 1024)
        return fail(VC_ERR_INVALID_ARG, "vc_mlp_head_bwd: B >= 1; hidden, H1, num_labels in (0, 1024]");
    mlp_head_bwd_kernel<<<(unsigned)(H1 + B + 1), 256, 0, stream>>>(h, W1, W2, hid, keep, dlogits, (int)B, (int)hidden, (int)H1,
                                                                   (int)num_labels, dh, dW1, db1, dW2, db2);
    return check_launch("vc_mlp_head_bwd");
}

}  // extern "C"
