// Attention rollout through Video Swin's shifted-window attention (head_dim 32), flash-style: the window's
// probabilities are recomputed from the kept q'|k rows and never stored.
//
// Swin has no CLS token: its head reads the mean of the last stage's tokens, so the rollout carries a row vector over
// ALL tokens of a stage, seeded uniform, and walks the blocks back.  One block step, with a = alpha:
//     r_out[j] = a * (1/heads) sum_h sum_{i in win(j)} r_in[i] * P_h[i][j] + (1 - a) * r_in[j]
//     P_h[i][.] = softmax2 over the window's tokens of q'_i . k_j + log2 e * table[idx(i, j)][h],
// pairs of different shift regions excluded (torchvision adds -100, the attention kernels -inf).  Window membership,
// window-local order, region codes and the relative-position index are window_common.hpp's (win_token_row,
// rel_code): the rows are gathered by index through the roll and the partition, as window.hip reads them.
//
// vc_window_rollout_step is three launches.  The score product is window.hip's: 32x32x16 bf16 MFMA on 32-row
// blocks, one operand staged in LDS with that file's chunk swizzle, the other read from global memory as fragments.
//   window_rollout_norm_kernel  the exact row normaliser.  One workgroup (4 waves) per (window, head, 128 queries),
//                           the window's k rows in LDS; a wave holds 32 queries (one per lane pair) and walks the
//                           32-key blocks: S^T = K . Q'^T, + bias (a gather from the head's table column in LDS),
//                           region mask, online maximum m_i and sum l_i per block of 32 keys.  Stores m_i and
//                           w_i = r_in[i] / l_i per (head, token) in the work buffer.
//   window_rollout_cols_kernel<GRAD>  the column sums.  One workgroup per (window, head, 128 keys), the window's q'
//                           rows, m and w in LDS; a wave holds 32 keys and walks the 32-query blocks in window order:
//                           S = Q' . K^T (the same products and the same accumulation as above, operands swapped),
//                           u_h[j] = sum_i w_i * exp2(s_ij - m_i).  u_h goes to work[h][row(j)]: no atomics.
//   window_rollout_finish<GRAD> r_out[n] = a * (sum_h work[h][n]) / heads + (1 - a) * r_in[n], heads in head order.
// Splitting the window's rows over workgroups matters more than the pipe: the late stages have few (window, head)
// pairs (Swin-T stage 4: 48), and one workgroup per pair left the device idle (the first version,
// fdot2 on the VALU with one workgroup per pair, took 1.7 x the forward).  No lse input: the entry stands alone on
// q'|k, and the exact normaliser costs the second pass over the scores.  Every token is in exactly one window, so
// every r_out entry is written; a clip's windows depend on nothing outside the clip (batch-invariant), and every sum
// runs in a fixed order (deterministic).
//
// vc_merge_rollout_spread is the hop through PatchMerging: a merged token gives an equal share of its relevance to
// each of its existing children.
//
// vc_window_grad_rollout_step is the class-specific step (Chefer, Gur & Wolf 2021): the same three launches with the
// probabilities weighted by the positive part of their gradient dP_h[i][j] = dO_h[i] . v_j,
//     u[j] = (1/heads) sum_h sum_{i in win(j)} r_in[i] * P_h[i][j] * max(dP_h[i][j], 0),
//     a_out[j] = alpha * u[j] + beta * a_in[j],   r_out[j] = a_out[j] + base[j].
// The normaliser kernel is the same one; the column and finish kernels are the <true> instantiations of their
// templates (as attention_rollout.hip's rollout_partial_kernel<GRAD>).  In the column kernel, under `if constexpr
// (GRAD)`, the window's dO rows are staged beside its q' rows and the lane's v row is read beside its k row, so both
// 32x32 products land in the same registers (72 KB of LDS at the full window: that instantiation's dynamic-LDS limit
// is raised).  Both entries share step_setup (validation and geometry) and step_launch.
#include "window_common.hpp"

namespace vc {
namespace wroll {

constexpr int NPMAX = 448;  // max padded window volume (8*7*7 = 392 -> 448)
constexpr int64_t LDS_MAX = 64 * 1024;
constexpr int64_t GLDS_MAX = 160 * 1024;  // the CU's LDS; above 64 KiB the kernel's dynamic-LDS limit is raised
constexpr float LOG2E = 1.4426950408889634f;
constexpr int LAB_PAD = 15;   // a padded window slot: its region matches no real token's (real codes are <= 7)
constexpr int LAB_NONE = 14;  // a lane without a row: matches nothing, a padded slot included
constexpr int NT = 256;       // 4 waves: 128 rows of the window per workgroup
constexpr int WAVES = NT / 64;

// LDS: rows [NP][64 B] (k in the normaliser kernel, q' in the column kernel; 16-B chunks swizzled as window.hip's K),
// the head's table column f32 [ntab -> multiple of 4], per window slot cl int [NP] (rel_code << 4 | region code), and
// in the column kernel mrow f32 [NP], wrow f32 [NP]
__host__ __device__ inline int64_t lds_bytes(int64_t NP, int64_t ntab) { return NP * 64 + (ntab + 3) / 4 * 16 + NP * 12; }
// the gradient column kernel: the dO rows [NP][64 B] after the q' rows, then the same (72 864 B at the full window)
__host__ __device__ inline int64_t grad_lds_bytes(int64_t NP, int64_t ntab) { return lds_bytes(NP, ntab) + NP * 64; }

struct Block {
    int b, wi_t, wi_h, wi_w, head, spl;
};

__device__ __forceinline__ Block decode_block(const WinGeom& g, int heads, int nspl) {
    Block k;
    int id = blockIdx.x;
    k.spl = id % nspl;
    id /= nspl;
    k.head = id % heads;
    const int wlin = id / heads;
    const int nwin = g.nwt * g.nwh * g.nww;
    k.b = wlin / nwin;
    int r = wlin - k.b * nwin;
    k.wi_t = r / (g.nwh * g.nww);
    r -= k.wi_t * g.nwh * g.nww;
    k.wi_h = r / g.nww;
    k.wi_w = r - k.wi_h * g.nww;
    return k;
}

// stage the window's rows of this head from a row-major bf16 matrix (col0: the column of the part wanted, 0 for q' and
// dO, heads*32 for k; zeros in the padded slots), 16-B chunks swizzled
__device__ __forceinline__ void stage_rows(const uint16_t* __restrict__ src, int64_t ld, int col0, const WinGeom& g,
                                           const Block& k, int vol, int NP, char* rows) {
    const int tid = threadIdx.x;
    // every load issued before the first LDS write (a rolled loop waits out one gather latency per NT chunks,
    // as window.hip found): <= 7 chunks of 16 B per thread at NP = 448
    constexpr int NCH = NPMAX * 4 / NT;
    uint4 v[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int c = tid + NT * j, n = c >> 2, ch = c & 3;
        v[j] = make_uint4(0, 0, 0, 0);
        if (n < vol) {
            const int64_t row = win_token_row(g, k.b, k.wi_t, k.wi_h, k.wi_w, n, nullptr);
            v[j] = *reinterpret_cast<const uint4*>(src + row * ld + col0 + k.head * 32 + ch * 8);
        }
    }
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int c = tid + NT * j, n = c >> 2, ch = c & 3;
        if (n < NP) *reinterpret_cast<uint4*>(rows + n * 64 + kchunk_swz(n, ch) * 16) = v[j];
    }
}

// stage_rows of qkv, the table column scaled by log2 e, and every slot's (code, region)
__device__ __forceinline__ void stage(const uint16_t* __restrict__ qkv, int64_t ld, int col0, const WinGeom& g,
                                      const FullWin& fw, const Block& k, int heads, int vol, int NP,
                                      const float* __restrict__ table, int ntab, char* rows, float* tab, int* cl) {
    const int tid = threadIdx.x;
    stage_rows(qkv, ld, col0, g, k, vol, NP, rows);
    for (int i0 = 0; i0 < ntab; i0 += NT * 8) {  // the same for the table column, eight loads in flight
        float t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = i0 + tid + NT * j;
            t[j] = i < ntab ? table[(int64_t)i * heads + k.head] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = i0 + tid + NT * j;
            if (i < ntab) tab[i] = t[j] * LOG2E;
        }
    }
    for (int n = tid; n < NP; n += NT) {
        int v = LAB_PAD;
        if (n < vol) {
            int lb = 0;
            win_token_row(g, k.b, k.wi_t, k.wi_h, k.wi_w, n, &lb);
            v = (rel_code(n, fw) << 4) | lb;
        }
        cl[n] = v;
    }
}

// stage every slot's row maximum and weight of this head (the normaliser kernel's), all loads before the first write
__device__ __forceinline__ void stage_mw(const float* __restrict__ mbuf, const float* __restrict__ wbuf, int64_t ntok,
                                         const WinGeom& g, const Block& k, int vol, int NP, float* mrow, float* wrow) {
    constexpr int NR = (NPMAX + NT - 1) / NT;
    float mv[NR], wv[NR];
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const int n = threadIdx.x + NT * j;
        mv[j] = 0.f;  // a padded slot: weight 0 (and its region matches no key's)
        wv[j] = 0.f;
        if (n < vol) {
            const int64_t row = win_token_row(g, k.b, k.wi_t, k.wi_h, k.wi_w, n, nullptr);
            mv[j] = mbuf[(int64_t)k.head * ntok + row];
            wv[j] = wbuf[(int64_t)k.head * ntok + row];
        }
    }
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const int n = threadIdx.x + NT * j;
        if (n < NP) {
            mrow[n] = mv[j];
            wrow[n] = wv[j];
        }
    }
}

__global__ void __launch_bounds__(NT)
window_rollout_norm_kernel(const uint16_t* __restrict__ qkv, int64_t ld, WinGeom g, FullWin fw, int heads, int vol, int NP,
                           const float* __restrict__ table, int ntab, const float* __restrict__ rin, int64_t ntok,
                           float* __restrict__ mbuf, float* __restrict__ wbuf) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Ks = smem;
    float* tab = reinterpret_cast<float*>(smem + (int64_t)NP * 64);
    int* cl = reinterpret_cast<int*>(tab + (ntab + 3) / 4 * 4);
    const Block k = decode_block(g, heads, (NP + 32 * WAVES - 1) / (32 * WAVES));
    const int C = heads * 32;
    stage(qkv, ld, C, g, fw, k, heads, vol, NP, table, ntab, Ks, tab, cl);
    __syncthreads();  // the only barrier: a wave without queries leaves after it

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, rr = lane & 31, h = lane >> 5;
    const int qb = k.spl * WAVES + wave;
    if (qb * 32 >= vol) return;
    const int qn = qb * 32 + rr;  // this lane's query (window-local); both lanes of a pair hold the same one
    const bool valid = qn < vol;
    const int64_t qrow = win_token_row(g, k.b, k.wi_t, k.wi_h, k.wi_w, valid ? qn : vol - 1, nullptr);
    v8bf qf[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
        qf[kk] = __builtin_bit_cast(v8bf, *reinterpret_cast<const v8s*>(qkv + qrow * ld + k.head * 32 + 16 * kk + 8 * h));
    const int clq = valid ? cl[qn] : LAB_NONE;
    const int labq = clq & 15;
    const int iq = (clq >> 4) + rel_code_max(fw);  // idx(q, k) = code(q) - code(k) + code_max
    int koff[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) koff[kk] = rr * 64 + kchunk_swz(rr, 2 * kk + h) * 16;

    // S^T block: reg 4g + e of lane (rr, h) = key 8g + 4h + e of the block, query rr.  The lane's half of the keys
    // keeps its own running maximum and sum; the two halves merge at the end.
    float m = -1e30f, l = 0.f;
    const int nkb = (vol + 31) / 32;
    for (int kb = 0; kb < nkb; ++kb) {
        v16f sc = v16f{};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const v8bf kf = __builtin_bit_cast(v8bf, *reinterpret_cast<const v8s*>(Ks + kb * 32 * 64 + koff[kk]));
            sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[kk], sc, 0, 0, 0);
        }
        float s[16];
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int4 c4 = *reinterpret_cast<const int4*>(cl + kb * 32 + 8 * g4 + 4 * h);
            const int ck[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
                s[4 * g4 + e] = (ck[e] & 15) == labq ? sc[4 * g4 + e] + tab[iq - (ck[e] >> 4)] : -INFINITY;
        }
        float bm = fmaxf(s[0], s[1]);
#pragma unroll
        for (int e = 2; e < 16; ++e) bm = fmaxf(bm, s[e]);
        const float mn = fmaxf(m, bm);
        float p[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) p[e] = __builtin_amdgcn_exp2f(s[e] - mn);
        const float sum = (((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]))) +
                          (((p[8] + p[9]) + (p[10] + p[11])) + ((p[12] + p[13]) + (p[14] + p[15])));
        l = l * __builtin_amdgcn_exp2f(m - mn) + sum;
        m = mn;
    }
    // a real token always shares its region with itself, so its merged l >= 1
    const float mo = __shfl_xor(m, 32, 64), lo = __shfl_xor(l, 32, 64);
    const float M = fmaxf(m, mo);
    const float L = l * __builtin_amdgcn_exp2f(m - M) + lo * __builtin_amdgcn_exp2f(mo - M);
    if (h == 0 && valid) {
        mbuf[(int64_t)k.head * ntok + qrow] = M;
        wbuf[(int64_t)k.head * ntok + qrow] = rin[qrow] / L;
    }
}

// GRAD (the gradient-weighted step): a dO image after the Q' image (LDS: Q' rows, dO rows, table, cl, mrow, wrow), the
// lane's v row in registers beside its k row, and a second MFMA chain dP = dO . V^T in the registers of S
template <bool GRAD>
__global__ void __launch_bounds__(NT)
window_rollout_cols_kernel(const uint16_t* __restrict__ qkv, int64_t ld, [[maybe_unused]] const uint16_t* __restrict__ dout,
                           [[maybe_unused]] int64_t lddo, WinGeom g, FullWin fw, int heads, int vol, int NP,
                           const float* __restrict__ table, int ntab, const float* __restrict__ mbuf,
                           const float* __restrict__ wbuf, int64_t ntok, float* __restrict__ work) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Qs = smem;
    [[maybe_unused]] char* Ds = smem + (int64_t)NP * 64;
    float* tab = reinterpret_cast<float*>(smem + (int64_t)NP * (GRAD ? 128 : 64));
    int* cl = reinterpret_cast<int*>(tab + (ntab + 3) / 4 * 4);
    float* mrow = reinterpret_cast<float*>(cl + NP);
    float* wrow = mrow + NP;
    const Block k = decode_block(g, heads, (NP + 32 * WAVES - 1) / (32 * WAVES));
    const int C = heads * 32;
    stage(qkv, ld, 0, g, fw, k, heads, vol, NP, table, ntab, Qs, tab, cl);
    if constexpr (GRAD) stage_rows(dout, lddo, 0, g, k, vol, NP, Ds);
    stage_mw(mbuf, wbuf, ntok, g, k, vol, NP, mrow, wrow);
    __syncthreads();  // the only barrier: a wave without keys leaves after it

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, rr = lane & 31, h = lane >> 5;
    const int jb = k.spl * WAVES + wave;
    if (jb * 32 >= vol) return;
    const int kn = jb * 32 + rr;  // this lane's key (window-local)
    const bool valid = kn < vol;
    const int64_t krow = win_token_row(g, k.b, k.wi_t, k.wi_h, k.wi_w, valid ? kn : vol - 1, nullptr);
    v8bf kf[2];
    [[maybe_unused]] v8bf vf[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const uint16_t* p = qkv + krow * ld + k.head * 32 + 16 * kk + 8 * h;
        kf[kk] = __builtin_bit_cast(v8bf, *reinterpret_cast<const v8s*>(p + C));
        if constexpr (GRAD) vf[kk] = __builtin_bit_cast(v8bf, *reinterpret_cast<const v8s*>(p + 2 * C));
    }
    const int clk = valid ? cl[kn] : LAB_NONE;
    const int labk = clk & 15;
    const int jk = rel_code_max(fw) - (clk >> 4);
    int qoff[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) qoff[kk] = rr * 64 + kchunk_swz(rr, 2 * kk + h) * 16;

    // S (and dP) block: reg 4g + e of lane (rr, h) = query 8g + 4h + e of the block, key rr; the queries in window order
    float u = 0.f;
    const int nqb = (vol + 31) / 32;
    for (int ib = 0; ib < nqb; ++ib) {
        v16f sc = v16f{};
        [[maybe_unused]] v16f dp = v16f{};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const v8bf qf = __builtin_bit_cast(v8bf, *reinterpret_cast<const v8s*>(Qs + ib * 32 * 64 + qoff[kk]));
            sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf, kf[kk], sc, 0, 0, 0);
            if constexpr (GRAD) {
                const v8bf df = __builtin_bit_cast(v8bf, *reinterpret_cast<const v8s*>(Ds + ib * 32 * 64 + qoff[kk]));
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(df, vf[kk], dp, 0, 0, 0);
            }
        }
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int i0 = ib * 32 + 8 * g4 + 4 * h;
            const int4 c4 = *reinterpret_cast<const int4*>(cl + i0);
            const float4 m4 = *reinterpret_cast<const float4*>(mrow + i0);
            const float4 w4 = *reinterpret_cast<const float4*>(wrow + i0);
            const int cq[4] = {c4.x, c4.y, c4.z, c4.w};
            const float mi[4] = {m4.x, m4.y, m4.z, m4.w}, wi[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool on = (cq[e] & 15) == labk;
                const float s = on ? sc[4 * g4 + e] + tab[(cq[e] >> 4) + jk] : -INFINITY;
                if constexpr (GRAD) {
                    // an excluded pair (another region, a padded slot, a lane without a key) adds an exact 0 whatever
                    // its dP.  The two forms differ on purpose: each keeps the bits it always had.
                    const float d = on ? fmaxf(dp[4 * g4 + e], 0.f) : 0.f;
                    u = __builtin_fmaf(wi[e] * __builtin_amdgcn_exp2f(s - mi[e]), d, u);
                } else {
                    u = __builtin_fmaf(wi[e], __builtin_amdgcn_exp2f(s - mi[e]), u);
                }
            }
        }
    }
    u += __shfl_xor(u, 32, 64);  // the pair's two halves of the queries (a + b == b + a: the same bits in both lanes)
    if (h == 0 && valid) work[(int64_t)k.head * ntok + krow] = u;
}

// a_out[n] = alpha * (sum_h work[h][n]) / heads + beta * a_in[n].  GRAD: beta is given and, with base and r_out (both or
// neither), r_out = a_out + base.  The plain step forms 1 - alpha here and keeps an expression of its own: it compiles
// to two products and a sum, the beta form to a product and an FMA, so one expression for both would change its bits.
template <bool GRAD>
__global__ void __launch_bounds__(256) window_rollout_finish(const float* __restrict__ work, const float* __restrict__ ain,
                                                            [[maybe_unused]] const float* __restrict__ base, int64_t ntok,
                                                            int heads, float alpha, [[maybe_unused]] float beta,
                                                            float* __restrict__ aout,
                                                            [[maybe_unused]] float* __restrict__ rout) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= ntok) return;
    float a = 0.f;
    for (int h = 0; h < heads; ++h) a += work[(int64_t)h * ntok + n];  // heads in head order
    if constexpr (GRAD) {
        const float o = alpha * (a / (float)heads) + beta * ain[n];
        aout[n] = o;
        if (rout) rout[n] = o + base[n];
    } else {
        aout[n] = alpha * (a / (float)heads) + (1.0f - alpha) * ain[n];
    }
}

// child (bt, h, w) of parent (bt, h / 2, w / 2): the parent's relevance over the number of its children that exist
__global__ void __launch_bounds__(256) merge_spread_kernel(const float* __restrict__ rp, int64_t nchild, int H, int W,
                                                          float* __restrict__ rc) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= nchild) return;
    const int H2 = (H + 1) / 2, W2 = (W + 1) / 2;
    const int w = (int)(n % W), h = (int)((n / W) % H);
    const int64_t bt = n / ((int64_t)W * H);
    const int i = h >> 1, j = w >> 1;
    const int cnt = ((2 * i + 1 < H) ? 2 : 1) * ((2 * j + 1 < W) ? 2 : 1);
    rc[n] = rp[(bt * H2 + i) * W2 + j] / (float)cnt;
}

static bool overlap(const float* a, int64_t na, const float* b, int64_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)nb * 4 && b0 < a0 + (uintptr_t)na * 4;
}

// what a step entry derives from its arguments
struct Step {
    int vol, NP, ntab;
    int64_t lds, glds, ntok, nblk;
    WinGeom g;
    FullWin fw;
};

// The validation and the geometry the two step entries share; `me` names the entry in the messages.  `need`: the f32
// pointers that must be given; base / r_out: the gradient step's optional pair (null in the plain step, which lists
// its r_out in `need`); dout / lddo are looked at when `grad`.  Aliasing is each entry's own.
static int step_setup(const char* me, bool grad, const uint16_t* qkv, int64_t ld, const uint16_t* dout, int64_t lddo,
                      std::initializer_list<const float*> need, const float* base, const float* r_out, int64_t B,
                      int64_t T, int64_t H, int64_t W, int64_t heads, int64_t head_dim, int wt, int wh, int ww, int st,
                      int sh, int sw, int full_t, int full_h, int full_w, int64_t work_elems, Step& s) {
    auto bad = [&](int code, const char* what) { return fail(code, std::string(me) + ": " + what); };
    bool null = !qkv || (grad && !dout);
    uintptr_t f32 = (uintptr_t)base | (uintptr_t)r_out;
    for (const float* p : need) {
        null |= !p;
        f32 |= (uintptr_t)p;
    }
    if (null) return bad(VC_ERR_INVALID_ARG, "null pointer");
    if (!base != !r_out) return bad(VC_ERR_INVALID_ARG, "base and r_out come together (both null or both given)");
    if (head_dim != 32) return bad(VC_ERR_UNSUPPORTED, "head_dim must be 32");
    if (B <= 0 || T <= 0 || H <= 0 || W <= 0 || heads <= 0 || T >= (1 << 20) || H >= (1 << 20) || W >= (1 << 20) ||
        heads > 65535 || ld < 3 * heads * 32 || ld % 8 || (grad && (lddo < heads * 32 || lddo % 8)))
        return bad(VC_ERR_INVALID_ARG, "bad shape / leading dimension");
    if (wt <= 0 || wh <= 0 || ww <= 0 || T % wt || H % wh || W % ww)
        return bad(VC_ERR_UNSUPPORTED, "the token grid must be whole windows (no padding)");
    if (st < 0 || sh < 0 || sw < 0 || st >= wt || sh >= wh || sw >= ww)
        return bad(VC_ERR_INVALID_ARG, "shift must be in [0, window)");
    if (wt > full_t || wh > full_h || ww > full_w) return bad(VC_ERR_INVALID_ARG, "window larger than the full window");
    if ((int64_t)full_t * full_h * full_w > NPMAX) return bad(VC_ERR_UNSUPPORTED, "full window volume > 448");
    if ((((uintptr_t)qkv) | ((uintptr_t)dout)) & 15)
        return bad(VC_ERR_INVALID_ARG, grad ? "qkv and dout must be 16-byte aligned" : "qkv must be 16-byte aligned");
    if (f32 & 3) return bad(VC_ERR_INVALID_ARG, "f32 pointers must be 4-byte aligned");
    s.vol = wt * wh * ww;
    s.NP = (s.vol + 63) / 64 * 64;
    const int64_t ntab = (int64_t)(2 * full_t - 1) * (2 * full_h - 1) * (2 * full_w - 1);
    s.ntab = (int)ntab;
    s.lds = lds_bytes(s.NP, ntab);
    s.glds = grad_lds_bytes(s.NP, ntab);
    // the gradient step's second bound is a guard for a larger NPMAX only: at a full-window volume <= 448 the table has
    // < 3584 entries and glds stays under 78 KB, so today the volume check above is the one that refuses an oversized window
    if (s.lds > LDS_MAX || (grad && s.glds > GLDS_MAX))
        return bad(VC_ERR_UNSUPPORTED, grad ? "the window's q' and dO rows and the table column exceed the LDS"
                                            : "the window's rows and the table column exceed the LDS");
    if (T * H * W >= (1LL << 31) / B) return bad(VC_ERR_INVALID_ARG, "grid too large");
    s.ntok = B * T * H * W;
    s.nblk = s.ntok / s.vol * heads * ((s.NP + 32 * WAVES - 1) / (32 * WAVES));  // (window, head, 128 rows)
    if (s.nblk > 0x7fffffff) return bad(VC_ERR_INVALID_ARG, "grid too large");
    if (work_elems < 3 * heads * s.ntok) return bad(VC_ERR_INVALID_ARG, "work too small (3 * heads * B*T*H*W floats)");
    s.g = WinGeom{(int)T, (int)H, (int)W, wt, wh, ww, st, sh, sw, (int)(T / wt), (int)(H / wh), (int)(W / ww)};
    s.fw = FullWin{full_t, full_h, full_w};
    return 0;
}

// the three launches; dout given: the gradient-weighted column kernel
static int step_launch(const char* me, const Step& s, const uint16_t* qkv, int64_t ld, const uint16_t* dout, int64_t lddo,
                       const float* table, const float* r_in, const float* a_in, const float* base, int heads, float alpha,
                       float beta, float* work, float* a_out, float* r_out, hipStream_t stream) {
    static bool attr_set = false;  // benign race (idempotent)
    if (dout && s.glds > 64 * 1024 && !attr_set) {
        hipError_t e = hipFuncSetAttribute((const void*)window_rollout_cols_kernel<true>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)GLDS_MAX);
        if (e != hipSuccess) return fail((int)e, std::string(me) + ": hipFuncSetAttribute: " + hipGetErrorString(e));
        attr_set = true;
    }
    const unsigned nblk = (unsigned)s.nblk;
    float* mbuf = work + heads * s.ntok;
    float* wbuf = work + 2 * heads * s.ntok;
    window_rollout_norm_kernel<<<nblk, NT, (size_t)s.lds, stream>>>(qkv, ld, s.g, s.fw, heads, s.vol, s.NP, table, s.ntab,
                                                                    r_in, s.ntok, mbuf, wbuf);
    int rc = check_launch(me);
    if (rc) return rc;
    if (dout)
        window_rollout_cols_kernel<true><<<nblk, NT, (size_t)s.glds, stream>>>(
            qkv, ld, dout, lddo, s.g, s.fw, heads, s.vol, s.NP, table, s.ntab, mbuf, wbuf, s.ntok, work);
    else
        window_rollout_cols_kernel<false><<<nblk, NT, (size_t)s.lds, stream>>>(
            qkv, ld, nullptr, 0, s.g, s.fw, heads, s.vol, s.NP, table, s.ntab, mbuf, wbuf, s.ntok, work);
    rc = check_launch(me);
    if (rc) return rc;
    const unsigned nfin = (unsigned)((s.ntok + 255) / 256);
    if (dout)
        window_rollout_finish<true><<<nfin, 256, 0, stream>>>(work, a_in, base, s.ntok, heads, alpha, beta, a_out, r_out);
    else
        window_rollout_finish<false><<<nfin, 256, 0, stream>>>(work, a_in, nullptr, s.ntok, heads, alpha, 0.f, a_out, nullptr);
    return check_launch(me);
}

}  // namespace wroll
}  // namespace vc

using namespace vc;
using namespace vc::wroll;

extern "C" int vc_window_rollout_step(const uint16_t* qkv, int64_t ld, const float* table, const float* r_in, int64_t B,
                                      int64_t T, int64_t H, int64_t W, int64_t heads, int64_t head_dim, int wt, int wh,
                                      int ww, int st, int sh, int sw, int full_t, int full_h, int full_w, float alpha,
                                      float* work, int64_t work_elems, float* r_out, hipStream_t stream) {
    const char* me = "vc_window_rollout_step";
    Step s;
    if (int rc = step_setup(me, false, qkv, ld, nullptr, 0, {table, r_in, work, r_out}, nullptr, nullptr, B, T, H, W, heads,
                            head_dim, wt, wh, ww, st, sh, sw, full_t, full_h, full_w, work_elems, s))
        return rc;
    if (overlap(r_out, s.ntok, r_in, s.ntok)) return fail(VC_ERR_INVALID_ARG, std::string(me) + ": r_out must not alias r_in");
    if (overlap(work, work_elems, r_in, s.ntok) || overlap(work, work_elems, r_out, s.ntok))
        return fail(VC_ERR_INVALID_ARG, std::string(me) + ": work must not alias r_in or r_out");
    // the finish kernel with r_in / r_out for a_in / a_out
    return step_launch(me, s, qkv, ld, nullptr, 0, table, r_in, r_in, nullptr, (int)heads, alpha, 0.f, work, r_out, nullptr,
                       stream);
}

extern "C" int vc_window_grad_rollout_step(const uint16_t* qkv, int64_t ld, const uint16_t* dout, int64_t lddo,
                                           const float* table, const float* r_in, const float* a_in, const float* base,
                                           int64_t B, int64_t T, int64_t H, int64_t W, int64_t heads, int64_t head_dim,
                                           int wt, int wh, int ww, int st, int sh, int sw, int full_t, int full_h,
                                           int full_w, float alpha, float beta, float* work, int64_t work_elems,
                                           float* a_out, float* r_out, hipStream_t stream) {
    const char* me = "vc_window_grad_rollout_step";
    auto bad = [&](const char* what) { return fail(VC_ERR_INVALID_ARG, std::string(me) + ": " + what); };
    Step s;
    if (int rc = step_setup(me, true, qkv, ld, dout, lddo, {table, r_in, a_in, work, a_out}, base, r_out, B, T, H, W, heads,
                            head_dim, wt, wh, ww, st, sh, sw, full_t, full_h, full_w, work_elems, s))
        return rc;
    const int64_t ntok = s.ntok;
    const float* ins[3] = {r_in, a_in, base};
    float* outs[2] = {a_out, r_out};
    for (float* o : outs) {
        if (!o) continue;
        for (const float* i : ins)
            if (i && overlap(o, ntok, i, ntok)) return bad("a_out / r_out must not alias r_in, a_in or base");
        if (overlap(work, work_elems, o, ntok)) return bad("work must not alias an input or an output");
    }
    for (const float* i : ins)
        if (i && overlap(work, work_elems, i, ntok)) return bad("work must not alias an input or an output");
    if (r_out && overlap(a_out, ntok, r_out, ntok)) return bad("a_out must not alias r_out");
    return step_launch(me, s, qkv, ld, dout, lddo, table, r_in, a_in, base, (int)heads, alpha, beta, work, a_out, r_out,
                       stream);
}

extern "C" int vc_merge_rollout_spread(const float* r_parent, int64_t B, int64_t T, int64_t H, int64_t W, float* r_child,
                                       hipStream_t stream) {
    if (!r_parent || !r_child) return fail(VC_ERR_INVALID_ARG, "vc_merge_rollout_spread: null pointer");
    if ((((uintptr_t)r_parent) | ((uintptr_t)r_child)) & 3)
        return fail(VC_ERR_INVALID_ARG, "vc_merge_rollout_spread: f32 pointers must be 4-byte aligned");
    if (B <= 0 || T <= 0 || H <= 0 || W <= 0 || T >= (1 << 20) || H >= (1 << 20) || W >= (1 << 20) ||
        T * H * W >= (1LL << 31) / B)
        return fail(VC_ERR_INVALID_ARG, "vc_merge_rollout_spread: bad shape");
    const int64_t nchild = B * T * H * W, nparent = B * T * ((H + 1) / 2) * ((W + 1) / 2);
    if (overlap(r_child, nchild, r_parent, nparent))
        return fail(VC_ERR_INVALID_ARG, "vc_merge_rollout_spread: r_child must not alias r_parent");
    merge_spread_kernel<<<(unsigned)((nchild + 255) / 256), 256, 0, stream>>>(r_parent, nchild, (int)H, (int)W, r_child);
    return check_launch("vc_merge_rollout_spread");
}
