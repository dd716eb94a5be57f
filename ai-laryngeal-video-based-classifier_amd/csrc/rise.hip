// The device work of RISE saliency (vclip_amd/rise.py; Petsiuk et al. 2018): the clip batch under F smooth random
// masks, and the score-weighted sum of those masks.
//
// The mask.  Mask f is a bit grid g_f uint8 [ct+2, ch+2, cw+2] and a shift (dt, dy, dx), both drawn on the host.  With
// the cell sizes St = ceil(T/ct), Sh, Sw, pixel (t, y, x) has u = t + dt, i = u / St, ft = float(u % St) / float(St)
// (one IEEE division), likewise (j, fy) and (k, fx), and
//     m_f(t, y, x) = the trilinear interpolation of the eight bits g_f[i..i+1][j..j+1][k..k+1],
// along x (four steps), then y (two), then t (one), each step fmaf(f, b - a, a).  i + 1 <= ct + 1 because
// u <= T - 1 + St - 1 < (ct + 1) * St.  Where the eight bits are equal every step returns that bit exactly.
//
// No division runs per mask.  A lane splits t, y and x into cell and remainder once, before the mask loop, and keeps
// the remainders and the grid offset of its unshifted corner; since 0 <= d < S, the shifted remainder is r + d or
// r + d - S, and the corner moves by one plane, row or column when it wraps.  The fractions float(r) / float(S),
// r = 0..S-1 of the three axes, are divided once per workgroup into an LDS table (St + Sh + Sw <= 4096 entries).
//
// Both kernels take four consecutive floats per lane (16-byte accesses when the element count is a multiple of 4
// and the pointers are 16-byte aligned, one float per lane otherwise; a quad may straddle rows: every float finds its
// own pixel, and the floats of one row share ft, fy and the row's wrap) and loop over the masks in rounds of
// `tile` = min(RISE_TILE, LDS_GRID / grid points) masks: the workgroup copies the round's bit grids, as floats, and
// shifts into LDS, then every lane walks the round's masks in index order reading its corners from LDS.  The grids
// are kept as floats so that the corner reads are aligned dwords (k and k + 1 in one ds_read2_b32): with the grids as
// bytes in LDS the same loops ran 4.3 x slower at every VALU count tried, the one- and two-byte LDS reads setting the
// pace.  The tile (8 masks at (4, 7, 7) cells) only sets how often LDS is refilled; no result depends on it.  33 KB of
// LDS and 104 / 112 VGPRs: four workgroups per CU.
//
// vc_rise_apply: out[f][b][.] = fmaf(m, x, (1 - m) * z) (base z) or m * x (no base), one read of clip and base, F
// stores.  Bound: vector instruction issue, not the F * n * 4 bytes it writes: the counters give 191 VALU and 26 LDS
// wave-instructions per wave and mask (256 floats written) and no LDS bank conflict, and at ViViT's 32 x 3 x 224^2 clip
// the launch stores 2.5 to 2.75 TB/s.  Each 1024-float workgroup also re-reads the round's grids
// (3.9 KB at (4, 7, 7) cells) from L2 per 32 KB it writes.
//
// vc_rise_accumulate: a = acc; for f in 0..F-1: a = fmaf(w[f][b], m_f, a); acc = a.  One lane owns a pixel for the
// whole launch, the masks come in index order and nothing is atomic, so F masks in one launch or in any split into
// consecutive launches give the same bits, as do two runs, and clip b's sums do not depend on B.  Bound: instruction
// issue (the same interpolation against 8 bytes of HBM traffic per pixel and launch); w[f][b] is a wave-uniform global
// read except where a wave straddles two clips.
#include "common.hpp"

namespace vc {
namespace rise {

constexpr int RISE_TILE = 32;        // masks per staging round at most (vc_rise_mask_tile reports it to the tests)
constexpr int LDS_GRID = 4096;       // grid points per round, held as floats (16 KB); one grid must fit
constexpr int LDS_FRAC = 4096;       // entries of the fraction table: St + Sh + Sw must fit

struct Geom {
    unsigned T, C, H, W;     // the clip; C = 1 for the accumulator [B, T, H, W]
    unsigned St, Sh, Sw;     // cell sizes
    unsigned gh, gw, G;      // grid rows (ch+2), columns (cw+2) and bytes per mask (ct+2)*gh*gw
    int layout;              // 0: [B,T,C,H,W]  1: [B,C,T,H,W]
};

// a pixel before the shift: the remainders of t = it*St + rt, y and x, the grid offset (it*gh + iy)*gw + ix of its
// corner, and its clip
struct Pix {
    unsigned rt, ry, rx, at, b;
    bool first;  // of its row within the lane's quad: the row part of the mask is computed here and reused after
};

__device__ __forceinline__ void split_row(const Geom& g, unsigned r, Pix& p) {  // r = flat index / W
    const unsigned y = r % g.H;
    unsigned q = r / g.H, t;
    if (g.layout == 0) {
        q /= g.C;
        t = q % g.T;
        p.b = q / g.T;
    } else {
        t = q % g.T;
        p.b = q / g.T / g.C;
    }
    const unsigned it = t / g.St, iy = y / g.Sh;
    p.rt = t - it * g.St;
    p.ry = y - iy * g.Sh;
    p.at = (it * g.gh + iy) * g.gw;  // split_col adds the column
}

template <int V>
__device__ __forceinline__ void split(const Geom& g, uint64_t i, Pix (&p)[V]) {
    unsigned r = (unsigned)(i / g.W), col = (unsigned)(i - (uint64_t)r * g.W);
    unsigned row_at;
    split_row(g, r, p[0]);
    row_at = p[0].at;
    p[0].first = true;
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const unsigned ix = col / g.Sw;
        p[e].rx = col - ix * g.Sw;
        p[e].at = row_at + ix;
        if (e + 1 < V) {
            p[e + 1] = p[e];
            p[e + 1].first = ++col == g.W;
            if (p[e + 1].first) {  // the quad runs into the next row
                col = 0;
                split_row(g, ++r, p[e + 1]);
                row_at = p[e + 1].at;
            }
        }
    }
}

// remainder r0 < S shifted by d < S: the new remainder, and whether the cell index went up by one
__device__ __forceinline__ unsigned shifted(unsigned r0, unsigned d, unsigned S, bool& wrapped) {
    const unsigned r = r0 + d;
    wrapped = r >= S;
    return wrapped ? r - S : r;
}

__device__ __forceinline__ float lerp(float f, float a, float b) { return __builtin_fmaf(f, b - a, a); }

// what the pixels of one row share under one mask: ft, fy and how far the wraps along t and y move the corner
struct RowPart {
    unsigned off;
    float ft, fy;
};

// frac: the table, [St | Sh | Sw] entries float(r) / float(S)
__device__ __forceinline__ RowPart row_part(const Geom& g, const float* frac, const int* sh, const Pix& p) {
    bool wt, wy;
    RowPart r;
    r.ft = frac[shifted(p.rt, (unsigned)sh[0], g.St, wt)];
    r.fy = frac[g.St + shifted(p.ry, (unsigned)sh[1], g.Sh, wy)];
    r.off = (wt ? g.gh * g.gw : 0u) + (wy ? g.gw : 0u);
    return r;
}

__device__ __forceinline__ float mask_at(const Geom& g, const float* frac, const float* grid, const int* sh,
                                         const RowPart& r, const Pix& p) {
    bool wx;
    const float fx = frac[g.St + g.Sh + shifted(p.rx, (unsigned)sh[2], g.Sw, wx)];
    const float* c = grid + p.at + r.off + (wx ? 1u : 0u);
    const unsigned row = g.gw, plane = g.gh * g.gw;
    const float a00 = lerp(fx, c[0], c[1]);
    const float a01 = lerp(fx, c[row], c[row + 1]);
    const float a10 = lerp(fx, c[plane], c[plane + 1]);
    const float a11 = lerp(fx, c[plane + row], c[plane + row + 1]);
    return lerp(r.ft, lerp(r.fy, a00, a01), lerp(r.fy, a10, a11));
}

// once per workgroup: the fractions of the three axes, each one IEEE division (the first barrier of stage() follows)
__device__ __forceinline__ void fill_fractions(const Geom& g, float* frac) {
    const unsigned nt = g.St, ny = g.St + g.Sh, nx = ny + g.Sw;
    for (unsigned j = threadIdx.x; j < nx; j += 256) {
        const unsigned r = j < nt ? j : (j < ny ? j - nt : j - ny), S = j < nt ? g.St : (j < ny ? g.Sh : g.Sw);
        frac[j] = (float)r / (float)S;
    }
}

// the round's nf bit grids, as 0.0f / 1.0f, and shifts into LDS; the barrier in front keeps the previous round's
// readers ahead of it
__device__ __forceinline__ void stage(const uint8_t* __restrict__ bits, const int* __restrict__ shifts, unsigned G,
                                      int nf, float* sgrid, int* sshift) {
    __syncthreads();
    const unsigned points = (unsigned)nf * G;
    for (unsigned j = threadIdx.x; j < points; j += 256) sgrid[j] = (float)bits[j];
    for (unsigned j = threadIdx.x; j < (unsigned)nf * 3; j += 256) sshift[j] = shifts[j];
    __syncthreads();
}

template <int V>
__global__ void __launch_bounds__(256) rise_apply_kernel(const float* __restrict__ clip, const float* __restrict__ base,
                                                         const uint8_t* __restrict__ bits,
                                                         const int* __restrict__ shifts, Geom g, unsigned n, int F,
                                                         int tile, float* __restrict__ out) {
    __shared__ float sgrid[LDS_GRID];
    __shared__ float frac[LDS_FRAC];
    __shared__ int sshift[RISE_TILE * 3];
    const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
    const bool live = i < n;  // n % V == 0: a lane is all inside or all outside; outside lanes only help staging
    float x[V], z[V] = {};
    Pix p[V];
    if (live) {
        if constexpr (V == 4) {
            const v4f a = *reinterpret_cast<const v4f*>(clip + i);
            x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
            if (base) {
                const v4f c = *reinterpret_cast<const v4f*>(base + i);
                z[0] = c.x; z[1] = c.y; z[2] = c.z; z[3] = c.w;
            }
        } else {
            x[0] = clip[i];
            if (base) z[0] = base[i];
        }
        split<V>(g, i, p);
    }
    fill_fractions(g, frac);
    for (int f0 = 0; f0 < F; f0 += tile) {
        const int nf = F - f0 < tile ? F - f0 : tile;
        stage(bits + (uint64_t)f0 * g.G, shifts + (uint64_t)f0 * 3, g.G, nf, sgrid, sshift);
        if (!live) continue;
        for (int f = 0; f < nf; ++f) {
            const float* grid = sgrid + (unsigned)f * g.G;
            const int* sh = sshift + f * 3;
            float y[V];
            RowPart rp;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                if (p[e].first) rp = row_part(g, frac, sh, p[e]);
                const float m = mask_at(g, frac, grid, sh, rp, p[e]);
                y[e] = base ? __builtin_fmaf(m, x[e], (1.0f - m) * z[e]) : m * x[e];
            }
            float* dst = out + (uint64_t)(f0 + f) * n + i;
            if constexpr (V == 4) {
                const v4f o = {y[0], y[1], y[2], y[3]};
                *reinterpret_cast<v4f*>(dst) = o;
            } else {
                dst[0] = y[0];
            }
        }
    }
}

template <int V>
__global__ void __launch_bounds__(256) rise_accumulate_kernel(const uint8_t* __restrict__ bits,
                                                              const int* __restrict__ shifts,
                                                              const float* __restrict__ w, Geom g, unsigned n, unsigned B,
                                                              int F, int tile, float* __restrict__ acc) {
    __shared__ float sgrid[LDS_GRID];
    __shared__ float frac[LDS_FRAC];
    __shared__ int sshift[RISE_TILE * 3];
    const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
    const bool live = i < n;
    float a[V];
    Pix p[V];
    if (live) {
        if constexpr (V == 4) {
            const v4f c = *reinterpret_cast<const v4f*>(acc + i);
            a[0] = c.x; a[1] = c.y; a[2] = c.z; a[3] = c.w;
        } else {
            a[0] = acc[i];
        }
        split<V>(g, i, p);
    }
    fill_fractions(g, frac);
    for (int f0 = 0; f0 < F; f0 += tile) {
        const int nf = F - f0 < tile ? F - f0 : tile;
        stage(bits + (uint64_t)f0 * g.G, shifts + (uint64_t)f0 * 3, g.G, nf, sgrid, sshift);
        if (!live) continue;
        for (int f = 0; f < nf; ++f) {
            const float* grid = sgrid + (unsigned)f * g.G;
            const int* sh = sshift + f * 3;
            const float* wf = w + (uint64_t)(f0 + f) * B;
            RowPart rp;
            float wb;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                if (p[e].first) {  // the clip changes only where the row does
                    rp = row_part(g, frac, sh, p[e]);
                    wb = wf[p[e].b];
                }
                a[e] = __builtin_fmaf(wb, mask_at(g, frac, grid, sh, rp, p[e]), a[e]);
            }
        }
    }
    if (!live) return;
    if constexpr (V == 4) {
        const v4f o = {a[0], a[1], a[2], a[3]};
        *reinterpret_cast<v4f*>(acc + i) = o;
    } else {
        acc[i] = a[0];
    }
}

static bool overlap(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

// the checks both entry points share; fills g (layout and C are the caller's) and the tile
static const char* geometry(int64_t T, int64_t H, int64_t W, int64_t ct, int64_t ch, int64_t cw, int64_t F, Geom& g,
                            int& tile) {
    if (T <= 0 || H <= 0 || W <= 0 || F <= 0) return "bad shape (every extent and F must be positive)";
    if (ct <= 0 || ch <= 0 || cw <= 0 || ct > T || ch > H || cw > W)
        return "cells must be positive and no more than the clip's (T, H, W)";
    const int64_t lim = 1LL << 31;
    if (T >= lim || H >= lim || W >= lim || F >= lim) return "an extent of 2^31 or more is not supported";
    const int64_t G = (ct + 2) * (ch + 2) * (cw + 2);  // each factor < 2^31 + 2
    if (ct + 2 > LDS_GRID || ch + 2 > LDS_GRID || G > LDS_GRID)
        return "a bit grid of more than 4096 points (ct+2)*(ch+2)*(cw+2) is not supported";
    g.T = (unsigned)T; g.H = (unsigned)H; g.W = (unsigned)W;
    g.St = (unsigned)((T + ct - 1) / ct); g.Sh = (unsigned)((H + ch - 1) / ch); g.Sw = (unsigned)((W + cw - 1) / cw);
    if ((int64_t)g.St + g.Sh + g.Sw > LDS_FRAC)
        return "cell sizes ceil(T/ct) + ceil(H/ch) + ceil(W/cw) of more than 4096 are not supported";
    g.gh = (unsigned)(ch + 2); g.gw = (unsigned)(cw + 2); g.G = (unsigned)G;
    const int64_t fit = LDS_GRID / G;
    tile = (int)(fit < RISE_TILE ? fit : RISE_TILE);
    return nullptr;
}

}  // namespace rise
}  // namespace vc

using namespace vc;
using namespace vc::rise;

extern "C" int vc_rise_mask_tile(void) { return RISE_TILE; }

extern "C" int vc_rise_apply(const float* clip, const float* base, const uint8_t* bits, const int32_t* shifts, int64_t B,
                             int64_t C, int64_t T, int64_t H, int64_t W, int layout, int64_t ct, int64_t ch, int64_t cw,
                             int64_t F, float* out, hipStream_t stream) {
    if (!clip || !bits || !shifts || !out) return fail(VC_ERR_INVALID_ARG, "vc_rise_apply: null pointer");
    if (layout != 0 && layout != 1) return fail(VC_ERR_INVALID_ARG, "vc_rise_apply: unknown layout (0: BTCHW, 1: BCTHW)");
    if (B <= 0 || C <= 0) return fail(VC_ERR_INVALID_ARG, "vc_rise_apply: bad shape (B and C must be positive)");
    Geom g;
    int tile;
    if (const char* why = geometry(T, H, W, ct, ch, cw, F, g, tile))
        return fail(VC_ERR_INVALID_ARG, (std::string("vc_rise_apply: ") + why).c_str());
    const int64_t lim = 1LL << 31;
    if (B >= lim || C >= lim || B * C >= lim || B * C * T >= lim || B * C * T * H >= lim || B * C * T * H * W >= lim)
        return fail(VC_ERR_INVALID_ARG, "vc_rise_apply: a clip batch of 2^31 or more elements is not supported");
    const int64_t n = B * C * T * H * W;
    if ((((uintptr_t)clip) | ((uintptr_t)base) | ((uintptr_t)shifts) | ((uintptr_t)out)) & 3)
        return fail(VC_ERR_INVALID_ARG, "vc_rise_apply: clip, base, shifts and out must be 4-byte aligned");
    if (overlap(out, F * n * 4, clip, n * 4) || (base && overlap(out, F * n * 4, base, n * 4)) ||
        overlap(out, F * n * 4, bits, F * (int64_t)g.G) || overlap(out, F * n * 4, shifts, F * 12))
        return fail(VC_ERR_INVALID_ARG, "vc_rise_apply: out must not alias clip, base, bits or shifts");
    g.C = (unsigned)C;
    g.layout = layout;
    const bool vec = n % 4 == 0 && !((((uintptr_t)clip) | ((uintptr_t)base) | ((uintptr_t)out)) & 15);
    const int64_t lanes = vec ? n / 4 : n;
    const unsigned blocks = (unsigned)((lanes + 255) / 256);
    if (vec)
        rise_apply_kernel<4><<<blocks, 256, 0, stream>>>(clip, base, bits, shifts, g, (unsigned)n, (int)F, tile, out);
    else
        rise_apply_kernel<1><<<blocks, 256, 0, stream>>>(clip, base, bits, shifts, g, (unsigned)n, (int)F, tile, out);
    return check_launch("vc_rise_apply");
}

extern "C" int vc_rise_accumulate(const uint8_t* bits, const int32_t* shifts, const float* w, int64_t B, int64_t T,
                                  int64_t H, int64_t W, int64_t ct, int64_t ch, int64_t cw, int64_t F, float* acc,
                                  hipStream_t stream) {
    if (!bits || !shifts || !w || !acc) return fail(VC_ERR_INVALID_ARG, "vc_rise_accumulate: null pointer");
    if (B <= 0) return fail(VC_ERR_INVALID_ARG, "vc_rise_accumulate: bad shape (B must be positive)");
    Geom g;
    int tile;
    if (const char* why = geometry(T, H, W, ct, ch, cw, F, g, tile))
        return fail(VC_ERR_INVALID_ARG, (std::string("vc_rise_accumulate: ") + why).c_str());
    const int64_t lim = 1LL << 31;
    if (B >= lim || B * T >= lim || B * T * H >= lim || B * T * H * W >= lim || F * B >= lim)
        return fail(VC_ERR_INVALID_ARG, "vc_rise_accumulate: 2^31 or more pixels or weights are not supported");
    const int64_t n = B * T * H * W;
    if ((((uintptr_t)shifts) | ((uintptr_t)w) | ((uintptr_t)acc)) & 3)
        return fail(VC_ERR_INVALID_ARG, "vc_rise_accumulate: shifts, w and acc must be 4-byte aligned");
    if (overlap(acc, n * 4, bits, F * (int64_t)g.G) || overlap(acc, n * 4, shifts, F * 12) || overlap(acc, n * 4, w, F * B * 4))
        return fail(VC_ERR_INVALID_ARG, "vc_rise_accumulate: acc must not alias bits, shifts or w");
    g.C = 1;
    g.layout = 0;
    const bool vec = n % 4 == 0 && !(((uintptr_t)acc) & 15);
    const int64_t lanes = vec ? n / 4 : n;
    const unsigned blocks = (unsigned)((lanes + 255) / 256);
    if (vec)
        rise_accumulate_kernel<4><<<blocks, 256, 0, stream>>>(bits, shifts, w, g, (unsigned)n, (unsigned)B, (int)F, tile, acc);
    else
        rise_accumulate_kernel<1><<<blocks, 256, 0, stream>>>(bits, shifts, w, g, (unsigned)n, (unsigned)B, (int)F, tile, acc);
    return check_launch("vc_rise_accumulate");
}
