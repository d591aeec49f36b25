// Long-axis attention (33 <= L <= 128 along T, W or H): the contract of bf_attn_fwd / bf_attn_bwd (include/bubbleformer_hip.h) for
// sequences that do not fit the one-wave kernels of attn.hip / attn_mfma.hip.  attn.hip dispatches L > 32 here and nothing else.
//
// One workgroup (4 waves) per (sequence, head) problem, persistent over problems.  The whole L x L score matrix of a problem sits in LDS
// as fp32 ([LP][LP + 1], LP = L rounded up to 16); q / k / v / dO are streamed through LDS in 16-column slices of the head dim (16-byte
// global loads), the q / k LayerNorm and affine applied as a slice is staged.  LayerNorm statistics, softmax, the rescale
// A = fl32(1/L) + (P - fl32(1/L)) s_head and every sum of parameter gradients are fp32 in both dtypes (one thread per row for softmax,
// keys >= L masked, padded query rows zero).  The products S = qn kn^T d^-1/2, dA = dO V^T, O = A V, dV = A^T dO, dqn = dS kn and
// dkn = dS^T qn run
//   bf16 mode: on v_mfma_f32_16x16x16_bf16 (operands rounded to bf16 as they leave LDS, fp32 accumulate), 16 x 16 blocks spread over
//              the four waves, as the short-axis MFMA kernels do;
//   fp32 mode: on fp32 VALU, exact fp32 (the parity mode): scores as an (LP/16) x (LP/16) register tile per thread, the other products
//              one thread per (16-row group, slice column) with the key (or query) sum in order.
// The backward recomputes P, keeps P and dS in LDS, and runs the q / k LayerNorm backward from a full L x d plane of dqn (then dkn) in
// the LDS that P held.  Parameter gradients (q / k LayerNorm affine, T5 table, head scale) are summed per workgroup in LDS by ONE
// thread per value in problem order, and each workgroup leaves one row in the AttnReduceJob layout of param_reduce.h: the step stays
// bit-reproducible (no float atomics on shared addresses; with no workspace the rows are added to the gradients with atomics instead).
#include "lane_ops.h"
#include "param_reduce.h"

namespace {

constexpr int NTL = 256;            // threads per workgroup
constexpr int CW = 16, CLD = CW + 1;     // columns per staged slice, its LDS row pitch
constexpr int LONG_LMAX = 128, LONG_DMAX = 128;

struct LGeo { long nseq; int L; long inner, outer_stride, inner_stride, tok_stride; };
struct LPar { const float *qw, *qb, *kw, *kb, *emb, *hscale; };
struct LGrd { float *dqw, *dqb, *dkw, *dkb, *demb, *dhscale; };

__device__ __forceinline__ long lseq_base(const LGeo& g, long s) { return (s / g.inner) * g.outer_stride + (s % g.inner) * g.inner_stride; }

// LayerNorm statistics of the q rows (part 0) and k rows (part 1) of one problem, one thread per row (16-byte loads), in attn.hip's order
template <typename T>
__device__ __forceinline__ void row_stats(const T* __restrict__ qkv, long tok0, long ts, long rs3, int L, int d, float* mu, float* rs) {
    constexpr int CH = Chunk<T>::N;
    const int t = threadIdx.x;
    if (t < 2 * L) {
        const int part = t < L ? 0 : 1, l = t - part * L;
        const T* row = qkv + (tok0 + l * ts) * rs3 + part * d;
        float m = 0.f;
        for (int e0 = 0; e0 < d; e0 += CH) {
            Chunk<T> v;
            v.load(row + e0);
#pragma unroll
            for (int j = 0; j < CH; ++j) m += v.get(j);
        }
        m /= (float)d;
        float var = 0.f;
        for (int e0 = 0; e0 < d; e0 += CH) {
            Chunk<T> v;
            v.load(row + e0);
#pragma unroll
            for (int j = 0; j < CH; ++j) { const float u = v.get(j) - m; var += u * u; }
        }
        mu[part * LONG_LMAX + l] = m;
        rs[part * LONG_LMAX + l] = rsqrtf(var / (float)d + BF_IN_EPS);
    }
}

// columns [c0, c0 + 16) of LP rows into dst[LP][CLD] (fp32), 16-byte loads; rows >= L and columns >= d are zero.  With mu: the
// LayerNorm'd and affine-transformed value xhat * w + b, otherwise x * mul.
template <typename T>
__device__ __forceinline__ void stage(float* __restrict__ dst, const T* __restrict__ src, long row_stride, long tok0, long ts, int L, int LP, int d,
                                      int c0, const float* mu, const float* rs, const float* w, const float* b, float mul) {
    constexpr int CH = Chunk<T>::N, CPR = CW / CH;       // d is a multiple of the chunk: a chunk is all inside or all outside
    for (int idx = threadIdx.x; idx < LP * CPR; idx += NTL) {
        const int l = idx / CPR, c = (idx % CPR) * CH, e0 = c0 + c;
        float* o = dst + l * CLD + c;
        if (l < L && e0 < d) {
            Chunk<T> v;
            v.load(src + (tok0 + l * ts) * row_stride + e0);
#pragma unroll
            for (int j = 0; j < CH; ++j) {
                const float x = v.get(j);
                if (mu) { const float xh = (x - mu[l]) * rs[l]; o[j] = xh * w[e0 + j] + b[e0 + j]; }
                else o[j] = x * mul;
            }
        } else {
#pragma unroll
            for (int j = 0; j < CH; ++j) o[j] = 0.f;
        }
    }
}

// ---- bf16 mode: the products on v_mfma_f32_16x16x16_bf16 (fp32 accumulate).  Operand layout: lane = row (lane & 15) of A / column of
// B, k = 4 (lane >> 4) + 0..3; result element r of a lane = row 4 (lane >> 4) + r, column lane & 15.
__device__ __forceinline__ s16x4 pack4(const float (&v)[4]) {
    const bf16x4 p = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
    return __builtin_bit_cast(s16x4, p);
}
template <int NA> constexpr int blocks_per_wave() { return (NA * NA + 3) / 4; }

// acc += X Y^T over one staged slice, for the 16 x 16 output blocks b = wave + 4 t of the LP x LP result
template <int NA>
__device__ __forceinline__ void tile_nt_mfma(const float* __restrict__ X, const float* __restrict__ Y, f32x4 (&acc)[blocks_per_wave<NA>()], int wave,
                                             int lane) {
    const int r16 = lane & 15, g = lane >> 4;
#pragma unroll
    for (int t = 0; t < blocks_per_wave<NA>(); ++t) {
        const int b = wave + 4 * t;
        if (b < NA * NA) {
            const float* xr = X + (16 * (b / NA) + r16) * CLD + 4 * g;
            const float* yr = Y + (16 * (b % NA) + r16) * CLD + 4 * g;
            const float xa[4] = {xr[0], xr[1], xr[2], xr[3]}, ya[4] = {yr[0], yr[1], yr[2], yr[3]};
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(pack4(xa), pack4(ya), acc[t], 0, 0, 0);
        }
    }
}

// one 16 x 16 block of C[r][c] = sum_{k < LP} Mx(r, k) X[k][c], rows 16 bi.., the 16 slice columns: Mx = M (row-major [LP][LP + 1]) or, with
// ta, its transpose; with rescale the matrix entries p become 1/L + (p - 1/L) hs on the way (rows of X >= L are zero, so padded entries of
// M never count)
template <int NA>
__device__ __forceinline__ f32x4 mm_block(const float* __restrict__ M, const float* __restrict__ X, int bi, bool ta, bool rescale, float invL,
                                          float hs, int lane) {
    constexpr int LDM = 16 * NA + 1;
    const int r16 = lane & 15, g = lane >> 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < NA; ++kk) {
        float a[4], b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = 16 * kk + 4 * g + j;
            float v = ta ? M[k * LDM + 16 * bi + r16] : M[(16 * bi + r16) * LDM + k];
            a[j] = rescale ? (invL + (v - invL) * hs) : v;
            b[j] = X[k * CLD + r16];
        }
        acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(pack4(a), pack4(b), acc, 0, 0, 0);
    }
    return acc;
}

// acc[a][b] += sum_c X[ti + 16a][c] * Y[tj + 16b][c] over one staged slice
template <int NA>
__device__ __forceinline__ void tile_nt(const float* __restrict__ X, const float* __restrict__ Y, float (&acc)[NA][NA], int ti, int tj) {
#pragma unroll 4
    for (int c = 0; c < CW; ++c) {
        float xv[NA], yv[NA];
#pragma unroll
        for (int a = 0; a < NA; ++a) { xv[a] = X[(ti + 16 * a) * CLD + c]; yv[a] = Y[(tj + 16 * a) * CLD + c]; }
#pragma unroll
        for (int a = 0; a < NA; ++a)
#pragma unroll
            for (int b = 0; b < NA; ++b) acc[a][b] += xv[a] * yv[b];
    }
}

// S = qn kn^T * d^-1/2 + bias into M[LP][LP + 1] (keys >= L: -inf), over the d / 16 slices of q and k
template <typename T, int NA>
__device__ __forceinline__ void scores(const T* __restrict__ qkv, long tok0, long ts, long rs3, int L, int d, const float* mu, const float* rs,
                                       const float* s_par, const float* s_emb, bool has_emb, float* M, float* X, float* Y) {
    constexpr int LP = 16 * NA, LDM = LP + 1;
    const float scale = rsqrtf((float)d);
    if constexpr (sizeof(T) == 2) {
        const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        f32x4 acc[blocks_per_wave<NA>()];
#pragma unroll
        for (int t = 0; t < blocks_per_wave<NA>(); ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < d; c0 += CW) {
            stage<T>(X, qkv, rs3, tok0, ts, L, LP, d, c0, mu, rs, s_par, s_par + LONG_DMAX, 1.f);
            stage<T>(Y, qkv + d, rs3, tok0, ts, L, LP, d, c0, mu + LONG_LMAX, rs + LONG_LMAX, s_par + 2 * LONG_DMAX, s_par + 3 * LONG_DMAX, 1.f);
            __syncthreads();
            tile_nt_mfma<NA>(X, Y, acc, wave, lane);
            __syncthreads();
        }
#pragma unroll
        for (int t = 0; t < blocks_per_wave<NA>(); ++t) {
            const int b = wave + 4 * t;
            if (b < NA * NA) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * (b / NA) + 4 * (lane >> 4) + r, j = 16 * (b % NA) + (lane & 15);
                    float s = acc[t][r] * scale;
                    if (has_emb) s += s_emb[t5_bucket(i - j)];
                    M[i * LDM + j] = j < L ? s : -INFINITY;
                }
            }
        }
        __syncthreads();
        return;
    }
    const int ti = threadIdx.x & 15, tj = threadIdx.x >> 4;
    float acc[NA][NA];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int b = 0; b < NA; ++b) acc[a][b] = 0.f;
    for (int c0 = 0; c0 < d; c0 += CW) {
        stage<T>(X, qkv, rs3, tok0, ts, L, LP, d, c0, mu, rs, s_par, s_par + LONG_DMAX, 1.f);
        stage<T>(Y, qkv + d, rs3, tok0, ts, L, LP, d, c0, mu + LONG_LMAX, rs + LONG_LMAX, s_par + 2 * LONG_DMAX, s_par + 3 * LONG_DMAX, 1.f);
        __syncthreads();
        tile_nt<NA>(X, Y, acc, ti, tj);
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int b = 0; b < NA; ++b) {
            const int i = ti + 16 * a, j = tj + 16 * b;
            float s = acc[a][b] * scale;
            if (has_emb) s += s_emb[t5_bucket(i - j)];
            M[i * LDM + j] = j < L ? s : -INFINITY;
        }
    __syncthreads();
}

// row softmax of M in place (rows >= L and keys >= L become 0); with `rescale` the rows become A = 1/L + (P - 1/L) * hs instead of P
__device__ __forceinline__ void softmax_rows(float* M, int L, int LP, bool rescale, float hs) {
    const int LDM = LP + 1, i = threadIdx.x;
    if (i < L) {
        float* row = M + i * LDM;
        float m = -INFINITY;
        for (int j = 0; j < L; ++j) m = fmaxf(m, row[j]);
        float sum = 0.f;
        for (int j = 0; j < L; ++j) { const float e = __expf(row[j] - m); row[j] = e; sum += e; }
        const float inv = 1.f / sum, invL = 1.0f / (float)L;
        for (int j = 0; j < L; ++j) {
            const float pr = row[j] * inv;
            row[j] = rescale ? (invL + (pr - invL) * hs) : pr;
        }
        for (int j = L; j < LP; ++j) row[j] = 0.f;
    } else if (i < LP) {
        for (int j = 0; j < LP; ++j) M[i * LDM + j] = 0.f;
    }
    __syncthreads();
}

template <typename T, int NA>
__global__ void __launch_bounds__(NTL) attn_fwd_long(const T* __restrict__ qkv, T* __restrict__ out, LGeo g, int heads, int d, LPar p,
                                                     float out_scale, int accumulate) {
    constexpr int LP = 16 * NA, LDM = LP + 1;
    extern __shared__ __attribute__((aligned(16))) float smem_long[];
    __shared__ float s_par[4 * LONG_DMAX];
    __shared__ float s_stat[4 * LONG_LMAX];      // mu q | mu k, then rstd q | rstd k
    __shared__ float s_emb[32];
    float* M = smem_long;
    float* X = M + LP * LDM;
    float* Y = X + LP * CLD;
    float* mu = s_stat;
    float* rs = s_stat + 2 * LONG_LMAX;
    for (int i = threadIdx.x; i < 4 * d; i += NTL) {
        const int q = i / d, e = i % d;
        s_par[q * LONG_DMAX + e] = (q == 0 ? p.qw : q == 1 ? p.qb : q == 2 ? p.kw : p.kb)[e];
    }
    const int L = g.L, E = heads * d;
    const long rs3 = 3L * E, nprob = g.nseq * heads;
    for (long pr = blockIdx.x; pr < nprob; pr += gridDim.x) {
        const long s = pr / heads;
        const int head = (int)(pr % heads);
        const long tok0 = lseq_base(g, s);
        const T* base = qkv + head * 3 * d;
        if (threadIdx.x < 32) s_emb[threadIdx.x] = p.emb ? p.emb[threadIdx.x * heads + head] : 0.f;
        row_stats<T>(base, tok0, g.tok_stride, rs3, L, d, mu, rs);
        __syncthreads();
        scores<T, NA>(base, tok0, g.tok_stride, rs3, L, d, mu, rs, s_par, s_emb, p.emb != nullptr, M, X, Y);
        softmax_rows(M, L, LP, p.hscale != nullptr, p.hscale ? p.hscale[head] : 1.f);
        // O = A V, one 16-column slice of V at a time
        const int c = threadIdx.x & 15, ib = threadIdx.x >> 4;
        for (int c0 = 0; c0 < d; c0 += CW) {
            stage<T>(X, base + 2 * d, rs3, tok0, g.tok_stride, L, LP, d, c0, nullptr, nullptr, nullptr, nullptr, 1.f);
            __syncthreads();
            if constexpr (sizeof(T) == 2) {
                const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
                for (int bi = wave; bi < NA; bi += 4) {
                    const f32x4 acc = mm_block<NA>(M, X, bi, false, false, 0.f, 1.f, lane);
                    const int e = c0 + (lane & 15);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = 16 * bi + 4 * (lane >> 4) + r;
                        if (i < L && e < d) {
                            const long o = (tok0 + i * g.tok_stride) * E + head * d + e;
                            float v = acc[r] * out_scale;
                            if (accumulate) v += to_f(out[o]);
                            out[o] = from_f<T>(v);
                        }
                    }
                }
                __syncthreads();
                continue;
            }
            float acc[NA];
#pragma unroll
            for (int a = 0; a < NA; ++a) acc[a] = 0.f;
            for (int j = 0; j < L; ++j) {
                const float v = X[j * CLD + c];
#pragma unroll
                for (int a = 0; a < NA; ++a) acc[a] += M[(ib + 16 * a) * LDM + j] * v;
            }
            const int e = c0 + c;
#pragma unroll
            for (int a = 0; a < NA; ++a) {
                const int i = ib + 16 * a;
                if (i < L && e < d) {
                    const long o = (tok0 + i * g.tok_stride) * E + head * d + e;
                    float r = acc[a] * out_scale;
                    if (accumulate) r += to_f(out[o]);
                    out[o] = from_f<T>(r);
                }
            }
            __syncthreads();
        }
    }
}

// accumulate: bit 0 = add what dqkv holds; bit 1 ("raw out", mode 2) = leave the q / k gradients with respect to the LayerNorm OUTPUTS
// and skip that backward and its parameter sums; bit 2 ("raw in", mode 5 = 1 | 4) = the q / k values dqkv holds are such raw gradients,
// added in front of the LayerNorm backward.  Same meaning as in attn_mfma.hip.
template <typename T, int NA>
__global__ void __launch_bounds__(NTL) attn_bwd_long(const T* __restrict__ qkv, const T* __restrict__ dout, T* __restrict__ dqkv, LGeo g, int heads,
                                                     int d, LPar p, LGrd gr, float out_scale, int mode, float* __restrict__ ws) {
    constexpr int LP = 16 * NA, LDM = LP + 1;
    extern __shared__ __attribute__((aligned(16))) float smem_long[];
    __shared__ float s_par[4 * LONG_DMAX];
    __shared__ float s_stat[4 * LONG_LMAX];
    __shared__ float s_emb[32];
    __shared__ float a_ln[4 * LONG_DMAX];        // this workgroup's parameter-gradient sums: dqw | dqb | dkw | dkb
    __shared__ float a_emb[32 * 16];             // [bucket][head]
    __shared__ float a_hs[16];
    const int ldq = d + 1;
    float* MP = smem_long;                                  // P, later the dqn / dkn plane [LP][d + 1]
    float* MS = MP + LP * (d > LP ? d + 1 : LDM);           // dA, then dS
    float* X = MS + LP * LDM;
    float* Y = X + LP * CLD;
    float* mu = s_stat;
    float* rs = s_stat + 2 * LONG_LMAX;
    const bool raw_out = mode & 2, raw_in = mode & 4, accumulate = mode & 1;
    for (int i = threadIdx.x; i < 4 * d; i += NTL) {
        const int q = i / d, e = i % d;
        s_par[q * LONG_DMAX + e] = (q == 0 ? p.qw : q == 1 ? p.qb : q == 2 ? p.kw : p.kb)[e];
        a_ln[q * LONG_DMAX + e] = 0.f;
    }
    for (int i = threadIdx.x; i < 32 * 16; i += NTL) a_emb[i] = 0.f;
    if (threadIdx.x < 16) a_hs[threadIdx.x] = 0.f;
    const int L = g.L, E = heads * d;
    const long rs3 = 3L * E, nprob = g.nseq * heads;
    const float scale = rsqrtf((float)d), invL = 1.0f / (float)L;
    const int c = threadIdx.x & 15, ib = threadIdx.x >> 4;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (long pr = blockIdx.x; pr < nprob; pr += gridDim.x) {
        const long s = pr / heads;
        const int head = (int)(pr % heads);
        const long tok0 = lseq_base(g, s), ts = g.tok_stride;
        const T* base = qkv + head * 3 * d;
        const T* dob = dout + head * d;
        T* dbase = dqkv + head * 3 * d;
        const float hs = p.hscale ? p.hscale[head] : 1.f;
        if (threadIdx.x < 32) s_emb[threadIdx.x] = p.emb ? p.emb[threadIdx.x * heads + head] : 0.f;
        row_stats<T>(base, tok0, ts, rs3, L, d, mu, rs);
        __syncthreads();
        // ---- P (recomputed)
        scores<T, NA>(base, tok0, ts, rs3, L, d, mu, rs, s_par, s_emb, p.emb != nullptr, MP, X, Y);
        softmax_rows(MP, L, LP, false, 1.f);
        // ---- dA = dO V^T into MS (padded rows / keys are zero: their staged rows are)
        if constexpr (sizeof(T) == 2) {
            f32x4 acc[blocks_per_wave<NA>()];
#pragma unroll
            for (int t = 0; t < blocks_per_wave<NA>(); ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int c0 = 0; c0 < d; c0 += CW) {
                stage<T>(X, dob, (long)E, tok0, ts, L, LP, d, c0, nullptr, nullptr, nullptr, nullptr, out_scale);
                stage<T>(Y, base + 2 * d, rs3, tok0, ts, L, LP, d, c0, nullptr, nullptr, nullptr, nullptr, 1.f);
                __syncthreads();
                tile_nt_mfma<NA>(X, Y, acc, wave, lane);
                __syncthreads();
            }
#pragma unroll
            for (int t = 0; t < blocks_per_wave<NA>(); ++t) {
                const int b = wave + 4 * t;
                if (b < NA * NA) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) MS[(16 * (b / NA) + 4 * (lane >> 4) + r) * LDM + 16 * (b % NA) + (lane & 15)] = acc[t][r];
                }
            }
            __syncthreads();
        } else {
            const int ti = threadIdx.x & 15, tj = threadIdx.x >> 4;
            float acc[NA][NA];
#pragma unroll
            for (int a = 0; a < NA; ++a)
#pragma unroll
                for (int b = 0; b < NA; ++b) acc[a][b] = 0.f;
            for (int c0 = 0; c0 < d; c0 += CW) {
                stage<T>(X, dob, (long)E, tok0, ts, L, LP, d, c0, nullptr, nullptr, nullptr, nullptr, out_scale);
                stage<T>(Y, base + 2 * d, rs3, tok0, ts, L, LP, d, c0, nullptr, nullptr, nullptr, nullptr, 1.f);
                __syncthreads();
                tile_nt<NA>(X, Y, acc, ti, tj);
                __syncthreads();
            }
#pragma unroll
            for (int a = 0; a < NA; ++a)
#pragma unroll
                for (int b = 0; b < NA; ++b) MS[(ti + 16 * a) * LDM + tj + 16 * b] = acc[a][b];
            __syncthreads();
        }
        // ---- dP = dA * hs (head-scale gradient sum (P - 1/L) * dA), dS = P (dP - rowsum(P dP)); one thread per row, rows in order
        float* red = Y;
        if (threadIdx.x < L) {
            const int i = threadIdx.x;
            const float* prow = MP + i * LDM;
            float* srow = MS + i * LDM;
            float dh = 0.f, dot = 0.f;
            for (int j = 0; j < L; ++j) {
                float a = srow[j];
                if (p.hscale) { dh += (prow[j] - invL) * a; a *= hs; }
                srow[j] = a;
            }
            for (int j = 0; j < L; ++j) dot += prow[j] * srow[j];
            for (int j = 0; j < L; ++j) srow[j] = prow[j] * (srow[j] - dot);
            red[i] = dh;
        }
        __syncthreads();
        if (threadIdx.x == 0 && p.hscale && gr.dhscale) {
            float t = 0.f;
            for (int i = 0; i < L; ++i) t += red[i];
            a_hs[head] += t;
        }
        // ---- T5 table gradient: diagonal sums (offset n = i - j, i ascending), then buckets (n ascending)
        if (p.emb && gr.demb) {
            float* diag = X;
            const int t = threadIdx.x;
            if (t < 2 * L - 1) {
                const int n = t - (L - 1);
                float sum = 0.f;
                for (int i = n > 0 ? n : 0; i < L && i - n < L; ++i) sum += MS[i * LDM + (i - n)];
                diag[t] = sum;
            }
            __syncthreads();
            if (t < 32) {
                float sum = 0.f;
                for (int u = 0; u < 2 * L - 1; ++u)
                    if (t5_bucket(u - (L - 1)) == t) sum += diag[u];
                a_emb[t * 16 + head] += sum;
            }
        }
        __syncthreads();
        // ---- dV = A^T dO, A = P rescaled; one 16-column slice of dO at a time
        for (int c0 = 0; c0 < d; c0 += CW) {
            stage<T>(X, dob, (long)E, tok0, ts, L, LP, d, c0, nullptr, nullptr, nullptr, nullptr, out_scale);
            __syncthreads();
            if constexpr (sizeof(T) == 2) {
                for (int bj = wave; bj < NA; bj += 4) {
                    const f32x4 acc = mm_block<NA>(MP, X, bj, true, p.hscale != nullptr, invL, hs, lane);
                    const int e = c0 + (lane & 15);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int j = 16 * bj + 4 * (lane >> 4) + r;
                        if (j < L && e < d) {
                            T* dst = dbase + (tok0 + j * ts) * rs3 + 2 * d + e;
                            float v = acc[r];
                            if (accumulate) v += to_f(*dst);
                            *dst = from_f<T>(v);
                        }
                    }
                }
                __syncthreads();
                continue;
            }
            float acc[NA];
#pragma unroll
            for (int a = 0; a < NA; ++a) acc[a] = 0.f;
            for (int i = 0; i < L; ++i) {
                const float o = X[i * CLD + c];
#pragma unroll
                for (int a = 0; a < NA; ++a) {
                    const float pr_ = MP[i * LDM + ib + 16 * a];
                    const float av = p.hscale ? (invL + (pr_ - invL) * hs) : pr_;
                    acc[a] += av * o;
                }
            }
            const int e = c0 + c;
#pragma unroll
            for (int a = 0; a < NA; ++a) {
                const int j = ib + 16 * a;
                if (j < L && e < d) {
                    T* dst = dbase + (tok0 + j * ts) * rs3 + 2 * d + e;
                    float v = acc[a];
                    if (accumulate) v += to_f(*dst);
                    *dst = from_f<T>(v);
                }
            }
            __syncthreads();
        }
        // ---- dqn = dS kn * d^-1/2 (part 0), then dkn = dS^T qn * d^-1/2 (part 1), each into the plane P held, then its LayerNorm backward
        for (int part = 0; part < 2; ++part) {
            const int o = 1 - part;     // the other side's slices: kn for dqn, qn for dkn
            for (int c0 = 0; c0 < d; c0 += CW) {
                stage<T>(X, base + o * d, rs3, tok0, ts, L, LP, d, c0, mu + o * LONG_LMAX, rs + o * LONG_LMAX, s_par + 2 * o * LONG_DMAX,
                         s_par + (2 * o + 1) * LONG_DMAX, 1.f);
                __syncthreads();
                if constexpr (sizeof(T) == 2) {
                    for (int bi = wave; bi < NA; bi += 4) {
                        const f32x4 acc = mm_block<NA>(MS, X, bi, part == 1, false, 0.f, 1.f, lane);
                        const int e = c0 + (lane & 15);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int i = 16 * bi + 4 * (lane >> 4) + r;
                            if (i < L && e < d) MP[i * ldq + e] = acc[r] * scale;
                        }
                    }
                    __syncthreads();
                    continue;
                }
                float acc[NA];
#pragma unroll
                for (int a = 0; a < NA; ++a) acc[a] = 0.f;
                for (int j = 0; j < L; ++j) {
                    const float x = X[j * CLD + c];
#pragma unroll
                    for (int a = 0; a < NA; ++a) acc[a] += (part == 0 ? MS[(ib + 16 * a) * LDM + j] : MS[j * LDM + ib + 16 * a]) * x;
                }
                const int e = c0 + c;
#pragma unroll
                for (int a = 0; a < NA; ++a) {
                    const int i = ib + 16 * a;
                    if (i < L && e < d) MP[i * ldq + e] = acc[a] * scale;
                }
                __syncthreads();
            }
            const long col = part * d;
            if (raw_out) {       // first of two passes over these tokens: the gradient with respect to the LayerNorm outputs, as it stands
                for (int idx = threadIdx.x; idx < L * d; idx += NTL) {
                    const int i = idx / d, e = idx % d;
                    T* dst = dbase + (tok0 + i * ts) * rs3 + col + e;
                    float v = MP[i * ldq + e];
                    if (accumulate) v += to_f(*dst);
                    *dst = from_f<T>(v);
                }
                __syncthreads();
                continue;
            }
            if (raw_in) {        // the other pass's raw gradient joins in front of the LayerNorm backward
                for (int idx = threadIdx.x; idx < L * d; idx += NTL) {
                    const int i = idx / d, e = idx % d;
                    MP[i * ldq + e] += to_f(dbase[(tok0 + i * ts) * rs3 + col + e]);
                }
                __syncthreads();
            }
            const float* w = s_par + 2 * part * LONG_DMAX;
            const float* pmu = mu + part * LONG_LMAX;
            const float* prs = rs + part * LONG_LMAX;
            float* m1s = Y;
            float* m2s = Y + LONG_LMAX;
            if (threadIdx.x < L) {       // row means of g = dn * w and g * xhat
                const int i = threadIdx.x;
                const T* xr = base + (tok0 + i * ts) * rs3 + col;
                float m1 = 0.f, m2 = 0.f;
                for (int e = 0; e < d; ++e) {
                    const float xh = (to_f(xr[e]) - pmu[i]) * prs[i];
                    const float gg = MP[i * ldq + e] * w[e];
                    m1 += gg; m2 += gg * xh;
                }
                m1s[i] = m1 / (float)d;
                m2s[i] = m2 / (float)d;
            }
            __syncthreads();
            if (threadIdx.x < d) {       // dx = rstd (g - m1 - xhat m2), one thread per column, rows in order; the affine sums on the way
                const int e = threadIdx.x;
                float sw = 0.f, sb = 0.f;
                for (int i = 0; i < L; ++i) {
                    const long r = (tok0 + i * ts) * rs3 + col + e;
                    const float xh = (to_f(base[r]) - pmu[i]) * prs[i];
                    const float dn = MP[i * ldq + e];
                    sw += dn * xh;
                    sb += dn;
                    float v = prs[i] * (dn * w[e] - m1s[i] - xh * m2s[i]);
                    if (accumulate && !raw_in) v += to_f(dbase[r]);
                    dbase[r] = from_f<T>(v);
                }
                a_ln[2 * part * LONG_DMAX + e] += sw;
                a_ln[(2 * part + 1) * LONG_DMAX + e] += sb;
            }
            __syncthreads();
        }
    }
    // ---- this workgroup's parameter-gradient row (AttnReduceJob layout: dqw | dqb | dkw | dkb [d] each, demb [32][heads], dhscale [heads])
    __syncthreads();
    const int nvals = 4 * d + 32 * heads + heads;
    for (int i = threadIdx.x; i < nvals; i += NTL) {
        float val;
        float* dst;
        if (i < 4 * d) {
            const int q = i / d, e = i % d;
            val = a_ln[q * LONG_DMAX + e];
            dst = q == 0 ? gr.dqw : q == 1 ? gr.dqb : q == 2 ? gr.dkw : gr.dkb;
            if (dst) dst += e;
        } else if (i < 4 * d + 32 * heads) {
            const int t = i - 4 * d;
            val = a_emb[(t / heads) * 16 + (t % heads)];
            dst = gr.demb ? gr.demb + t : nullptr;
        } else {
            const int t = i - 4 * d - 32 * heads;
            val = a_hs[t];
            dst = gr.dhscale ? gr.dhscale + t : nullptr;
        }
        if (ws) ws[(long)blockIdx.x * nvals + i] = val;
        else if (dst && val != 0.f) atomicAdd(dst, val);
    }
}

// dst += sum over workspace rows, one writer per value in row order (param_reduce.h)
__global__ void __launch_bounds__(64 * BF_RED_FL) attn_long_ws_reduce(AttnReduceJob j) {
    __shared__ float red[1][BF_RED_FL][64];
    attn_reduce_block(j, blockIdx.x, blockIdx.y, gridDim.y, red);
}

size_t fwd_lds(int LP) { return ((size_t)LP * (LP + 1) + 2 * (size_t)LP * CLD) * sizeof(float); }
size_t bwd_lds(int LP, int d) { return ((size_t)LP * ((d > LP ? d : LP) + 1) + (size_t)LP * (LP + 1) + 2 * (size_t)LP * CLD) * sizeof(float); }

// raises a kernel's dynamic-LDS limit to the most its instantiation ever asks for (the backward's plan grows with d): once per device
template <typename K>
int long_set_lds(K kernel, size_t max_shm, BfPerDeviceOnce& once) {
    if (max_shm > 64 * 1024 && !once.flag()) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)max_shm);
        if (e != hipSuccess) return bf_fail(e, __FILE__, __LINE__);
        once.flag() = true;
    }
    return 0;
}

// persistent backward workgroups: at most this many (one workspace row each); a fixed number, so the rows -- and the order in which the
// reduction adds them -- do not depend on the device
constexpr long LONG_BWD_GRID = 512;

template <typename T, int NA>
int go_fwd_long(const void* qkv, void* out, const LGeo& g, int heads, int d, const LPar& p, float out_scale, int accumulate, hipStream_t st) {
    const size_t shm = fwd_lds(16 * NA);
    static BfPerDeviceOnce once;
    if (int rc = long_set_lds(attn_fwd_long<T, NA>, shm, once)) return rc;
    const long nprob = g.nseq * heads;
    const int grid = (int)std::min<long>(nprob, 256L * 8);
    hipLaunchKernelGGL((attn_fwd_long<T, NA>), dim3(grid), dim3(NTL), shm, st, (const T*)qkv, (T*)out, g, heads, d, p, out_scale, accumulate);
    BF_CHECK_LAUNCH();
    return 0;
}

template <typename T, int NA>
int go_bwd_long(const void* qkv, const void* dout, void* dqkv, const LGeo& g, int heads, int d, const LPar& p, const LGrd& gr, float out_scale,
                int mode, float* ws, long ws_floats, int* rows_out, hipStream_t st) {
    const size_t shm = bwd_lds(16 * NA, d);
    static BfPerDeviceOnce once;
    if (int rc = long_set_lds(attn_bwd_long<T, NA>, bwd_lds(16 * NA, LONG_DMAX), once)) return rc;
    const long nprob = g.nseq * heads;
    const int nvals = 4 * d + 32 * heads + heads;
    long grid = std::min<long>(nprob, LONG_BWD_GRID);
    if (ws && ws_floats < grid * nvals) { grid = ws_floats / nvals; if (grid < 1) { grid = std::min<long>(nprob, LONG_BWD_GRID); ws = nullptr; } }
    hipLaunchKernelGGL((attn_bwd_long<T, NA>), dim3((int)grid), dim3(NTL), shm, st, (const T*)qkv, (const T*)dout, (T*)dqkv, g, heads, d, p, gr,
                       out_scale, mode, ws);
    BF_CHECK_LAUNCH();
    if (rows_out) { *rows_out = ws ? (int)grid : 0; return 0; }       // the caller reduces the rows later (AttnReduceJob)
    if (ws) {
        const AttnReduceJob j{ws, (int)grid, d, heads, gr.dqw, gr.dqb, gr.dkw, gr.dkb, gr.demb, gr.dhscale};
        hipLaunchKernelGGL(attn_long_ws_reduce, dim3(bf_cdiv(nvals, 64), 1), dim3(64 * BF_RED_FL), 0, st, j);
        BF_CHECK_LAUNCH();
    }
    return 0;
}

}  // namespace

// dispatched from bf_attn_fwd / bf_attn_bwd (attn.hip) for 33 <= L <= 128; both dtypes, any head dim the chunk admits up to 128
int bf_attn_fwd_long(int dtype, const void* qkv, void* out, long nseq, int L, long inner, long outer_stride, long inner_stride, long tok_stride,
                     int heads, int d, const float* qw, const float* qb, const float* kw, const float* kb, const float* emb, const float* hscale,
                     float out_scale, int accumulate, hipStream_t st) {
    BF_REQUIRE(L > 32 && L <= LONG_LMAX && d <= LONG_DMAX && heads <= 16, "bf_attn_fwd_long: unsupported shape");
    const LGeo g{nseq, L, inner, outer_stride, inner_stride, tok_stride};
    const LPar p{qw, qb, kw, kb, emb, hscale};
    const int na = (L + 15) / 16;
#define GO(NA) if (na == NA) return dtype == BF_DTYPE_BF16 ? go_fwd_long<bf16, NA>(qkv, out, g, heads, d, p, out_scale, accumulate, st) \
                                                        : go_fwd_long<float, NA>(qkv, out, g, heads, d, p, out_scale, accumulate, st)
    GO(3); GO(4); GO(5); GO(6); GO(7); GO(8);
#undef GO
    return bf_fail_msg("bf_attn_fwd_long: unsupported shape", __FILE__, __LINE__);
}

int bf_attn_bwd_long(int dtype, const void* qkv, const void* dout, void* dqkv, long nseq, int L, long inner, long outer_stride, long inner_stride,
                     long tok_stride, int heads, int d, const float* qw, const float* qb, const float* kw, const float* kb, const float* emb,
                     const float* hscale, float* dqw, float* dqb, float* dkw, float* dkb, float* demb, float* dhscale, float out_scale,
                     int accumulate, float* ws, long ws_floats, int* rows_out, hipStream_t st) {
    BF_REQUIRE(L > 32 && L <= LONG_LMAX && d <= LONG_DMAX && heads <= 16, "bf_attn_bwd_long: unsupported shape");
    const LGeo g{nseq, L, inner, outer_stride, inner_stride, tok_stride};
    const LPar p{qw, qb, kw, kb, emb, hscale};
    const LGrd gr{dqw, dqb, dkw, dkb, demb, dhscale};
    const int na = (L + 15) / 16;
#define GO(NA) if (na == NA) return dtype == BF_DTYPE_BF16 \
        ? go_bwd_long<bf16, NA>(qkv, dout, dqkv, g, heads, d, p, gr, out_scale, accumulate, ws, ws_floats, rows_out, st) \
        : go_bwd_long<float, NA>(qkv, dout, dqkv, g, heads, d, p, gr, out_scale, accumulate, ws, ws_floats, rows_out, st)
    GO(3); GO(4); GO(5); GO(6); GO(7); GO(8);
#undef GO
    return bf_fail_msg("bf_attn_bwd_long: unsupported shape", __FILE__, __LINE__);
}
