// The LDS transform of the field-error spectra (spectra.hip, complex fp64) and of the spectral criterion (spectral_loss.hip, complex fp32),
// and the radial shell of a mode: one text, so that the two files' promise of the same shells and the same operations in the same order holds
// by construction.  A Stockham autosort in LDS over the mixed-radix factorisation of the side: 4s, then 2, 3, 5, then every other prime factor
// by one generic radix-p stage of p terms per output (a prime side is a plain DFT: correct, merely slow).  Device templates over the complex
// type C (float2 or double2) and plain host functions; nothing here holds state.  Each user keeps its own sizes (lines per workgroup, LDS
// struct, line stride) and compiles this text under its own flags.
#pragma once
#include "bf_common.h"
#include <algorithm>

constexpr int FFT_NT = 256;                        // the workgroup size the stage loops stride by: every user asserts that its own equals it

template <class C> using fft_real = decltype(C().x);
template <class C> __device__ __forceinline__ C cmul(C a, C b) { return C(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
template <class C> __device__ __forceinline__ C cadd(C a, C b) { return C(a.x + b.x, a.y + b.y); }
template <class C> __device__ __forceinline__ C csub(C a, C b) { return C(a.x - b.x, a.y - b.y); }
template <class C> __device__ __forceinline__ C mul_mi(C a) { return C(a.y, -a.x); }       // a * (-i)

struct Plan { int n, nf; short r[12]; };           // n = product of r[0 .. nf)
inline Plan make_plan(int n) {
    Plan p{n, 0, {}};
    int m = n;
    auto take = [&](int r) { while (m % r == 0) { p.r[p.nf++] = (short)r; m /= r; } };
    take(4); take(2); take(3); take(5);
    for (int r = 7; m > 1; r += 2) take(r);
    return p;
}
// shells of an H x W plane: 1 + the largest q with q^2 <= S^2 / 2, S = min(H, W)
inline int shell_count(int H, int W) {
    const long S = std::min(H, W), v = S * S / 2;
    long q = (long)sqrt((double)v);
    while ((q + 1) * (q + 1) <= v) ++q;
    while (q * q > v) --q;
    return (int)q + 1;
}
// the shell of mode (fy, fx): the largest q with q^2 H^2 W^2 <= S^2 (fy^2 W^2 + fx^2 H^2), in int64 (the floating-point root only proposes a
// candidate that the integer inequalities correct)
__device__ __forceinline__ int shell_of(long fy, long fx, long H, long W) {
    const long S = min(H, W), D = H * H * W * W, V = S * S * (fy * fy * W * W + fx * fx * H * H);
    long q = (long)sqrt((double)V / (double)D);
    while ((q + 1) * (q + 1) * D <= V) ++q;
    while (q > 0 && q * q * D > V) --q;
    return (int)q;
}
// exp(-2 pi i j / n): formed in fp64, rounded once to C's element type
template <class C> __device__ __forceinline__ C twiddle(int j, int n) {
    double sn, cs;
    sincospi(2.0 * (double)j / (double)n, &sn, &cs);
    return C((fft_real<C>)cs, (fft_real<C>)-sn);
}

template <int R, class C> __device__ __forceinline__ void butterfly(C* v) {
    typedef fft_real<C> T;
    if constexpr (R == 2) {
        const C a = v[0]; v[0] = cadd(a, v[1]); v[1] = csub(a, v[1]);
    } else if constexpr (R == 3) {
        const T s3 = (T)0.86602540378443864676;
        const C t = cadd(v[1], v[2]), m = C(v[0].x - (T)0.5 * t.x, v[0].y - (T)0.5 * t.y), d = csub(v[1], v[2]);
        const C r = mul_mi(C(s3 * d.x, s3 * d.y));
        v[0] = cadd(v[0], t); v[1] = cadd(m, r); v[2] = csub(m, r);
    } else if constexpr (R == 4) {
        const C a0 = cadd(v[0], v[2]), a1 = csub(v[0], v[2]), a2 = cadd(v[1], v[3]), a3 = mul_mi(csub(v[1], v[3]));
        v[0] = cadd(a0, a2); v[1] = cadd(a1, a3); v[2] = csub(a0, a2); v[3] = csub(a1, a3);
    } else {
        static_assert(R == 5, "butterfly: radix 2, 3, 4 or 5");
        const T c1 = (T)0.30901699437494742410, c2 = (T)-0.80901699437494742410, s1 = (T)0.95105651629515357212, s2 = (T)0.58778525229247312917;
        const C a1 = cadd(v[1], v[4]), a2 = cadd(v[2], v[3]), b1 = csub(v[1], v[4]), b2 = csub(v[2], v[3]);
        const C r1 = C(v[0].x + c1 * a1.x + c2 * a2.x, v[0].y + c1 * a1.y + c2 * a2.y);
        const C r2 = C(v[0].x + c2 * a1.x + c1 * a2.x, v[0].y + c2 * a1.y + c1 * a2.y);
        const C i1 = mul_mi(C(s1 * b1.x + s2 * b2.x, s1 * b1.y + s2 * b2.y));
        const C i2 = mul_mi(C(s2 * b1.x - s1 * b2.x, s2 * b1.y - s1 * b2.y));
        v[0] = cadd(v[0], cadd(a1, a2)); v[1] = cadd(r1, i1); v[4] = csub(r1, i1); v[2] = cadd(r2, i2); v[3] = csub(r2, i2);
    }
}

// one Stockham stage of radix R over `lines` lines of N, `ls` elements apart: butterfly j of a line reads x[j + t * N/R], turned by w^(t k) with
// k = j % Ns and w = exp(-2 pi i / (Ns R)), and writes y[(j - k) R + k + t Ns]
template <int R, class C> __device__ __forceinline__ void stage(const C* x, C* y, const C* tw, int N, int Ns, int lines, int ls) {
    const int T = N / R, stride = T / Ns;
    for (int i = threadIdx.x; i < lines * T; i += FFT_NT) {
        const int l = i / T, j = i - l * T, k = j % Ns;
        const C* src = x + l * ls + j;
        C v[R];
        v[0] = src[0];
#pragma unroll
        for (int t = 1; t < R; ++t) v[t] = cmul(src[t * T], tw[t * k * stride]);
        butterfly<R>(v);
        C* dst = y + l * ls + (j - k) * R + k;
#pragma unroll
        for (int t = 0; t < R; ++t) dst[t * Ns] = v[t];
    }
}
// any other prime factor p: a thread per OUTPUT adds its p terms in order; both turns are one table entry, stepped modulo N
template <class C> __device__ __forceinline__ void stage_generic(const C* x, C* y, const C* tw, int N, int Ns, int p, int lines, int ls) {
    const int T = N / p, stride = T / Ns;
    for (int i = threadIdx.x; i < lines * N; i += FFT_NT) {
        const int l = i / N, o = i - l * N, k = o % Ns, u = (o / Ns) % p, j = (o / (Ns * p)) * Ns + k;
        const int step = (k * stride + u * T) % N;
        const C* src = x + l * ls + j;
        C acc = src[0];
        for (int t = 1, idx = step; t < p; ++t) {
            acc = cadd(acc, cmul(src[t * T], tw[idx]));
            idx += step; if (idx >= N) idx -= N;
        }
        y[l * ls + o] = acc;
    }
}
// `lines` transforms of length plan.n from x, the lines `ls` >= plan.n elements apart, tw[j] = twiddle(j, plan.n); returns the buffer (x or y)
// that holds them.  Every thread of a workgroup of FFT_NT calls this; the caller has synchronised after filling x, and the result is synchronised.
template <class C> __device__ __forceinline__ C* fft_lines(C* x, C* y, const C* tw, const Plan& plan, int lines, int ls) {
    const int N = plan.n;
    int Ns = 1;
    for (int f = 0; f < plan.nf; ++f) {
        const int r = plan.r[f];
        if (r == 4) stage<4>(x, y, tw, N, Ns, lines, ls);
        else if (r == 2) stage<2>(x, y, tw, N, Ns, lines, ls);
        else if (r == 3) stage<3>(x, y, tw, N, Ns, lines, ls);
        else if (r == 5) stage<5>(x, y, tw, N, Ns, lines, ls);
        else stage_generic(x, y, tw, N, Ns, r, lines, ls);
        __syncthreads();
        C* t = x; x = y; y = t;
        Ns *= r;
    }
    return x;
}
// the same on dense lines, ls = plan.n.  An overload, not a stride handed in by the caller: formed here the stride is the value the stages
// already hold as N, and the fp64 user compiles to the instruction stream it had when the lines were N apart by definition.
template <class C> __device__ __forceinline__ C* fft_lines(C* x, C* y, const C* tw, const Plan& plan, int lines) {
    return fft_lines(x, y, tw, plan, lines, plan.n);
}
